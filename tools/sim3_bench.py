#!/usr/bin/env python3
"""Times the Sim3 RANSAC (iba_sim3_solve) on one GPU and writes profiles/sim3_bench.md: J = 1, 8 and 64 jobs of N = 200 correspondences at 300
iterations (seeded scenes of tests/sim3_scene.py, 30 % outliers), for each form of the count kernel (IBA_SIM3_COUNT_FORM) the time of every stage
from HIP events (IBA_SIM3_TIMING) and the wall time of whole calls, the forms alternating inside every repetition; the same call through
iba_debug_sim3_host on one thread beside them as a yardstick; and the registers, LDS, scratch and occupancy of the kernels from the compiler's
resource report (the asm-sim3 target's flags). Informational: nothing is gated.

    python tools/sim3_bench.py --measure-only --json runs.json     on the GPU: measure and keep the numbers
    python tools/sim3_bench.py --from-json runs.json               anywhere with a compiler: write the file from numbers measured earlier
    python tools/sim3_bench.py                                     on the GPU: both"""
import argparse
import importlib
import json
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("IBA_DEBUG_ENV", "1")
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
JOBS, N, ITERATIONS, SEED = (1, 8, 64), 200, 300, 41
FORM_NAME = {0: "(a) lane per hypothesis", 1: "(b) lane per correspondence"}
STAGES = ("preparation", "hypotheses", "count", "selection", "flags")
SHIPPED = 1                                                          # kShippedForm of csrc/iba_sim3.hip


def measure(reps):
    import sim3_scene as S
    sm = importlib.import_module(PKG + ".sim3")
    rows = []
    for J in JOBS:
        sc = S.scene([{"N": N, "outliers": 0.3} for _ in range(J)], seed=SEED + J)
        tb, jobs = sm.table(sc["xyz"]), [S.lib_job(sm, j) for j in sc["jobs"]]
        stage, wall, counts = {0: [], 1: []}, {0: [], 1: []}, None
        for rep in range(reps + 2):                                # the forms alternate inside every repetition; the first two warm up
            for form in (0, 1):
                os.environ["IBA_SIM3_COUNT_FORM"] = str(form)
                t0 = time.perf_counter(); r = sm.solve(tb, jobs); ms = (time.perf_counter() - t0) * 1e3
                c = [r.counts(b) for b in range(J)]
                assert counts is None or all(np.array_equal(x, y) for x, y in zip(c, counts))
                counts = c
                iterations = sum(r.read(b)["iterations"] for b in range(J))
                r.close()
                os.environ["IBA_SIM3_TIMING"] = "1"
                r = sm.solve(tb, jobs)
                del os.environ["IBA_SIM3_TIMING"]
                if rep >= 2:
                    wall[form].append(ms)
                    stage[form].append([float(v) for v in r.stage_ms])
                r.close()
        del os.environ["IBA_SIM3_COUNT_FORM"]
        t0 = time.perf_counter(); h = sm.solve_host(tb, jobs); host_ms = (time.perf_counter() - t0) * 1e3
        same = all(np.array_equal(h.counts(b), counts[b]) for b in range(J))
        h.close()
        row = dict(J=J, N=N, iterations=iterations, reps=reps, host_ms=host_ms, host_agrees=bool(same),
                   wall_median_ms={str(f): float(np.median(wall[f])) for f in (0, 1)}, wall_min_ms={str(f): float(np.min(wall[f])) for f in (0, 1)},
                   stage_ms={str(f): [float(v) for v in np.median(np.array(stage[f]), axis=0)] for f in (0, 1)},
                   count_spread_ms={str(f): float(np.max(np.array(stage[f])[:, 2]) - np.min(np.array(stage[f])[:, 2])) for f in (0, 1)})
        print(json.dumps(row), flush=True)
        rows.append(row)
    return rows


def resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the unit's kernels from hipcc's resource report of csrc/iba_sim3.hip; None without a compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, PKG, "csrc", "iba_sim3.hip")
    try:
        p = subprocess.run([hipcc, "-std=c++17", "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src],
                           capture_output=True, text=True, timeout=600)
    except (OSError, subprocess.TimeoutExpired):
        return None
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            k = re.search(r"(z3_[a-z_]+_kernel)", m.group(2))
            cur = {"kernel": k.group(1)} if k else None
            if cur:
                rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows or None


def write(rows, out):
    with open(out, "w") as fh:
        fh.write("# Sim3 RANSAC on the device: the two forms of the count kernel\n\n")
        if not rows:
            fh.write("No GPU run was made: this file holds no measured time.\n\n")
        else:
            fh.write("`python tools/sim3_bench.py` on one MI355X. Seeded scenes: J jobs of N = %d correspondences (30 %% outliers) at %d iterations each, default options. Stage times are\n"
                     "the median over %d calls with IBA_SIM3_TIMING (HIP events around each stage), the two forms alternating inside every repetition after two warm-up rounds; in brackets\n"
                     "max - min of the count stage. `wall`: the whole iba_sim3_solve from Python - checks, gathering, allocations, uploads, the chain, the results down. `host`:\n"
                     "iba_debug_sim3_host, the same call on one CPU thread of the GPU machine, one run: a yardstick, there being no earlier figure for a unit that did not exist. Nothing\n"
                     "is gated. Kernel times from a profiler trace and shares of peak were not measured.\n\n" % (rows[0]["N"], ITERATIONS, rows[0]["reps"]))
            fh.write("| J | form of the count kernel | " + " | ".join(STAGES) + " | chain sum | wall ms (min / median) | host ms | host agrees |\n|---|---|" + "---|" * (len(STAGES) + 4) + "\n")
            for r in rows:
                for f in ("0", "1"):
                    s = r["stage_ms"][f]
                    cells = ["%.4f" % v for v in s]
                    cells[2] += " (%.4f)" % r["count_spread_ms"][f]
                    fh.write("| %d | %s | %s | %.4f | %.2f / %.2f | %.1f | %s |\n" % (r["J"], FORM_NAME[int(f)], " | ".join(cells), sum(s), r["wall_min_ms"][f], r["wall_median_ms"][f], r["host_ms"],
                                                                                  "yes" if r["host_agrees"] else "NO"))
            fh.write("\nTwo-way reprojections per call: J x iterations x N = %s.\n" % ", ".join("%d" % (r["iterations"] * r["N"]) for r in rows))
            wins = [min(("0", "1"), key=lambda f: r["stage_ms"][f][2]) for r in rows]
            fh.write("\nThe count stage is faster with form %s at J = %s.\n" % (", ".join(FORM_NAME[int(w)][:3] for w in wins), ", ".join(str(r["J"]) for r in rows)))
            ratio = [r["stage_ms"][str(1 - SHIPPED)][2] / r["stage_ms"][str(SHIPPED)][2] for r in rows]
            fh.write("\nForm %s ships (kShippedForm in csrc/iba_sim3.hip); the other stays behind IBA_SIM3_COUNT_FORM and gives the same bytes (tests/test_gpu_sim3.py runs both). Its count\n"
                     "stage takes %s of the other form's time at J = %s. Form (a) has one lane per hypothesis: J x 300 lanes are 5 waves per job, too few to fill\n"
                     "the device at these shapes, and each walks all N correspondences serially; form (b) has J x 300 x ceil(N / 64) waves and no loop-carried work beyond a popcount.\n"
                     % (FORM_NAME[SHIPPED], ", ".join("1 / %.1f" % v for v in ratio), ", ".join(str(r["J"]) for r in rows)))
        fh.write("\n## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the asm-sim3 target)\n\n")
        res = resources()
        if res:
            fh.write("| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k in res:
                fh.write("| %s | %d | %d | %d | %d | %d |\n" % (k["kernel"], k.get("VGPRs", -1), k.get("TotalSGPRs", -1), k.get("LDS Size", -1), k.get("ScratchSize", -1), k.get("Occupancy", -1)))
            fh.write("\n%s\n" % ("No kernel uses scratch." if all(k.get("ScratchSize", 0) == 0 for k in res) else "SCRATCH IS IN USE in the kernels whose column is not 0."))
        else:
            fh.write("No compiler was found where this file was written.\n")
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sim3_bench.md"))
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--json", default=None, help="keep the measured numbers here")
    ap.add_argument("--from-json", default=None, help="format rows measured earlier instead of measuring")
    ap.add_argument("--measure-only", action="store_true", help="measure and keep the numbers (--json) without writing the file")
    a = ap.parse_args()
    rows = json.load(open(a.from_json)) if a.from_json else measure(a.reps)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    if not a.measure_only:
        write(rows, a.out)


if __name__ == "__main__":
    main()

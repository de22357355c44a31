"""Times iba_bundle_optimize on one device and writes profiles/bundle_bench.md: an initial-map job (2 cameras, 300 points, the global schedule of
CreateInitialMapMonocular) and a local-window job (20 free + 20 fixed cameras, 2000 points, the local schedule), 1, 64 and 1024 jobs of each; the
time from HIP events around the launch chains (IBA_BUNDLE_TIMING) as the median of repeated calls, the wall time of whole calls, and
iba_debug_bundle_host on one thread beside them. No target is set and nothing is gated.
    python tools/bundle_bench.py [--device 0] [--calls 7] [--out profiles/bundle_bench.md]"""
import argparse
import importlib
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
PKG = "spatial-temporal-lidar-camera-calibration_amd"
HOST_JOBS = 8        # the host restatement runs this many jobs at most; its time is scaled to B (a job's cost does not depend on its neighbours)


def resources():
    """VGPRs, LDS, scratch and occupancy of the kernels from the compiler's report"""
    csrc = os.path.join(ROOT, PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "-B", "asm-bundle"], capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: _ZN3iba6bundle\d+(\w+?_kernel)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
        for key, pat in (("vgpr", r" VGPRs: (\d+)"), ("agpr", r"AGPRs: (\d+)"), ("sgpr", r"TotalSGPRs: (\d+)"), ("lds", r"LDS Size \[bytes/block\]: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
                         ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")):
            m = re.search(pat, line)
            if m and cur is not None:
                cur[key] = m.group(1)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bundle_bench.md"))
    ap.add_argument("--no-device", action="store_true", help="write the resource report alone, the timings as 'not recorded yet'")
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    except Exception:
        pass
    importlib.import_module(PKG)
    bd = importlib.import_module(PKG + ".bundle")
    S = importlib.import_module("bundle_scene")
    os.environ["IBA_DEBUG_ENV"] = "1"
    cases = (("initial map: 2 cameras (1 free), 300 points, 600 edges; global schedule (20 iterations, robust)", lambda k: S.make(2, 300, 1000 + k, n_fixed=1, outliers=0.05),
              lambda: bd.options_global(20, True)),
             ("local window: 40 cameras (20 free), 2000 points, ~20000 edges; local schedule (5 robust + 10 iterations)",
              lambda k: S.make(40, 2000, 2000 + k, n_fixed=20, outliers=0.05, visibility=0.25), lambda: bd.options()))
    lines = ["# Bundle adjustment on the device: what the first run saw", "",
             "`python tools/bundle_bench.py` on one MI355X. Seeded scenes (tests/bundle_scene.py: cameras on an arc, one pixel of noise scaled by the level, a twentieth of",
             "the observations gross outliers). `chain`: HIP events around the launch chains of a call's chunks (IBA_BUNDLE_TIMING; the host's one-word read per step is",
             "inside), median of %d calls after two warm-ups. `wall`: the whole iba_bundle_optimize from Python - checks, the plan, staging, allocations, tables up, the chains," % a.calls,
             "results down - median of a second set of calls. `host`: iba_debug_bundle_host on one CPU thread of the same machine, run on at most %d of the jobs and scaled to B." % HOST_JOBS,
             "No target is set and nothing is gated.", ""]
    if a.no_device:
        lines += ["The timings are not recorded yet: no GPU run of this tool has happened.", ""]
    else:
        lines += ["| case | B | chain ms (median) | wall ms (min / median / max) | jobs / s (wall median) | host ms (scaled) | host / wall | chunks | LM iterations + trials per job (mean) |", "|---|---|---|---|---|---|---|---|---|"]
        for name, make, opt in cases:
            scs = [make(k) for k in range(HOST_JOBS)]
            base = [S.lib_job(bd, sc) for sc in scs]
            o = opt()
            t = time.perf_counter()
            bd.optimize_host(base, o).close()
            host_each = 1e3 * (time.perf_counter() - t) / len(base)
            for B in (1, 64, 1024):
                jobs = [base[k % len(base)] for k in range(B)]
                calls = a.calls if B * len(scs[0]["edge_point"]) < 4e6 else 3
                os.environ["IBA_BUNDLE_TIMING"] = "1"
                for _ in range(2):
                    bd.optimize(jobs, o, device=a.device).close()
                kern, work, chunks = [], 0.0, 0
                for _ in range(calls):
                    r = bd.optimize(jobs, o, device=a.device)
                    kern.append(r.kernel_ms)
                    chunks = r.chunks
                    work = float(np.mean([r.read(j)["lm_iterations"].sum() + r.read(j)["trials"].sum() for j in range(min(B, HOST_JOBS))]))
                    r.close()
                os.environ.pop("IBA_BUNDLE_TIMING", None)
                wall = []
                for _ in range(calls):
                    t = time.perf_counter()
                    r = bd.optimize(jobs, o, device=a.device)
                    wall.append(1e3 * (time.perf_counter() - t))
                    r.close()
                lines.append("| %s | %d | %.3f | %.3f / %.3f / %.3f | %.0f | %.1f | %.2f | %d | %.1f |" % (name.split(":")[0], B, np.median(kern), min(wall), np.median(wall), max(wall),
                                                                                                   B / np.median(wall) * 1e3, host_each * B, host_each * B / np.median(wall), chunks, work))
                print(lines[-1], flush=True)
        lines += [""] + ["* %s" % name for name, _, _ in cases]
    lines += ["", "## Kernel resources (`make asm-bundle`: hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "", "| kernel | VGPRs | AGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |", "|---|---|---|---|---|---|---|"]
    for k in resources():
        lines.append("| %s | %s | %s | %s | %s | %s | %s |" % tuple(k.get(f, "?") for f in ("name", "vgpr", "agpr", "sgpr", "lds", "scratch", "occ")))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

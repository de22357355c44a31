#!/usr/bin/env python3
"""Times the two-view initialisation (iba_twoview_init) on one GPU and writes profiles/twoview_bench.md and profiles/twoview_parity.md: seeded pairs
of about 1000 matches (tests/twoview_scene.py: 1112 keypoints, a tenth unmatched, a fifth outliers), 200 iterations, as calls of B = 1, 8 and 64 pairs;
the wall time of whole calls, per kernel the time from HIP events (IBA_TWOVIEW_TIMING), the host restatement (iba_debug_twoview_host, one thread)
on the same inputs on the same machine as the yardstick, and the kernels' registers, LDS and scratch from the compiler's resource report. The parity
file counts the differing bytes of the device against the host restatement on those inputs and against the numpy restatement on the tests' scene
list, and records the measured residuals of rule T2. Nothing is gated.

    python tools/twoview_bench.py --json runs.json          on the GPU: measure and keep the numbers
    python tools/twoview_bench.py --from-json runs.json     anywhere: write the two files from numbers measured earlier"""
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

import twoview_ref as R  # noqa: E402
import twoview_scene as S  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
N_KP, ITERATIONS, BATCHES = 1112, 200, (1, 8, 64)
STAGES = ("hypotheses", "scores", "selection", "motion hypotheses", "CheckRT", "k-th cosine", "acceptance")
KERNELS = ("tv_hyp_kernel", "tv_score_kernel", "tv_select_kernel", "tv_motion_kernel", "tv_checkrt_kernel", "tv_kth_kernel", "tv_accept_kernel")


def batch(B):
    return [S.with_sets(S.make_pair(100 + b, n=N_KP), ITERATIONS, 500 + b) for b in range(B)]


def lib_pairs(tv, pairs):
    return [tv.pair(p["xy1"], p["xy2"], p["matches12"], p["K"], p["sets"]) for p in pairs]


def result_bytes(r, b, stages):
    d = r.read(b)
    out = [np.asarray(d[k]).tobytes() for k in sorted(d)] + [a.tobytes() for a in r.matches(b) + r.points(b)]
    if stages:
        out += [a.tobytes() for a in r.iterations_of(b).values()]
        for h in range(8):
            out += [np.asarray(v).tobytes() for v in r.hypothesis(b, h).values()]
    return b"".join(out)


def measure(reps):
    tv = importlib.import_module(PKG + ".twoview")
    rows = []
    for B in BATCHES:
        pairs = batch(B)
        lp = lib_pairs(tv, pairs)
        for _ in range(2):
            tv.init(lp, iterations=ITERATIONS).close()             # warm-up: code objects, first allocations
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter(); r = tv.init(lp, iterations=ITERATIONS); wall.append((time.perf_counter() - t0) * 1e3); r.close()
        os.environ["IBA_TWOVIEW_TIMING"] = "1"
        stage = []
        for _ in range(reps):
            r = tv.init(lp, iterations=ITERATIONS)
            stage.append([float(v) for v in r.stage_ms])
            status = [r.read(b)["status"] for b in range(B)]
            r.close()
        del os.environ["IBA_TWOVIEW_TIMING"]
        host = []
        for _ in range(3 if B < 64 else 1):
            t0 = time.perf_counter(); h = tv.init_host(lp, iterations=ITERATIONS); host.append((time.perf_counter() - t0) * 1e3); h.close()
        d, h = tv.init(lp, iterations=ITERATIONS, keep_stages=1), tv.init_host(lp, iterations=ITERATIONS, keep_stages=1)
        diff = 0
        for b in range(B):
            x, y = np.frombuffer(result_bytes(d, b, True), np.uint8), np.frombuffer(result_bytes(h, b, True), np.uint8)
            diff += int((x != y).sum()) if len(x) == len(y) else -1
        nbytes = sum(len(result_bytes(d, b, True)) for b in range(B))
        hits = d.sweep_cap_hits
        d.close(); h.close()
        rows.append(dict(B=B, reps=reps, matches=[S.n_matches(p) for p in pairs][:8], wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)), wall_max_ms=max(wall),
                         stage_ms={s: float(v) for s, v in zip(STAGES, np.median(np.array(stage), axis=0))}, host_median_ms=float(np.median(host)), host_runs=len(host),
                         statuses={tv.STATUS_NAMES[s]: status.count(s) for s in sorted(set(status))}, differing_bytes_vs_host=diff, compared_bytes=nbytes, sweep_cap_hits=hits))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def parity():
    """the device against the numpy restatement on the tests' scene list, and T2's measured residuals on its design matrices"""
    tv = importlib.import_module(PKG + ".twoview")
    pairs, refs = S.scene_pairs(), S.scene_reference()
    r = tv.init(lib_pairs(tv, pairs), iterations=S.ITERATIONS, keep_stages=1)
    scenes = []
    for b, ((name, _, _, _), e) in enumerate(zip(S.SCENES, refs)):
        diffs = S.differences(r, b, e)
        ulp = int(S.ulp_apart(r.read(b)["parallax_deg"], e["parallax_deg"]).max())
        scenes.append(dict(scene=name, status=tv.STATUS_NAMES[e["status"]], N=int(e["n_matches"]), differing=diffs, parallax_ulp=ulp, compared_bytes=len(result_bytes(r, b, True))))
    hits = r.sweep_cap_hits
    r.close()
    eps, worst, worst_norm, n, cap = 2.0 ** -52, {}, 0.0, 0, 0
    for (name, _, _, _), p in zip(S.SCENES, pairs):
        if p["sets"] is None or name == "no_model":
            continue
        lst = np.nonzero(p["matches12"] >= 0)[0]
        mn = np.concatenate([R.normalize(p["xy1"])[0][lst], R.normalize(p["xy2"])[0][p["matches12"][lst]]], 1)
        for A in list(R.design_h(mn[p["sets"]])) + list(R.design_f(mn[p["sets"]])):
            v, v64, sw = tv.null_vector(A)
            sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
            smin = sv[-1] if A.shape[0] >= A.shape[1] else 0.0
            key = "%d x %d" % A.shape
            worst[key] = max(worst.get(key, 0.0), abs(np.linalg.norm(A.astype(np.float64) @ v64) - smin) / sv[0] / eps)
            worst_norm = max(worst_norm, abs(np.linalg.norm(v64) - 1.0) / eps)
            n += 1
            cap += sw == R.MAX_SWEEPS
    out = dict(scenes=scenes, sweep_cap_hits=hits, t2=dict(matrices=n, worst_residual_eps=worst, worst_norm_eps=worst_norm, cap_hits=int(cap)))
    print(json.dumps(out), flush=True)
    return out


def resources():
    """VGPRs, SGPRs, LDS and scratch per kernel from hipcc's resource report of csrc/iba_twoview.hip; None without a compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, PKG, "csrc", "iba_twoview.hip")
    try:
        p = subprocess.run([hipcc, "-std=c++17", "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-o", os.devnull, src],
                           capture_output=True, text=True, timeout=900)
    except (OSError, subprocess.TimeoutExpired):
        return None
    rows, cur = [], None
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(Function Name|TotalSGPRs|VGPRs|ScratchSize \[bytes/lane\]|Occupancy \[waves/SIMD\]|LDS Size \[bytes/block\]):\s+(\S+)", line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = {"kernel": next((k for k in KERNELS if k in m.group(2)), m.group(2))}
            rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows or None


def write_bench(rows, out):
    with open(out, "w") as fh:
        fh.write("# Two-view initialisation on the device: what the first run saw\n\n")
        if not rows:
            fh.write("No GPU run was made: this file holds no measured time.\n\n")
        else:
            fh.write("`python tools/twoview_bench.py` on one MI355X. Seeded pairs of %d keypoints (a pinhole camera 700 / 700 / 620 / 188, depths 6-20 m, a 1 m baseline, 0.3 px of noise, a fifth\n"
                     "of the matches random, a tenth of frame 1 unmatched: about 1000 matches a pair), %d iterations, B pairs a call. `wall`: the whole iba_twoview_init from Python - checks,\n"
                     "T1, the match lists, allocations, the tables up, the launch chain, the results down, acos and the scatter of the points - after two warm-up calls. `host`: iba_debug_twoview_host on\n"
                     "the same inputs on the same machine, one thread (the restatement is single-threaded; the machine's 16-CPU limit does not enter). Kernel times are the\n"
                     "median over a second set of calls with IBA_TWOVIEW_TIMING (HIP events around the kernels). No target is set and nothing is gated.\n\n" % (N_KP, ITERATIONS))
            fh.write("| B | wall ms (min / median / max) | pairs / s (median) | host ms (median of n) | host / device | statuses |\n|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %d | %.2f / %.2f / %.2f | %.0f | %.1f (%d) | %.1f | %s |\n" % (r["B"], r["wall_min_ms"], r["wall_median_ms"], r["wall_max_ms"], 1e3 * r["B"] / r["wall_median_ms"],
                                                                                     r["host_median_ms"], r["host_runs"], r["host_median_ms"] / r["wall_median_ms"],
                                                                                     ", ".join("%s %d" % kv for kv in r["statuses"].items())))
            fh.write("\n| kernel | " + " | ".join("B = %d ms" % r["B"] for r in rows) + " |\n|---|" + "---|" * len(rows) + "\n")
            for s in STAGES:
                fh.write("| %s | " % s + " | ".join("%.3f" % r["stage_ms"][s] for r in rows) + " |\n")
            fh.write("| sum | " + " | ".join("%.3f" % sum(r["stage_ms"].values()) for r in rows) + " |\n")
            fh.write("\nThe rest of the wall time is the host around the chain: the checks, T1 over every keypoint, the tables, the allocations and the copies.\n")
        fh.write("\n## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)\n\n")
        res = resources()
        if res:
            fh.write("| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k in res:
                fh.write("| %s | %d | %d | %d | %d | %d |\n" % (k["kernel"], k.get("VGPRs", -1), k.get("TotalSGPRs", -1), k.get("LDS Size", -1), k.get("ScratchSize", -1), k.get("Occupancy", -1)))
            fh.write("\nThe hypothesis kernel's LDS is rule T2's work matrices, 225 doubles for each of the 32 lanes of a block in a lane-minor slab; its registers are the\n"
                     "3 x 3 solves and products that follow. The motion kernel's scratch is its 8 x 9 and 8 x 3 result arrays; it runs one lane per pair.\n")
        else:
            fh.write("No compiler was found where this file was written.\n")
    print(open(out).read())


def write_parity(rows, par, out):
    with open(out, "w") as fh:
        fh.write("# Two-view initialisation: parity of the device, and rule T2's residuals\n\n")
        if not par:
            fh.write("No GPU run was made: this file holds no measured figure.\n")
            return
        fh.write("`python tools/twoview_bench.py` on one MI355X.\n\n## The device against tests/twoview_ref.py on the tests' scene list (one call, %d iterations, keep_stages)\n\n" % S.ITERATIONS)
        fh.write("Every field of the result, the match list, the inlier flags, points, triangulated, and every kept stage (Hi, H12i, Fi, both scores, per motion hypothesis R, t,\n"
                 "n_good, points, verdicts), as bytes. parallax_deg is counted apart, in float32 ulps: both sides call a libm acos.\n\n")
        fh.write("| scene | status | N | bytes compared | differing | parallax_deg, worst ulp |\n|---|---|---|---|---|---|\n")
        for s in par["scenes"]:
            fh.write("| %s | %s | %d | %d | %s | %d |\n" % (s["scene"], s["status"], s["N"], s["compared_bytes"], sum(n for _, n in s["differing"]) if s["differing"] else 0, s["parallax_ulp"]))
        by_scene = {name: int(e["sweep_cap_hits"]) for (name, _, _, _), e in zip(S.SCENES, S.scene_reference())}
        fh.write("\nNull-vector solves of that call whose 30th sweep still rotated (the debug counter): %d on the device; the reference counts %d, %d of them in the scene\n"
                 "whose T1 is not finite, where every hypothesis is NaN and no test of T2 can hold.\n" % (par["sweep_cap_hits"], sum(by_scene.values()), by_scene["no_model"]))
        if rows:
            fh.write("\n## The device against the host restatement on the benchmark's pairs (%d iterations, keep_stages)\n\n| B | bytes compared | differing | sweep-cap hits |\n|---|---|---|---|\n" % ITERATIONS)
            for r in rows:
                fh.write("| %d | %d | %d | %d |\n" % (r["B"], r["compared_bytes"], r["differing_bytes_vs_host"], r["sweep_cap_hits"]))
            fh.write("\nHere parallax_deg is among the bytes: one libm on one machine. A sweep-cap hit is a solve that had converged and idled: T2's relative threshold sits at the\n"
                     "rounding level of gamma itself; the answer is the converged one.\n")
        t2 = par["t2"]
        fh.write("\n## Rule T2 against numpy.linalg.svd in float64\n\nOn the %d design matrices of the scene list (every set of every scene with finite coordinates), the float64 vector the\n"
                 "float32 answer is rounded from (iba_debug_twoview_null_vector): |norm(A v) - sigma_min| / sigma_max in units of 2^-52, bound 256; sigma_min of an 8 x 9 matrix is 0.\n\n"
                 "| size | worst residual / 2^-52 |\n|---|---|\n" % t2["matrices"])
        for k, v in sorted(t2["worst_residual_eps"].items()):
            fh.write("| %s | %.2f |\n" % (k, v))
        fh.write("\nWorst | norm(v) - 1 | / 2^-52: %.2f. Solves that reached the sweep cap: %d.\n" % (t2["worst_norm_eps"], t2["cap_hits"]))
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "twoview_bench.md"))
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "twoview_parity.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None, help="keep the measured numbers here")
    ap.add_argument("--from-json", default=None, help="format numbers measured earlier instead of measuring")
    ap.add_argument("--measure-only", action="store_true", help="measure and keep the numbers (--json); write neither file")
    a = ap.parse_args()
    if a.from_json:
        data = json.load(open(a.from_json))
    else:
        data = {"parity": parity(), "rows": measure(a.reps)}
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(data, open(a.json, "w"), indent=1)
    if a.measure_only:
        return
    write_bench(data["rows"], a.out)
    write_parity(data["rows"], data["parity"], a.parity_out)


if __name__ == "__main__":
    main()

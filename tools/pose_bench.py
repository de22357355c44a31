"""Times iba_pose_optimize on one device and writes profiles/pose_bench.md: B = 1, 64 and 1024 jobs of 300 edges and one job of 4096 edges; the wall
time of whole calls after two warm-ups, the kernel time from HIP events (IBA_POSE_TIMING), and iba_debug_pose_host on one thread beside it. No target
is set and nothing is gated.   python tools/pose_bench.py [--device 0] [--calls 7] [--out profiles/pose_bench.md]"""
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
CASES = (("B = 1, 300 edges", 1, 300), ("B = 64, 300 edges", 64, 300), ("B = 1024, 300 edges", 1024, 300), ("B = 1, 4096 edges", 1, 4096))


def resources():
    """VGPRs, LDS, scratch and occupancy of the two kernels from the compiler's report"""
    csrc = os.path.join(ROOT, PKG, "csrc")
    r = subprocess.run(["make", "-C", csrc, "-s", "-B", "asm-pose"], capture_output=True, text=True)
    rows, cur = [], None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"name": "pose_optimize_kernel" if "optimize" in m.group(1) else "pose_eval_kernel"}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_bench.md"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's first)
    except Exception:
        pass
    importlib.import_module(PKG)
    ps = importlib.import_module(PKG + ".pose")
    S = importlib.import_module("pose_scene")
    os.environ["IBA_DEBUG_ENV"] = "1"
    lines = ["# Pose optimisation on the device: what the first run saw", "",
             "`python tools/pose_bench.py` on one MI355X. Seeded scenes (tests/pose_scene.py: one pixel of noise scaled by the level, a fifth of the observations gross",
             "outliers, a start pose 0.02 rad and 0.15 m off), default options (4 rounds of up to 10 iterations). `wall`: the whole iba_pose_optimize from Python - checks,",
             "staging, allocations, the edges up, ONE kernel, the results down - after two warm-up calls, %d calls. `kernel`: HIP events around the kernel" % a.calls,
             "(IBA_POSE_TIMING), median of a second set of calls. `host`: iba_debug_pose_host on the same jobs, one thread. No target is set and nothing is gated.", "",
             "| case | wall ms (min / median / max) | kernel ms (median) | jobs / s (wall median) | host ms | host / wall | LM iterations + trials per job (mean) |", "|---|---|---|---|---|---|---|"]
    for name, B, n in CASES:
        scs = [S.make(n, 1000 + k, outliers=0.2) for k in range(min(B, 64))]
        jobs = [ps.job(sc["T_start"], sc["xyz"], sc["obs"], sc["inv_sigma2"], sc["K"]) for sc in scs]
        jobs = [jobs[k % len(jobs)] for k in range(B)]
        os.environ.pop("IBA_POSE_TIMING", None)
        for _ in range(2):
            ps.optimize(jobs, device=a.device).close()
        wall = []
        for _ in range(a.calls):
            t = time.perf_counter()
            r = ps.optimize(jobs, device=a.device)
            wall.append(1e3 * (time.perf_counter() - t))
            r.close()
        os.environ["IBA_POSE_TIMING"] = "1"
        kern, work = [], 0.0
        for _ in range(a.calls):
            r = ps.optimize(jobs, device=a.device)
            kern.append(r.kernel_ms)
            work = float(np.mean([r.read(j)["lm_iterations"].sum() + r.read(j)["trials"].sum() for j in range(min(B, 64))]))
            r.close()
        t = time.perf_counter()
        ps.optimize_host(jobs).close()
        host = 1e3 * (time.perf_counter() - t)
        lines.append("| %s | %.3f / %.3f / %.3f | %.3f | %.0f | %.1f | %.1f | %.1f |" % (name, min(wall), np.median(wall), max(wall), np.median(kern), B / np.median(wall) * 1e3, host, host / np.median(wall), work))
        print(lines[-1], flush=True)
    lines += ["", "## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)", "", "| kernel | VGPRs | AGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |", "|---|---|---|---|---|---|---|"]
    for k in resources():
        lines.append("| %s | %s | %s | %s | %s | %s | %s |" % tuple(k.get(f, "?") for f in ("name", "vgpr", "agpr", "sgpr", "lds", "scratch", "occ")))
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()

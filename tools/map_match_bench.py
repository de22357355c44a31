#!/usr/bin/env python3
"""Times the local-map point matching (iba_map_match) on one GPU and writes profiles/map_match_bench.md: a seeded map of 2000 points seen by frames of
2000 keypoints, as calls of 1, 64 and 1024 jobs of 2000 points each; per stage the time from HIP events (IBA_MAP_MATCH_TIMING), the wall time of whole
calls, the same calls through iba_debug_map_match_host on one thread, and the registers and LDS of the two new kernels from the compiler's resource
report. Nothing is gated and no figure is promised.

    python tools/map_match_bench.py --measure-only --json runs.json     on the GPU: measure and keep the numbers
    python tools/map_match_bench.py --from-json runs.json               anywhere with a compiler: write the file from numbers measured earlier
    python tools/map_match_bench.py                                     on the GPU: both"""
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
os.environ.setdefault("IBA_DEBUG_ENV", "1")
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
N_POINTS, N_KP, N_FRAMES, SEED = 2000, 2000, 8, 17
JOB_COUNTS = (1, 64, 1024)
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
K = (718.0, 718.0, 607.0, 185.0)
STAGES = ("frustum", "grid (cell, scan, fill) + list count", "scan + list write with distances", "resolve")
KERNELS = ("mapm_frustum_kernel", "mapm_resolve_kernel")


def scene():
    """one table of N_POINTS points, N_FRAMES frames whose keypoints are noisy projections of most of the points (descriptors a few bits off) plus
    clutter, and a pose per frame"""
    rng = np.random.default_rng(SEED)
    xyz = np.stack([rng.uniform(-12, 12, N_POINTS), rng.uniform(-3, 3, N_POINTS), rng.uniform(3, 30, N_POINTS)], 1)
    d0 = np.linalg.norm(xyz, axis=1)
    desc = rng.integers(0, 256, (N_POINTS, 32)).astype(np.uint8)
    table = dict(xyz=xyz, normal=xyz / d0[:, None], min_dist=d0 / 3, max_dist=d0 * rng.uniform(1.0, 3.5, N_POINTS), desc=desc)
    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])).astype(np.float32)
    frames, poses = [], []
    for f in range(N_FRAMES):
        T = np.eye(3, 4)
        T[:, 3] = (0.05 * f, 0.0, 0.1 * f)
        pc = xyz + T[:, 3]
        uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
        ok = np.flatnonzero((uv[:, 0] > 2) & (uv[:, 0] < BOUNDS[1] - 2) & (uv[:, 1] > 2) & (uv[:, 1] < BOUNDS[3] - 2))
        pick = ok[:int(0.8 * N_KP)]
        level = np.clip(np.ceil(np.log(table["max_dist"][pick] / np.linalg.norm(pc[pick], axis=1)) / np.log(1.2)), 0, 7).astype(np.int32)
        flips = np.unpackbits(desc[pick], axis=1) ^ (rng.uniform(size=(len(pick), 256)) < 0.08)
        n_extra = N_KP - len(pick)
        xy = np.concatenate([uv[pick] + rng.normal(0, 1.0, (len(pick), 2)), np.stack([rng.uniform(0, BOUNDS[1], n_extra), rng.uniform(0, BOUNDS[3], n_extra)], 1)])
        frames.append(dict(xy=xy, octave=np.concatenate([level, rng.integers(0, 8, n_extra).astype(np.int32)]), angle=np.zeros(N_KP),
                           desc=np.concatenate([np.packbits(flips.astype(np.uint8), axis=1), rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])))
        poses.append(T)
    return table, frames, poses, sf


def measure(reps):
    mm = importlib.import_module(PKG + ".map_match")
    om = importlib.import_module(PKG + ".orb_match")
    table, frames, poses, sf = scene()
    lf = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], BOUNDS) for f in frames]
    lt = mm.points(table["xyz"], table["normal"], table["min_dist"], table["max_dist"], table["desc"])
    rows = []
    for J in JOB_COUNTS:
        lj = [mm.job(j % N_FRAMES, poses[j % N_FRAMES], K, sf, 1.0, N_POINTS) for j in range(J)]
        for _ in range(2):
            mm.match(lf, lt, lj).close()                       # warm-up: code objects, first allocations
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter(); m = mm.match(lf, lt, lj); wall.append((time.perf_counter() - t0) * 1e3); m.close()
        os.environ["IBA_MAP_MATCH_TIMING"] = "1"
        stage = []
        for _ in range(reps):
            m = mm.match(lf, lt, lj)
            stage.append([float(v) for v in m.stage_ms])
            counts = [m.counts(j) for j in range(J)]
            chunks = m.n_chunks
            m.close()
        del os.environ["IBA_MAP_MATCH_TIMING"]
        host = []
        for _ in range(1 if J > 64 else 3):
            t0 = time.perf_counter(); m = mm.match_host(lf, lt, lj); host.append((time.perf_counter() - t0) * 1e3)
            same = all(m.counts(j)["n_matches"] == counts[j]["n_matches"] and m.counts(j)["n_candidates"] == counts[j]["n_candidates"] for j in range(J))
            m.close()
        ms = np.median(np.array(stage), axis=0)
        rows.append(dict(n_jobs=J, chunks=chunks, reps=reps, wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)), host_min_ms=min(host), host_agrees=bool(same),
                         stage_ms={s: float(v) for s, v in zip(STAGES, ms)}, points=sum(c["n_points"] for c in counts), in_view=int(sum(c["status"][0] for c in counts)),
                         candidates=sum(c["n_candidates"] for c in counts), matches=sum(c["n_matches"] for c in counts)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def resources():
    """VGPRs, SGPRs, LDS and scratch of the two new kernels from hipcc's resource report of csrc/iba_map_match.hip; None without a compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, PKG, "csrc", "iba_map_match.hip")
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
            name = next((k for k in KERNELS if k in m.group(2)), None)
            cur = {"kernel": name} if name else None
            if cur:
                rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows or None


def write(rows, out):
    with open(out, "w") as fh:
        fh.write("# Local-map point matching on the device: what the first run saw\n\n")
        if not rows:
            fh.write("No GPU run was made: this file holds no measured time.\n\n")
        else:
            fh.write("`python tools/map_match_bench.py` on one MI355X. A seeded table of %d map points and %d frames of %d keypoints in %d x %d bounds (four fifths of a frame's\n"
                     "keypoints are projections of points with a pixel of noise and about 20 flipped descriptor bits, the rest clutter); a job lists all %d points against one\n"
                     "frame under that frame's pose, th = 1; jobs cycle over the frames. `wall`: the whole iba_map_match from Python - checks, flat tables, allocations, frames,\n"
                     "table and slots up, the launch chain, the results down - after two warm-up calls. Stage times are the median over a second set of calls with\n"
                     "IBA_MAP_MATCH_TIMING (HIP events around the kernels). `host`: iba_debug_map_match_host, the same call on one CPU thread of the GPU machine, least of its\n"
                     "runs. No target is set and nothing is gated.\n\n" % (N_POINTS, N_FRAMES, N_KP, int(BOUNDS[1]), int(BOUNDS[3]), N_POINTS))
            fh.write("| jobs | chunks | wall ms (min / median) | jobs / s (median) | host ms | host / wall | points | in view | candidates | matches | host agrees |\n|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %d | %d | %.2f / %.2f | %.0f | %.1f | %.1f | %d | %d | %d | %d | %s |\n" % (
                    r["n_jobs"], r["chunks"], r["wall_min_ms"], r["wall_median_ms"], 1e3 * r["n_jobs"] / r["wall_median_ms"], r["host_min_ms"], r["host_min_ms"] / r["wall_median_ms"],
                    r["points"], r["in_view"], r["candidates"], r["matches"], "yes" if r["host_agrees"] else "NO"))
            for r in rows:
                fh.write("\n## %d jobs\n\n| stage | ms |\n|---|---|\n" % r["n_jobs"])
                for s in STAGES:
                    fh.write("| %s | %.3f |\n" % (s, r["stage_ms"][s]))
                fh.write("\nThe stages sum to %.2f ms of the median wall time %.2f ms; the rest is the host around the chain and the copies.\n" % (sum(r["stage_ms"].values()), r["wall_median_ms"]))
            fh.write("\nThe resolve is one wave per job and sequential over the job's points by the rule's definition: its time is that of the longest job, not of the sum, and a\n"
                     "call of few jobs uses few compute units.\n")
        fh.write("\n## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)\n\n")
        res = resources()
        if res:
            fh.write("| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k in res:
                fh.write("| %s | %d | %d | %d | %d | %d |\n" % (k["kernel"], k.get("VGPRs", -1), k.get("TotalSGPRs", -1), k.get("LDS Size", -1), k.get("ScratchSize", -1), k.get("Occupancy", -1)))
            fh.write("\nThe resolve kernel's LDS is the claimed bitmap of %d keypoints; a block is one wave. The frustum kernel's is its seven status counters.\n" % 32768)
        else:
            fh.write("No compiler was found where this file was written.\n")
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "map_match_bench.md"))
    ap.add_argument("--reps", type=int, default=7)
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

#!/usr/bin/env python3
"""Times the new-map-point creation (iba_triangulate) on one GPU and writes profiles/triangulate_bench.md: a seeded cloud seen by keyframes of 2000
keypoints along a trajectory, one call of 64 jobs of 20 neighbours each; the wall time of whole calls, per stage the time from HIP events
(IBA_TRIANGULATE_TIMING) for the pick kernel at 8, 16 and 64 lanes per query (IBA_TRIANGULATE_PICK_LANES), the same call through
iba_debug_triangulate_host on one thread, and the registers, LDS, scratch and occupancy of the kernels from the compiler's resource report. Nothing
is gated and no figure is promised.

    python tools/triangulate_bench.py --measure-only --json runs.json     on the GPU: measure and keep the numbers
    python tools/triangulate_bench.py --from-json runs.json               anywhere with a compiler: write the file from numbers measured earlier
    python tools/triangulate_bench.py                                     on the GPU: both"""
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
N_JOBS, N_NEIGHBOURS, N_KP, N_POINTS, N_NODES, SEED = 64, 20, 2000, 9000, 100, 23
BOUNDS = (0.0, 1241.0, 0.0, 376.0)
K = (718.0, 718.0, 607.0, 185.0)
WIDTHS = (8, 16, 64)
STAGES = ("prologue + segments", "pick", "compaction + triangulation", "resolve + counts + scan + gather")
KERNELS = ("trg_prologue_kernel", "trg_segment_kernel", "trg_pick_kernelILi8E", "trg_pick_kernelILi16E", "trg_pick_kernelILi64E", "trg_compact_kernel", "trg_triangulate_kernel",
           "trg_resolve_kernel", "trg_count_kernel", "trg_gather_kernel")


def scene():
    """N_JOBS + N_NEIGHBOURS keyframes advancing along x over one cloud; a keyframe's keypoints are noisy projections of the points it sees (descriptors
    about 20 bits off), a point's node is its index modulo N_NODES (about 20 keypoints per node), two fifths of the keypoints have a point already"""
    rng = np.random.default_rng(SEED)
    n_kf = N_JOBS + N_NEIGHBOURS
    xyz = np.stack([rng.uniform(-14, 14 + 0.15 * n_kf, N_POINTS), rng.uniform(-3, 3, N_POINTS), rng.uniform(4, 30, N_POINTS)], 1)
    desc = rng.integers(0, 256, (N_POINTS, 32)).astype(np.uint8)
    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])).astype(np.float32)
    frames, kfs = [], []
    for f in range(n_kf):
        T = np.eye(3, 4)
        T[:, 3] = (-0.15 * f, 0.0, 0.0)
        pc = xyz + T[:, 3]
        uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
        ok = np.flatnonzero((uv[:, 0] > 2) & (uv[:, 0] < BOUNDS[1] - 2) & (uv[:, 1] > 2) & (uv[:, 1] < BOUNDS[3] - 2))
        pick = rng.permutation(ok)[:N_KP]
        assert len(pick) == N_KP, len(ok)
        octave = np.clip(np.round(np.log(pc[pick, 2] / 4.0) / np.log(1.2)), 0, 7).astype(np.int32)
        flips = np.unpackbits(desc[pick], axis=1) ^ (rng.uniform(size=(N_KP, 256)) < 0.08)
        frames.append(dict(xy=uv[pick] + rng.normal(0, 0.7, (N_KP, 2)), octave=octave, angle=np.zeros(N_KP), desc=np.packbits(flips.astype(np.uint8), axis=1)))
        kfs.append(dict(Tcw=T, node=(pick % N_NODES).astype(np.int32), has_point=(rng.uniform(size=N_KP) < 0.4).astype(np.uint8), median_depth=float(np.median(pc[pick, 2]))))
    jobs = [dict(current=N_NEIGHBOURS + j, neighbours=[N_NEIGHBOURS + j - 1 - i for i in range(N_NEIGHBOURS)]) for j in range(N_JOBS)]
    return frames, kfs, jobs, sf


def measure(reps):
    tr = importlib.import_module(PKG + ".triangulate")
    om = importlib.import_module(PKG + ".orb_match")
    frames, kfs, jobs, sf = scene()
    lf = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], BOUNDS) for f in frames]
    lk = [tr.keyframe(i, k["Tcw"], K, k["node"], k["has_point"], k["median_depth"]) for i, k in enumerate(kfs)]
    lj = [tr.job(j["current"], j["neighbours"], sf, sf * sf, 1.2) for j in jobs]
    for _ in range(2):
        tr.triangulate(lf, lk, lj).close()                     # warm-up: code objects, first allocations
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); t = tr.triangulate(lf, lk, lj); wall.append((time.perf_counter() - t0) * 1e3); t.close()
    os.environ["IBA_TRIANGULATE_TIMING"] = "1"
    by_width, counts, chunks = {}, None, 0
    for w in WIDTHS:
        os.environ["IBA_TRIANGULATE_PICK_LANES"] = str(w)
        tr.triangulate(lf, lk, lj).close()
        stage = []
        for _ in range(reps):
            t = tr.triangulate(lf, lk, lj)
            stage.append([float(v) for v in t.stage_ms])
            got = [t.counts(j) for j in range(len(lj))]
            chunks = t.n_chunks
            t.close()
        assert counts is None or all(np.array_equal(a["status"], b["status"]) and np.array_equal(a["n_matches"], b["n_matches"]) for a, b in zip(counts, got))
        counts = got
        by_width[str(w)] = {s: float(v) for s, v in zip(STAGES, np.median(np.array(stage), axis=0))}
    del os.environ["IBA_TRIANGULATE_TIMING"], os.environ["IBA_TRIANGULATE_PICK_LANES"]
    t0 = time.perf_counter(); h = tr.triangulate_host(lf, lk, lj); host_ms = (time.perf_counter() - t0) * 1e3
    same = all(np.array_equal(h.counts(j)["status"], counts[j]["status"]) and np.array_equal(h.counts(j)["n_matches"], counts[j]["n_matches"]) for j in range(len(lj)))
    h.close()
    status = np.sum([c["status"] for c in counts], axis=0)
    row = dict(n_jobs=N_JOBS, chunks=chunks, reps=reps, wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)), host_ms=host_ms, host_agrees=bool(same), stage_ms=by_width,
               slots=int(status.sum()), status=[int(v) for v in status], matches=int(sum(c["n_matches"].sum() for c in counts)), created=int(sum(c["n_created"] for c in counts)))
    print(json.dumps(row), flush=True)
    return [row]


def resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the unit's kernels from hipcc's resource report of csrc/iba_triangulate.hip; None without a compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, PKG, "csrc", "iba_triangulate.hip")
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
            cur = {"kernel": name.replace("ILi", "<").replace("E", ">") if name and "ILi" in name else name} if name else None
            if cur:
                rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return rows or None


def write(rows, out):
    names = ("CREATED", "HAS_POINT", "NO_NODE", "PAIR_SKIPPED", "NO_MATCH", "PARALLAX", "DEGENERATE", "DEPTH1", "DEPTH2", "REPROJ1", "REPROJ2", "ZERO_DIST", "SCALE", "SUPERSEDED")
    with open(out, "w") as fh:
        fh.write("# New-map-point creation on the device: what the first run saw\n\n")
        if not rows:
            fh.write("No GPU run was made: this file holds no measured time.\n\n")
        else:
            r = rows[0]
            fh.write("`python tools/triangulate_bench.py` on one MI355X. %d keyframes of %d keypoints advance along x over a seeded cloud of %d points (0.7 pixel of noise, about 20\n"
                     "flipped descriptor bits, a point's node is its index modulo %d: about %d keypoints per node, two fifths of the keypoints have a point already); one call of %d\n"
                     "jobs, each a keyframe against the %d before it: %d slots. `wall`: the whole iba_triangulate from Python - checks, node order, flat tables, allocations,\n"
                     "uploads, the launch chain, the results down - after two warm-up calls, at the shipped pick width. Stage times are the median over further calls with\n"
                     "IBA_TRIANGULATE_TIMING (HIP events around the kernels), once per pick width. `host`: iba_debug_triangulate_host, the same call on one CPU thread of the GPU\n"
                     "machine, one run. No target is set and nothing is gated: these are the first figures for this workload.\n\n"
                     % (N_JOBS + N_NEIGHBOURS, N_KP, N_POINTS, N_NODES, N_KP // N_NODES, N_JOBS, N_NEIGHBOURS, r["slots"]))
            fh.write("| jobs | chunks | wall ms (min / median) | host ms | host / wall | slots | matches | created | host agrees |\n|---|---|---|---|---|---|---|---|---|\n")
            fh.write("| %d | %d | %.2f / %.2f | %.1f | %.1f | %d | %d | %d | %s |\n" % (r["n_jobs"], r["chunks"], r["wall_min_ms"], r["wall_median_ms"], r["host_ms"],
                                                                                    r["host_ms"] / r["wall_median_ms"], r["slots"], r["matches"], r["created"], "yes" if r["host_agrees"] else "NO"))
            fh.write("\nSlots per status: " + ", ".join("%s %d" % (n, v) for n, v in zip(names, r["status"]) if v) + ".\n")
            fh.write("\n## Stages, per pick width (ms, median of %d calls)\n\n| stage | %s |\n|---|%s\n" % (r["reps"], " | ".join("%d lanes" % w for w in WIDTHS), "---|" * len(WIDTHS)))
            for s in STAGES:
                fh.write("| %s | %s |\n" % (s, " | ".join("%.3f" % r["stage_ms"][str(w)][s] for w in WIDTHS)))
            fh.write("| sum | %s |\n" % " | ".join("%.3f" % sum(r["stage_ms"][str(w)].values()) for w in WIDTHS))
            fh.write("\nThe stages sum to about %.1f ms of the median wall time %.2f ms; the rest is the host around the chain - the checks, the node order, the flat tables, the\n"
                     "allocations - and the copies, above all the 21 bytes of every slot (status, match, distance, point) that come down: %.0f MB here.\n"
                     % (min(sum(v.values()) for v in r["stage_ms"].values()), r["wall_median_ms"], 21e-6 * r["slots"]))
            best = min(WIDTHS, key=lambda w: r["stage_ms"][str(w)]["pick"])
            fh.write("\nThe pick is fastest at %d lanes per query on this scene; the bytes are the same for all three (tests/test_gpu_triangulate.py runs all three).\n" % best)
        fh.write("\n## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950)\n\n")
        res = resources()
        if res:
            fh.write("| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k in res:
                fh.write("| %s | %d | %d | %d | %d | %d |\n" % (k["kernel"], k.get("VGPRs", -1), k.get("TotalSGPRs", -1), k.get("LDS Size", -1), k.get("ScratchSize", -1), k.get("Occupancy", -1)))
            fh.write("\nNo kernel spills: the two 4 x 4 float64 arrays of the Jacobi in the triangulate kernel stay in registers (its loops are unrolled, as in tv_checkrt_kernel),\n"
                     "which is what its register count pays for.\n")
        else:
            fh.write("No compiler was found where this file was written.\n")
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangulate_bench.md"))
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

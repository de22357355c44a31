#!/usr/bin/env python3
"""Times the map-point refresh (iba_refresh) on one GPU and writes profiles/refresh_bench.md: a seeded scene shaped like a local map - of the order
of 2 x 10^5 points whose observation counts are mostly under 10 with a tail into the hundreds; the wall time of whole calls, per launch the time
from HIP events (IBA_REFRESH_TIMING) for every narrow width (IBA_REFRESH_NARROW_LANES) and both median forms (IBA_REFRESH_MEDIAN), interleaved, the
same call through iba_debug_refresh_host on one thread, and the registers, LDS, scratch and occupancy of the kernel's shapes from the compiler's
resource report. Nothing is gated and no figure is promised.

    python tools/refresh_bench.py --measure-only --json runs.json     on the GPU: measure and keep the numbers
    python tools/refresh_bench.py --from-json runs.json               anywhere with a compiler: write the file from numbers measured earlier
    python tools/refresh_bench.py                                     on the GPU: both"""
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
N_POINTS, N_KEYFRAMES, N_KP, SEED = 200000, 1009, 2000, 37          # 1009 is prime: start + j * stride (mod 1009) names distinct keyframes
WIDTHS, FORMS = (4, 8, 16, 32), (0, 1)
FORM_NAME = {0: "search", 1: "kept row"}
STAGES = ("narrow", "wave", "block")


def scene(n_points=N_POINTS):
    rng = np.random.default_rng(SEED)
    counts = 1 + rng.geometric(0.28, n_points)                                       # most points: a handful of observations
    tail = rng.uniform(size=n_points) < 0.02
    counts[tail] = np.minimum(np.exp(rng.normal(4.2, 0.9, int(tail.sum()))).astype(np.int64) + 10, 1000)      # a tail into the hundreds
    counts[rng.uniform(size=n_points) < 0.002] = 0
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    owner = np.repeat(np.arange(n_points), counts)
    j = np.arange(off[-1]) - off[:-1][owner]
    start, stride = rng.integers(0, N_KEYFRAMES, n_points), rng.integers(1, N_KEYFRAMES, n_points)
    obs_kf = ((start[owner] + j * stride[owner]) % N_KEYFRAMES).astype(np.int32)
    obs_kp = rng.integers(0, N_KP, len(obs_kf)).astype(np.int32)
    frames = [dict(xy=np.zeros((N_KP, 2), np.float32), octave=rng.integers(0, 8, N_KP).astype(np.int32), angle=np.zeros(N_KP, np.float32),
                   desc=rng.integers(0, 256, (N_KP, 32), dtype=np.uint8)) for _ in range(N_KEYFRAMES)]
    poses = []
    for k in range(N_KEYFRAMES):
        T = np.eye(3, 4)
        T[:, 3] = (-0.05 * k, 0.01 * (k % 7), 0.0)
        poses.append(T)
    xyz = np.stack([rng.uniform(-5, 55, n_points), rng.uniform(-3, 3, n_points), rng.uniform(4, 30, n_points)], 1)
    table = dict(xyz=xyz, normal=np.tile([0.0, 0.0, 1.0], (n_points, 1)), min_dist=np.ones(n_points), max_dist=np.full(n_points, 40.0), desc=rng.integers(0, 256, (n_points, 32), dtype=np.uint8))
    bad_kf = rng.uniform(size=N_KEYFRAMES) < 0.02
    ref = np.where(counts > 0, obs_kf[np.minimum(off[:-1], len(obs_kf) - 1)], 0).astype(np.int32)
    return dict(frames=frames, poses=poses, table=table, bad_kf=bad_kf, point_bad=(rng.uniform(size=n_points) < 0.01).astype(np.uint8), ref=ref, off=off, obs_kf=obs_kf, obs_kp=obs_kp, counts=counts)


def measure(reps, n_points=N_POINTS):
    rf = importlib.import_module(PKG + ".refresh")
    mm = importlib.import_module(PKG + ".map_match")
    om = importlib.import_module(PKG + ".orb_match")
    sc = scene(n_points)
    sf = np.cumprod(np.concatenate([[1.0], np.full(7, 1.2)])).astype(np.float32)
    lf = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], (0.0, 1241.0, 0.0, 376.0)) for f in sc["frames"]]
    kfs = [rf.keyframe(k, sc["poses"][k], sf, sc["bad_kf"][k]) for k in range(N_KEYFRAMES)]
    t = sc["table"]
    tb = mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"])
    args = [lf, kfs, tb, sc["point_bad"], sc["ref"], sc["off"], sc["obs_kf"], sc["obs_kp"]]
    for _ in range(2):
        rf.refresh(*args).close()                              # warm-up: code objects, first allocations
    wall = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = rf.refresh(*args); wall.append((time.perf_counter() - t0) * 1e3); r.close()
    os.environ["IBA_REFRESH_TIMING"] = "1"
    configs = [(w, f) for w in WIDTHS for f in FORMS]
    stage, paths, counts = {c: [] for c in configs}, {}, None
    for rep in range(reps + 1):                                # the configurations alternate inside every repetition; the first one warms every shape up
        for w, f in configs:
            os.environ["IBA_REFRESH_NARROW_LANES"], os.environ["IBA_REFRESH_MEDIAN"] = str(w), str(f)
            r = rf.refresh(*args)
            if rep:
                stage[(w, f)].append([float(v) for v in r.stage_ms])
            c = r.counts()
            paths[w] = [int(v) for v in c["path"]]
            assert counts is None or all(np.array_equal(counts[k], c[k]) for k in ("status", "desc_state", "geo_state")) and counts["n_desc_changed"] == c["n_desc_changed"]
            counts = c
            r.close()
    del os.environ["IBA_REFRESH_TIMING"], os.environ["IBA_REFRESH_NARROW_LANES"], os.environ["IBA_REFRESH_MEDIAN"]
    t0 = time.perf_counter(); h = rf.refresh_host(*args); host_ms = (time.perf_counter() - t0) * 1e3
    d = rf.refresh(*args)
    same = all(np.array_equal(a, b) for a, b in zip(h.read().values(), d.read().values()))
    h.close(); d.close()
    n_obs = sc["counts"]
    row = dict(n_points=int(n_points), n_keyframes=N_KEYFRAMES, n_kp=N_KP, n_obs=int(n_obs.sum()), obs_median=float(np.median(n_obs)), obs_under_10=float(np.mean(n_obs < 10)),
               obs_over_64=int(np.sum(n_obs > 64)), obs_max=int(n_obs.max()), pairs=int(np.sum(n_obs.astype(np.int64) ** 2)), reps=reps, wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)),
               host_ms=host_ms, host_agrees=bool(same), stage_ms={"%d/%d" % c: [float(v) for v in np.median(np.array(s), axis=0)] for c, s in stage.items()},
               stage_spread={"%d/%d" % c: [float(v) for v in (np.max(np.array(s), axis=0) - np.min(np.array(s), axis=0))] for c, s in stage.items()}, paths={str(w): p for w, p in paths.items()},
               status=[int(v) for v in counts["status"]], desc_state=[int(v) for v in counts["desc_state"]], geo_state=[int(v) for v in counts["geo_state"]], n_desc_changed=int(counts["n_desc_changed"]))
    print(json.dumps(row), flush=True)
    return [row]


def resources():
    """VGPRs, SGPRs, LDS, scratch and occupancy of the kernel's shapes from hipcc's resource report of csrc/iba_refresh.hip (the asm-refresh target's
    flags); None without a compiler"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    src = os.path.join(ROOT, PKG, "csrc", "iba_refresh.hip")
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
            k = re.search(r"refresh_kernelILi(\d+)ELb([01])E", m.group(2))
            cur = {"kernel": "refresh_kernel<%s, %s>" % (k.group(1), FORM_NAME[int(k.group(2))]), "order": (int(k.group(1)), int(k.group(2)))} if k else None
            if cur:
                rows.append(cur)
        elif cur is not None:
            cur[m.group(1).split(" [")[0]] = int(m.group(2))
    return sorted(rows, key=lambda r: r["order"]) or None


def write(rows, out):
    with open(out, "w") as fh:
        fh.write("# Map-point refresh on the device: what the first run saw\n\n")
        if not rows:
            fh.write("No GPU run was made: this file holds no measured time.\n\n")
        else:
            r = rows[0]
            fh.write("`python tools/refresh_bench.py` on one MI355X. A seeded scene shaped like a local map: %d points over %d keyframes of %d keypoints each, %d observations in all;\n"
                     "the observation count of a point has the median %.0f, %.1f %% of the points have fewer than 10, %d have more than 64 and the longest list holds %d; the sum of N^2\n"
                     "over the points - the distances one evaluation of every matrix takes - is %.3g. All points are listed. `wall`: the whole iba_refresh from Python - checks, flat\n"
                     "tables, allocations, uploads (%.0f MB of keypoint descriptors among them), three launches, the results down - after two warm-up calls, in the shipped configuration.\n"
                     "Launch times are the median over %d further calls with IBA_REFRESH_TIMING (HIP events around each launch), the configurations alternating inside every repetition.\n"
                     "`host`: iba_debug_refresh_host, the same call on one CPU thread of the GPU machine, one run; it is the yardstick, there being no earlier figure for a unit that\n"
                     "did not exist. No target is set and nothing is gated. Kernel times from a profiler trace and shares of peak were not measured.\n\n"
                     % (r["n_points"], r["n_keyframes"], r["n_kp"], r["n_obs"], r["obs_median"], 100 * r["obs_under_10"], r["obs_over_64"], r["obs_max"], r["pairs"],
                        32e-6 * r["n_keyframes"] * r["n_kp"], r["reps"]))
            fh.write("| points | observations | wall ms (min / median) | host ms | host / wall | descriptors changed | host agrees |\n|---|---|---|---|---|---|---|\n")
            fh.write("| %d | %d | %.1f / %.1f | %.1f | %.1f | %d | %s |\n" % (r["n_points"], r["n_obs"], r["wall_min_ms"], r["wall_median_ms"], r["host_ms"], r["host_ms"] / r["wall_median_ms"],
                                                                        r["n_desc_changed"], "yes" if r["host_agrees"] else "NO"))
            fh.write("\nPoints per status (REFRESHED, BAD, EMPTY): %s; per desc_state (NONE, PICKED, KEPT): %s; per geo_state (NONE, UPDATED, NO_REF, DEGENERATE): %s.\n"
                     % (r["status"], r["desc_state"], r["geo_state"]))
            fh.write("\n## Launches, per narrow width and median form (ms, median of %d calls; in brackets max - min of the sum's parts)\n\n" % r["reps"])
            fh.write("| narrow lanes | median form | points narrow / wave / block | narrow | wave | block | sum |\n|---|---|---|---|---|---|---|\n")
            for w in WIDTHS:
                for f in FORMS:
                    s, sp = r["stage_ms"]["%d/%d" % (w, f)], r["stage_spread"]["%d/%d" % (w, f)]
                    fh.write("| %d | %s | %s | %.3f | %.3f | %.3f | %.3f (%.3f) |\n" % (w, FORM_NAME[f], " / ".join(str(v) for v in r["paths"][str(w)]), s[0], s[1], s[2], sum(s), sum(sp)))
            best = min(r["stage_ms"], key=lambda k: sum(r["stage_ms"][k]))
            bw, bf = (int(v) for v in best.split("/"))
            fh.write("\nThe least sum of the three launches on this scene is %.3f ms, at %d narrow lanes with the %s form. A narrower group leaves fewer idle lanes on the short lists but sends\n"
                     "more points to the wave shape; the bytes are the same in all eight configurations (tests/test_gpu_refresh.py runs all eight).\n"
                     % (sum(r["stage_ms"][best]), bw, FORM_NAME[bf]))
            fh.write("\nThe launches are a small part of the median wall time %.1f ms: the rest is the host around them - the checks (every observation's keyframe, keypoint and octave), the\n"
                     "flat tables, the allocations - and the copies of the frames' descriptors, the table and the lists.\n" % r["wall_median_ms"])
        fh.write("\n## Kernel resources (hipcc -Rpass-analysis=kernel-resource-usage, gfx950; the asm-refresh target)\n\n")
        res = resources()
        if res:
            fh.write("| kernel <lanes per point, median form> | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | waves / SIMD |\n|---|---|---|---|---|---|\n")
            for k in res:
                fh.write("| %s | %d | %d | %d | %d | %d |\n" % (k["kernel"], k.get("VGPRs", -1), k.get("TotalSGPRs", -1), k.get("LDS Size", -1), k.get("ScratchSize", -1), k.get("Occupancy", -1)))
            fh.write("\n%s\n" % ("No shape uses scratch." if all(k.get("ScratchSize", 0) == 0 for k in res) else "SCRATCH IS IN USE in the shapes whose column is not 0."))
        else:
            fh.write("No compiler was found where this file was written.\n")
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--points", type=int, default=N_POINTS, help="a smaller scene, for a rehearsal of the tool")
    ap.add_argument("--json", default=None, help="keep the measured numbers here")
    ap.add_argument("--from-json", default=None, help="format rows measured earlier instead of measuring")
    ap.add_argument("--measure-only", action="store_true", help="measure and keep the numbers (--json) without writing the file")
    a = ap.parse_args()
    rows = json.load(open(a.from_json)) if a.from_json else measure(a.reps, a.points)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    if not a.measure_only:
        write(rows, a.out)


if __name__ == "__main__":
    main()

"""F-LOAM odometry on the device: iba_floam_odom_run at B = 1 / 8 / 64 tracks of 8 scans (64-line room scans of tests/floam_ref.py, origins 0.2 m
apart; the tracks of a batch are the same scans) beside the same track driven through the public calls that existed before it: iba_floam_extract,
the lattice filter on the host (tests/floam_odom_ref.py), iba_create of a four-frame handle and iba_floam_map_register per step, the map update on
the host. Nothing is gated: nobody has measured these numbers before, the file records them. On a GPU it writes profiles/floam_odom_bench.md.
Timing: HOST WALL TIME of the blocking calls (perf_counter, after warm-up calls; best and median of --reps), divided by the scans of the batch. The tool
rewrites the timing part of the file only: everything from the "Compiler resource report" heading on is kept as it stands, entered by hand.
    python tools/floam_odom_bench.py [--out profiles/floam_odom_bench.md] [--reps 5] [--warmup 2]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import floam_odom_ref as O  # noqa: E402
import floam_ref as F  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
RES_HEADING = "## Compiler resource report"
N_SCANS, STEP, RES, CROP, INIT = 8, 0.2, 0.4, 100.0, 12


def timed(f, warmup, reps):
    for _ in range(warmup):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def public_calls_track(pkg, abi, h, n):
    """one track through today's public calls; -> poses"""
    feats = h.floam_extract(list(range(n)), num_lines=64)
    T = [np.eye(4)]
    me, ms = O.init_map(feats[0]["edge_xyz"], feats[0]["surf_xyz"], T[0])
    sched = O.pass_schedule(n, INIT)
    for k in range(1, n):
        se, ss = O.downsample(feats[k]["edge_xyz"], feats[k]["surf_xyz"], RES)
        T_pred = O.predict(T[k - 2] if k >= 2 else T[0], T[k - 1])
        hk = pkg.IbaHandle(abi.Problem.from_scans([se, ss, me, ms]), abi.reference_yaml_params(0))
        r = hk.floam_map_register([(0, 1, 2, 3, T_pred)], outer_passes=sched[k])[0]
        hk.close()
        T.append(r["T"])
        me, ms, _, _ = O.update_map(me, ms, se, ss, r["T"], RES, CROP)
    return T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floam_odom_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi")
    scans = [F.room_scan(64, per_ring=300, seed=60 + k, origin=(STEP * k, 0.0)) for k in range(N_SCANS)]
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    track = (list(range(N_SCANS)), np.eye(4))
    rows = []
    last = None
    for B in (1, 8, 64):
        keep = []
        best, med = timed(lambda: keep.append(h.floam_odom([track] * B, map_resolution=RES, crop_half=CROP, init_passes=INIT, extract=dict(num_lines=64))), a.warmup, a.reps)
        last = keep[-1][0]
        err = float(np.linalg.norm(last[-1]["T"][:3, 3] - [STEP * (N_SCANS - 1), 0, 0]))
        rows.append((B, best, med, best / (B * N_SCANS), med / (B * N_SCANS), err))
    poses = []
    pb, pm = timed(lambda: poses.append(public_calls_track(pkg, abi, h, N_SCANS)), 1, max(2, a.reps // 2))
    d_pose = float(np.max(np.abs(poses[-1][-1] - last[-1]["T"])))
    h.close()
    lines = ["# F-LOAM odometry on the device: resources and a first measurement", "",
             "`python tools/floam_odom_bench.py` on one MI355X. Tracks of %d 64-line room scans (%d points each, origins %.1f m apart), map_resolution %.1f, the" % (N_SCANS, len(scans[0]), STEP, RES),
             "reference's pass schedule (11, 10, .. passes). The tracks of a batch are the same scans. All times are HOST WALL TIME of the whole blocking call",
             "from Python, NOT kernel time: after %d warm-up calls, best and median of %d. Nothing comparable existed before, so there is no target and nothing" % (a.warmup, a.reps),
             "here is gated. Last scan of a track: %d / %d down-sampled edge / surf points against a map of %d / %d." % (last[-1]["n_src_edge"], last[-1]["n_src_surf"], last[-2]["n_map_edge"], last[-2]["n_map_surf"]), "",
             "| B tracks | call best ms | call median ms | best ms per scan | median ms per scan | final position error m |", "|---|---|---|---|---|---|"]
    lines += ["| %d | %.2f | %.2f | %.3f | %.3f | %.4f |" % r for r in rows]
    lines += ["", "The same track through the public calls that existed before (iba_floam_extract once, then per step: the lattice filter of `tests/floam_odom_ref.py` in",
              "numpy on the host, `iba_create` of a four-frame handle, `iba_floam_map_register`, the map update in numpy), ONE track: best %.1f ms, median %.1f ms =" % (pb, pm),
              "%.2f / %.2f ms per scan. Its final pose differs from the device loop's by %.2e at most per entry (the host path builds its kd index on the host" % (pb / N_SCANS, pm / N_SCANS, d_pose),
              "from the same float32 clouds)."]
    tail = ""
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = f.read()
        if RES_HEADING in old:
            tail = old[old.index(RES_HEADING):]
    if not tail:
        tail = RES_HEADING + "\n\nNot recorded yet: compile csrc with -Rpass-analysis=kernel-resource-usage and enter the table here by hand.\n"
    text = "\n".join(lines) + "\n\n" + tail
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Times the robust smoother (iba_smooth_*) on one GPU and writes profiles/backend_bench.md: per N, the first update of a graph with a prior, odometry
and loops, the update after one more loop was appended (what the back end pays per accepted loop), and the time per LM trial — next to the per-trial
time profiles/pgo_bench.md records for the same N. Nothing is gated."""
import argparse
import importlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

import smooth_ref as S  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"


def pgo_trial_ms(path=os.path.join(ROOT, "profiles", "pgo_bench.md")):
    """{N: ms per trial} of the K = 128 rows of profiles/pgo_bench.md's timing table, read from the file as it stands"""
    out = {}
    try:
        for line in open(path):
            c = [x.strip() for x in line.strip().strip("|").split("|")]
            if len(c) == 11 and c[0].isdigit() and c[2] == "128":
                out[int(c[0])] = float(c[9])
    except OSError:
        pass
    return out



def build(sm, g, upto=None):
    s = sm.Smoother()
    for n in g.nodes:
        s.add_node(n)
    for f in range(g.F if upto is None else upto):
        if g.fi[f] < 0:
            s.add_prior(g.fj[f], g.Z[f], g.var[f])
        else:
            s.add_between(g.fi[f], g.fj[f], g.Z[f], g.var[f], g.robust[f])
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backend_bench.md"))
    ap.add_argument("--sizes", default="500,2000,4541")
    a = ap.parse_args()
    sm = importlib.import_module(PKG + ".smooth")
    pgo = pgo_trial_ms()
    rows = []
    for N in [int(x) for x in a.sizes.split(",")]:
        loops = max(4, N // 75)
        g, _ = S.make_graph(N, loops=loops, false_loops=1, seed=7)
        w = build(sm, g)          # warm-up: module load, allocations
        w.update()
        w.close()
        s = build(sm, g, upto=g.F - 1)
        t0 = time.perf_counter(); r1 = s.update(); t1 = time.perf_counter()
        f = g.F - 1
        s.add_between(g.fi[f], g.fj[f], g.Z[f], g.var[f], g.robust[f])
        t2 = time.perf_counter(); r2 = s.update(); t3 = time.perf_counter()
        lin = []
        for _ in range(7):
            t = time.perf_counter(); s.lib.iba_smooth_linearize(s.h, None, None, None, None, None, None); lin.append(time.perf_counter() - t)
        s.close()
        rows.append((N, g.F, loops + 1, (t1 - t0) * 1e3, r1.trials, r1.stop, (t3 - t2) * 1e3, r2.trials, r2.stop, (t1 - t0 + t3 - t2) * 1e3 / max(r1.trials + r2.trials, 1),
                     sorted(lin)[3] * 1e3, min(pgo.items(), key=lambda kv: abs(kv[0] - N)) if pgo else None))
    # one loop verification and one whole run on the closed circuit of tests/backend_ref.py (30 scans of 2500 points; frames 20 .. 29 revisit 0 .. 9)
    pkg = importlib.import_module(PKG)
    abi = importlib.import_module(PKG + ".abi")
    be = importlib.import_module(PKG + ".backend")
    synth = importlib.import_module(PKG + ".synth")
    import backend_ref as B
    import submap_ref as V
    scans, _, raw = B.circuit(synth, 2)
    S_LC = 2                                        # lc_submap_size of the run below: the loop (20, 0) sees the sub-map of frames [0, 2)
    run_kw = dict(voxel=0.2, lc_submap_size=S_LC, cloud_lag=0, scan_coarse_max_iter=30, scan_refine_max_iter=30, sc_num_exclude_recent=3, sc_tree_period=2,
                  sc_lidar_height=B.SCENE["lidar_height"])
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    ver, members = [], list(range(0, S_LC))
    for _ in range(7):
        t = time.perf_counter()
        lc = h.submap_handle([([20], [np.eye(4)], None, 0.2), (members, [raw[f] for f in members], V.inverse34(raw[0]), 0.2)])
        reg = lc.scan_register([(0, 1, np.eye(4))], estimation=0, coarse_dist=1.0, coarse_max_iter=30, refine_dist=0.3, refine_max_iter=30)[0].reg
        lc.close()
        ver.append(time.perf_counter() - t)
    runs = []
    for _ in range(3):
        t = time.perf_counter(); out = be.backend_run(h, raw[:, :3], **run_kw); runs.append(time.perf_counter() - t)
    h.close()
    first = out["detections"][0]
    with open(a.out, "w") as fh:
        fh.write("# Robust smoothing on the device: what one run saw\n\n")
        fh.write("`python tools/backend_bench.py` on one MI355X: wall time of the whole C-ABI call from Python (plan on the host, uploads, launch chains, one\n"
                 "synchronise per LM trial). Graph: tests/smooth_ref.py make_graph(N, loops, 1 false loop, seed 7) at the reference's variances, segment 128.\n"
                 "`first update`: every factor but the last loop; `update after one more loop`: that loop appended, then iba_smooth_update from the estimates\n"
                 "(the plan is rebuilt). `ms per trial` is over both updates; the last column is the per-trial time profiles/pgo_bench.md has for iba_pgo\n"
                 "(K = 128) at the nearest N it was run at. Nothing here is gated.\n\n")
        fh.write("| N | factors | loops | first update ms | trials | stop | update after one more loop ms | trials | stop | ms per trial | linearise ms (median of 7) | iba_pgo ms per trial |\n")
        fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            fh.write("| %d | %d | %d | %.1f | %d | %s | %.1f | %d | %s | %.3f | %.3f | %s |\n" % (r[0], r[1], r[2], r[3], r[4], sm.STOP[r[5]], r[6], r[7], sm.STOP[r[8]], r[9], r[10],
                                                                                                  "%.3f (N = %d)" % (r[11][1], r[11][0]) if r[11] else "-"))
        fh.write("\nOne loop verification, the revisit (query frame 20, history frame 0) of the closed circuit of tests/backend_ref.py (30 scans of 2500 points, voxel 0.2)\n"
                 "as iba_backend_run performs it at lc_submap_size %d: a two-frame iba_submap_handle (the query's cloud; the sub-map of frames [0, %d) in the\n"
                 "history frame), iba_scan_register from the identity (coarse 1.0 m, refine 0.3 m, up to 30 iterations each; %d refine iterations ran, fitness %.3f,\n"
                 "rmse %.3f), the handle destroyed: median of 7 %.2f ms, best %.2f ms. The whole iba_backend_run on that circuit (30 frames, %d detections of which\n"
                 "%d accepted, %d updates; its first detection is this loop: fitness %.3f): median of 3 %.1f ms.\n"
                 % (S_LC, S_LC, reg.iterations, reg.fitness, reg.inlier_rmse, sorted(ver)[3] * 1e3, min(ver) * 1e3, len(out["detections"]),
                    sum(d["accepted"] for d in out["detections"]), len(out["updates"]), first["fitness"], sorted(runs)[1] * 1e3))
    print(open(a.out).read())


if __name__ == "__main__":
    main()

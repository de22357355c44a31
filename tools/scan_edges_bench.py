"""Odometry edges of a keyframe sequence registered scan to scan, two ways, in one session (profiles/scan_edges_bench.md):
  baseline   what the library offered before iba_scan_*: a loop of iba_icp_register(with_scaling = 0) calls, one per edge, each given its source
             scan as doubles, plus the information matrix through iba_geo_correspondences + numpy
  new        one iba_scan_register with info_dist set
alternated, medians and spread over --reps repetitions after a warm-up, host clock around the blocking calls. Also E = 1 on the first edge, both
block shapes of the pass kernel, and both estimations.
  python tools/scan_edges_bench.py [--frames 200] [--points 10000] [--reps 10] [--out FILE.json]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401,E402  (first: its bundled HIP runtime is the process's one, see tests/conftest.py)

pkg = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd")
synth = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd.synth")
abi = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd.abi")


def rotvec(w):
    th = np.linalg.norm(w); k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def med(v):
    v = np.asarray(v) * 1e3
    return dict(median_ms=float(np.median(v)), min_ms=float(v.min()), max_ms=float(v.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200); ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=10); ap.add_argument("--gate", type=float, default=0.3); ap.add_argument("--info", type=float, default=1.2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    prob, _ = synth.make_scene(n_frames=a.frames, pts_per_frame=a.points, n_keypoints=20, seed=0)
    scans = [prob.frame_points(f) for f in range(a.frames)]
    Tl = prob.arrays["Tl_next"].reshape(-1, 3, 4)
    rng = np.random.default_rng(1)
    edges = []
    for f in range(a.frames - 1):
        T = np.eye(4); T[:3] = Tl[f]
        w = rng.normal(size=3); w *= 3e-3 / np.linalg.norm(w); d = rng.normal(size=3); d *= 0.03 / np.linalg.norm(d)
        P = np.eye(4); P[:3, :3] = rotvec(w); P[:3, 3] = d
        edges.append((f, f + 1, P @ T))
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params())
    srcd = [s.astype(np.float64) for s in scans]

    def baseline(ed):
        out = []
        for s, t, T in ed:
            r = h.icp_register(srcd[s], T, frames=(t, t + 1), max_corr_dist=a.gate, with_scaling=0)[0]
            Tf = r.T_np()
            q = srcd[s] @ Tf[:3, :3].T + Tf[:3, 3]
            _, gt = h.geo_correspondences(t, q, a.info * a.info)
            p = scans[t][gt].astype(np.float64)
            I = np.zeros((6, 6)); n = len(p); sx = p.sum(0); M = p.T @ p
            I[3:, 3:] = n * np.eye(3); I[:3, :3] = np.trace(M) * np.eye(3) - M
            G = np.array([[0, -sx[2], sx[1]], [sx[2], 0, -sx[0]], [-sx[1], sx[0], 0]]); I[:3, 3:] = G; I[3:, :3] = G.T
            out.append((r, I))
        return out

    def new(ed, est=0):
        return h.scan_register(ed, estimation=est, refine_dist=a.gate, info_dist=a.info)

    res = dict(frames=a.frames, points=a.points, edges=len(edges), gate=a.gate, info=a.info, reps=a.reps)
    b0 = baseline(edges); n0 = new(edges); n1 = new(edges, 1)      # warm-up, and what the two ways computed
    res["passes_new_p2p"] = 1 + max(r.reg.iterations for r in n0) + 1
    res["edge_evaluations_p2p"] = int(sum(r.reg.iterations + 1 for r in n0)); res["edge_evaluations_p2l"] = int(sum(r.reg.iterations + 1 for r in n1))
    res["passes_new_p2l"] = 1 + max(r.reg.iterations for r in n1) + 1
    res["same_iterations_as_baseline"] = int(sum(x[0].iterations == y.reg.iterations for x, y in zip(b0, n0)))
    res["max_T_difference_from_baseline"] = float(max(np.max(np.abs(x[0].T_np() - y.reg.T_np())) for x, y in zip(b0, n0)))
    res["max_info_rel_difference_from_baseline"] = float(max(np.max(np.abs(x[1] - y.info_np())) / np.max(np.abs(x[1])) for x, y in zip(b0, n0)))
    tb, tn, tp, tb1, tn1 = [], [], [], [], []
    for _ in range(a.reps):
        t = time.perf_counter(); baseline(edges); tb.append(time.perf_counter() - t)
        t = time.perf_counter(); new(edges); tn.append(time.perf_counter() - t)
        t = time.perf_counter(); new(edges, 1); tp.append(time.perf_counter() - t)
        t = time.perf_counter(); h.icp_register(srcd[0], edges[0][2], frames=(1, 2), max_corr_dist=a.gate, with_scaling=0); tb1.append(time.perf_counter() - t)
        t = time.perf_counter(); h.scan_register(edges[:1], refine_dist=a.gate); tn1.append(time.perf_counter() - t)
    res["baseline_loop"] = med(tb); res["new_p2p"] = med(tn); res["new_p2l"] = med(tp)
    res["baseline_ms_per_edge"] = res["baseline_loop"]["median_ms"] / len(edges); res["new_p2p_ms_per_edge"] = res["new_p2p"]["median_ms"] / len(edges)
    res["E1_baseline_icp_register"] = med(tb1); res["E1_new_scan_register"] = med(tn1)
    for threads in (64, 256):                                       # one pass of all edges in each block shape
        h.debug_scan_threads(threads)
        for est, name in ((0, "p2p"), (1, "p2l"), (2, "info")):
            h.scan_step(edges, a.gate, est)
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter(); h.scan_step(edges, a.gate, est); ts.append(time.perf_counter() - t)
            res["step_%s_threads%d" % (name, threads)] = med(ts)
    h.debug_scan_threads(0)
    h.scan_step(edges, a.gate, 0); res["rule_threads"] = h.last_scan_threads
    h.close()
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()

"""The rebuild bound of the pair search's visible-chunk list, swept on an optimiser's own batches: the black-box calls of the global stage on
the bench scene (200 keyframes x 10 k points, the start of bench.py's global_then_local, recorded here as bench.py's extras.mads_trace_replay
records them) replayed through iba_eval_bbo on a fresh handle per setting (iba_debug_set_pairs_visible_bound: factor on the batch's own bound,
floors, pair searches between two rebuilds). Per setting: rebuilds, pair searches, how many of them walked the list, the mean number of items
a listed search walked (of the grid's 31 400), seconds; and the items of a list built around a bench batch (64 candidates around x_gt).
usage: python tools/vis_sweep.py"""
import ctypes as C
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: F401  (one HIP runtime per process: torch's first)

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pkg = importlib.import_module(PKG)
synth = importlib.import_module(PKG + ".synth")
abi = importlib.import_module(PKG + ".abi")

prob, meta = synth.make_scene(n_frames=int(os.environ.get("FRAMES", "200")), pts_per_frame=10000, n_keypoints=2000, seed=0)
params = abi.reference_yaml_params()
L = pkg.load_library()
L.iba_debug_set_pairs_visible_bound.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_int32]
h = pkg.IbaHandle(prob, params, device=0)
xg0 = meta["x_gt"] + np.array([0.009, -0.006, 0.005, 0.06, -0.04, 0.05, 0.4])
xg, mr, tr, bs = h.calibrate_mads(xg0, record=True, max_bb_eval=100000)
h.close()
print("trace: %d evaluations in %d batches" % (len(tr), len(bs)), flush=True)
mo = pkg.mads_options(xg0)
xr = np.ascontiguousarray(tr[:, :7])
buf = (pkg.IbaBbo * pkg.IBA_MAX_BATCH)()
bench_xs = synth.perturb(meta["x_gt"], np.random.default_rng(0), n=64)


def run(infl, rf, tf, gap):
    hh = pkg.IbaHandle(prob, params, device=0)
    assert L.iba_debug_set_pairs_visible_bound(hh.h, infl, rf, tf, gap) == 0
    at, used, walked, searches0 = 0, 0, 0, hh.pairs_builds
    t0 = time.perf_counter()
    for nb in bs:
        nb = int(nb)
        assert L.iba_eval_bbo(hh.h, C.c_void_p(xr[at:at + nb].ctypes.data), C.c_int32(nb), C.c_double(mo.he_threshold), C.c_double(mo.valid_rate), buf) == 0
        at += nb
        items, _, u, _ = hh.pairs_visible
        used += u; walked += items * u
    t = time.perf_counter() - t0
    _, rebuilds, _, full = hh.pairs_visible
    searches = hh.pairs_builds - searches0
    hh.close()
    hb = pkg.IbaHandle(prob, params, device=0)   # the list a bench batch gets
    assert L.iba_debug_set_pairs_visible_bound(hb.h, infl, rf, tf, gap) == 0
    hb.eval_full(bench_xs); hb.eval_full(bench_xs)
    bench_items = hb.pairs_visible[0]
    hb.close()
    print("infl %4.1f floors %.0e / %.0e gap %d: rebuilds %3d, pair searches (launch planes) %4d, calls on the list %4d, mean items walked %6.0f of %d, %.4f s | bench batch: %d items"
          % (infl, rf, tf, gap, rebuilds, searches, used, walked / max(used, 1), full, t, bench_items), flush=True)


run(4.0, 1e-3, 1e-2, 4)   # (twice: the first replay of a process carries its warm-up)
for infl in (2.0, 4.0, 8.0, 16.0):
    for rf, tf in ((1e-3, 1e-2), (3e-3, 3e-2), (1e-2, 1e-1)):
        run(infl, rf, tf, 4)
for gap in (0, 1, 2, 8):
    run(4.0, 1e-3, 1e-2, gap)
for gap in (0, 1):
    run(16.0, 1e-2, 1e-1, gap)

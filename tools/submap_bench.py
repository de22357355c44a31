"""iba_submap_build at the reference's sizes: wall time per call (host clock around the blocking call: it ends in a device synchronise and the
copy of the clouds) for
  one     one 50-member sub-map of 120 k-point scans at voxel 0.4 (MergeLoadPCD with LCSubmapSize 25: about 6 M points in)
  batch   64 such sub-maps in one call
  single  200 single-scan down-samples in one call (LoadPCD)
and beside them the numpy restatement tests/submap_ref.py on the same inputs, the only comparator there is (for `batch` and `single` it is timed
on a few sub-maps and multiplied: the figure says so). The device result of `one` is compared with the restatement byte for byte before anything
is timed. Warm-up, then the median of the repetitions. Prints one JSON line; --md FILE appends a table.
  python tools/submap_bench.py [--reps 7] [--md build/submap_bench.md] [--quick] [--no-ref]
--quick: `one` and `single` only, two repetitions (the kernel-trace run: rocprofv3 --kernel-trace --stats -- python tools/submap_bench.py --quick --no-ref)."""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np

import submap_ref as V

PKG = "spatial-temporal-lidar-camera-calibration_amd"


def med(v):
    return float(np.median(v))


def timed(fn, reps):
    fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); t.append(time.perf_counter() - t0)
    return r, t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--md", default=None)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--no-ref", action="store_true", help="skip the numpy restatement's timings")
    ap.add_argument("--frames", type=int, default=52)
    ap.add_argument("--points", type=int, default=120000)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi"); synth = importlib.import_module(PKG + ".synth")
    F, P, voxel, n_mem = a.frames, a.points, 0.4, min(50, a.frames)
    t0 = time.perf_counter()
    prob, meta = synth.make_scene(n_frames=F, pts_per_frame=P, n_keypoints=50, seed=11)
    scans = [prob.frame_points(f) for f in range(F)]
    Twl = meta["Twl"]
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    setup_s = time.perf_counter() - t0

    def window(k):
        fr = [(k + i) % F for i in range(n_mem)]
        return (fr, [Twl[f] for f in fr], V.inverse34(Twl[fr[n_mem // 2]]), voxel)

    shapes = {"one": [window(0)], "single": [([k % F], [np.eye(4)], None, voxel) for k in range(200)]}
    if not a.quick:
        shapes["batch"] = [window(k) for k in range(64)]
    reps = 2 if a.quick else a.reps
    out = {"frames": F, "points_per_scan": P, "voxel": voxel, "members": n_mem, "reps": reps, "setup_s": setup_s, "shapes": {}}
    ref_one = None
    if not a.no_ref:
        t0 = time.perf_counter()
        ref_one = V.build([(scans[f], T) for f, T in zip(*shapes["one"][0][:2])], voxel, shapes["one"][0][2])
        ref_one_s = time.perf_counter() - t0
        dev = h.submap_build(shapes["one"])[0]
        assert dev["xyz"].tobytes() == ref_one["xyz"].tobytes() and dev["count"].tobytes() == ref_one["count"].tobytes() and dev["n_dropped"] == ref_one["n_dropped"], "device and restatement differ"
    for name in ("one", "batch", "single"):
        if name not in shapes:
            continue
        subs = shapes[name]
        res, t = timed(lambda: h.submap_build(subs), reps)
        pts_in = int(sum(len(scans[f]) for s in subs for f in s[0]))
        vox = int(sum(len(r["xyz"]) for r in res))
        rec = {"sub_maps": len(subs), "points_in": pts_in, "voxels_out": vox, "largest_voxel": int(max(int(r["count"].max()) for r in res)), "ms": med(t) * 1e3, "ms_min": min(t) * 1e3, "ms_max": max(t) * 1e3,
               "points_per_s": pts_in / med(t)}
        if not a.no_ref:
            if name == "one":
                rec["numpy_s"] = ref_one_s; rec["numpy_timed_sub_maps"] = 1
            else:
                k = 1 if name == "batch" else 3
                t0 = time.perf_counter()
                for s in subs[:k]:
                    V.build([(scans[f], T) for f, T in zip(s[0], s[1])], s[3], s[2])
                rec["numpy_s"] = (time.perf_counter() - t0) / k * len(subs); rec["numpy_timed_sub_maps"] = k
        out["shapes"][name] = rec
    h.close()
    print(json.dumps(out))
    if a.md:
        with open(a.md, "a") as f:
            f.write("| shape | sub-maps | points in | voxels out | largest voxel | iba_submap_build, ms (median; min .. max) | points / s | numpy restatement, s (sub-maps timed) |\n|---|---|---|---|---|---|---|---|\n")
            for k, r in out["shapes"].items():
                f.write("| %s | %d | %d | %d | %d | %.2f (%.2f .. %.2f) | %.3g | %s |\n" % (k, r["sub_maps"], r["points_in"], r["voxels_out"], r["largest_voxel"], r["ms"], r["ms_min"], r["ms_max"], r["points_per_s"],
                                                                             ("%.1f (%d)" % (r["numpy_s"], r["numpy_timed_sub_maps"])) if "numpy_s" in r else "not timed"))
    return 0


if __name__ == "__main__":
    sys.exit(main())

"""Byte parity of the correspondence passes (iba_icp_*, iba_scan_*, iba_floam_map_*) and of iba_calibrate_lm between two builds of the library:
one handle of seeded synthetic clouds, a fixed list of calls, one SHA-256 per output buffer. Run it once per library (IBA_LIB selects the build,
as the package's __init__.py allows) and compare the lists: a refactor of the shared pass skeleton (csrc/iba_flat_pass.hpp) must not move a byte.
The shapes are the smallest at which each shared piece can go wrong: 3 001 points are no multiple of 64 or 256 (trailing waves without a partial),
17 000 points give a depth-10 tree (node table above 6 KB: four-wave blocks) and 266 chunks (the sum kernel's thread loop takes a second turn), a
10-point map makes a F-LOAM pair degenerate. iba_calibrate_lm runs on a handle of its own, the tests' small scene.
    IBA_LIB=/path/to/libiba_mi355x.so python tools/pass_parity.py [--out hashes.txt]"""
import argparse
import hashlib
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import floam_map_ref as F  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
SIZES = (10, 50, 700, 3001, 17000)   # frames 0-4; 5-8: src_edge, src_surf, map_edge, map_surf of room_scene


def raw(x):
    if isinstance(x, dict):
        return b"".join(raw(x[k]) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return b"".join(raw(v) for v in x)
    if isinstance(x, (int, float, np.integer, np.floating)):
        return np.asarray(x).tobytes()
    return np.ascontiguousarray(x).tobytes() if isinstance(x, np.ndarray) else bytes(x)   # (a ctypes structure: its bytes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi"); synth = importlib.import_module(PKG + ".synth")
    lines = []

    def note(name, *bufs):
        lines.append("%-44s %s" % (name, hashlib.sha256(raw(bufs)).hexdigest()))
        print(lines[-1], flush=True)

    rng = np.random.default_rng(20)
    base = rng.normal(size=(SIZES[-1], 3)) * [8.0, 6.0, 1.5]
    clouds = [(base[rng.permutation(len(base))[:n]] + rng.normal(0, 0.02, (n, 3))).astype(np.float32) for n in SIZES]
    room = F.room_scene(7)
    clouds += [room[k] for k in ("src_edge", "src_surf", "map_edge", "map_surf")]
    h = pkg.IbaHandle(abi.Problem.from_scans(clouds), abi.reference_yaml_params(1))

    def start(seed, rot=0.01, trans=0.05):
        r = np.random.default_rng(seed)
        return F.rigid(r.normal(size=3) * rot, r.normal(size=3) * trans)

    # iba_icp_*: a two-tile target (3 001 + 17 000: four-wave blocks) and a one-tile target (700: one-wave blocks), B = 1 and 5
    for tag, frames, src in (("two_tiles", (3, 5), clouds[4].astype(np.float64) + 0.01), ("one_tile", (2, 3), clouds[3].astype(np.float64) + 0.01)):
        for B in (1, 5):
            T = np.stack([start(100 + b) for b in range(B)])
            note("icp_step %s B%d" % (tag, B), *h.icp_step(src, T, 1.0, frames=frames, pairs=True))
            note("icp_register %s B%d" % (tag, B), h.icp_register(src, T, frames=frames, max_corr_dist=1.0, max_iter=5))
    # iba_scan_*: the 50-, 3 001- and 17 000-point frames in both roles
    edges = [(s, t, start(200 + 10 * s + t)) for s, t in ((1, 3), (3, 4), (4, 3), (4, 1), (3, 1), (1, 4))]
    for threads in (0, 64, 256):
        h.debug_scan_threads(threads)
        for est in (0, 1, 2):
            note("scan_step est%d threads%d" % (est, threads), *h.scan_step(edges, 1.0, est, pairs=True))
    h.debug_scan_threads(0)
    note("scan_information", *h.scan_information(edges, 1.0))
    for est in (0, 1):
        note("scan_register est%d" % est, h.scan_register(edges, estimation=est, coarse_dist=2.0, coarse_max_iter=4, refine_dist=0.8, refine_max_iter=4, info_dist=1.0))
    # iba_floam_map_*: the room, the room against a 10-point edge map (degenerate), the room against an unrelated 17 000-point surf map
    pairs = [(5, 6, 7, 8, F.perturbed(room["T_gt"], 1)), (5, 6, 0, 8, F.perturbed(room["T_gt"], 2)), (5, 6, 7, 4, F.perturbed(room["T_gt"], 3)),
             (5, 6, 7, 8, F.perturbed(room["T_gt"], 4, 1.0, 0.1))]
    note("floam_map_step", *h.floam_map_step(pairs, nn=True, records=True))
    note("floam_map_step B1", *h.floam_map_step(pairs[:1], nn=True, records=True))
    reg = h.floam_map_register(pairs)
    assert reg[1]["status"] == 1 and reg[0]["status"] == 0, [r["status"] for r in reg]
    note("floam_map_register", reg)
    h.close()
    # iba_calibrate_lm on the tests' small scene (12 keyframes x 4 000 points)
    prob, meta = synth.make_scene(n_frames=12, pts_per_frame=4000, seed=1)
    h = pkg.IbaHandle(prob, abi.reference_yaml_params())
    x0 = synth.perturb(meta["x_gt"], np.random.default_rng(5), rot=1e-3, trans=0.01, scale_rel=3e-3, n=1)[0]
    x, r = h.calibrate_lm(x0, max_outer_iterations=6)
    note("calibrate_lm", x, r)
    h.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""The picture pair the reference's README shows (doc/proj_XX_gt.png / proj_XX_pred.png), from this library: one frame of a synthetic scene (synth.py)
rendered under two extrinsics — the ground truth and a prediction (by default the ground truth moved by a degree and a few centimetres; --pred takes
any x) — as depth-coloured overlays, with the sparse depth image and the per-point colours beside them. PNG when PIL imports, .npy otherwise.

    python tools/project_demo.py --out /tmp/proj --frame 2"""
import argparse
import importlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"


def save(path, img):
    """an [H, W, 3] uint8 image as PNG when PIL is there, else the array"""
    try:
        from PIL import Image
        Image.fromarray(img).save(path + ".png")
        return path + ".png"
    except ImportError:
        np.save(path + ".npy", img)
        return path + ".npy"


def background(W, H):
    """a stand-in for the camera image (the synthetic scene has none): a grey ramp with a grid, so that the colours of the points are not all alike"""
    yy, xx = np.mgrid[0:H, 0:W]
    g = (40 + 80 * yy / max(H - 1, 1) + 30 * ((xx // 40 + yy // 40) % 2)).astype(np.uint8)
    return np.stack([g, g, (g // 2 + 60).astype(np.uint8)], axis=2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="proj", help="prefix of the files written")
    ap.add_argument("--frame", type=int, default=0)
    ap.add_argument("--frames", type=int, default=4)
    ap.add_argument("--points", type=int, default=20000)
    ap.add_argument("--splat", type=int, default=1)
    ap.add_argument("--pred", type=float, nargs=7, default=None, help="the predicted extrinsic x (7 numbers); default: the ground truth perturbed")
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); synth = importlib.import_module(PKG + ".synth"); abi = importlib.import_module(PKG + ".abi")
    pj = importlib.import_module(PKG + ".project")
    prob, meta = synth.make_scene(n_frames=a.frames, pts_per_frame=a.points, seed=1)
    x_gt = np.asarray(meta["x_gt"], np.float64)
    x_pred = np.asarray(a.pred, np.float64) if a.pred is not None else x_gt + np.array([0.017, -0.01, 0.012, 0.04, -0.03, 0.05, 0.0])
    h = pkg.IbaHandle(prob, abi.reference_yaml_params())
    p = pj.run(h, np.stack([x_gt, x_pred]), [a.frame, a.frame], splat=a.splat)
    W, H = p.size(0)
    img = background(W, H)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    for job, tag in ((0, "gt"), (1, "pred")):
        c = p.counts(job)
        print("%s: %s" % (tag, c))
        print("  overlay   ->", save("%s_%s" % (a.out, tag), p.overlay(job, img)))
        depth = p.depth(job)
        np.save("%s_%s_depth.npy" % (a.out, tag), depth)
        np.save("%s_%s_point_rgb.npy" % (a.out, tag), p.colorize(job, img))
        print("  depth     -> %s_%s_depth.npy (%d of %d pixels hold a depth)" % (a.out, tag, c["n_pixels"], W * H))
        print("  colours   -> %s_%s_point_rgb.npy (%d of %d points visible)" % (a.out, tag, c["n_visible"], c["n_points"]))
    p.close(); h.close()


if __name__ == "__main__":
    main()

"""GPU tier of the scan-to-image projection (include/iba_mi355x.h, iba_project_*): every product of every job — pixel doubles, z32, flags, the depth and
index images, the counts, the colours, the overlay — BYTE FOR BYTE against the numpy restatement tests/project_ref.py, which is fed the pose
iba_projection_pose returns. No tolerance anywhere: minima and integer counts do not depend on arrival order, and the quotients are the IEEE ones
(tests/test_gpu_division.py). Small images on purpose: 40 x 24 pixels under up to 4097 points is all occlusion."""
import importlib

import numpy as np
import pytest

import project_ref as R

pytestmark = pytest.mark.gpu
PKG = "spatial-temporal-lidar-camera-calibration_amd"
CAM = (32.0, 24.0, 16.0, 12.0, 40.0, 24.0)   # fx != fy; with the identity pose u = (32 X + 16 Z) / Z
SIZES = (0, 1, 300, 4097)                    # 4097 crosses a 4096-point slice; iba_create permutes every frame into kd-leaf order
# the identity (exact image borders), a small and a larger motion
XS = np.array([[0, 0, 0, 0, 0, 0, 1.0], [0.02, -0.03, 0.01, 0.05, -0.04, 0.1, 1.0], [-0.3, 0.2, 0.4, -0.5, 0.3, 1.0, 2.5]])


@pytest.fixture(scope="module")
def pj(pkg):
    return importlib.import_module(PKG + ".project")


def _scan(n, seed):
    """n points in front of the camera, a third of them outside the image; from 300 points on with the planted cases at seeded positions"""
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 30.0, n)
    pts = np.stack([rng.uniform(-0.9, 1.0, n) * z, rng.uniform(-0.8, 0.8, n) * z, z], axis=1).astype(np.float32)
    if n >= 300:
        at = rng.permutation(n)[:24]
        pts[at[0]] = (np.nan, 0, 2); pts[at[1]] = (1, np.inf, 3)                         # non-finite
        pts[at[2]] = (0.3, 0.2, -4); pts[at[3]] = (0, 0, -0.5); pts[at[4]] = (0, 0, 0)   # behind the camera, and in its centre
        pts[at[5]] = (0.1, 0.1, 0.05); pts[at[6]] = (1, 1, 150)                          # outside the depth range
        pts[at[7]] = pts[at[8]] = pts[at[9]] = (0.26, 0.13, 1.0)                         # duplicates: equal z32 in one pixel, in front of everything there
        pts[at[10]] = pts[at[11]] = (-0.4, 0.3, 0.75)
        # the image border under the identity pose: u = 0 and v = 0 exactly (inside), u = W and v = H exactly (outside), the corner pixels
        pts[at[12]] = (-1, 0, 2); pts[at[13]] = (1.5, 0, 2); pts[at[14]] = (0, -1, 2); pts[at[15]] = (0, 1, 2)
        pts[at[16]] = (-1, -1, 2); pts[at[17]] = (np.nextafter(np.float32(1.5), np.float32(0)), np.nextafter(np.float32(1), np.float32(0)), 2)
        pts[at[18]] = (-1, np.nextafter(np.float32(1), np.float32(0)), 2); pts[at[19]] = (np.nextafter(np.float32(1.5), np.float32(0)), -1, 2)
    return pts


@pytest.fixture(scope="module")
def scans():
    return [_scan(n, 100 + i) for i, n in enumerate(SIZES)]


@pytest.fixture(scope="module")
def handle(pkg, abi, scans):
    h = pkg.IbaHandle(abi.Problem.from_scans(scans, intr=CAM), device=0)
    yield h
    h.close()


def _ref(p, job, pts, camera, o):
    return R.project(pts, p.pose(job), camera, splat=o.splat, occlusion_tol=o.occlusion_tol, z_min=o.z_min, z_max=o.z_max, v_focal_is_fx=o.v_focal_is_fx)


def _same_bytes(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero(a.reshape(-1).view(np.uint8) != b.reshape(-1).view(np.uint8))
        raise AssertionError((what, "first differing byte", int(bad[0]), "of", a.nbytes, "differing", len(bad)))


def _check_job(p, job, pts, camera, o, img=None):
    """every product of one job against the restatement; -> the restatement's result"""
    ref = _ref(p, job, pts, camera, o)
    uv, z, fl = p.points(job)
    assert p.size(job) == (int(camera[4]), int(camera[5]))
    _same_bytes(uv, ref["uv"], "uv"); _same_bytes(z, ref["z"], "z32"); _same_bytes(fl, ref["flags"], "flags")
    _same_bytes(p.depth(job), ref["depth"], "depth"); _same_bytes(p.index(job), ref["index"], "index")
    assert p.counts(job) == ref["counts"]
    _same_bytes(p.overlay(job, None), R.overlay(ref, None, o.z_near, o.z_far), "overlay on black")
    if img is not None:
        _same_bytes(p.colorize(job, img), R.colorize(ref, img), "colours")
        _same_bytes(p.overlay(job, img), R.overlay(ref, img, o.z_near, o.z_far), "overlay")
    return ref


def _products(p, job):
    return [a.tobytes() for a in p.points(job)] + [p.depth(job).tobytes(), p.index(job).tobytes(), repr(sorted(p.counts(job).items())).encode(), p.pose(job).tobytes()]


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(7).integers(0, 256, (24, 40, 3), dtype=np.uint8)


@pytest.mark.parametrize("splat", [0, 1, 2, 4])
def test_ragged_frames(pj, handle, scans, image, splat):
    o = pj.project_options(splat=splat)
    frames = [0, 1, 2, 3, 2, 3]
    p = pj.run(handle, XS[[0, 0, 0, 0, 1, 1]], frames, o)
    try:
        assert len(p) == 6
        seen = dict(skipped=0, behind=0, ties=0, hidden=0)
        for job, f in enumerate(frames):
            ref = _check_job(p, job, scans[f], CAM, o, image)
            c = ref["counts"]
            seen["skipped"] += c["n_skipped"]; seen["behind"] += c["n_points"] - c["n_skipped"] - c["n_in_front"]; seen["hidden"] += c["n_inside"] - c["n_visible"]
            ins = np.flatnonzero(ref["flags"] & R.INSIDE)
            keys = np.stack([np.floor(ref["uv"][ins, 0]), np.floor(ref["uv"][ins, 1]), ref["z"][ins].astype(np.float64)], axis=1)
            seen["ties"] += len(keys) - len(np.unique(keys, axis=0))
        assert min(seen.values()) > 0, seen   # the planted cases are in play
        # the identity pose puts the planted border points exactly on the border: the corner pixels hold points, u = W is outside
        uv, _, fl = p.points(3)
        assert ((uv[:, 0] == 0.0) & (fl & R.INSIDE > 0)).any() and ((uv[:, 0] == 40.0) & (fl & R.INSIDE == 0) & (fl & R.IN_FRONT > 0)).any()
        assert ((uv[:, 1] == 0.0) & (fl & R.INSIDE > 0)).any() and ((uv[:, 1] == 24.0) & (fl & R.INSIDE == 0) & (fl & R.IN_FRONT > 0)).any()
    finally:
        p.close()


def test_jobs_chunks_and_repeatability(pj, handle, scans, monkeypatch):
    o = pj.project_options(splat=1)
    frames9 = [1, 2, 3] * 3
    x9 = np.repeat(XS, 3, axis=0)
    one = pj.run(handle, x9[4:5], frames9[4:5], o)
    nine = pj.run(handle, x9, frames9, o)
    again = pj.run(handle, x9, frames9, o)
    # 16 bytes per pixel and job: two 40 x 24 jobs per chunk, so the nine jobs run as five chunks
    monkeypatch.setenv("IBA_PROJECT_BUDGET", str(2 * 16 * 40 * 24))
    split = pj.run(handle, x9, frames9, o)
    monkeypatch.setenv("IBA_PROJECT_BUDGET", "1")   # less than one job: a chunk still holds one
    single = pj.run(handle, x9, frames9, o)
    monkeypatch.delenv("IBA_PROJECT_BUDGET")
    try:
        assert (len(one), len(nine), one.n_chunks, nine.n_chunks, split.n_chunks, single.n_chunks) == (1, 9, 1, 1, 5, 9)
        for job, f in enumerate(frames9):
            _check_job(nine, job, scans[f], CAM, o)
            want = _products(nine, job)
            assert _products(again, job) == want and _products(split, job) == want and _products(single, job) == want
        assert _products(one, 0) == _products(nine, 4)
        img = np.random.default_rng(11).integers(0, 256, (24, 40, 3), dtype=np.uint8)
        assert split.colorize(8, img).tobytes() == nine.colorize(8, img).tobytes() and split.overlay(8, img).tobytes() == nine.overlay(8, img).tobytes()
        with pytest.raises(Exception, match="job 9 is outside the result's 9 jobs") as e:
            nine.depth(9)
        assert e.value.status == 1
    finally:
        for p in (one, nine, again, split, single):
            p.close()


@pytest.fixture(scope="module")
def scene(pkg, synth, abi):
    """three keyframes with keypoints, fy set apart from fx (the evaluator forms v with fx: iba_global.cpp:73)"""
    prob, meta = synth.make_scene(n_frames=3, pts_per_frame=2000, seed=5, intr=dict(synth.KITTI00, fy=700.0))
    h = pkg.IbaHandle(prob, abi.reference_yaml_params(), device=0)
    yield prob, meta, h
    h.close()


@pytest.mark.parametrize("v_focal_is_fx", [0, 1])
def test_v_focal_option_and_the_evaluators_projection(pj, scene, v_focal_is_fx):
    prob, meta, h = scene
    cam = tuple(prob.arrays["intrinsics"][:6])
    assert cam[0] != cam[1]
    x = meta["x_gt"]
    # the evaluator keeps every point with a positive depth: a depth range that excludes none of them
    o = pj.project_options(splat=0, v_focal_is_fx=v_focal_is_fx, z_min=1e-9, z_max=1e9)
    p = pj.run(h, np.tile(x, (3, 1)), [0, 1, 2], o)
    try:
        n_pairs = 0
        for f in range(3):
            _check_job(p, f, prob.frame_points(f), cam, o)
            if not v_focal_is_fx:
                continue
            uv, _, fl = p.points(f)
            kp, pt = h.correspondences(x, f)
            kuv = prob.frame_keypoints(f).astype(np.float64)[kp]
            assert (fl[pt] & R.INSIDE).all()
            du, dv = uv[pt, 0] - kuv[:, 0], uv[pt, 1] - kuv[:, 1]
            assert (du * du + dv * dv <= h.params.max_pixel_dist * h.params.max_pixel_dist).all()
            n_pairs += len(kp)
        assert n_pairs > 50 or not v_focal_is_fx
    finally:
        p.close()


def test_camera_override_renders_a_scans_only_handle(pj, handle, scans):
    sub = handle.submap_handle([([2], [np.eye(4)], None, 0.5), ([3], [np.eye(4)], None, 0.5)])
    try:
        with pytest.raises(Exception, match="frame 1 has no intrinsics") as e:
            pj.run(sub, XS[:1], [1])
        assert e.value.status == 1
        o = pj.project_options(splat=2, camera=CAM)
        p = pj.run(sub, XS[[1, 2]], [0, 1], o)
        try:
            for job in range(2):
                idx = sub.debug_scan_index(job)
                pts = np.zeros((len(idx["perm"]), 3), np.float32)
                pts[idx["perm"]] = idx["xyz_tree"].T   # the voxel cloud in its original (voxel) order
                assert len(pts) > 50
                _check_job(p, job, pts, CAM, o)
        finally:
            p.close()
    finally:
        sub.close()


def test_colours_without_a_visible_point(pj, handle, scans, image):
    o = pj.project_options(z_min=200.0, z_max=300.0)   # nothing is in front
    p = pj.run(handle, XS[:1], [2], o)
    try:
        ref = _check_job(p, 0, scans[2], CAM, o, image)
        assert ref["counts"]["n_visible"] == 0 and ref["counts"]["n_pixels"] == 0
        assert not p.colorize(0, image).any() and p.overlay(0, image).tobytes() == image.tobytes() and not p.overlay(0, None).any()
    finally:
        p.close()

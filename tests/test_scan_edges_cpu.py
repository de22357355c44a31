"""CPU tier of the scan-to-scan edges (iba_scan_*, include/iba_mi355x.h): symbols, struct layouts and the ABI version through the ctypes
mirror, the numpy restatement tests/scan_ref.py against known answers, and the argument errors that are answered without a device."""
import ctypes as C
import re

import numpy as np
import pytest

import icp_ref as R
import scan_ref as S

NAMES = ("iba_default_scan_options", "iba_scan_step", "iba_scan_register", "iba_scan_information")


# ---- 1. the boundary: these fail before the feature exists ----
def test_scan_symbols_are_declared_and_exported_and_the_abi_is_4(pkg):
    pkg.build_extension()
    lib = pkg.load_library()
    hdr = open(pkg.HEADER_PATH).read()
    declared = set(re.findall(r"\b(iba_[a-z_0-9]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, n
        assert getattr(lib, n) is not None, n
    assert int(re.search(r"#define IBA_ABI_VERSION (\d+)", hdr).group(1)) == pkg.ABI_VERSION == lib.iba_abi_version() == 4
    assert int(re.search(r"#define IBA_SCAN_NMOM (\d+)", hdr).group(1)) == 32
    for name, v in (("POINT_TO_POINT", 0), ("POINT_TO_PLANE", 1), ("INFORMATION", 2)):
        assert int(re.search(r"#define IBA_SCAN_%s (\d+)" % name, hdr).group(1)) == v


def test_scan_struct_layouts_match_the_library(pkg, abi):
    lib = pkg.load_library()
    o = abi.IbaScanOptions()
    assert lib.iba_default_scan_options(C.byref(o)) == 0
    assert o.struct_size == C.sizeof(abi.IbaScanOptions) == 80   # 2 x i32, f64, i32 + pad, 3 x f64, i32 + pad, 3 x f64: ten 8-byte slots
    assert (o.estimation, o.coarse_dist, o.coarse_max_iter, o.coarse_rel_fitness, o.coarse_rel_rmse) == (0, 0.0, 30, 1e-4, 1e-4)
    assert (o.refine_dist, o.refine_max_iter, o.refine_rel_fitness, o.refine_rel_rmse, o.info_dist) == (0.3, 30, 1e-6, 1e-6, 0.0)
    assert C.sizeof(abi.IbaScanEdge) == 8 + 128 and abi.IbaScanEdge.T.offset == 8
    assert C.sizeof(abi.IbaScanResult) == 168 + 8 + 288 + 8
    assert (abi.IbaScanResult.n_planar.offset, abi.IbaScanResult.info.offset, abi.IbaScanResult.n_info.offset) == (168, 176, 464)
    assert abi.SCAN_NMOM == 32 and (abi.SCAN_POINT_TO_POINT, abi.SCAN_POINT_TO_PLANE, abi.SCAN_INFORMATION) == (0, 1, 2)
    assert lib.iba_default_scan_options(None) == 1


# ---- 3. argument errors answered before a device is touched (a handle needs a device: what runs here is the NULL handle) ----
def test_null_handle_is_refused_by_every_entry_point(pkg, abi):
    lib = pkg.load_library()
    e = (abi.IbaScanEdge * 1)()
    mom = np.zeros(32); info = np.zeros(36); n = np.zeros(1, np.int32)
    lib.iba_scan_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_int32, C.c_void_p, C.c_void_p]
    lib.iba_scan_register.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.iba_scan_information.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]
    assert lib.iba_scan_step(None, e, 1, C.c_double(1.0), 0, mom.ctypes.data_as(C.c_void_p), None) == 1
    o = abi.IbaScanOptions(); lib.iba_default_scan_options(C.byref(o)); out = (abi.IbaScanResult * 1)()
    assert lib.iba_scan_register(None, e, 1, C.byref(o), out) == 1
    assert lib.iba_scan_information(None, e, 1, C.c_double(1.0), info.ctypes.data_as(C.c_void_p), n.ctypes.data_as(C.c_void_p)) == 1


# ---- 2. the restatement against known answers ----
def test_vec6_to_mat4_is_scipys_extrinsic_xyz():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(0)
    for _ in range(20):
        x = np.r_[rng.uniform(-1.5, 1.5, 3), rng.uniform(-5, 5, 3)]
        U = S.vec6_to_mat4(x)
        assert np.max(np.abs(U[:3, :3] - Rotation.from_euler("xyz", x[:3]).as_matrix())) <= 1e-15 * 4
        assert np.array_equal(U[:3, 3], x[3:]) and np.array_equal(U[3], [0, 0, 0, 1])
    if R.have_longdouble():
        assert S.vec6_to_mat4(x, np.longdouble).dtype == np.longdouble


def _three_planes(rng, n=600):
    """points on three mutually non-parallel planes with their true normals"""
    nrm = np.array([[0, 0, 1.0], [0, 1.0, 0], [0.6, 0, 0.8]])
    pts, ns = [], []
    for k in range(3):
        a = np.linalg.svd(nrm[k][None])[2][1:]        # a basis of the plane
        uv = rng.uniform(-10, 10, (n // 3, 2))
        pts.append(uv @ a + nrm[k] * (k + 1.0)); ns.append(np.tile(nrm[k], (n // 3, 1)))
    return np.concatenate(pts), np.concatenate(ns)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_one_point_to_plane_step_recovers_a_small_planted_motion_to_first_order(dtype):
    rng = np.random.default_rng(1)
    p, n = _three_planes(rng)
    x = np.array([2e-4, -1e-4, 3e-4, 2e-3, -1e-3, 1.5e-3])
    M = S.vec6_to_mat4(x)                              # the motion that takes the source onto the target
    Mi = np.linalg.inv(M)
    src = p @ Mi[:3, :3].T + Mi[:3, 3]                 # exact partners: pair i is (src_i, p_i)
    m = S.p2l_sums(src, p, n, np.ones(len(p), bool), R.d2_of(src, p), dtype)
    assert m[0] == m[2] == len(p) and m.dtype == dtype
    U = np.asarray(S.p2l_update(m), np.float64)
    assert np.max(np.abs(U - M)) <= 5 * np.max(np.abs(x)) ** 2       # first order: the error is of the order of |x|^2
    # the sums are what their definitions say (one pair at a time, independent code)
    q = src; r = ((q - p) * n).sum(1); J = np.c_[np.cross(q, n), n]
    A = J.T @ J; b = J.T @ r
    got = np.zeros((6, 6)); o = 3
    for i in range(6):
        for j in range(i, 6):
            got[i, j] = got[j, i] = float(m[o]); o += 1
    assert np.max(np.abs(got - A)) <= 1e-12 * np.max(np.abs(A)) and np.max(np.abs(np.asarray(m[24:30], np.float64) - b)) <= 1e-12 * max(np.max(np.abs(b)), 1e-300) + 1e-15
    assert abs(float(m[30]) - (r * r).sum()) <= 1e-12 * (r * r).sum()


def test_the_point_to_plane_loop_recovers_the_planted_motion_to_rounding():
    rng = np.random.default_rng(2)
    tgt, n = _three_planes(rng, 900)
    tgt = tgt.astype(np.float32).astype(np.float64)
    # the normals of the rounded points' planes are still the true ones to 1e-7; the source is an exact rigid image of a target subset
    M = S.rigid([1e-3, -2e-3, 1.5e-3], [0.01, -0.02, 0.015])
    pick = rng.choice(len(tgt), 300, replace=False)
    Mi = np.linalg.inv(M)
    src = tgt[pick] @ Mi[:3, :3].T + Mi[:3, 3]
    r = S.register(src, tgt, np.eye(4), 0.5, S.P2L, normals=n, has=np.ones(len(tgt), bool), brute=True)
    assert r["converged"] == 1 and r["n_corr"] == r["n_planar"] == 300 and r["iterations"] <= 6
    assert np.max(np.abs(r["T"] - M)) <= 1e-9
    # point-to-point on the same data lands on it too
    r0 = S.register(src, tgt, np.eye(4), 0.5, S.P2P, brute=True)
    assert r0["converged"] == 1 and np.max(np.abs(r0["T"] - M)) <= 1e-9
    # parallel planes only: no update is defined
    flat = np.c_[rng.uniform(-5, 5, (200, 2)), np.zeros(200)]
    nz = np.tile([0, 0, 1.0], (200, 1))
    rf = S.register(flat + [0, 0, 0.01], flat, np.eye(4), 0.5, S.P2L, normals=nz, has=np.ones(200, bool), brute=True)
    assert rf["converged"] == -1 and rf["iterations"] == 0
    # fewer than 6 pairs with a normal: none either; the pairs still count
    has = np.zeros(len(tgt), bool); has[pick[:5]] = True
    rn = S.register(src, tgt, np.eye(4), 0.5, S.P2L, normals=n, has=has, brute=True)
    assert rn["converged"] == -1 and rn["n_corr"] == 300 and rn["n_planar"] == 5


def test_information_matrix_of_a_hand_written_three_point_set():
    t = np.array([[1.0, 0, 0], [0, 2.0, 0], [0, 0, 3.0]])
    want = np.array([[13, 0, 0, 0, -3, 2],
                     [0, 10, 0, 3, 0, -1],
                     [0, 0, 5, -2, 1, 0],
                     [0, 3, -2, 3, 0, 0],
                     [-3, 0, 1, 0, 3, 0],
                     [2, -1, 0, 0, 0, 3.0]])
    assert np.array_equal(S.info_from_sums(S.info_sums(t)), want)
    assert np.array_equal(S.information(t), want)
    rng = np.random.default_rng(3)
    t = rng.normal(size=(500, 3)) * [20, 8, 2]
    a, b = S.info_from_sums(S.info_sums(t)), S.information(t)
    assert np.array_equal(a, a.T) and np.max(np.abs(a - b)) <= 1e-12 * np.max(np.abs(b))
    if R.have_longdouble():
        c = S.info_from_sums(S.info_sums(t, np.longdouble))
        assert c.dtype == np.longdouble and np.max(np.abs(np.asarray(c, np.float64) - a)) <= 1e-12 * np.max(np.abs(a))


def test_ldlt_solves_and_refuses():
    rng = np.random.default_rng(4)
    B = rng.normal(size=(40, 6)); A = B.T @ B; b = rng.normal(size=6)
    x = S.ldlt6_solve(A, b)
    assert np.max(np.abs(x - np.linalg.solve(A, b))) <= 1e-12 * np.max(np.abs(x))
    B[:, 2] = 0.0
    assert S.ldlt6_solve(B.T @ B, b) is None                       # an exactly singular system
    B[:, 2] = B[:, 0] * (1 + 1e-15)
    assert S.ldlt6_solve(B.T @ B, b) is None                       # singular to working precision: the pivot rule


def test_two_stage_restatement_chains_the_stages():
    src, tgt, T = S.room_pair(5, n=1500)
    T0 = S.perturb_rigid(T, np.random.default_rng(6))
    c = dict(gate=1.0, max_iter=3, rel_fitness=1e-4, rel_rmse=1e-4); f = dict(gate=0.3, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6)
    two = S.register_two_stage(src, tgt, T0, c, f, brute=True)
    a = S.register(src, tgt, T0, 1.0, max_iter=3, rel_fitness=1e-4, rel_rmse=1e-4, brute=True)
    b = S.register(src, tgt, a["T"], 0.3, brute=True)
    assert np.array_equal(two["T"], b["T"]) and two["iterations"] == b["iterations"]
    # the reference's call as written: 1 coarse iteration, 0 refine iterations -> the refine stage only evaluates
    lit = S.register_two_stage(src, tgt, T0, dict(c, max_iter=1), dict(f, max_iter=0), brute=True)
    one = S.register(src, tgt, T0, 1.0, max_iter=1, rel_fitness=1e-4, rel_rmse=1e-4, brute=True)
    assert np.array_equal(lit["T"], one["T"]) and lit["iterations"] == 0 and lit["converged"] == 0

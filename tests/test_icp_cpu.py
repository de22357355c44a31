"""CPU tier of the ICP driver (iba_icp_*, include/iba_mi355x.h): the numpy restatement tests/icp_ref.py against known answers, and the new entry
points' symbols and struct layouts through the ctypes mirror (no GPU)."""
import ctypes as C
import re

import numpy as np
import pytest

import icp_ref as R


def _similarity(rng, c=None, reflect=False):
    w = rng.normal(size=3); w *= rng.uniform(0.2, 2.5) / np.linalg.norm(w)
    Rm = R.rotvec(w)
    if reflect:
        Rm = Rm @ np.diag([1.0, 1.0, -1.0])
    return (rng.uniform(0.2, 12.0) if c is None else c), Rm, rng.uniform(-20, 20, 3)


@pytest.mark.parametrize("dtype", [np.float64, np.longdouble])
def test_umeyama_recovers_a_planted_similarity_in_one_step(dtype):
    rng = np.random.default_rng(0)
    for _ in range(5):
        c, Rm, t = _similarity(rng)
        q = rng.normal(size=(200, 3)) * [10, 4, 1]
        p = c * q @ Rm.T + t
        info = {}
        T = R.umeyama(q, p, True, dtype, info)
        assert not info["reflect"] and abs(info["c"] - c) <= 1e-12 * c
        assert np.max(np.abs(np.asarray(T[:3, :3], np.float64) - c * Rm)) <= 1e-11 * c and np.max(np.abs(np.asarray(T[:3, 3], np.float64) - t)) <= 1e-10
        assert T.dtype == dtype


def test_source_that_is_a_similarity_image_of_a_target_subset_registers_in_one_iteration():
    rng = np.random.default_rng(1)
    tgt = (rng.normal(size=(3000, 3)) * [15, 6, 1.2]).astype(np.float32)
    c, Rm, t = _similarity(rng, c=9.7)
    pick = rng.choice(len(tgt), 400, replace=False)
    src = (tgt[pick].astype(np.float64) - t) @ Rm / c
    Tp = np.eye(4); Tp[:3, :3] = c * Rm; Tp[:3, 3] = t
    T0 = R.perturb(Tp, rng, rot=(1e-4, 2e-4), trans=(1e-3, 2e-3), scale=1e-4)   # near enough that every nearest neighbour is the planted one
    r = R.register(src, tgt, T0, gate=0.5, max_iter=5)
    assert r["counts"][0] == 400 and r["converged"] == 1 and r["iterations"] <= 2
    assert np.max(np.abs(r["T"] - Tp)) <= 1e-9
    one = R.evaluate(T0, src, tgt, 0.5)
    assert np.array_equal(one["idx"], pick)
    U = R.umeyama(one["q"], tgt[one["idx"]].astype(np.float64))
    assert np.max(np.abs(U @ T0 - Tp)) <= 1e-9   # ONE Umeyama step lands on the planted transform


def test_reflection_takes_the_S_branch():
    rng = np.random.default_rng(2)
    c, Rm, t = _similarity(rng, reflect=True)
    q = rng.normal(size=(100, 3)) * [5, 3, 0.05]   # nearly planar: the reflected fit is almost as good, Umeyama must still return a rotation
    p = c * q @ Rm.T + t
    info = {}
    T = R.umeyama(q, p, True, np.float64, info)
    assert info["reflect"]
    A = T[:3, :3] / info["c"]
    assert abs(np.linalg.det(A) - 1.0) <= 1e-12 and np.max(np.abs(A @ A.T - np.eye(3))) <= 1e-12
    if R.have_longdouble():
        info2 = {}
        T2 = R.umeyama(q, p, True, np.longdouble, info2)
        assert info2["reflect"] and np.max(np.abs(np.asarray(T2, np.float64) - T)) <= 1e-10 * max(1.0, np.max(np.abs(T)))


def test_without_scaling_c_is_one():
    rng = np.random.default_rng(3)
    c, Rm, t = _similarity(rng, c=3.0)
    q = rng.normal(size=(50, 3)); p = c * q @ Rm.T + t
    info = {}
    T = R.umeyama(q, p, False, np.float64, info)
    assert info["c"] == 1.0 and np.max(np.abs(T[:3, :3] - Rm)) <= 1e-12


def test_icp_calib_conventions_round_trip():
    rng = np.random.default_rng(4)
    c, Rm, t = _similarity(rng, c=9.7)
    rigid = np.c_[Rm, t]
    T = R.init_from_sim3(rigid, c)
    assert np.allclose(T[:3, :3], c * Rm.T, rtol=0, atol=1e-13) and np.allclose(T[:3, 3], -Rm.T @ t, rtol=0, atol=1e-12)
    back, s = R.sim3_from_result(T)
    assert abs(s - c) <= 1e-13 * c and np.max(np.abs(back - rigid)) <= 1e-12


def test_moments_longdouble_twin_and_guard():
    if not R.have_longdouble():
        pytest.skip("np.longdouble carries no more than a double here")
    assert np.finfo(np.longdouble).nmant >= 63
    rng = np.random.default_rng(5)
    q = rng.normal(size=(1000, 3)) * 20; p = q + rng.normal(0, 0.02, (1000, 3))
    a, b = R.moments(q, p, R.d2_of(q, p), q.mean(0)), R.moments(q, p, R.d2_of(q, p), q.mean(0), np.longdouble)
    assert b.dtype == np.longdouble and a[0] == b[0] == 1000
    big = np.max(np.abs(a))
    assert np.max(np.abs(a - np.asarray(b, np.float64))) <= 1e-12 * big


def test_canyon_scene_meets_the_margin_condition_of_the_loop_test():
    """the inputs of the GPU loop test (tests/test_gpu_icp.py) are checked here too, without a device: the restatement converges, recovers the
    planted similarity to the noise level and stays clear of the gate and of nearest / second-nearest ties at every evaluation"""
    tgt, src, Tp = R.canyon(1)
    T0 = R.perturb(Tp, np.random.default_rng(101), scale=0.01)
    r = R.register(src, tgt, T0, gate=0.2, margins=True)
    assert r["converged"] == 1 and r["counts"][0] < 3000 and r["counts"][-1] == 3000
    assert r["gate_margin"] > 1e-9 and r["gap"] > 1e-9
    assert np.max(np.abs(r["T"] - Tp)) < 5e-3


# ---- the new entry points through the ctypes mirror: these fail before the feature exists ----
def test_icp_symbols_are_declared_and_exported(pkg):
    pkg.build_extension()
    lib = pkg.load_library()
    hdr = open(pkg.HEADER_PATH).read()
    declared = set(re.findall(r"\b(iba_[a-z_0-9]+)\s*\(", hdr))
    for n in ("iba_default_icp_options", "iba_icp_step", "iba_icp_register", "iba_icp_calib"):
        assert n in declared, n
        assert getattr(lib, n) is not None, n
    assert int(re.search(r"#define IBA_ABI_VERSION (\d+)", hdr).group(1)) == pkg.ABI_VERSION == lib.iba_abi_version() >= 3
    assert int(re.search(r"#define IBA_ICP_NMOM (\d+)", hdr).group(1)) == 21


def test_icp_struct_layouts_match_header(pkg, abi):
    lib = pkg.load_library()
    o = abi.IbaIcpOptions()
    assert lib.iba_default_icp_options(C.byref(o)) == 0
    assert o.struct_size == C.sizeof(abi.IbaIcpOptions) == 48   # the library's sizeof(iba_icp_options): i32, pad, f64, i32, pad, f64, f64, i32, pad
    assert (o.max_corr_dist, o.max_iter, o.relative_fitness, o.relative_rmse, o.with_scaling) == (1.0, 30, 1e-6, 1e-6, 1)
    assert C.sizeof(abi.IbaIcpResult) == 16 * 8 + 3 * 8 + 3 * 4 + 4 and abi.IbaIcpResult.scale.offset == 128 and abi.IbaIcpResult.n_corr.offset == 152
    assert abi.ICP_NMOM == 21 and (abi.ICP_CONVERGED, abi.ICP_MAX_ITER, abi.ICP_DEGENERATE) == (1, 0, -1)
    assert lib.iba_default_icp_options(None) == 1
    # a NULL handle is refused before anything touches a device
    lib.iba_icp_step.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.iba_icp_step(None, 0, 1, None, 0, None, 1, C.c_double(1.0), None, None, None) == 1

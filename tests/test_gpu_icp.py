"""GPU tier of the ICP driver, each test through the C ABI (iba_icp_step / iba_icp_register / iba_icp_calib, include/iba_mi355x.h):
sets bit-exact against iba_geo_correspondences, moments against a long-double restatement, tiles, batch invariance byte for byte, the whole
loop against tests/icp_ref.py, recovery of a planted similarity, edges. Figures are printed before they are asserted; with
IBA_ICP_PARITY_OUT=<file> they are also appended there as JSON lines (profiles/icp_parity.md quotes such a run)."""
import json
import os

import numpy as np
import pytest

import icp_ref as R
from parity_gate import check_entries_vs_truth
from test_geo_correspondences import GOLD, CASES, _case, scan_120k_case

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
I4 = np.eye(4)


def _note(**kw):
    print("icp-figures", json.dumps(kw))
    p = os.environ.get("IBA_ICP_PARITY_OUT")
    if p:
        with open(p, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _handle(pkg, abi, tiles):
    return pkg.IbaHandle(abi.Problem.from_scans([np.asarray(t, np.float32).reshape(-1, 3) for t in tiles]), abi.reference_yaml_params())


def _check_moments(m_dev, q, p, d2, what):
    """test 2's bar: every moment within 1e-10 of the long-double restatement, or no further from it than 1.5 x the f64 restatement's own distance
    (tests/parity_gate.py: entries above 1e-6 of the largest relative to themselves, the others to the largest); the pivot entries exactly."""
    if not R.have_longdouble():
        pytest.skip("np.longdouble carries no more than a double here")
    piv = m_dev[18:21]
    t = R.moments(q, p, d2, piv, np.longdouble)
    o = R.moments(q, p, d2, piv, np.float64)
    assert m_dev[0] == len(q)
    ok, rep = check_entries_vs_truth(m_dev[1:18], o[1:18], np.asarray(t[1:18], np.float64))
    err_dev = np.abs(m_dev[1:18].astype(np.longdouble) - t[1:18]); err_o = np.abs(o[1:18].astype(np.longdouble) - t[1:18])
    ratio = float(np.max(err_dev / np.maximum(err_o, np.finfo(np.float64).tiny))) if len(q) else 0.0
    _note(test="moments", what=what, n=len(q), device=rep["device"], f64=rep["oracle"], bar=rep["bar"], worst_ratio_device_over_f64=ratio)
    assert ok, (what, rep)
    return rep


def test_one_pass_sets_equal_geo_correspondences_and_moments_hold(pkg, abi):
    z = np.load(GOLD)
    cases = [(name,) + tuple(_case(z, name)[:3]) for name in CASES] + [("scan120k",) + tuple(scan_120k_case())]
    for name, src, tgt, md in cases:
        src = np.asarray(src, np.float64).reshape(-1, 3); tgt32 = np.asarray(tgt, np.float32).reshape(-1, 3)
        h = _handle(pkg, abi, [tgt32])
        gs, gt = h.geo_correspondences(0, src, md)
        gate = float(np.sqrt(md))
        if name == "scan_exact":   # d^2 = 0 = max_distance: kept by <=, not by <. A strictly positive gate keeps exactly those pairs instead
            assert md == 0.0
            gate = 1e-12
        if len(src) == 0:
            m = h.icp_step(src, I4, 1.0)
            assert np.all(m == 0.0)
            h.close()
            continue
        m, pf, pi = h.icp_step(src, I4, gate, pairs=True)
        kept = np.nonzero(pi[0] != NONE)[0]
        d2 = R.d2_of(src[kept], tgt32[pi[0][kept]].astype(np.float64))
        if name != "scan_exact":   # no fixture pair sits on the gate: < and <= agree
            idx_all, d2_all = R.nearest(src, tgt32, brute=len(src) * len(tgt32) <= 4_000_000)
            assert not np.any(d2_all == md) and not np.any(d2_all == gate * gate), name
        assert np.array_equal(kept, gs) and np.array_equal(pi[0][kept], gt), (name, len(kept), len(gs))
        assert np.all(pf[0][kept] == 0) and np.all(pf[0][pi[0] == NONE] == NONE)
        assert np.all(d2 < gate * gate)
        _check_moments(m[0], src[kept], tgt32[pi[0][kept]].astype(np.float64), d2, name)
        m2 = h.icp_step(src, I4, gate)   # without the pair output: the same bytes
        assert m2.tobytes() == m.tobytes()
        h.close()


def _tilings(tgt, rng):
    n = len(tgt)
    yield "one", [np.arange(n)]
    for k in (3, 7):
        lab = rng.integers(0, k, n)
        yield "random%d" % k, [np.nonzero(lab == i)[0] for i in range(k)]
        edges = np.quantile(tgt[:, 0], np.linspace(0, 1, k + 1)[1:-1])
        lab = np.searchsorted(edges, tgt[:, 0])
        yield "spatial%d" % k, [np.nonzero(lab == i)[0] for i in range(k)]


def test_tiles_give_the_same_sets_and_moments(pkg, abi):
    rng = np.random.default_rng(11)
    tgt = (rng.normal(size=(20000, 3)) * [15, 6, 1.2]).astype(np.float32)
    src = tgt[rng.integers(0, len(tgt), 2500)].astype(np.float64) + rng.normal(0, 0.2, (2500, 3))
    T = I4.copy(); T[:3, :3] = R.rotvec([0.0, 0.0, 1e-3]); T[:3, 3] = [0.01, -0.02, 0.005]
    gate = 0.3
    ref_pairs, ref_m = None, None
    for name, parts in _tilings(tgt, rng):
        h = _handle(pkg, abi, [tgt[p] for p in parts])
        m, pf, pi = h.icp_step(src, T, gate, frames=(0, len(parts)), pairs=True)
        h.close()
        kept = pi[0] != NONE
        glob = np.full(len(src), -1, np.int64)
        for f, p in enumerate(parts):
            sel = kept & (pf[0] == f)
            glob[sel] = p[pi[0][sel]]
        assert np.all(glob[kept] >= 0)
        if ref_pairs is None:
            ref_pairs, ref_m = glob, m[0]
            assert 500 < kept.sum() < len(src) - 100   # the gate bites
        assert np.array_equal(glob, ref_pairs), name
        q = R.transform(T, src)[kept]; p = tgt[glob[kept]].astype(np.float64)
        _check_moments(m[0], q, p, R.d2_of(q, p), "tiles:" + name)
        assert np.array_equal(m[0][18:21], ref_m[18:21])
    # duplicates across two tiles: the lower (frame, index) wins; an empty tile among the others changes nothing
    a = tgt[:4000]
    h = _handle(pkg, abi, [a, np.zeros((0, 3), np.float32), a[::-1].copy(), a[:10]])
    m, pf, pi = h.icp_step(src, T, gate, frames=(0, 4), pairs=True)
    kept = pi[0] != NONE
    assert kept.sum() > 100 and np.all(pf[0][kept] == 0)
    m1, pf1, pi1 = h.icp_step(src, T, gate, frames=(0, 1), pairs=True)
    assert np.array_equal(pi1, pi) and np.array_equal(m1[0][:2], m[0][:2])
    mr, pfr, pir = h.icp_step(src, T, gate, frames=(2, 4), pairs=True)   # the reversed copy first: frame 2, index mirrored
    assert np.array_equal(pfr[0][kept], np.full(kept.sum(), 2)) and np.array_equal(pir[0][kept], 3999 - pi[0][kept])
    h.close()


def _loop_case(seed, scale, gate):
    tgt, src, Tp = R.canyon(seed)
    return tgt, src, Tp, R.perturb(Tp, np.random.default_rng(100 + seed), scale=scale), gate


def _res_bytes(r):
    return bytes(r)


def test_batch_invariance_byte_for_byte(pkg, abi):
    tgt, src, Tp, T0, gate = _loop_case(1, 0.01, 0.2)
    rng = np.random.default_rng(5)
    others = [R.perturb(Tp, rng, scale=s) for s in rng.uniform(-0.01, 0.01, 63)]
    h = _handle(pkg, abi, [tgt])
    m1 = h.icp_step(src, T0, gate)
    m5 = h.icp_step(src, np.stack(others[:2] + [T0] + others[2:4]), gate)
    m64 = h.icp_step(src, np.stack(others[:40] + [T0] + others[40:]), gate)
    assert m1[0].tobytes() == m5[2].tobytes() == m64[40].tobytes()
    assert h.icp_step(src, T0, gate).tobytes() == m1.tobytes()
    r1 = h.icp_register(src, T0, max_corr_dist=gate)
    r1b = h.icp_register(src, T0, max_corr_dist=gate)
    r5 = h.icp_register(src, np.stack(others[:2] + [T0] + others[2:4]), max_corr_dist=gate)
    r64 = h.icp_register(src, np.stack(others[:40] + [T0] + others[40:]), max_corr_dist=gate)
    assert r1[0].converged == 1 and r1[0].iterations >= 3
    assert _res_bytes(r1[0]) == _res_bytes(r1b[0]) == _res_bytes(r5[2]) == _res_bytes(r64[40])
    assert len({r.iterations for r in r64}) > 1   # the starts really stop at different iterations: finished ones dropped out of the launches
    h.close()


# (scale error of the start, gate, seeds): the two configurations of the issue (0.3 % / 0.3 m, 1 % / 0.5 m) and one in which the gate bites on this
# scene generator (1 % / 0.2 m: 2.5 k of 3 k pairs at the start). The seeds were chosen on the CPU by the margin condition below, never by a device result.
LOOP_CASES = [(0.003, 0.3, (1, 2, 3)), (0.01, 0.5, (1, 2)), (0.01, 0.2, (1, 2))]


@pytest.mark.parametrize("scale,gate,seeds", LOOP_CASES)
def test_full_loop_against_the_restatement_and_recovery(pkg, abi, scale, gate, seeds):
    if not R.have_longdouble():
        pytest.skip("np.longdouble carries no more than a double here")
    for seed in seeds:
        tgt, src, Tp, T0, _ = _loop_case(seed, scale, gate)
        # the condition on the inputs, on the CPU, before the device result is looked at
        ref = R.register(src, tgt, T0, gate, margins=True)
        assert ref["gate_margin"] > 1e-9 and ref["gap"] > 1e-9, (seed, ref["gate_margin"], ref["gap"])
        truth = R.register(src, tgt, T0, gate, dtype=np.longdouble)
        assert truth["counts"] == ref["counts"] and truth["iterations"] == ref["iterations"]
        d_ref = float(np.max(np.abs(ref["T"].astype(np.longdouble) - truth["T"])))
        h = _handle(pkg, abi, [tgt])
        r = h.icp_register(src, T0, max_corr_dist=gate)[0]
        # the per-iteration kept-pair counts of the device: one pass at every transform the restatement went through is not available from the
        # loop itself, so the loop is replayed with max_iter = k (evaluation only at k = 0)
        counts = [h.icp_register(src, T0, max_corr_dist=gate, max_iter=k)[0].n_corr for k in range(ref["iterations"] + 1)]
        h.close()
        d_dev = float(np.max(np.abs(r.T_np().astype(np.longdouble) - truth["T"])))
        e_dev, e_ref = float(np.max(np.abs(r.T_np() - Tp))), float(np.max(np.abs(ref["T"] - Tp)))
        _note(test="loop", seed=seed, scale=scale, gate=gate, iterations=ref["iterations"], counts=ref["counts"], device_counts=counts, gate_margin=ref["gate_margin"], gap=ref["gap"],
              f64_from_longdouble=d_ref, device_from_longdouble=d_dev, device_err_planted=e_dev, f64_err_planted=e_ref)
        assert counts == ref["counts"]
        assert (r.iterations, r.n_corr, r.converged) == (ref["iterations"], ref["n_corr"], ref["converged"])
        assert d_dev <= 4.0 * d_ref, (seed, d_dev, d_ref)
        assert e_dev <= 1.01 * e_ref, (seed, e_dev, e_ref)      # recovery: no worse than the restatement on the same input
        assert abs(r.fitness - ref["fitness"]) <= 1e-15 and abs(r.inlier_rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]


def test_icp_calib_writes_a_sim3_that_reads_back(pkg, abi, tmp_path):
    import ctypes as C
    tgt, src, Tp, T0, gate = _loop_case(2, 0.003, 0.3)
    rigid0, s0 = R.sim3_from_result(T0)             # the start in readSim3 form
    h = _handle(pkg, abi, [tgt])
    rigid, s, res = h.icp_calib(src, rigid0, s0, max_corr_dist=gate)
    direct = h.icp_register(src, R.init_from_sim3(rigid0, s0), max_corr_dist=gate)[0]
    want_rigid, want_s = R.sim3_from_result(direct.T_np())
    assert res.converged == 1 and abs(s - want_s) <= 1e-11 * want_s and np.max(np.abs(rigid - want_rigid)) <= 1e-10
    planted_rigid, planted_s = R.sim3_from_result(Tp)
    assert abs(s - planted_s) < 2e-3 and np.max(np.abs(rigid - planted_rigid)) < 5e-3
    # re-referenced: the same cloud seen from another LiDAR pose, the queries moved instead of the scans
    P = np.eye(4); P[:3, :3] = R.rotvec([0.02, -0.01, 0.3]); P[:3, 3] = [1.5, -0.7, 0.2]
    tgt_w = (tgt.astype(np.float64) @ P[:3, :3].T + P[:3, 3]).astype(np.float32)   # the stored scans are in the world frame here ...
    hw = _handle(pkg, abi, [tgt_w])
    rigid_w, s_w, res_w = hw.icp_calib(src, rigid0, s0, ref_lidar_pose12=P[:3].ravel(), max_corr_dist=gate)   # ... and refpose brings the result back
    hw.close()
    assert res_w.converged == 1 and abs(s_w - s) < 1e-4 and np.max(np.abs(rigid_w - rigid)) < 1e-3   # (float32 rounding of the moved cloud, and a stop one iteration apart)
    lib = pkg.load_library()
    path = str(tmp_path / "icp_sim3.txt").encode()
    r12 = np.ascontiguousarray(rigid.ravel())
    lib.iba_write_sim3.argtypes = [C.c_char_p, C.c_void_p, C.c_double]
    lib.iba_read_sim3.argtypes = [C.c_char_p, C.c_void_p, C.POINTER(C.c_double)]
    assert lib.iba_write_sim3(path, r12.ctypes.data_as(C.c_void_p), C.c_double(s)) == 0
    back = np.zeros(12); sb = C.c_double(0)
    assert lib.iba_read_sim3(path, back.ctypes.data_as(C.c_void_p), C.byref(sb)) == 0
    assert np.array_equal(back, r12) and sb.value == s
    h.close()


def test_edges(pkg, abi):
    rng = np.random.default_rng(9)
    tgt = (rng.normal(size=(3000, 3)) * [10, 4, 1]).astype(np.float32)
    src = tgt[:500].astype(np.float64) + rng.normal(0, 0.05, (500, 3))
    h = _handle(pkg, abi, [tgt, np.zeros((0, 3), np.float32)])
    # n_src = 0
    assert np.all(h.icp_step(np.zeros((0, 3)), I4, 1.0) == 0.0)
    r = h.icp_register(np.zeros((0, 3)), I4)[0]
    assert (r.n_corr, r.iterations, r.converged) == (0, 0, -1) and np.array_equal(r.T_np(), I4)
    # an empty target tile alone: nothing is kept
    m = h.icp_step(src, I4, 1.0, frames=(1, 2))
    assert m[0][0] == 0 and np.all(np.isfinite(m))
    # a gate so small that nothing is kept: the defined status, no NaN, T unchanged
    T0 = I4.copy(); T0[:3, 3] = [0.01, 0.0, 0.0]
    r = h.icp_register(src, T0, max_corr_dist=1e-9)[0]
    assert (r.n_corr, r.iterations, r.converged) == (0, 0, -1) and np.array_equal(r.T_np(), T0)
    assert r.fitness == 0.0 and r.inlier_rmse == 0.0 and np.isfinite(r.scale)
    # max_iter = 0: evaluation only
    r = h.icp_register(src, T0, max_corr_dist=0.5, max_iter=0)[0]
    m = h.icp_step(src, T0, 0.5)
    assert (r.iterations, r.converged) == (0, 0) and r.n_corr == int(m[0][0]) > 400 and np.array_equal(r.T_np(), T0)
    assert r.inlier_rmse == np.sqrt(m[0][1] / m[0][0])
    # rigid: c stays 1
    r = h.icp_register(src, T0, max_corr_dist=0.5, with_scaling=0)[0]
    assert r.converged == 1 and abs(r.scale - 1.0) <= 1e-12
    # bad arguments: IBA_ERR_INVALID_ARG with a message
    for kw in (dict(frames=(0, 3)), dict(frames=(1, 1)), dict(frames=(-1, 1))):
        with pytest.raises(pkg.IbaError) as e:
            h.icp_step(src, I4, 1.0, **kw)
        assert e.value.status == 1 and "frame range" in str(e.value)
    with pytest.raises(pkg.IbaError) as e:
        h.icp_step(src, I4, -1.0)
    assert e.value.status == 1 and "max_corr_dist" in str(e.value)
    import ctypes as C
    mom = np.zeros(21)
    st = h.lib.iba_icp_step(h.h, 0, 1, src.ctypes.data_as(C.c_void_p), 500, None, 1, C.c_double(1.0), mom.ctypes.data_as(C.c_void_p), None, None)
    assert st == 1 and b"NULL" in h.lib.iba_last_error(h.h)
    h.lib.iba_icp_register.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    out = (abi.IbaIcpResult * 1)()
    st = h.lib.iba_icp_register(h.h, 0, 1, src.ctypes.data_as(C.c_void_p), 500, I4.ctypes.data_as(C.c_void_p), 1, None, out)
    assert st == 1 and b"options" in h.lib.iba_last_error(h.h)
    h.close()

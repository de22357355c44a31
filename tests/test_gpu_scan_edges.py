"""GPU tier of the scan-to-scan edges, each test through the C ABI (iba_scan_step / iba_scan_register / iba_scan_information,
include/iba_mi355x.h): sets against iba_geo_correspondences, sums against a long-double restatement, batch invariance byte for byte, the
point-to-point loop against iba_icp_register, the point-to-plane loop against tests/scan_ref.py, recovery, two stages, information, edges of
the domain. Figures are printed before they are asserted; with IBA_SCAN_PARITY_OUT=<file> they are also appended there as JSON lines
(profiles/scan_edges_parity.md quotes such a run). Inputs and seeds were chosen on the CPU from the restatement alone."""
import json
import os

import numpy as np
import pytest

import icp_ref as R
import scan_ref as S
from parity_gate import check_entries_vs_truth
from test_geo_correspondences import scan_120k_case

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
I4 = np.eye(4)


def _note(**kw):
    print("scan-figures", json.dumps(kw))
    p = os.environ.get("IBA_SCAN_PARITY_OUT")
    if p:
        with open(p, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _handle(pkg, abi, scans, plane_cache=1):
    return pkg.IbaHandle(abi.Problem.from_scans([np.asarray(t, np.float32).reshape(-1, 3) for t in scans]), abi.reference_yaml_params(plane_cache))


def _normals(h, frame, n_pts, idx=None):
    """the device's own cost-path normals of `frame` (iba_debug_plane, which = 0) at the original indices idx (all when None) and the rule
    that says which of them exist: at least max(norm_min_pts, 3) kept neighbours and a finite normal"""
    nrm = np.zeros((n_pts, 3)); has = np.zeros(n_pts, bool)
    for i in (range(n_pts) if idx is None else np.unique(idx)):
        n, _, _, k = h.debug_plane(frame, int(i), which=0)
        nrm[i] = n; has[i] = k >= max(h.params.norm_min_pts, 3) and bool(np.all(np.isfinite(n)))
    nrm[~has] = 0.0
    return nrm, has


def _margins(T, src, tgt, gate):
    """CPU condition on an input: (distance of the nearest d^2 from the gate, smallest nearest / second-nearest gap) at T"""
    q = R.transform(T, np.asarray(src, np.float64))
    idx, d2 = R.nearest(q, tgt)
    return float(np.min(np.abs(d2 - gate * gate))), float(np.min(R.second_gap(q, np.asarray(tgt, np.float64)))), idx, d2, q


def _ld():
    if not R.have_longdouble():
        pytest.skip("np.longdouble carries no more than a double here")


def _held(dev, f64, truth, what, **kw):
    ok, rep = check_entries_vs_truth(dev, f64, np.asarray(truth, np.float64))
    _note(test="sums", what=what, device=rep["device"], f64=rep["oracle"], bar=rep["bar"], **kw)
    assert ok, (what, rep)


def _edge_cases(synth):
    """(name, scans, edges): the room pair both ways, odometry edges of make_scene, and a 5000-point scan against the 120 k-point scan"""
    src, tgt, T = S.room_pair(1, n=12000)
    rng = np.random.default_rng(21)
    yield "room", [src, tgt], [(0, 1, S.perturb_rigid(T, rng)), (1, 0, S.perturb_rigid(np.linalg.inv(T), rng))], 0.3
    prob, _ = synth.make_scene(n_frames=4, pts_per_frame=10000, n_keypoints=50, seed=3)
    Tl = prob.arrays["Tl_next"].reshape(-1, 3, 4)
    scans = [prob.frame_points(f) for f in range(4)]
    ed = []
    for f in range(3):
        Tt = np.eye(4); Tt[:3] = Tl[f]
        ed.append((f, f + 1, S.perturb_rigid(Tt, rng)))
    yield "make_scene", scans, ed, 0.3
    s120, t120, _ = scan_120k_case()
    Tq = S.rigid([1e-3, 2e-3, -1e-3], [0.02, -0.01, 0.01])
    yield "scan120k", [s120.astype(np.float32), t120], [(0, 1, Tq)], 0.25


def test_sets_equal_geo_correspondences_and_sums_hold_against_long_double(pkg, abi, synth):
    """checks 4 and 5 (and 11's equalities) on the same edges"""
    _ld()
    info_gate = 1.2
    for name, scans, edges, gate in _edge_cases(synth):
        h = _handle(pkg, abi, scans)
        m0, pairs = h.scan_step(edges, gate, 0, pairs=True)
        m1 = h.scan_step(edges, gate, 1)
        m2, pairs_i = h.scan_step(edges, info_gate, 2, pairs=True)
        info, n_info = h.scan_information(edges, info_gate)
        assert h.scan_step(edges, gate, 0).tobytes() == m0.tobytes()          # without the pair output, and again: the same bytes
        for e, (s, t, T) in enumerate(edges):
            src = np.asarray(scans[s], np.float32).astype(np.float64); tgt = np.asarray(scans[t], np.float32)
            gm, gap, idx_all, d2_all, q_all = _margins(T, src, tgt, gate)
            gm_i = float(np.min(np.abs(d2_all - info_gate ** 2)))
            _note(test="sets", what=name, edge=e, n_src=len(src), gate_margin=gm, info_gate_margin=gm_i, gap=gap)
            assert gm > 1e-9 and gm_i > 1e-9 and gap > 1e-9, (name, e, gm, gm_i, gap)        # the condition on the INPUT, from the CPU alone
            for g, pi in ((gate, pairs[e]), (info_gate, pairs_i[e])):                         # 4: sets, index for index, original source order
                gs, gt = h.geo_correspondences(t, q_all, g * g)
                kept = np.nonzero(pi != NONE)[0]
                assert np.array_equal(kept, gs) and np.array_equal(pi[kept], gt), (name, e, g, len(kept), len(gs))
            assert 0.3 * len(src) < (pairs[e] != NONE).sum() < len(src)                       # the gate bites
            kept = np.nonzero(pairs[e] != NONE)[0]; pi = pairs[e][kept]
            q = q_all[kept]; p = tgt[pi].astype(np.float64); d2 = R.d2_of(q, p)
            # 5: point-to-point
            assert m0[e][0] == len(kept) and np.all(m0[e][21:] == 0.0)
            piv = m0[e][18:21]
            _held(m0[e][1:18], S.p2p_sums(q, p, d2, piv)[1:18], S.p2p_sums(q, p, d2, piv, np.longdouble)[1:18], name + ":p2p", edge=e, n=len(kept))
            # 5: point-to-plane with the device's own normals
            nrm, has = _normals(h, t, len(tgt), pi)
            o, tr = S.p2l_sums(q, p, nrm[pi], has[pi], d2), S.p2l_sums(q, p, nrm[pi], has[pi], d2, np.longdouble)
            assert m1[e][0] == len(kept) and m1[e][2] == has[pi].sum() > 0.5 * len(kept) and m1[e][31] == 0.0
            assert m1[e][1] == m0[e][1]
            _held(m1[e][3:24], o[3:24], tr[3:24], name + ":JtJ", edge=e, n_planar=int(m1[e][2]))
            _held(np.r_[m1[e][24:31]], o[24:31], tr[24:31], name + ":Jtr,r2", edge=e)
            # 5 / 11: information
            ki = np.nonzero(pairs_i[e] != NONE)[0]; ti = tgt[pairs_i[e][ki]].astype(np.float64)
            assert m2[e][0] == len(ki) == n_info[e] and np.all(m2[e][10:] == 0.0)
            _held(m2[e][1:10], S.info_sums(ti)[1:10], S.info_sums(ti, np.longdouble)[1:10], name + ":info", edge=e, n=len(ki))
            assert np.array_equal(info[e], S.info_from_sums(m2[e])) and np.array_equal(info[e], info[e].T)
        h.close()


def _ring_handle(pkg, abi, n_frames=200, n=6000):
    """200 small scans of one room (independent samplings, each moved a little) + a 50-point scan + the 120 k-point scan"""
    rng = np.random.default_rng(31)
    scans, poses = [], []
    for f in range(n_frames):
        Tf = S.rigid(rng.normal(0, 3e-3, 3), rng.normal(0, 0.03, 3))
        Ti = np.linalg.inv(Tf)
        scans.append((S.room(9, n, 0.01, f)[0] @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)); poses.append(Tf)
    scans.append(scans[0][:50].copy())
    scans.append(scan_120k_case()[1])
    edges = [(f, f + 1, np.linalg.inv(poses[f + 1]) @ poses[f] @ S.rigid(rng.normal(0, 2e-3, 3), rng.normal(0, 0.02, 3))) for f in range(n_frames - 1)]
    return _handle(pkg, abi, scans), edges, n_frames


@pytest.mark.parametrize("est", [0, 1])
def test_batch_invariance_byte_for_byte(pkg, abi, est):
    """check 6"""
    h, edges, F = _ring_handle(pkg, abi)
    k = 77
    alone = h.scan_step([edges[k]], 0.3, est)
    assert alone[0][0] > 100
    allm = h.scan_step(edges, 0.3, est)
    assert h.last_scan_threads == 64
    rev = h.scan_step(edges[::-1], 0.3, est)
    small, big = (F, 3, I4), (F + 1, 5, S.rigid([0, 0, 1e-3], [0.01, 0, 0]))    # 50 source points; 120 k source points
    into_big = (k, F + 1, I4)                                                      # a 120 k-point TARGET: the batch runs in 256-thread blocks
    mixed = h.scan_step([small, edges[k], big, into_big], 0.3, est)
    assert h.last_scan_threads == 256
    assert alone[0].tobytes() == allm[k].tobytes() == rev[len(edges) - 1 - k].tobytes() == mixed[1].tobytes()
    assert allm.tobytes() == rev[::-1].tobytes() == h.scan_step(edges, 0.3, est).tobytes()
    sb = h.scan_step([small, big], 0.3, est)
    assert sb[0].tobytes() == mixed[0].tobytes() and sb[1].tobytes() == mixed[2].tobytes() and mixed[0][0] > 0 and mixed[2][0] > 0
    for threads in (64, 256):                                                      # the sums do not depend on the block shape
        h.debug_scan_threads(threads)
        assert h.scan_step(edges, 0.3, est).tobytes() == allm.tobytes() and h.last_scan_threads == threads
    h.debug_scan_threads(0)
    kw = dict(estimation=est, refine_dist=0.3, info_dist=1.2)
    r1 = h.scan_register([edges[k]], **kw); ra = h.scan_register(edges, **kw); rr = h.scan_register(edges[::-1], **kw)
    rm = h.scan_register([small, edges[k], big, into_big], **kw)
    assert bytes(r1[0]) == bytes(ra[k]) == bytes(rr[len(edges) - 1 - k]) == bytes(rm[1]) == bytes(h.scan_register([edges[k]], **kw)[0])
    assert r1[0].reg.iterations >= 2 and r1[0].n_info > 0
    assert len({r.reg.iterations for r in ra}) > 1      # the edges really stop at different iterations: finished ones dropped out of the launches
    _note(test="batch", est=est, iterations=sorted({r.reg.iterations for r in ra}), converged=sum(r.reg.converged == 1 for r in ra))
    h.close()


# seeds of the loop tests: chosen on the CPU by the margin condition of the restatement (with its own PCA normals for point-to-plane), never by a device result
LOOP_SEEDS = (1, 2, 3)


def _loop_case(seed):
    src, tgt, T = S.room_pair(seed, n=10000)
    return src, tgt, T, S.perturb_rigid(T, np.random.default_rng(100 + seed)), 0.3


def test_point_to_point_equals_the_existing_path(pkg, abi):
    """check 7"""
    _ld()
    for seed in LOOP_SEEDS:
        src, tgt, Tp, T0, gate = _loop_case(seed)
        srcd = src.astype(np.float64)
        ref = S.register(srcd, tgt, T0, gate, margins=True)
        assert ref["gate_margin"] > 1e-9 and ref["gap"] > 1e-9, (seed, ref["gate_margin"], ref["gap"])
        truth = S.register(srcd, tgt, T0, gate, dtype=np.longdouble)
        assert truth["counts"] == ref["counts"] and truth["iterations"] == ref["iterations"]
        h = _handle(pkg, abi, [src, tgt])
        new = h.scan_register([(0, 1, T0)], refine_dist=gate)[0].reg
        old = h.icp_register(srcd, T0, frames=(1, 2), max_corr_dist=gate, with_scaling=0)[0]
        counts_new = [h.scan_register([(0, 1, T0)], refine_dist=gate, refine_max_iter=k)[0].reg.n_corr for k in range(ref["iterations"] + 1)]
        counts_old = [h.icp_register(srcd, T0, frames=(1, 2), max_corr_dist=gate, with_scaling=0, max_iter=k)[0].n_corr for k in range(ref["iterations"] + 1)]
        h.close()
        d_ref = float(np.max(np.abs(ref["T"].astype(np.longdouble) - truth["T"])))
        d_new = float(np.max(np.abs(new.T_np().astype(np.longdouble) - truth["T"]))); d_old = float(np.max(np.abs(old.T_np().astype(np.longdouble) - truth["T"])))
        _note(test="p2p-vs-icp", seed=seed, iterations=ref["iterations"], counts=ref["counts"], counts_new=counts_new, counts_old=counts_old, f64_from_longdouble=d_ref,
              scan_from_longdouble=d_new, icp_from_longdouble=d_old, gate_margin=ref["gate_margin"], gap=ref["gap"])
        assert counts_new == counts_old == ref["counts"]
        assert (new.iterations, new.converged, new.n_corr) == (old.iterations, old.converged, old.n_corr) == (ref["iterations"], ref["converged"], ref["n_corr"])
        assert d_new <= 4.0 * d_ref, (seed, d_new, d_ref)
        assert abs(new.scale - 1.0) <= 1e-12


def test_point_to_plane_loop_against_the_restatement(pkg, abi):
    """check 8"""
    _ld()
    for seed in LOOP_SEEDS:
        src, tgt, Tp, T0, gate = _loop_case(seed)
        srcd = src.astype(np.float64)
        h = _handle(pkg, abi, [src, tgt])
        nrm, has = _normals(h, 1, len(tgt))
        ref = S.register(srcd, tgt, T0, gate, S.P2L, normals=nrm, has=has, margins=True)
        assert ref["gate_margin"] > 1e-9 and ref["gap"] > 1e-9, (seed, ref["gate_margin"], ref["gap"])   # a reason to pick another seed, never to skip
        truth = S.register(srcd, tgt, T0, gate, S.P2L, normals=nrm, has=has, dtype=np.longdouble)
        assert truth["counts"] == ref["counts"] and truth["iterations"] == ref["iterations"]
        r = h.scan_register([(0, 1, T0)], estimation=1, refine_dist=gate)[0]
        counts = [h.scan_register([(0, 1, T0)], estimation=1, refine_dist=gate, refine_max_iter=k)[0].reg.n_corr for k in range(ref["iterations"] + 1)]
        h.close()
        d_ref = float(np.max(np.abs(ref["T"].astype(np.longdouble) - truth["T"]))); d_dev = float(np.max(np.abs(r.reg.T_np().astype(np.longdouble) - truth["T"])))
        e_dev, e_ref = float(np.max(np.abs(r.reg.T_np() - Tp))), float(np.max(np.abs(ref["T"] - Tp)))
        _note(test="p2l-loop", seed=seed, iterations=ref["iterations"], counts=ref["counts"], device_counts=counts, n_planar=ref["n_planar"], has=float(has.mean()), gate_margin=ref["gate_margin"],
              gap=ref["gap"], f64_from_longdouble=d_ref, device_from_longdouble=d_dev, device_err_planted=e_dev, f64_err_planted=e_ref, start_err=float(np.max(np.abs(T0 - Tp))))
        assert counts == ref["counts"]
        assert (r.reg.iterations, r.reg.n_corr, r.reg.converged, r.n_planar) == (ref["iterations"], ref["n_corr"], ref["converged"], ref["n_planar"])
        assert d_dev <= 4.0 * d_ref, (seed, d_dev, d_ref)
        assert e_dev <= 1.01 * e_ref and e_ref < float(np.max(np.abs(T0 - Tp)))
        assert abs(r.reg.fitness - ref["fitness"]) <= 1e-15 and abs(r.reg.inlier_rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]


def test_recovery_on_make_scene_odometry_edges(pkg, abi, synth):
    """check 9. The scans are HDL-64-like ring patterns 1 m apart: with a 0.3 m gate point-to-point slides along the ground rings and ends
    FURTHER from the truth than a start a few cm off (the restatement shows it on the CPU: 0.04-0.06 -> 0.10-0.14 at 10 k and 20 k points per
    scan); at 0.15 m and 20 k points per scan it ends nearer. That gate and size are used here for both estimations."""
    prob, _ = synth.make_scene(n_frames=4, pts_per_frame=20000, n_keypoints=50, seed=3)
    Tl = prob.arrays["Tl_next"].reshape(-1, 3, 4)
    scans = [prob.frame_points(f) for f in range(4)]
    gate = 0.15
    truth, edges = [], []
    for f in range(3):
        Tt = np.eye(4); Tt[:3] = Tl[f]
        truth.append(Tt); edges.append((f, f + 1, S.perturb_rigid(Tt, np.random.default_rng(50 + f), rot=(3e-3, 5e-3), trans=(0.05, 0.08))))
    h = _handle(pkg, abi, scans)
    its = {}
    for est in (0, 1):
        res = h.scan_register(edges, estimation=est, refine_dist=gate)
        its[est] = [r.reg.iterations for r in res]
        for f, r in enumerate(res):
            src = scans[f].astype(np.float64); tgt = scans[f + 1]
            nrm, has = _normals(h, f + 1, len(tgt)) if est else (None, None)
            ref = S.register(src, tgt, edges[f][2], gate, est, normals=nrm, has=has)
            e0, e_dev, e_ref = (float(np.max(np.abs(M - truth[f]))) for M in (edges[f][2], r.reg.T_np(), ref["T"]))
            _note(test="recovery", est=est, edge=f, start=e0, device=e_dev, f64=e_ref, iterations=r.reg.iterations, f64_iterations=ref["iterations"], converged=r.reg.converged)
            assert e_dev < e0 and e_ref < e0, (est, f, e0, e_dev, e_ref)
            assert e_dev <= 1.01 * e_ref, (est, f, e_dev, e_ref)
    _note(test="recovery-iterations", point_to_point=its[0], point_to_plane=its[1])   # recorded, not asserted
    h.close()


def test_two_stages_and_the_references_literal_call(pkg, abi):
    """check 10"""
    src, tgt, Tp, T0, _ = _loop_case(1)
    src2, tgt2, Tp2, T02, _ = _loop_case(2)
    h = _handle(pkg, abi, [src, tgt, src2, tgt2])
    edges = [(0, 1, T0), (2, 3, T02)]
    for est in (0, 1):
        c = dict(estimation=est, refine_dist=1.0, refine_max_iter=4, refine_rel_fitness=1e-4, refine_rel_rmse=1e-4)
        two = h.scan_register(edges, estimation=est, coarse_dist=1.0, coarse_max_iter=4, refine_dist=0.3, info_dist=1.2)
        a = h.scan_register(edges, **c)
        b = h.scan_register([(s, t, r.reg.T_np()) for (s, t, _), r in zip(edges, a)], estimation=est, refine_dist=0.3, info_dist=1.2)
        for x, y in zip(two, b):
            assert bytes(x) == bytes(y)
        assert two[0].reg.iterations >= 1
        # backend_opt.cpp:31,39,43 as written with config/loam/backend.yml: 1 coarse iteration, 0 refine iterations
        lit = h.scan_register(edges, estimation=est, coarse_dist=1.0, coarse_max_iter=1, refine_dist=0.3, refine_max_iter=0)
        one = h.scan_register(edges, estimation=est, refine_dist=1.0, refine_max_iter=1, refine_rel_fitness=1e-4, refine_rel_rmse=1e-4)
        # refine_max_iter = 0 returns the start with its fitness / rmse
        ev = h.scan_register(edges, estimation=est, refine_dist=0.3, refine_max_iter=0)
        m = h.scan_step(edges, 0.3, est)
        for k in range(2):
            assert np.array_equal(lit[k].reg.T_np(), one[k].reg.T_np()) and (lit[k].reg.iterations, lit[k].reg.converged) == (0, 0)
            assert np.array_equal(ev[k].reg.T_np(), np.asarray(edges[k][2])) and (ev[k].reg.iterations, ev[k].reg.converged) == (0, 0)
            assert ev[k].reg.n_corr == int(m[k][0]) > 1000 and ev[k].reg.inlier_rmse == np.sqrt(m[k][1] / m[k][0]) and ev[k].reg.fitness == m[k][0] / len(scans_of(h, edges[k][0]))
            assert ev[k].n_info == 0 and not np.any(ev[k].info_np())
    h.close()


def scans_of(h, f):
    return h.problem.frame_points(f)


def test_information_of_register_is_information_at_its_final_transform(pkg, abi):
    """check 11 (the equalities with the sums and the sets are in the first test)"""
    src, tgt, Tp, T0, _ = _loop_case(3)
    h = _handle(pkg, abi, [src, tgt])
    for est in (0, 1):
        r = h.scan_register([(0, 1, T0)], estimation=est, refine_dist=0.3, info_dist=1.2)[0]
        info, n = h.scan_information([(0, 1, r.reg.T_np())], 1.2)
        assert np.array_equal(r.info_np(), info[0]) and r.n_info == n[0] > 0.9 * len(src)
        assert np.array_equal(info[0], info[0].T) and info[0][3, 3] == info[0][4, 4] == info[0][5, 5] == n[0]
        assert np.all(np.linalg.eigvalsh(info[0]) > 0)
    h.close()


def test_edges_of_the_domain(pkg, abi):
    """check 12 and the argument errors"""
    rng = np.random.default_rng(41)
    src, tgt, T = S.room_pair(4, n=10000)
    # an isolated cluster in the target: 3 points 5 cm apart, 1.9 m from everything else (fewer than norm_min_pts = 5 neighbours inside 0.6 m) ...
    lone = np.array([[0, 0, 0.4], [0.05, 0, 0.4], [0, 0.05, 0.4]], np.float32) + np.float32([3.0, 2.0, 0])
    tgt_l = np.concatenate([tgt, lone])
    # ... and source points that land on it
    Ti = np.linalg.inv(T)
    src_l = np.concatenate([src, ((lone.astype(np.float64) + rng.normal(0, 0.005, (3, 3))) @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)])
    flat = np.c_[rng.uniform(-5, 5, (4000, 2)), np.zeros(4000)].astype(np.float32)            # one exact plane
    # (its source: 3000 of its points moved by 2 mrad and 1-2 cm, so that point-to-point has exact partners to lock onto inside the plane)
    flat_src = (flat[rng.choice(4000, 3000, replace=False)].astype(np.float64) @ R.rotvec([0, 0, 2e-3]).T + [0.01, -0.01, 0.02]).astype(np.float32)
    empty = np.zeros((0, 3), np.float32)
    h = _handle(pkg, abi, [src_l, tgt_l, flat_src, flat, empty])
    # no plane at a target point: counted in fitness, absent from n_planar, the sums equal the restatement's under that rule
    m, pairs = h.scan_step([(0, 1, T)], 0.3, 1, pairs=True)
    pi = pairs[0]; kept = np.nonzero(pi != NONE)[0]
    nrm, has = _normals(h, 1, len(tgt_l), pi[kept])
    on_lone = pi[kept] >= len(tgt)
    assert on_lone.sum() == 3 and np.array_equal(kept[on_lone], len(src) + np.arange(3)) and not has[len(tgt):].any()
    assert m[0][0] == len(kept) and m[0][2] == has[pi[kept]].sum() <= len(kept) - 3
    q = R.transform(T, src_l.astype(np.float64))[kept]; p = tgt_l[pi[kept]].astype(np.float64)
    o = S.p2l_sums(q, p, nrm[pi[kept]], has[pi[kept]], R.d2_of(q, p))
    assert np.max(np.abs(m[0][3:31] - o[3:31]) / np.maximum(np.abs(o[3:31]), 1e-6 * np.max(np.abs(o[3:24])))) <= 1e-10
    r = h.scan_register([(0, 1, T)], estimation=1, refine_dist=0.3, refine_max_iter=0)[0]
    assert r.reg.n_corr == len(kept) and r.n_planar == int(m[0][2]) and r.reg.fitness == len(kept) / len(src_l)
    # a planar-only scene: no point-to-plane update is defined; point-to-point converges
    rp = h.scan_register([(2, 3, I4)], estimation=1, refine_dist=0.3)[0]
    assert (rp.reg.converged, rp.reg.iterations) == (-1, 0) and np.array_equal(rp.reg.T_np(), I4) and rp.n_planar > 1000 and rp.reg.n_corr == 3000
    r0 = h.scan_register([(2, 3, I4)], estimation=0, refine_dist=0.3)[0]
    assert r0.reg.converged == 1 and r0.reg.iterations >= 1
    # empty scans: defined answers, no launch
    for e in ((4, 1, I4), (0, 4, I4)):
        mm, pp = h.scan_step([e], 0.3, 0, pairs=True)
        assert not np.any(mm) and np.all(pp[0] == NONE)
        rr = h.scan_register([e], refine_dist=0.3, info_dist=1.0)[0]
        assert (rr.reg.n_corr, rr.reg.iterations, rr.reg.converged, rr.n_info) == (0, 0, -1, 0) and np.array_equal(rr.reg.T_np(), I4)
    mm = h.scan_step([(4, 1, I4), (0, 1, T), (0, 4, I4)], 0.3, 1)                              # ... also inside a batch
    assert not np.any(mm[0]) and not np.any(mm[2]) and mm[1].tobytes() == m[0].tobytes()
    # a gate so small that nothing is kept
    rr = h.scan_register([(0, 1, T)], refine_dist=1e-9)[0]
    assert (rr.reg.n_corr, rr.reg.iterations, rr.reg.converged) == (0, 0, -1) and rr.reg.fitness == 0.0 and rr.reg.inlier_rmse == 0.0
    # argument errors: IBA_ERR_INVALID_ARG with a message
    bad = I4.copy(); bad[1, 3] = np.nan
    for edges, word in (([(0, 5, I4)], "outside"), ([(-1, 1, I4)], "outside"), ([(1, 1, I4)], "itself"), ([(0, 1, bad)], "not finite"), ([], "E must be"), ([(0, 1, I4)] * 4097, "E must be")):
        for call in (lambda: h.scan_step(edges, 0.3), lambda: h.scan_register(edges), lambda: h.scan_information(edges, 1.0)):
            with pytest.raises(pkg.IbaError) as ex:
                call()
            assert ex.value.status == 1 and word in str(ex.value), (word, str(ex.value))
    for call, word in ((lambda: h.scan_step([(0, 1, I4)], -1.0), "max_corr_dist"), (lambda: h.scan_step([(0, 1, I4)], 0.3, 7), "estimation"),
                       (lambda: h.scan_register([(0, 1, I4)], estimation=2), "estimation"), (lambda: h.scan_register([(0, 1, I4)], refine_dist=0.0), "refine_dist"),
                       (lambda: h.scan_register([(0, 1, I4)], struct_size=8), "struct_size"), (lambda: h.scan_information([(0, 1, I4)], float("inf")), "max_dist")):
        with pytest.raises(pkg.IbaError) as ex:
            call()
        assert ex.value.status == 1 and word in str(ex.value), (word, str(ex.value))
    h.close()
    # plane_cache = 0: point-to-plane fails with a message, point-to-point runs
    h0 = _handle(pkg, abi, [src, tgt], plane_cache=0)
    for call in (lambda: h0.scan_step([(0, 1, T)], 0.3, 1), lambda: h0.scan_register([(0, 1, T)], estimation=1)):
        with pytest.raises(pkg.IbaError) as ex:
            call()
        assert ex.value.status == 1 and "plane_cache" in str(ex.value)
    assert h0.scan_register([(0, 1, T)], refine_dist=0.3)[0].reg.n_corr > 1000
    h0.close()

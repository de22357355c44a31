"""GPU tier of iba_submap_handle (include/iba_mi355x.h): voxel clouds become the frames of a new handle without leaving the device, and the kd index,
the leaf-ordered arrays and the boxes are built there (csrc/iba_index_kernels.hpp). Every comparison is EQUALITY OF BYTES against the host route of
the same public API: iba_submap_build -> float32 -> iba_create (handle B below), whose index the host builds with std::nth_element. There is no
tolerance anywhere in this file. The clouds (tests/index_ref.py, chosen on the CPU from the restatements alone): P = 0, 1, 24, 25, 49, 63, 64, 65, a P
with P % 4 != 0, a lattice full of ties, a cloud with both signed zeros in its split dimension, a merged cloud, and one above 49 152 voxels (depth
11). Figures are printed before they are asserted; with IBA_SUBMAP_HANDLE_PARITY_OUT=<file> they are appended there as JSON lines
(profiles/submap_handle_parity.md quotes such a run)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import index_ref as X
import submap_ref as V

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


def _note(**kw):
    print("submap-handle-figures", json.dumps(kw))
    p = os.environ.get("IBA_SUBMAP_HANDLE_PARITY_OUT")
    if p:
        with open(p, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _f32(cloud):
    return np.ascontiguousarray(cloud["xyz"], np.float64).astype(np.float32)            # round to nearest even: the narrowing every scan gets on its way into a handle


def _host_route(pkg, abi, src, subs, plane_cache=1):
    """the route of the parent commit: the clouds come up, are narrowed, and a handle is created from the arrays (the host builds the index)"""
    return pkg.IbaHandle(abi.Problem.from_scans([_f32(c) for c in src.submap_build(subs)]), abi.reference_yaml_params(plane_cache))


@pytest.fixture(scope="module")
def world(pkg, abi, synth):
    """src: the scans; A: iba_submap_handle on every case in ONE call; B: the host route on the same cases. Both with plane_cache = 1."""
    scans, poses, ids = X.scene(synth)
    cases = X.cases(synth)
    src = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    subs = [c for _, c in cases]
    A = src.submap_handle(subs, abi.reference_yaml_params(1))
    B = _host_route(pkg, abi, src, subs)
    w = dict(src=src, A=A, B=B, names=[n for n, _ in cases], subs=subs, frame={n: i for i, (n, _) in enumerate(cases)})
    yield w
    for h in (A, B, src):
        h.close()


def test_index_identity(world, synth):
    """every array iba_debug_scan_index reads of A equals B's as raw bytes, and both equal the numpy restatement on the CPU's restatement of the cloud"""
    A, B = world["A"], world["B"]
    cpu = X.clouds(synth)
    for f, name in enumerate(world["names"]):
        P = A.frame_num_points(f)
        assert P == B.frame_num_points(f) == len(cpu[name]), (name, P, B.frame_num_points(f), len(cpu[name]))
        a, b = A.debug_scan_index(f), B.debug_scan_index(f)
        d = X.first_difference(a, b)
        _note(test="index", cloud=name, P=P, depth=a["depth"], nodes=len(a["node_dim"]), chunks=len(a["chunk_box"]), difference=d)
        assert d is None, (name, d)
        assert a["depth"] == X.depth_for(P)
        r = X.first_difference(a, X.build(cpu[name]))
        assert r is None, (name, "against the restatement", r)
    assert A.frame_num_points(len(world["names"])) == -1 and A.lib.iba_num_points(A.h) == B.lib.iba_num_points(B.h)
    z = A.debug_scan_index(world["frame"]["zeros"])
    bits = z["xyz_tree"][1].view(np.uint32)
    assert (bits == 0x80000000).any() and (bits == 0).any()                              # both zeros reached the device arrays with their signs


def _reg_bytes(r):
    g = r.reg
    return (np.array(g.T[:]).tobytes(), np.float64(g.scale).tobytes(), np.float64(g.fitness).tobytes(), np.float64(g.inlier_rmse).tobytes(), g.n_corr, g.iterations, g.converged,
            r.n_planar, np.array(r.info[:]).tobytes(), r.n_info)


def _T4(p):
    return np.vstack([V.pose34(p), [0, 0, 0, 1]])


def test_consumers_answer_the_same_bytes(world, pkg, synth):
    A, B, F = world["A"], world["B"], world["frame"]
    rng = np.random.default_rng(3)
    _, poses, _ = X.scene(synth)
    T14 = V.inverse34(poses[4]) @ _T4(poses[1])                                          # scan 1's frame -> the merged cloud's frame
    nudge = np.eye(4); nudge[:3, 3] = [0.05, -0.03, 0.02]
    # the lattice cloud is scan 4 snapped, the merged cloud holds scan 4 in its own frame: that edge surely pairs points
    edges = [(F["lattice"], F["merged"], nudge), (F["P%4"], F["merged"], nudge @ T14), (F["P=65"], F["P%4"], I4), (F["merged"], F["deep"], _T4(poses[4])),
             (F["P=0"], F["merged"], I4), (F["zeros"], F["P=0"], I4), (F["P=1"], F["P=25"], I4)]
    for est in (0, 1, 2):
        ma, pa = A.scan_step(edges, 1.0, estimation=est, pairs=True)
        mb, pb = B.scan_step(edges, 1.0, estimation=est, pairs=True)
        kept = [int((p != 0xFFFFFFFF).sum()) for p in pa]
        _note(test="scan_step", estimation=est, kept=kept, equal=bool(ma.tobytes() == mb.tobytes()))
        assert ma.tobytes() == mb.tobytes(), (est, np.argwhere(ma != mb)[:5].tolist())
        assert all(x.tobytes() == y.tobytes() for x, y in zip(pa, pb)), est
        assert kept[0] > 200 and kept[3] > 200 and kept[4] == 0 and kept[5] == 0, kept    # the edges really pair points; an empty frame pairs none
        assert A.scan_step(edges, 1.0, estimation=est).tobytes() == ma.tobytes()           # without pair_idx: the same sums
    for est in (0, 1):
        opts = dict(estimation=est, coarse_dist=1.0, coarse_max_iter=30, coarse_rel_fitness=1e-4, coarse_rel_rmse=1e-4, refine_dist=0.3, refine_max_iter=30, info_dist=0.3)
        ra, rb = A.scan_register(edges[:5], **opts), B.scan_register(edges[:5], **opts)
        _note(test="scan_register", estimation=est, iterations=[r.reg.iterations for r in ra], n_corr=[r.reg.n_corr for r in ra], n_info=[r.n_info for r in ra])
        assert [_reg_bytes(r) for r in ra] == [_reg_bytes(r) for r in rb], est
        assert ra[0].reg.iterations >= 2 and ra[0].reg.n_corr > 200
    ia, na = A.scan_information(edges[:5], 0.3); ib, nb = B.scan_information(edges[:5], 0.3)
    assert ia.tobytes() == ib.tobytes() and na.tobytes() == nb.tobytes()
    # Scan Context on every cloud
    fr = list(range(len(world["names"])))
    da, db = A.sc_describe(fr), B.sc_describe(fr)
    xa, xb = da.read(), db.read()
    da.close(); db.close()
    for key in ("desc", "ring", "ring_f", "sector", "skipped"):
        assert xa[key].tobytes() == xb[key].tobytes(), key
    assert np.count_nonzero(xa["desc"][F["deep"]]) > 50
    # the neighbour lists and the plane memo
    for name in ("deep", "zeros", "lattice", "merged", "P=65", "P=25", "P=1"):
        f = F[name]; P = A.frame_num_points(f)
        pts = np.unique(np.r_[np.arange(min(P, 64)), rng.integers(0, P, 64)]).astype(np.uint32)
        ka, kb = A.debug_knn(f, pts, k=30), B.debug_knn(f, pts, k=30)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ka, kb)), name
        planes = 0
        for p in pts[:40]:
            for which in (0, 1):
                qa, qb = A.debug_plane(f, int(p), which), B.debug_plane(f, int(p), which)
                assert qa[0].tobytes() == qb[0].tobytes() and np.float64(qa[1]).tobytes() == np.float64(qb[1]).tobytes() and np.float64(qa[2]).tobytes() == np.float64(qb[2]).tobytes() and qa[3] == qb[3], (name, int(p), which)
                planes += qa[3] > 0
        _note(test="knn-plane", cloud=name, points=len(pts), lists_full=int((ka[2] == min(30, P)).sum()), planes_with_neighbours=int(planes))
    q = rng.normal(0, 10, (200, 3))
    for name in ("deep", "zeros", "P=65"):
        ga, gb = A.debug_nn(F[name], q), B.debug_nn(F[name], q)
        assert ga[0].tobytes() == gb[0].tobytes() and ga[1].tobytes() == gb[1].tobytes(), name


def test_batch_independence_repeatability_and_submaps_of_submaps(world, pkg, abi):
    src, A, B, F = world["src"], world["A"], world["B"], world["frame"]
    prm = abi.reference_yaml_params(0)
    for name in ("zeros", "merged", "P=49", "P%4"):
        mine = world["subs"][F[name]]
        ref = A.debug_scan_index(F[name])
        alone = src.submap_handle([mine], prm)
        others = [world["subs"][F[n]] for n in ("P=65", "lattice", "P=0", "P=24", "deep", "P=1", "P=63")]
        batch = src.submap_handle(others[:3] + [mine] + others[3:], prm)                 # member 3 of M = 8
        again = src.submap_handle([mine], prm)
        for what, h, f in (("alone", alone, 0), ("member 3 of 8", batch, 3), ("second call", again, 0)):
            d = X.first_difference(h.debug_scan_index(f), ref)
            _note(test="batch", cloud=name, what=what, difference=d)
            assert d is None, (name, what, d)
        for h in (alone, batch, again):
            h.close()
    # a sub-map of sub-maps: iba_submap_build and iba_submap_handle on A against the same on B
    shift = np.eye(4); shift[:3, 3] = [0.3, 0.1, 0.0]
    sub2 = [([F["merged"], F["P%4"], F["P=0"]], [I4, shift, I4], None, 0.8), ([F["deep"]], [I4], shift, 1.5)]
    ca, cb = A.submap_build(sub2), B.submap_build(sub2)
    for x, y in zip(ca, cb):
        assert x["xyz"].tobytes() == y["xyz"].tobytes() and x["count"].tobytes() == y["count"].tobytes() and x["n_dropped"] == y["n_dropped"] and len(x["xyz"]) > 100
    ha, hb = A.submap_handle(sub2, prm), B.submap_handle(sub2, prm)
    for f in range(2):
        d = X.first_difference(ha.debug_scan_index(f), hb.debug_scan_index(f))
        assert d is None and ha.frame_num_points(f) == len(ca[f]["xyz"]), (f, d)
    ha.close(); hb.close()


def test_loop_closure_through_the_public_api_alone(pkg, abi, synth):
    """iba_sc_replay_plan -> iba_sc_detect -> iba_submap_handle -> iba_scan_register, the source a one-member cloud (LoadPCD) and the target the merged
    cloud (MergeLoadPCD) of ONE call, against the same chain through the host route: T, fitness, inlier_rmse, iterations and info as bytes"""
    from test_gpu_sc import CITY, _rz, city
    scans, poses = city(synth)
    n = len(scans)
    h = pkg.IbaHandle(abi.Problem.from_scans([np.asarray(s, np.float32).reshape(-1, 3) for s in scans]), abi.reference_yaml_params(0))
    db = h.sc_describe(list(range(n)), lidar_height=CITY["lidar_height"])
    plan = pkg.sc_replay_plan(list(range(1, n + 1)), lidar_height=CITY["lidar_height"])
    q = n - 4
    r = db.detect([(q, int(plan[q]))])[0]
    db.close()
    m = r.loop_node
    assert m == q - CITY["first"], (m, q)
    fr = list(range(max(m - 3, 0), m + 4))
    subs = [([q], [I4], None, 0.4), (fr, [poses[f] for f in fr], V.inverse34(poses[m]), 0.4)]
    T0 = _rz(-float(r.yaw_rad))
    opts = dict(estimation=0, coarse_dist=1.0, coarse_max_iter=30, refine_dist=0.3, refine_max_iter=30, info_dist=0.3)
    out = []
    dev = h.submap_handle(subs, abi.reference_yaml_params(1))
    host = _host_route(pkg, abi, h, subs)
    for est in (0, 1):
        opts["estimation"] = est
        a, b = dev.scan_register([(0, 1, T0)], **opts)[0], host.scan_register([(0, 1, T0)], **opts)[0]
        _note(test="loop-closure", estimation=est, query=q, loop_node=m, src_voxels=dev.problem.arrays["pt_offset"].tolist()[1], iterations=a.reg.iterations, host_iterations=b.reg.iterations, fitness=a.reg.fitness,
              rmse=a.reg.inlier_rmse, n_info=a.n_info, equal=bool(_reg_bytes(a) == _reg_bytes(b)))
        out.append((a, b))
    for x in (dev, host, h):
        x.close()
    for a, b in out:
        assert _reg_bytes(a) == _reg_bytes(b)
        assert a.reg.iterations >= 2 and a.reg.fitness > 0.5 and a.n_info > 100
    T_gt = np.linalg.inv(poses[m]) @ poses[q]
    assert float(np.linalg.norm(out[0][0].reg.T_np()[:3, 3] - T_gt[:3, 3])) <= 0.1           # (the bound of tests/test_gpu_sc.py's loop closure, on cloud against cloud)


def _raises(pkg, call, status, word):
    with pytest.raises(pkg.IbaError) as ex:
        call()
    assert ex.value.status == status and word in str(ex.value), (status, word, ex.value.status, str(ex.value))


def test_edges_of_the_domain(world, pkg, abi, synth):
    src, F = world["src"], world["frame"]
    L = src.lib
    prm = abi.reference_yaml_params(0)
    ok = ([0], [I4], None, 0.4)
    scans = X.scene(synth)[0]
    n_src = len(scans)
    bad = I4.copy(); bad[1, 3] = np.nan
    for sub, word in ((([n_src], [I4], None, 0.4), "outside"), (([-1], [I4], None, 0.4), "outside"), (([0], [bad], None, 0.4), "pose of member 0 is not finite"),
                      (([0], [I4], bad, 0.4), "out12 is not finite"), (([0], [I4], None, 0.0), "voxel"), (([], [], None, 0.4), "n_members")):
        _raises(pkg, lambda: src.submap_handle([sub], prm), 1, word)
        _raises(pkg, lambda: src.submap_handle([ok, sub], prm), 1, "sub-map 1")
        _raises(pkg, lambda: src.submap_handle([sub], prm), 1, "iba_submap_handle")
    _raises(pkg, lambda: src.submap_handle([], prm), 1, "M must be in [1, 4096]")
    _raises(pkg, lambda: src.submap_handle([ok] * 4097, prm), 1, "M must be in [1, 4096]")
    # NULL arguments, a struct_size of another library: *out stays NULL
    fr = np.zeros(1, np.int32); ps = np.eye(3, 4).ravel().copy()
    d = (abi.IbaSubmapDesc * 1)()
    d[0].struct_size = C.sizeof(abi.IbaSubmapDesc); d[0].n_members = 1; d[0].frames = fr.ctypes.data; d[0].poses12 = ps.ctypes.data; d[0].voxel = 0.4
    L.iba_submap_handle.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    out = C.c_void_p(0x1234)
    assert L.iba_submap_handle(None, d, 1, C.byref(prm), C.byref(out)) == 1
    assert L.iba_submap_handle(src.h, None, 1, C.byref(prm), C.byref(out)) == 1 and b"NULL" in L.iba_last_error(src.h) and not out.value
    out = C.c_void_p(0x1234)
    assert L.iba_submap_handle(src.h, d, 1, None, C.byref(out)) == 1 and b"NULL" in L.iba_last_error(src.h) and not out.value
    assert L.iba_submap_handle(src.h, d, 1, C.byref(prm), None) == 1 and b"NULL" in L.iba_last_error(src.h)
    for field, value, word in (("frames", None, "NULL"), ("poses12", None, "NULL"), ("struct_size", 32, "struct_size")):
        keep = getattr(d[0], field)
        setattr(d[0], field, value)
        out = C.c_void_p(0x1234)
        assert L.iba_submap_handle(src.h, d, 1, C.byref(prm), C.byref(out)) == 1 and word.encode() in L.iba_last_error(src.h) and not out.value, field
        setattr(d[0], field, keep)
    wrong = abi.reference_yaml_params(0); wrong.norm_max_pts = 65
    _raises(pkg, lambda: src.submap_handle([ok], wrong), 4, "norm_max_pts")
    # a coordinate beyond float32 after narrowing: a finite f64 average (the pose moves the scan to 1e39), refused with a message
    far = I4.copy(); far[0, 3] = 1e39
    _raises(pkg, lambda: src.submap_handle([ok, ([0], [far], None, 0.4)], prm), 4, "not finite after narrowing")
    # an all-empty call gives a valid handle of M empty frames; edges on it answer as empty scans do
    e = src.submap_handle([world["subs"][F["P=0"]]] * 3, abi.reference_yaml_params(1))
    assert [e.frame_num_points(f) for f in range(3)] == [0, 0, 0] and e.lib.iba_num_points(e.h) == 0
    ix = e.debug_scan_index(1)
    assert ix["depth"] == 0 and len(ix["perm"]) == 0 and np.isnan(ix["frame_box"]).all()
    assert not e.scan_step([(0, 1, I4)], 1.0).any() and e.scan_register([(0, 2, I4)])[0].reg.converged == abi.ICP_DEGENERATE
    e.close()
    # 4096 sub-maps in one call
    many = src.submap_handle([world["subs"][F["P=25"]]] * 4096, prm)
    one = world["A"].debug_scan_index(F["P=25"])
    assert all(X.first_difference(many.debug_scan_index(f), one) is None for f in (0, 1, 2047, 4095))
    many.close()
    # the new handle does not depend on the source's lifetime
    s2 = pkg.IbaHandle(abi.Problem.from_scans(scans[:2]), prm)
    sub = [([0], [I4], None, 0.4), ([1], [I4], None, 0.4)]
    keep_h = s2.submap_handle(sub, abi.reference_yaml_params(1))
    want = _host_route(pkg, abi, s2, sub)
    s2.close()
    assert X.first_difference(keep_h.debug_scan_index(1), want.debug_scan_index(1)) is None
    assert keep_h.scan_step([(0, 1, I4)], 1.0, estimation=1).tobytes() == want.scan_step([(0, 1, I4)], 1.0, estimation=1).tobytes()
    keep_h.close(); want.close()

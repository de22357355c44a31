"""GPU tier of the voxel down-sampling / merged sub-map clouds, each test through the C ABI (iba_submap_build, include/iba_mi355x.h): every voxel
of every sub-map byte for byte against tests/submap_ref.py, the same bytes twice and whatever the batch, the edges of the domain with their
messages, and the reference's loop closure (MergeLoadPCD target -> coarse -> refine registration) through the public API alone against
tests/scan_ref.py on the restatement's sub-map. Figures are printed before they are asserted; with IBA_SUBMAP_PARITY_OUT=<file> they are also
appended there as JSON lines (profiles/submap_parity.md quotes such a run). Inputs and seeds were chosen on the CPU from the restatements alone."""
import json
import os

import numpy as np
import pytest

import icp_ref as R
import scan_ref as S
import submap_ref as V

pytestmark = pytest.mark.gpu
I4 = np.eye(4)
VOXELS = (0.1, 0.4, 2.0)


def _note(**kw):
    print("submap-figures", json.dumps(kw))
    p = os.environ.get("IBA_SUBMAP_PARITY_OUT")
    if p:
        with open(p, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _handle(pkg, abi, scans, plane_cache=0):
    """a scans-only handle (the sub-map pass reads no plane memo: plane_cache = 0 keeps creation short)"""
    return pkg.IbaHandle(abi.Problem.from_scans([np.asarray(t, np.float32).reshape(-1, 3) for t in scans]), abi.reference_yaml_params(plane_cache))


def _ref(scans, sub):
    frames, poses, out, voxel = sub
    return V.build([(scans[f], T) for f, T in zip(frames, poses)], voxel, out)


def _same(dev, ref, what):
    """every voxel: count of voxels, per-voxel counts, dropped points, order and every coordinate as raw bytes"""
    assert dev["n_dropped"] == ref["n_dropped"], (what, dev["n_dropped"], ref["n_dropped"])
    assert len(dev["xyz"]) == len(ref["xyz"]) == len(dev["count"]) == len(ref["count"]), (what, len(dev["xyz"]), len(ref["xyz"]))
    assert dev["count"].dtype == np.int32 and dev["xyz"].dtype == np.float64
    assert dev["count"].tobytes() == ref["count"].tobytes(), what
    if dev["xyz"].tobytes() != ref["xyz"].tobytes():
        bad = np.flatnonzero(np.any(dev["xyz"].view(np.uint64) != ref["xyz"].view(np.uint64), axis=1))
        raise AssertionError((what, "voxels that differ", len(bad), "first", int(bad[0]), dev["xyz"][bad[0]].tolist(), ref["xyz"][bad[0]].tolist(), int(ref["count"][bad[0]])))


_cache = {}


def _scene(synth):
    """52 scans of 6000 points along make_scene's trajectory + a scan with NaN / Inf points, a scan snapped to a 0.25 m lattice, an empty scan"""
    if "scene" not in _cache:
        prob, meta = synth.make_scene(n_frames=52, pts_per_frame=6000, n_keypoints=50, seed=5)
        scans = [prob.frame_points(f).copy() for f in range(52)]
        poses = [meta["Twl"][f].copy() for f in range(52)]
        rng = np.random.default_rng(17)
        bad = scans[3].copy()
        hit = rng.choice(len(bad), 90, replace=False)
        bad[hit[:30], rng.integers(0, 3, 30)] = np.nan
        bad[hit[30:60], rng.integers(0, 3, 30)] = np.inf
        bad[hit[60:], rng.integers(0, 3, 30)] = -np.inf
        snapped = (np.round(scans[4].astype(np.float64) * 4.0) / 4.0).astype(np.float32)      # multiples of 0.25: exact in float32
        scans += [bad, snapped, np.zeros((0, 3), np.float32)]
        _cache["scene"] = (scans, poses, dict(bad=52, snapped=53, empty=54))
    return _cache["scene"]


def _members(poses, first, n):
    fr = list(range(first, first + n))
    return fr, [poses[f] for f in fr]


def _cases(scans, poses, ids):
    """(name, (frames, poses, out, voxel)): 1, 2, 7 and 50 members x with / without the output transform x voxel 0.1 / 0.4 / 2.0, and the special scans"""
    out = []
    for n, first in ((1, 9), (2, 20), (7, 30), (50, 1)):
        fr, ps = _members(poses, first, n)
        ref = fr[len(fr) // 2]
        for with_out in (False, True):
            for voxel in VOXELS:
                out.append(("%d-member out=%d voxel=%g" % (n, with_out, voxel), (fr, ps, V.inverse34(poses[ref]) if with_out else None, voxel)))
    tilt = S.rigid([0.02, -0.01, 0.3], [1.0, -2.0, 0.5])
    out.append(("LoadPCD", ([7], [I4], None, 0.4)))
    out.append(("non-finite points alone", ([ids["bad"]], [I4], None, 0.4)))
    out.append(("non-finite points among members", ([2, ids["bad"], 3], [poses[2], tilt, poses[3]], V.inverse34(poses[2]), 0.4)))
    for voxel in (0.5, 0.4, 2.0):      # identity pose, voxel 0.5: minb is a multiple of 0.25 and (q - minb) / voxel an integer for about half of the coordinates
        out.append(("snapped voxel=%g" % voxel, ([ids["snapped"]], [I4], None, voxel)))
    out.append(("snapped among members", ([ids["snapped"], 4], [I4, I4], None, 0.5)))
    out.append(("an empty scan as a member", ([5, ids["empty"], 6], [poses[5], I4, poses[6]], None, 0.4)))
    out.append(("all members empty", ([ids["empty"], ids["empty"]], [I4, tilt], tilt, 0.4)))
    out.append(("a frame twice in one sub-map", ([8, 8], [poses[8], tilt], None, 0.4)))
    return out


def test_every_voxel_equals_the_restatement_byte_for_byte(pkg, abi, synth):
    scans, poses, ids = _scene(synth)
    cases = _cases(scans, poses, ids)
    h = _handle(pkg, abi, scans)
    dev = h.submap_build([c for _, c in cases])
    again = h.submap_build([c for _, c in cases])
    h.close()
    assert len(dev) == len(cases)
    on_face = 0
    for (name, c), d, a in zip(cases, dev, again):
        r = _ref(scans, c)
        _note(test="bytes", case=name, members=len(c[0]), points_in=int(sum(len(scans[f]) for f in c[0])), voxels=len(r["xyz"]), dropped=r["n_dropped"], largest_voxel=int(r["count"].max()) if len(r["count"]) else 0)
        _same(d, r, name)
        _same(a, r, name + " (second call)")
        if name == "snapped voxel=0.5":
            q, _ = V.concatenate([(scans[ids["snapped"]], I4)])
            t = (q - r["minb"]) / 0.5
            on_face = int((t == np.floor(t)).sum())
    assert on_face > 1000, on_face                                   # the snapped case really puts coordinates on voxel faces
    by = dict((n, d) for (n, _), d in zip(cases, dev))
    assert by["non-finite points alone"]["n_dropped"] == 90 and by["non-finite points among members"]["n_dropped"] == 90
    assert len(by["all members empty"]["xyz"]) == 0 and by["all members empty"]["n_dropped"] == 0
    assert by["50-member out=1 voxel=0.4"]["count"].sum() == 50 * 6000


def test_same_bytes_twice_alone_first_of_64_and_last_of_64(pkg, abi, synth):
    scans, poses, ids = _scene(synth)
    h = _handle(pkg, abi, scans)
    fr, ps = _members(poses, 12, 7)
    mine = (fr, ps, V.inverse34(poses[15]), 0.4)
    rng = np.random.default_rng(23)
    others = []
    for k in range(63):                                               # other sub-maps: other members, poses, voxels (other widths of the key fields)
        n = int(rng.integers(1, 9)); first = int(rng.integers(0, 52 - n))
        f2, p2 = _members(poses, first, n)
        if k % 5 == 0:
            f2 = f2 + [ids["bad"]]; p2 = p2 + [S.rigid(rng.normal(0, 0.1, 3), rng.normal(0, 2, 3))]
        others.append((f2, p2, None if k % 2 else V.inverse34(poses[first]), float(rng.choice([0.05, 0.1, 0.4, 2.0, 7.5]))))
    alone = h.submap_build([mine])[0]
    alone2 = h.submap_build([mine])[0]
    first = h.submap_build([mine] + others)
    last = h.submap_build(others + [mine])
    h.close()
    _same(alone, _ref(scans, mine), "alone")
    for what, d in (("again", alone2), ("first of 64", first[0]), ("last of 64", last[63])):
        _same(d, alone, what)
    for k in range(63):                                               # ... and the others do not depend on their place either
        _same(first[1 + k], last[k], "other %d" % k)
    _same(first[1], _ref(scans, others[0]), "other 0 against the restatement")
    _note(test="batch", voxels=len(alone["xyz"]), batch_voxels=int(sum(len(d["xyz"]) for d in first)))


def _raises(pkg, call, status, word):
    with pytest.raises(pkg.IbaError) as ex:
        call()
    assert ex.value.status == status and word in str(ex.value), (status, word, ex.value.status, str(ex.value))


def test_edges_of_the_domain(pkg, abi, synth):
    import ctypes as C
    far_in = np.array([[0, 0, 0], [131071.0, 0, 0]], np.float32)       # voxel 1: minb = -0.5, the far index = floor(131071.5) = 131071 < 2^17
    far_out = np.array([[0, 0, 0], [0, 131071.5, 0]], np.float32)      # floor(131072.0) = 131072: one more than the key holds
    cloud = S.room(3, 4000)[0].astype(np.float32)
    h = _handle(pkg, abi, [cloud, far_in, far_out, np.zeros((0, 3), np.float32)])
    ok = ([0], [I4], None, 0.4)
    # the extent: just inside, just outside (IBA_ERR_UNSUPPORTED, naming the sub-map), and the neighbours of a refused sub-map in the same call
    r = h.submap_build([([1], [I4], None, 1.0)])[0]
    _same(r, V.build([(far_in, I4)], 1.0), "extent just inside")
    assert len(r["xyz"]) == 2 and np.array_equal(r["xyz"][1], [131071.0, 0, 0])
    assert V.indices(far_out.astype(np.float64), 1.0)[0][:, 1].max() == abi.SUBMAP_MAX_AXIS_VOXELS
    _raises(pkg, lambda: h.submap_build([([2], [I4], None, 1.0)]), 4, "131072")
    _raises(pkg, lambda: h.submap_build([ok, ([2], [I4], None, 1.0)]), 4, "sub-map 1")
    _same(h.submap_build([([2], [I4], None, 2.0)])[0], V.build([(far_out, I4)], 2.0), "the same scan with a larger voxel")
    # argument errors: IBA_ERR_INVALID_ARG with a message, before any launch
    bad = I4.copy(); bad[1, 3] = np.nan
    inf = I4.copy(); inf[0, 0] = np.inf
    for sub, word in ((([4], [I4], None, 0.4), "outside"), (([-1], [I4], None, 0.4), "outside"), (([0, 7], [I4, I4], None, 0.4), "outside"),
                      (([0], [bad], None, 0.4), "pose of member 0 is not finite"), (([0, 0], [I4, inf], None, 0.4), "pose of member 1 is not finite"),
                      (([0], [I4], bad, 0.4), "out12 is not finite"), (([0], [I4], None, 0.0), "voxel"), (([0], [I4], None, -0.4), "voxel"),
                      (([0], [I4], None, float("nan")), "voxel"), (([0], [I4], None, float("inf")), "voxel"), (([], [], None, 0.4), "n_members")):
        _raises(pkg, lambda: h.submap_build([sub]), 1, word)
        _raises(pkg, lambda: h.submap_build([ok, sub]), 1, "sub-map 1")
    _raises(pkg, lambda: h.submap_build([]), 1, "M must be in [1, 4096]")
    _raises(pkg, lambda: h.submap_build([ok] * 4097), 1, "M must be in [1, 4096]")
    # NULL descriptors / members / result, a struct_size of another library
    fr = np.zeros(1, np.int32); ps = np.eye(3, 4).ravel().copy()
    d = (abi.IbaSubmapDesc * 1)()
    d[0].struct_size = C.sizeof(abi.IbaSubmapDesc); d[0].n_members = 1; d[0].frames = fr.ctypes.data; d[0].poses12 = ps.ctypes.data; d[0].voxel = 0.4
    assert len(h.submap_build_raw(d, 1)[0]["xyz"]) > 100
    h.lib.iba_submap_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    res = C.c_void_p(None)
    assert h.lib.iba_submap_build(h.h, None, 1, C.byref(res)) == 1 and b"NULL" in h.lib.iba_last_error(h.h) and not res.value
    assert h.lib.iba_submap_build(h.h, d, 1, None) == 1 and b"NULL" in h.lib.iba_last_error(h.h)
    d[0].frames = None
    _raises(pkg, lambda: h.submap_build_raw(d, 1), 1, "NULL")
    d[0].frames = fr.ctypes.data; d[0].poses12 = None
    _raises(pkg, lambda: h.submap_build_raw(d, 1), 1, "NULL")
    d[0].poses12 = ps.ctypes.data; d[0].struct_size = 32
    _raises(pkg, lambda: h.submap_build_raw(d, 1), 1, "struct_size")
    # 4096 sub-maps in one call; a sub-map of an empty scan is no error
    many = h.submap_build([ok] * 4096)
    one = h.submap_build([ok])[0]
    assert len(many) == 4096 and all(m["xyz"].tobytes() == one["xyz"].tobytes() and m["count"].tobytes() == one["count"].tobytes() for m in many)
    e = h.submap_build([([3], [I4], I4, 0.4)])[0]
    assert len(e["xyz"]) == 0 and len(e["count"]) == 0 and e["n_dropped"] == 0
    h.close()


# ---- the reference's loop closure through the public API alone ----
LOOP = dict(seed=7, frames=12, ref=5, k=3, cur=6, voxel=0.4, history_pts=8000, revisit_pts=6000)


def loop_closure_inputs(synth):
    """make_scene draws its trajectory and its world first, from the seed and the frame count alone: two calls that differ only in the points per scan
    are two passes along the SAME trajectory through the SAME world with independent samplings and noise — the second pass revisits every
    place of the first. History = pass one; the current scan = frame `cur` of pass two, 1 m ahead of the history frame `ref`.
    -> (history scans, poses, member frames, output transform, current scan float32, T_gt current -> history frame, perturbed start)"""
    c = LOOP
    pa, ma = synth.make_scene(n_frames=c["frames"], pts_per_frame=c["history_pts"], n_keypoints=50, seed=c["seed"])
    pb, mb = synth.make_scene(n_frames=c["frames"], pts_per_frame=c["revisit_pts"], n_keypoints=50, seed=c["seed"])
    assert np.array_equal(ma["Twl"], mb["Twl"])
    hist = [pa.frame_points(f).copy() for f in range(c["frames"])]
    fr = list(range(c["ref"] - c["k"], c["ref"] + c["k"] + 1))
    out = V.inverse34(ma["Twl"][c["ref"]])
    cur = pb.frame_points(c["cur"]).copy()
    assert not np.array_equal(cur[:100], hist[c["cur"]][:100])
    T_gt = out @ ma["Twl"][c["cur"]]
    T0 = S.perturb_rigid(T_gt, np.random.default_rng(c["seed"] + 100), rot=(3e-3, 5e-3), trans=(0.05, 0.08))
    return hist, ma["Twl"], fr, out, cur, T_gt, T0


COARSE = dict(gate=1.0, max_iter=30, rel_fitness=1e-4, rel_rmse=1e-4)
REFINE = dict(gate=0.3, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6)


def test_loop_closure_through_the_public_api(pkg, abi, synth):
    assert R.have_longdouble(), "np.longdouble carries no more than a double here: the long-double twin of the loop is the truth of this test"
    hist, Twl, fr, out, cur, T_gt, T0 = loop_closure_inputs(synth)
    sub = (fr, [Twl[f] for f in fr], out, LOOP["voxel"])
    ref_cloud = _ref(hist, sub)
    h = _handle(pkg, abi, hist)
    dev_cloud = h.submap_build([sub])[0]
    h.close()
    _same(dev_cloud, ref_cloud, "the loop closure's sub-map")          # the registration below runs on bit-equal inputs
    tgt = dev_cloud["xyz"].astype(np.float32)                          # narrowed as every scan is when it goes into a handle
    tgt_ref = ref_cloud["xyz"].astype(np.float32)
    srcd = cur.astype(np.float64)
    ref = S.register_two_stage(srcd, tgt_ref, T0, COARSE, REFINE, margins=True)
    assert ref["gate_margin"] > 1e-9 and ref["gap"] > 1e-9, (ref["gate_margin"], ref["gap"])   # the condition on the INPUT, from the CPU alone
    truth = S.register_two_stage(srcd, tgt_ref, T0, COARSE, REFINE, dtype=np.longdouble)
    assert truth["counts"] == ref["counts"] and truth["iterations"] == ref["iterations"]
    h2 = pkg.IbaHandle(abi.Problem.from_scans([cur, tgt]), abi.reference_yaml_params(1))
    r = h2.scan_register([(0, 1, T0)], estimation=0, coarse_dist=COARSE["gate"], coarse_max_iter=COARSE["max_iter"], refine_dist=REFINE["gate"], refine_max_iter=REFINE["max_iter"])[0].reg
    h2.close()
    d_ref = float(np.max(np.abs(ref["T"].astype(np.longdouble) - truth["T"]))); d_dev = float(np.max(np.abs(r.T_np().astype(np.longdouble) - truth["T"])))
    e0, e_ref, e_dev = (float(np.max(np.abs(M - T_gt))) for M in (T0, ref["T"], r.T_np()))
    _note(test="loop-closure", members=len(fr), points_in=int(sum(len(hist[f]) for f in fr)), voxels=len(tgt), n_src=len(cur), iterations=ref["iterations"], device_iterations=r.iterations,
          n_corr=ref["n_corr"], device_n_corr=r.n_corr, gate_margin=ref["gate_margin"], gap=ref["gap"], f64_from_longdouble=d_ref, device_from_longdouble=d_dev,
          start_err=e0, restatement_err=e_ref, device_err=e_dev)
    assert (r.iterations, r.converged, r.n_corr) == (ref["iterations"], ref["converged"], ref["n_corr"])
    assert d_dev <= 4.0 * d_ref, (d_dev, d_ref)                        # the gates of tests/test_gpu_scan_edges.py for this loop, unchanged
    assert abs(r.fitness - ref["fitness"]) <= 1e-15 and abs(r.inlier_rmse - ref["rmse"]) <= 1e-12 * ref["rmse"]
    assert e_dev <= 1.01 * e_ref, (e_dev, e_ref)                       # the restatement's own error against the ground truth + the ICP layer's tolerance

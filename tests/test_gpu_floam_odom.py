"""GPU tier of the lattice voxel filter with a crop box, each test through the C ABI (iba_lattice_build, include/iba_mi355x.h): every centroid of every
sub-map byte for byte against tests/floam_odom_ref.py, the edge cases of the cell and crop rules, the same bytes twice and whatever the batch, the
argument errors with their messages, and iba_submap_build's bytes unmoved on the same input. Figures are printed before they are asserted."""
import ctypes as C
import json

import numpy as np
import pytest

import floam_odom_ref as O
import floam_ref as F
import submap_ref as V

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


def _note(**kw):
    print("floam-odom-figures", json.dumps(kw))


def _handle(pkg, abi, scans):
    return pkg.IbaHandle(abi.Problem.from_scans([np.asarray(t, np.float32).reshape(-1, 3) for t in scans]), abi.reference_yaml_params(0))


def _ref(scans, sub):
    frames, poses, out, leaf, crop = sub
    return O.lattice([(scans[f], T) for f, T in zip(frames, poses)], leaf, out, crop)


def _same(dev, ref, what):
    """counts of voxels, dropped and cropped points, per-voxel counts, order and every coordinate as raw bytes"""
    assert dev["n_dropped"] == ref["n_dropped"], (what, dev["n_dropped"], ref["n_dropped"])
    if "n_cropped" in ref:
        assert dev["n_cropped"] == ref["n_cropped"], (what, dev["n_cropped"], ref["n_cropped"])
    assert len(dev["xyz"]) == len(ref["xyz"]) == len(dev["count"]) == len(ref["count"]), (what, len(dev["xyz"]), len(ref["xyz"]))
    assert dev["count"].dtype == np.int32 and dev["xyz"].dtype == np.float64
    assert dev["count"].tobytes() == ref["count"].tobytes(), what
    if dev["xyz"].tobytes() != ref["xyz"].tobytes():
        bad = np.flatnonzero(np.any(dev["xyz"].view(np.uint64) != ref["xyz"].view(np.uint64), axis=1))
        raise AssertionError((what, "voxels that differ", len(bad), "first", int(bad[0]), dev["xyz"][bad[0]].tolist(), ref["xyz"][bad[0]].tolist(), int(ref["count"][bad[0]])))


def _rigid(deg_z, t, tilt=0.0):
    c, s = np.cos(np.radians(deg_z)), np.sin(np.radians(deg_z))
    ct, st = np.cos(tilt), np.sin(tilt)
    T = np.eye(4)
    T[:3, :3] = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]]) @ np.array([[1, 0, 0], [0, ct, -st], [0, st, ct]])
    T[:3, 3] = t
    return T


_cache = {}


def _clouds():
    """frame 0: the hand-made cloud of the cell and crop edge cases; 1: a cell of 300 points, a cell of exactly one, a NaN and an Inf point;
    2, 3: 16-line room scans 0.2 m apart; 4: an empty scan; 5, 6: the extent just inside / just outside the key"""
    if "clouds" not in _cache:
        below = np.nextafter(np.float32(0.0), np.float32(-1.0))
        hand = np.array([[-0.1, 0.1, -0.4], [0.0, -0.0, below], [-1.0, -0.5, 0.0], [0.5, 1.0, 1.5], [-0.25, 0.75, -0.75], [0.25, 0.25, 0.25],
                         [-1.0, 0, 0], [1.0, 0, 0], [0, -2.0, 0], [0, 2.0, 0], [0, 0, -3.0], [0, 0, 3.0], [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0],          # on every face of the box (-1,-2,-3)..(1,2,3)
                         [np.nextafter(np.float32(1.0), np.float32(2.0)), 0, 0], [0, np.nextafter(np.float32(-2.0), np.float32(-3.0)), 0], [0, 0, 3.5]],  # just outside it
                        np.float32)
        rng = np.random.default_rng(11)
        big = np.r_[rng.uniform(0.0, 0.39, (300, 3)), [[5.1, 5.1, 5.1]], [[np.nan, 0.1, 0.1]], [[0.1, np.inf, 0.1]], rng.uniform(-0.39, -0.01, (7, 3))].astype(np.float32)
        room = [F.room_scan(16, per_ring=300, seed=21 + k, origin=(0.2 * k, 0.0)) for k in range(2)]
        far_in = np.array([[-0.5, 0, 0], [131070.5, 0, 0]], np.float32)       # leaf 1: cells -1 .. 131070 = 2^17 cells
        far_out = np.array([[0, -0.5, 0], [0, 131071.5, 0]], np.float32)      # cells -1 .. 131071: one more than the key holds
        _cache["clouds"] = [hand, big, room[0], room[1], np.zeros((0, 3), np.float32), far_in, far_out]
    return _cache["clouds"]


BOX = (np.array([-1.0, -2.0, -3.0]), np.array([1.0, 2.0, 3.0]))


def _cases():
    tilt = _rigid(30.0, [1.0, -2.0, 0.5], 0.05)
    step = _rigid(1.0, [0.2, 0.0, 0.0])
    room_box = (np.array([-10.0, -7.0, -0.5]), np.array([6.0, 3.0, 2.0]))     # keeps the walls at x = -9 and y = -6.5, cuts the other two and the floor
    return [
        ("hand leaf=0.4", ([0], [I4], None, 0.4, None)),
        ("hand leaf=0.5 (exact multiples)", ([0], [I4], None, 0.5, None)),
        ("hand leaf=0.5 crop on the faces", ([0], [I4], None, 0.5, BOX)),
        ("hand crop to one point", ([0], [I4], None, 0.4, (np.array([0.25, 0.25, 0.25]), np.array([0.25, 0.25, 0.25])))),
        ("a cell of 300 points, a cell of 1, NaN / Inf", ([1], [I4], None, 0.4, None)),
        ("the same cropped", ([1], [I4], None, 0.4, (np.full(3, -1.0), np.full(3, 1.0)))),
        ("two members, a pose, out12", ([2, 3], [I4, step], V.inverse34(tilt), 0.4, None)),
        ("two members, a pose, out12, crop", ([2, 3], [tilt, tilt @ step], V.inverse34(tilt), 0.8, (room_box[0] + [1.0, -2.0, 0.5], room_box[1] + [1.0, -2.0, 0.5]))),
        ("emptied by the crop", ([2], [I4], None, 0.4, (np.full(3, 100.0), np.full(3, 101.0)))),
        ("room leaf=0.4", ([2], [I4], None, 0.4, None)),
        ("room leaf=0.8 crop", ([2], [I4], None, 0.8, room_box)),
        ("room leaf=0.2 crop", ([3], [I4], None, 0.2, room_box)),
        ("an empty scan as a member", ([2, 4], [I4, tilt], None, 0.4, room_box)),
        ("all members empty", ([4], [I4], tilt, 0.4, room_box)),
        ("a frame twice", ([3, 3], [I4, tilt], None, 0.4, None)),
    ]


def test_every_centroid_equals_the_restatement_byte_for_byte(pkg, abi):
    scans = _clouds()
    cases = _cases()
    h = _handle(pkg, abi, scans)
    dev = h.lattice_build([c for _, c in cases])
    again = h.lattice_build([c for _, c in cases])
    alone = [h.lattice_build([c])[0] for _, c in cases[:8]]
    h.close()
    assert len(dev) == len(cases)
    by = {}
    for (name, c), d, a in zip(cases, dev, again):
        r = _ref(scans, c)
        by[name] = (d, r)
        _note(test="bytes", case=name, points_in=int(sum(len(scans[f]) for f in c[0])), voxels=len(r["xyz"]), dropped=r["n_dropped"], cropped=r["n_cropped"],
              largest_cell=int(r["count"].max()) if len(r["count"]) else 0)
        _same(d, r, name)
        _same(a, d, name + " (second call)")
    for (name, _), d in zip(cases[:8], alone):
        _same(d, by[name][0], name + " (alone)")
    # the cases really are what their names say
    d, r = by["hand leaf=0.4"]
    # (-0.1, 0.1, float32(-0.4) = -0.4000000060): cells -1, 0, -2; (0, -0, the largest float below 0): cells 0, 0, -1
    assert [-1, 0, -2] in r["idx"].tolist() and [0, 0, -1] in r["idx"].tolist() and [0, 0, 0] in r["idx"].tolist()
    d, r = by["hand leaf=0.5 crop on the faces"]
    assert d["n_cropped"] == 3 and int(d["count"].sum()) == len(scans[0]) - 3
    d, r = by["hand crop to one point"]
    assert len(d["xyz"]) == 1 and d["xyz"][0].tolist() == [0.25, 0.25, 0.25] and d["n_cropped"] == len(scans[0]) - 1
    d, r = by["a cell of 300 points, a cell of 1, NaN / Inf"]
    assert d["n_dropped"] == 2 and d["count"].max() >= 300 and d["count"].min() == 1 and d["n_cropped"] == 0
    d, r = by["the same cropped"]
    assert d["n_dropped"] == 2 and d["n_cropped"] == 1
    d, r = by["emptied by the crop"]
    assert len(d["xyz"]) == 0 and d["n_cropped"] == len(scans[2]) and d["n_dropped"] == 0
    d, r = by["room leaf=0.8 crop"]
    assert 0 < d["n_cropped"] < len(scans[2]) and len(d["xyz"]) > 50
    d, r = by["all members empty"]
    assert len(d["xyz"]) == 0 and d["n_cropped"] == 0


def test_submap_build_keeps_its_bytes_and_answers_no_cropped_points(pkg, abi):
    scans = _clouds()
    h = _handle(pkg, abi, scans)
    tilt = _rigid(30.0, [1.0, -2.0, 0.5], 0.05)
    subs = [([2], [I4], None, 0.4), ([2, 3], [I4, tilt], V.inverse34(tilt), 0.4), ([1], [I4], None, 0.4), ([0], [I4], None, 0.5)]
    lat = h.lattice_build([s + (None,) for s in subs])
    dev = h.submap_build(subs)
    for k, (s, d) in enumerate(zip(subs, dev)):
        _same(d, V.build([(scans[f], T) for f, T in zip(s[0], s[1])], s[3], s[2]), "submap_build %d after a lattice call" % k)
    assert lat[0]["xyz"].tobytes() != dev[0]["xyz"].tobytes()          # two different grids
    # iba_submap_n_cropped on a result of iba_submap_build: 0; -1 for NULL or a sub-map out of range
    L = h.lib
    arr, M, _keep = h._submap_descs(subs)
    L.iba_submap_build.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_void_p)]
    L.iba_submap_n_cropped.argtypes = [C.c_void_p, C.c_int32]; L.iba_submap_n_cropped.restype = C.c_int64
    L.iba_submap_free.argtypes = [C.c_void_p]; L.iba_submap_free.restype = None
    res = C.c_void_p(None)
    assert L.iba_submap_build(h.h, arr, M, C.byref(res)) == 0
    assert [L.iba_submap_n_cropped(res, s) for s in range(-1, M + 1)] == [-1, 0, 0, 0, 0, -1] and L.iba_submap_n_cropped(None, 0) == -1
    L.iba_submap_free(res)
    h.close()


def _raises(pkg, call, status, word):
    with pytest.raises(pkg.IbaError) as ex:
        call()
    assert ex.value.status == status and word in str(ex.value), (status, word, ex.value.status, str(ex.value))


def test_edges_of_the_domain_and_argument_errors(pkg, abi):
    from importlib import import_module
    fo = import_module(pkg.__name__ + ".floam_odom")
    scans = _clouds()
    h = _handle(pkg, abi, scans)
    ok = ([2], [I4], None, 0.4, None)
    # the extent: max i - min i + 1 = 2^17 passes, one more is refused with iba_submap_build's wording, naming the sub-map
    r = h.lattice_build([([5], [I4], None, 1.0, None)])[0]
    _same(r, _ref(scans, ([5], [I4], None, 1.0, None)), "extent just inside")
    assert O.span(O.cells(scans[5].astype(np.float64), 1.0)).max() == abi.SUBMAP_MAX_AXIS_VOXELS and len(r["xyz"]) == 2
    assert O.span(O.cells(scans[6].astype(np.float64), 1.0)).max() == abi.SUBMAP_MAX_AXIS_VOXELS + 1
    _raises(pkg, lambda: h.lattice_build([([6], [I4], None, 1.0, None)]), 4, "the extent along axis 1 is 131073 voxels; the key holds 131072 per axis")
    _raises(pkg, lambda: h.lattice_build([ok, ([6], [I4], None, 1.0, None)]), 4, "iba_lattice_build: sub-map 1")
    # ... and a crop that removes the far point makes the same sub-map pass: the crop takes effect before the extent is known
    c = ([6], [I4], None, 1.0, (np.full(3, -1.0), np.full(3, 1.0)))
    _same(h.lattice_build([c])[0], _ref(scans, c), "the far point cropped")
    # argument errors: IBA_ERR_INVALID_ARG with a message, before any launch
    bad = I4.copy(); bad[1, 3] = np.nan
    nan_box = (np.array([0.0, np.nan, 0.0]), np.ones(3)); inf_box = (np.zeros(3), np.array([1.0, 1.0, np.inf])); swapped = (np.array([0.0, 2.0, 0.0]), np.ones(3))
    for sub, word in ((([7], [I4], None, 0.4, None), "outside"), (([-1], [I4], None, 0.4, None), "outside"),
                      (([2], [bad], None, 0.4, None), "pose of member 0 is not finite"), (([2], [I4], bad, 0.4, None), "out12 is not finite"),
                      (([2], [I4], None, 0.0, None), "leaf must be positive and finite"), (([2], [I4], None, -0.4, None), "leaf"), (([2], [I4], None, float("nan"), None), "leaf"),
                      (([2], [I4], None, float("inf"), None), "leaf"), (([], [], None, 0.4, None), "n_members"),
                      (([2], [I4], None, 0.4, nan_box), "crop_lo / crop_hi are not finite"), (([2], [I4], None, 0.4, inf_box), "crop_lo / crop_hi are not finite"),
                      (([2], [I4], None, 0.4, swapped), "crop_lo must not exceed crop_hi")):
        _raises(pkg, lambda: h.lattice_build([sub]), 1, word)
        _raises(pkg, lambda: h.lattice_build([ok, sub]), 1, "iba_lattice_build: sub-map 1")
    _raises(pkg, lambda: h.lattice_build([]), 1, "M must be in [1, 4096]")
    _raises(pkg, lambda: h.lattice_build([ok] * 4097), 1, "M must be in [1, 4096]")
    # NULL descriptors / members / result, a struct_size of another library
    arr, M, _keep = fo.make_descs([ok])
    assert len(fo.lattice_build_raw(h, arr, 1)[0]["xyz"]) > 100
    L = h.lib
    res = C.c_void_p(None)
    assert L.iba_lattice_build(h.h, None, 1, C.byref(res)) == 1 and b"NULL" in L.iba_last_error(h.h) and not res.value
    assert L.iba_lattice_build(h.h, arr, 1, None) == 1 and b"NULL" in L.iba_last_error(h.h)
    keep_frames = arr[0].frames
    arr[0].frames = None
    _raises(pkg, lambda: fo.lattice_build_raw(h, arr, 1), 1, "NULL")
    arr[0].frames = keep_frames; arr[0].struct_size = C.sizeof(abi.IbaSubmapDesc)
    _raises(pkg, lambda: fo.lattice_build_raw(h, arr, 1), 1, "iba_lattice_desc.struct_size")
    # a box with lo == hi is a box; has_crop = 0 ignores a (valid) box
    arr[0].struct_size = C.sizeof(fo.IbaLatticeDesc); arr[0].has_crop = 0
    arr[0].crop_lo[:] = [5.0, 5.0, 5.0]; arr[0].crop_hi[:] = [5.0, 5.0, 5.0]
    _same(fo.lattice_build_raw(h, arr, 1)[0], _ref(scans, ok), "has_crop = 0")
    arr[0].has_crop = 1
    assert len(fo.lattice_build_raw(h, arr, 1)[0]["xyz"]) == 0
    h.close()


# ================= the track loop (iba_floam_odom_run) =================
import floam_map_ref as M

CFG = O.TRACK
COUNTERS = ("passes", "iterations", "evaluations", "n_edge", "n_surf", "status")
_feat = {}


def _track_scans():
    """frames 0..7: the shared track; 8: a scan of two rings only (few edge points; F.ring_scan); 9: an empty scan"""
    if "track" not in _cache:
        thin = F.ring_scan(16, {7: 300, 8: 300}, seed=5)
        _cache["track"] = O.track_scans() + [thin, np.zeros((0, 3), np.float32)]
    return _cache["track"]


def _features(f):
    if f not in _feat:
        e = F.extract(_track_scans()[f], O.track_extract_options())
        _feat[f] = (e["edge_xyz"], e["surf_xyz"]) + O.downsample(e["edge_xyz"], e["surf_xyz"], CFG["map_resolution"])
    return _feat[f]


def _run(h, tracks, **kw):
    kw.setdefault("keep_maps", 1)
    kw.setdefault("map_resolution", CFG["map_resolution"]); kw.setdefault("crop_half", CFG["crop_half"]); kw.setdefault("init_passes", CFG["init_passes"])
    kw.setdefault("extract", dict(num_lines=CFG["lines"]))
    return h.floam_odom(tracks, **kw)


T30 = _rigid(30.0, [1.5, -0.7, 0.3])
TRACKS = [(list(range(8)), I4), (list(range(7, -1, -1)), I4), ([3, 4], I4)]


@pytest.fixture(scope="module")
def odom_handle(pkg, abi):
    h = _handle(pkg, abi, _track_scans())
    yield h
    h.close()


@pytest.fixture(scope="module")
def batch(odom_handle):
    return _run(odom_handle, TRACKS)


def _bytes_equal(a, b, what):
    assert a is not None and a.dtype == np.float32 and a.shape == b.shape and a.tobytes() == b.tobytes(), (what, None if a is None else a.shape, b.shape)


def _check_layers(steps, frames, T0, crop_half=CFG["crop_half"], solve=True, what="", min_map_edge=10):
    """(i)-(iv) of every step, each layer from the device's own intermediates of the layer before"""
    sched = O.pass_schedule(len(frames), CFG["init_passes"])
    x0 = None
    for k, (s, f) in enumerate(zip(steps, frames)):
        at = "%s step %d" % (what, k)
        raw_e, raw_s, ds_e, ds_s = _features(f)
        _bytes_equal(s["src_edge"], ds_e, at + " (i) edge"); _bytes_equal(s["src_surf"], ds_s, at + " (i) surf")
        assert (s["n_src_edge"], s["n_src_surf"]) == (len(ds_e), len(ds_s))
        if k == 0:
            me, ms = O.init_map(raw_e, raw_s, T0)
            assert np.array_equal(s["T"], T0) and np.array_equal(s["T_pred"], T0) and [s[c] for c in COUNTERS] == [0] * 6
        else:
            prev = steps[k - 1]
            want = O.predict(steps[k - 2]["T"] if k >= 2 else T0, prev["T"])
            d_pred = float(np.max(np.abs(s["T_pred"] - want)))
            assert d_pred <= 1e-12, (at, "(ii)", d_pred)
            enabled = len(prev["map_edge"]) > min_map_edge and len(prev["map_surf"]) > 50
            assert s["passes"] == (sched[k] if enabled else 0) and s["status"] == (0 if enabled else 1), (at, s["passes"], sched[k], s["status"])
            if solve:
                ref = M.register(s["T_pred"], s["src_edge"], s["src_surf"], prev["map_edge"], prev["map_surf"], dict(outer_passes=sched[k], min_map_edge=min_map_edge))
                err = float(np.max(np.abs(s["T"] - ref["T"])))
                print("floam-odom-figures", at, "(iii) vs ref", err, {c: s[c] for c in COUNTERS})
                assert [s[c] for c in COUNTERS] == [ref[c] for c in COUNTERS], (at, [s[c] for c in COUNTERS], [ref[c] for c in COUNTERS])
                assert err <= 1e-8, (at, err)                             # the gate of tests/test_gpu_floam_map.py's registration test
            me, ms, re, rs = O.update_map(prev["map_edge"], prev["map_surf"], s["src_edge"], s["src_surf"], s["T"], CFG["map_resolution"], crop_half)
        _bytes_equal(s["map_edge"], me, at + " (iv) edge"); _bytes_equal(s["map_surf"], ms, at + " (iv) surf")
        assert (s["n_map_edge"], s["n_map_surf"]) == (len(me), len(ms)), at


@pytest.mark.parametrize("b", range(len(TRACKS)))
def test_every_layer_of_every_step_against_the_restatement(batch, b):
    frames, T0 = TRACKS[b]
    assert len(batch[b]) == len(frames)
    _check_layers(batch[b], frames, T0, what="track %d" % b)


def test_whole_track_gate(batch):
    e_dev = O.track_error(batch[0][-1]["T"], CFG["n_scans"] - 1)
    print("floam-odom-figures whole track: device", e_dev, "restatement (CPU)", O.E_REF, "bound", 1.5 * O.E_REF + 1e-3)
    assert e_dev <= 1.5 * O.E_REF + 1e-3, (e_dev, O.E_REF)
    rev = batch[1][-1]["T"][:3, 3] - np.array([-CFG["step"] * 7, 0.0, 0.0])   # the reversed track ends 1.4 m behind its start
    print("floam-odom-figures reversed track: device", float(np.linalg.norm(rev)))


def test_first_scan_with_a_rotated_start_pose(odom_handle):
    r = _run(odom_handle, [([0, 1], T30)])[0]
    _check_layers(r, [0, 1], T30, what="T0 30 degrees")
    raw_e = _features(0)[0]
    assert not np.array_equal(r[0]["map_edge"], raw_e) and len(r[0]["map_edge"]) == len(raw_e)
    ident = _run(odom_handle, [([0], I4)])[0]
    _bytes_equal(ident[0]["map_edge"], O.init_map(raw_e, _features(0)[1], I4)[0], "identity")
    assert np.array_equal(ident[0]["map_edge"], raw_e) and np.array_equal(ident[0]["map_surf"], _features(0)[1])   # the raw features, value for value
    assert len(ident) == 1 and ident[0]["passes"] == 0


def _same_track(a, b, what):
    assert len(a) == len(b), what
    for k, (x, y) in enumerate(zip(a, b)):
        for key in x:
            if isinstance(x[key], np.ndarray):
                assert y[key] is not None and x[key].tobytes() == y[key].tobytes(), (what, k, key)
            else:
                assert x[key] == y[key] or (x[key] is None and y[key] is None), (what, k, key, x[key], y[key])


def test_two_calls_give_the_same_bytes_and_a_track_does_not_depend_on_the_batch(odom_handle, batch):
    again = _run(odom_handle, TRACKS)
    for b in range(len(TRACKS)):
        _same_track(again[b], batch[b], "second call, track %d" % b)
        _same_track(_run(odom_handle, [TRACKS[b]])[0], batch[b], "track %d alone" % b)
    # without keep_maps only the last map is readable, and it is the same map
    last = _run(odom_handle, [TRACKS[2]], keep_maps=0)[0]
    assert last[0]["map_edge"] is None and last[0]["map_surf"] is None
    assert last[1]["map_edge"].tobytes() == batch[2][1]["map_edge"].tobytes() and last[1]["map_surf"].tobytes() == batch[2][1]["map_surf"].tobytes()
    assert np.array_equal(last[1]["T"], batch[2][1]["T"])


def test_a_map_too_small_is_degenerate_and_the_track_goes_on(odom_handle):
    floor = 300                                                          # min_map_edge: above the two-ring scan's edge points, below a room scan's
    assert len(_features(8)[0]) < floor and len(_features(8)[1]) > 50 and len(_features(0)[2]) > floor    # from the restatement alone
    frames = [8, 0, 1]
    r = _run(odom_handle, [(frames, I4)], map=dict(min_map_edge=floor))[0]
    assert r[1]["status"] == 1 and r[1]["passes"] == 0 and np.array_equal(r[1]["T"], r[1]["T_pred"]) and np.array_equal(r[1]["T"], I4)
    assert r[1]["n_map_edge"] > floor and r[2]["passes"] == 10 and r[2]["status"] == 0             # the map was updated and the next step solves
    _check_layers(r, frames, I4, what="degenerate", min_map_edge=floor)


def test_a_small_crop_box_removes_map_points(odom_handle):
    half = 9.3                                                           # the wall at x = -9 leaves the box once the track has moved 0.3 m
    frames = list(range(8))
    r = _run(odom_handle, [(frames, I4)], crop_half=half)[0]
    _check_layers(r, frames, I4, crop_half=half, solve=False, what="crop")
    full = _run(odom_handle, [(frames, I4)])[0]
    print("floam-odom-figures crop: map points per step", [(s["n_map_edge"], s["n_map_surf"]) for s in r], "uncropped", [(s["n_map_edge"], s["n_map_surf"]) for s in full])
    assert r[-1]["n_map_surf"] < full[-1]["n_map_surf"] and r[-1]["n_map_edge"] < full[-1]["n_map_edge"]
    assert r[-1]["map_surf"][:, 0].min() >= r[-1]["T"][0, 3] - half - 1e-6 and full[-1]["map_surf"][:, 0].min() < -8.5


def test_odom_argument_errors(pkg, odom_handle):
    from importlib import import_module
    fo = import_module(pkg.__name__ + ".floam_odom")
    h = odom_handle
    ok = ([0, 1], I4)
    bad = I4.copy(); bad[2, 3] = np.inf
    run = lambda tracks, **kw: _run(h, tracks, **kw)
    _raises(pkg, lambda: run([]), 1, "B must be in [1, 256]")
    _raises(pkg, lambda: run([ok] * 257), 1, "B must be in [1, 256]")
    _raises(pkg, lambda: run([([], I4)]), 1, "n_scans must be in [1, 65536]")
    _raises(pkg, lambda: run([ok, ([0] * 65537, I4)]), 1, "track 1: n_scans must be in [1, 65536]")
    _raises(pkg, lambda: run([([0, 10], I4)]), 1, "scan 1 names frame 10 outside")
    _raises(pkg, lambda: run([([-1], I4)]), 1, "outside")
    _raises(pkg, lambda: run([ok, ([0], bad)]), 1, "track 1: T0 is not finite")
    for v in (0.0, -0.4, float("nan"), float("inf")):
        _raises(pkg, lambda: run([ok], map_resolution=v), 1, "map_resolution must be positive and finite")
        _raises(pkg, lambda: run([ok], crop_half=v), 1, "crop_half must be positive and finite")
    _raises(pkg, lambda: run([ok], init_passes=-1), 1, "init_passes must not be negative")
    _raises(pkg, lambda: run([ok], extract=dict(num_lines=16, struct_size=8)), 1, "iba_floam_odom_run: extract: iba_floam_options.struct_size")
    _raises(pkg, lambda: run([ok], map=dict(struct_size=8)), 1, "iba_floam_odom_run: map: iba_floam_map_options.struct_size")
    _raises(pkg, lambda: run([ok], extract=dict(num_lines=17)), 1, "iba_floam_odom_run: extract: num_lines must be 16, 32 or 64")
    _raises(pkg, lambda: run([ok], map=dict(k=4)), 1, "iba_floam_odom_run: map: ")
    _raises(pkg, lambda: run([ok], map=dict(huber_delta=-1.0)), 1, "iba_floam_odom_run: map: ")
    o = fo.odom_options(extract=dict(num_lines=16)); o.struct_size = 16
    _raises(pkg, lambda: fo.odom(h, [ok], o), 1, "iba_floam_odom_options.struct_size")
    L = fo._odom_lib()
    o = fo.odom_options(extract=dict(num_lines=16))
    arr, _keep = fo.make_tracks([ok])
    res = C.c_void_p(None)
    assert L.iba_floam_odom_run(h.h, None, 1, C.byref(o), C.byref(res)) == 1 and b"NULL" in L.iba_last_error(h.h) and not res.value
    assert L.iba_floam_odom_run(h.h, C.byref(arr), 1, None, C.byref(res)) == 1 and b"NULL" in L.iba_last_error(h.h)
    assert L.iba_floam_odom_run(h.h, C.byref(arr), 1, C.byref(o), None) == 1 and b"NULL" in L.iba_last_error(h.h)
    arr[0].frames = None
    assert L.iba_floam_odom_run(h.h, C.byref(arr), 1, C.byref(o), C.byref(res)) == 1 and b"frames is NULL" in L.iba_last_error(h.h)
    # accessors out of range
    assert L.iba_floam_odom_num(None) == 0 and L.iba_floam_odom_n_scans(None, 0) == -1 and not L.iba_floam_odom_steps(None, 0)
    # more scans than one down-sampling chain takes
    _raises(pkg, lambda: run([([0] * 2049, I4)]), 4, "2048 scans")

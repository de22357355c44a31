"""GPU tier of the F-LOAM feature extraction, each test through the C ABI (iba_floam_extract and the accessors of its result, include/iba_mi355x.h)
against tests/floam_ref.py byte for byte: edge and surf indices, their coordinates, the counts, the skip counters and the ring sizes. The scans come
from floam_ref.fixtures(); tests/test_floam_cpu.py asserts that none of them has a kept point within 0.01 degrees of a ring boundary or within
1e-3 m of a distance limit (a condition on the inputs: the f64 atan of two correct libraries may differ by an ulp). The handle stores every scan in
kd-leaf order, so the original order the rules speak of is never the storage order."""
import importlib

import numpy as np
import pytest

import floam_ref as F

pytestmark = pytest.mark.gpu
KEYS = ("edge_index", "edge_xyz", "surf_index", "surf_xyz", "ring_points")
COUNTERS = ("n_nonfinite", "n_out_of_range", "n_no_ring")
_cache = {}


def _state(pkg, abi):
    """one handle over every fixture scan, and the restatement's answer per (fixture name): both built once"""
    if not _cache:
        fx = F.fixtures()
        names = list(fx)
        _cache["names"] = names
        _cache["h"] = pkg.IbaHandle(abi.Problem.from_scans([fx[k][0] for k in names]), abi.reference_yaml_params(0))
        _cache["ref"] = {}
    return _cache


def _ref(name):
    r = _cache["ref"]
    if name not in r:
        scan, opt = F.fixtures()[name]
        r[name] = F.extract(scan, opt)
    return r[name]


def _same(dev, ref, what):
    for k in KEYS:
        d, r = np.ascontiguousarray(dev[k]), np.ascontiguousarray(ref[k])
        assert d.dtype == r.dtype and d.shape == r.shape, (what, k, d.dtype, r.dtype, d.shape, r.shape)
        if d.tobytes() != r.tobytes():
            bad = np.flatnonzero((d.view(np.uint32) != r.view(np.uint32)).reshape(len(d), -1).any(axis=1))
            raise AssertionError((what, k, "first rows that differ", bad[:8].tolist(), d[bad[:3]].tolist(), r[bad[:3]].tolist()))
    assert {k: dev[k] for k in COUNTERS} == {k: ref[k] for k in COUNTERS}, what


def _run(pkg, abi, names, **fields):
    st = _state(pkg, abi)
    return st["h"].floam_extract([st["names"].index(k) for k in names], **fields)


def _check(pkg, abi, name):
    """fixture `name` through the device with the fixture's own options"""
    opt = F.fixtures()[name][1]
    dev = _run(pkg, abi, [name], **{k: v for k, v in opt.items() if v != F.DEFAULTS[k]})
    assert len(dev) == 1
    ref = _ref(name)
    print("floam-figures", name, "edges", len(ref["edge_index"]), "surfs", len(ref["surf_index"]), "largest ring", int(ref["ring_points"].max()) if len(ref["ring_points"]) else 0)
    _same(dev[0], ref, name)
    return dev[0], ref


def _raises(pkg, call, status, *words):
    with pytest.raises(pkg.IbaError) as ex:
        call()
    assert ex.value.status == status and all(w in str(ex.value) for w in words), (status, words, ex.value.status, str(ex.value))


def test_three_scans_of_a_64_line_room_equal_the_restatement(pkg, abi):
    names = ["room64_0", "room64_1", "room64_2"]
    dev = _run(pkg, abi, names)
    for k, d in zip(names, dev):
        _same(d, _ref(k), k)
        assert len(d["edge_index"]) > 1000 and len(d["surf_index"]) > 1000 and d["ring_points"].min() >= 131     # every ring takes part


@pytest.mark.parametrize("name", ["room16", "room32"])
def test_16_and_32_line_rooms_equal_the_restatement(pkg, abi, name):
    d, _ = _check(pkg, abi, name)
    assert len(d["edge_index"]) > 300


def test_ring_sizes_130_131_and_8192_and_the_refusal_of_8193(pkg, abi):
    d, r = _check(pkg, abi, "sizes")
    assert d["ring_points"][[5, 6, 7, 40]].tolist() == [130, 131, 200, 8192]
    scan = F.fixtures()["sizes"][0]
    ring = F.classify(scan, F.options())[0]
    out = np.concatenate([d["edge_index"], d["surf_index"]])
    assert not (ring[out] == 5).any() and (ring[out] == 6).sum() == 131 - 10 - 6                    # 130 points: nothing; 131: all but the six unassigned entries
    _check(pkg, abi, "sizes_one_sector")                                                             # one sector of 8181 entries: the longest sort the kernel runs
    st = _state(pkg, abi)
    i = st["names"].index("too_long")
    _raises(pkg, lambda: st["h"].floam_extract([st["names"].index("tiny"), i]), 4, "scan 1", "frame %d" % i, "ring 41", "8193")


def test_the_21st_pick_the_last_entry_of_a_sector_and_marks_across_sectors(pkg, abi):
    d, _ = _check(pkg, abi, "quirks")
    p, info = F.quirk_ring()
    e, s = d["edge_index"].tolist(), d["surf_index"].tolist()
    spikes, k, ln = info["spikes"], info["kink"], info["sector_len"]
    assert len([q for q in spikes if q in e]) == 20 and len([q for q in spikes if q not in e and q not in s]) == 1
    for sec in range(5):
        assert 5 + ln * (sec + 1) - 1 not in e + s                                                  # the entry no sector owns
    assert 5 + (len(p) - 10) - 1 not in e + s
    assert k in e and all(q in e + s for q in range(k + 2, k + 6)) and all(q not in e + s for q in range(k - 5, k))


def test_ties_follow_the_lower_position_and_values_on_the_thresholds(pkg, abi):
    d, r = _check(pkg, abi, "lattice")
    p, c1, g = F.lattice_ring()
    v = F.curvature(p)
    assert (v == 0.0).sum() > 100 and (v == 6.25).sum() > 20 and (v == 0.1).sum() >= 5
    e, s = d["edge_index"].tolist(), d["surf_index"].tolist()
    assert all(q in s for q in range(c1 + 2, c1 + 7)) and g in e and g + 1 not in e + s
    for lo, hi in F.sector_bounds(len(p), 6):                                                       # within a sector: surfs ascending by (value, position), edges descending
        ss = [q for q in s if lo + 5 <= q < hi + 5]
        assert ss == sorted(ss, key=lambda q: (v[q - 5], q))
        ee = [q for q in e if lo + 5 <= q < hi + 5]
        assert ee == sorted(ee, key=lambda q: (v[q - 5], q), reverse=True)


def test_poisoned_scan_counts_exactly_and_closes_up_over_the_removals(pkg, abi):
    d, r = _check(pkg, abi, "poison")
    assert {k: d[k] for k in COUNTERS} == F.poison_scan()[1]
    scan = F.fixtures()["poison"][0]
    kept = np.concatenate([d["edge_index"], d["surf_index"]])
    assert np.isfinite(scan[kept]).all() and F.classify(scan, F.options())[0][kept].min() >= 0
    assert d["edge_xyz"].tobytes() == scan[d["edge_index"]].tobytes() and d["surf_xyz"].tobytes() == scan[d["surf_index"]].tobytes()


def test_a_scan_does_not_depend_on_the_batch_and_two_calls_give_the_same_bytes(pkg, abi):
    names = ["room64_0", "room64_1", "room64_2"]
    a = _run(pkg, abi, names)
    b = _run(pkg, abi, names)
    c = _run(pkg, abi, ["room64_2"])
    d = _run(pkg, abi, ["room64_1", "room64_1", "room64_0", "quirks", "empty", "sizes"])
    for x, y, what in [(a[0], b[0], "again 0"), (a[1], b[1], "again 1"), (a[2], b[2], "again 2"), (a[2], c[0], "[2]"), (a[1], d[0], "[1,1,0] 0"), (a[1], d[1], "[1,1,0] 1"), (a[0], d[2], "[1,1,0] 2")]:
        _same(x, y, what)
    _same(d[3], _ref("quirks"), "mixed quirks")
    _same(d[5], _ref("sizes"), "mixed sizes")


@pytest.mark.parametrize("name", ["empty", "tiny", "room64_one_sector", "room64_no_edges", "room64_many"])
def test_empty_tiny_and_extreme_options(pkg, abi, name):
    d, r = _check(pkg, abi, name)
    if name in ("empty", "tiny"):
        assert len(d["edge_index"]) == 0 and len(d["surf_index"]) == 0
    if name == "room64_no_edges":
        assert len(d["edge_index"]) == 0 and len(d["surf_index"]) > 10000
    if name == "empty":                                                                              # a batch of nothing but empty scans launches nothing
        st = _state(pkg, abi)
        i = st["names"].index("empty")
        two = st["h"].floam_extract([i, i])
        assert len(two) == 2 and all(len(x["surf_index"]) == 0 for x in two)


def test_argument_checks_answer_with_the_status_and_a_message(pkg, abi):
    st = _state(pkg, abi)
    h, nf = st["h"], len(st["names"])
    floam = importlib.import_module(pkg.__name__ + ".floam")
    bad = lambda **kw: (lambda: h.floam_extract([0], **kw))
    _raises(pkg, bad(num_lines=48), 1, "num_lines")
    _raises(pkg, bad(min_distance=float("nan")), 1, "not finite")
    _raises(pkg, bad(min_distance=10.0, max_distance=5.0), 1, "above max_distance")
    _raises(pkg, bad(min_ring_points=10), 1, "min_ring_points")
    _raises(pkg, bad(num_sectors=0), 1, "num_sectors")
    _raises(pkg, bad(num_sectors=65), 1, "num_sectors")
    _raises(pkg, bad(max_edges_per_sector=-1), 1, "max_edges_per_sector")
    _raises(pkg, bad(max_edges_per_sector=65), 1, "max_edges_per_sector")
    _raises(pkg, bad(neighbour_span=4), 1, "neighbour_span")
    _raises(pkg, bad(edge_curvature=float("inf")), 1, "not finite")
    _raises(pkg, bad(neighbour_gap2=float("nan")), 1, "not finite")
    _raises(pkg, lambda: h.floam_extract([0, nf]), 1, "scan 1", "outside the handle")
    _raises(pkg, lambda: h.floam_extract([-1]), 1, "outside the handle")
    _raises(pkg, lambda: h.floam_extract([]), 1, "frames is NULL")
    o = floam.floam_options()
    o.struct_size = 48
    _raises(pkg, lambda: h.floam_extract([0], opt=o), 1, "struct_size")
    L = floam._lib()
    import ctypes as C
    fr = np.zeros(1, np.int32)
    assert L.iba_floam_extract(h.h, fr.ctypes.data, 1, C.byref(floam.floam_options()), None) == 1 and "result pointer" in L.iba_last_error(h.h).decode()
    res = C.c_void_p(5)
    assert L.iba_floam_extract(h.h, fr.ctypes.data, 0, C.byref(floam.floam_options()), C.byref(res)) == 1 and not res.value and "n must be" in L.iba_last_error(h.h).decode()
    assert L.iba_floam_extract(h.h, fr.ctypes.data, 1, None, C.byref(res)) == 1 and "options are NULL" in L.iba_last_error(h.h).decode()

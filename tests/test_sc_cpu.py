"""CPU tier of the Scan Context entry points (iba_sc_*, include/iba_mi355x.h): symbols, the struct layouts and the ABI version through the ctypes
mirror, refusals without a device, iba_sc_replay_plan against a stateful class that mirrors detectLoopClosureID's counter, the numpy restatement
tests/sc_ref.py against known answers and against a plainly written np.linalg.norm / np.dot evaluation, and the brute-force ring-key rule against the
index sets the reference's own nanoflann returned (tests/golden/sc_ringkey_nanoflann.npz)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import sc_ref as SC

NAMES = ("iba_default_sc_options", "iba_sc_describe", "iba_sc_db_size", "iba_sc_db_read", "iba_sc_db_free", "iba_sc_last_error", "iba_sc_distance", "iba_sc_detect", "iba_sc_replay_plan")
O = SC.options()


# ---- 1. the boundary: these fail before the feature exists ----
def test_sc_symbols_are_declared_and_exported_and_the_abi_is_still_4(pkg, abi):
    pkg.build_extension()
    lib = pkg.load_library()
    hdr = open(pkg.HEADER_PATH).read()
    declared = set(re.findall(r"\b(iba_[a-z_0-9]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, n
        assert getattr(lib, n) is not None, n
    assert int(re.search(r"#define IBA_ABI_VERSION (\d+)", hdr).group(1)) == pkg.ABI_VERSION == lib.iba_abi_version() == 4
    for t in ("iba_sc_options", "iba_sc_query", "iba_sc_result"):
        assert "typedef struct %s {" % t in hdr
    # the two sentences that called Scan Context the caller's work are gone
    assert "ScanContext and PCD IO\n * stay the caller's" not in hdr and "Scan Context, the pose graph and PCD IO are" not in hdr


def test_struct_layouts_match_the_header_and_the_defaults_are_the_references(pkg, abi):
    o, q, r = abi.IbaScOptions, abi.IbaScQuery, abi.IbaScResult
    assert C.sizeof(o) == 56 and [getattr(o, n).offset for n, _ in o._fields_] == [0, 4, 8, 12, 16, 20, 24, 32, 40, 48]
    assert C.sizeof(q) == 16 and [getattr(q, n).offset for n, _ in q._fields_] == [0, 4, 8, 12]
    assert C.sizeof(r) == 288 and [getattr(r, n).offset for n, _ in r._fields_] == [0, 4, 8, 12, 16, 24, 28, 32, 96, 160]
    hdr = open(pkg.HEADER_PATH).read()
    body = re.search(r"typedef struct iba_sc_options \{(.*?)\} iba_sc_options;", hdr, re.S).group(1)
    assert re.findall(r"(?:int32_t|double)\s+(\w+);", body) == [n for n, _ in o._fields_]            # same fields in the same order
    body = re.search(r"typedef struct iba_sc_result \{(.*?)\} iba_sc_result;", hdr, re.S).group(1)
    assert re.findall(r"(?:int32_t|double|float)\s+(\w+)(?:\[\w+\])?;", body) == [n for n, _ in r._fields_]
    assert (abi.SC_MAX_RING, abi.SC_MAX_SECTOR, abi.SC_MAX_CANDIDATES, abi.SC_NO_WINNER) == (64, 256, 16, SC.NO_WINNER)
    d = pkg.sc_options()
    assert d.struct_size == 56
    assert {k: getattr(d, k) for k in SC.DEFAULTS} == SC.DEFAULTS


def test_null_and_out_of_range_arguments_are_refused_without_a_device(pkg, abi):
    lib = pkg.load_library()
    lib.iba_sc_last_error.argtypes = [C.c_void_p]; lib.iba_sc_last_error.restype = C.c_char_p
    lib.iba_sc_describe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    lib.iba_sc_detect.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    lib.iba_sc_distance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.iba_sc_db_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32] + [C.c_void_p] * 5
    lib.iba_sc_db_size.argtypes = [C.c_void_p]; lib.iba_sc_db_free.argtypes = [C.c_void_p]; lib.iba_sc_db_free.restype = None
    lib.iba_sc_replay_plan.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
    o = pkg.sc_options()
    fr = np.zeros(2, np.int32); res = C.c_void_p(None); q = (abi.IbaScQuery * 1)(); out = (abi.IbaScResult * 1)()
    err = lambda: lib.iba_sc_last_error(None).decode()
    assert lib.iba_default_sc_options(None) == 1 and "NULL" in err()
    assert lib.iba_sc_describe(None, fr.ctypes.data, 2, C.byref(o), C.byref(res)) == 1 and "handle is NULL" in err() and not res.value
    assert lib.iba_sc_detect(None, q, 1, C.byref(o), out) == 1 and "database is NULL" in err()
    assert lib.iba_sc_distance(None, fr.ctypes.data, 1, C.byref(o), None, None) == 1 and "database is NULL" in err()
    assert lib.iba_sc_db_read(None, 0, 1, None, None, None, None, None) == 1 and "database is NULL" in err()
    assert lib.iba_sc_db_size(None) == 0
    lib.iba_sc_db_free(None)
    sizes = np.arange(1, 5, dtype=np.int32); end = np.zeros(4, np.int32)
    assert lib.iba_sc_replay_plan(None, 4, C.byref(o), end.ctypes.data) == 1 and "NULL" in err()
    assert lib.iba_sc_replay_plan(sizes.ctypes.data, 4, None, end.ctypes.data) == 1 and "options are NULL" in err()
    assert lib.iba_sc_replay_plan(sizes.ctypes.data, 4, C.byref(o), None) == 1 and "NULL" in err()
    assert lib.iba_sc_replay_plan(sizes.ctypes.data, 0, C.byref(o), end.ctypes.data) == 1 and "n must be at least 1" in err()
    for fields, word in ((dict(num_sector=257), "num_sector must be in [1, 256]"), (dict(num_ring=0), "num_ring must be in [1, 64]"), (dict(num_candidates=17), "num_candidates must be in [1, 16]"),
                         (dict(tree_period=0), "tree_period"), (dict(num_exclude_recent=-1), "num_exclude_recent"), (dict(max_radius=-1.0), "max_radius"), (dict(dist_thres=float("nan")), "dist_thres"),
                         (dict(struct_size=52), "struct_size")):
        with pytest.raises(pkg.IbaError) as ex:
            pkg.sc_replay_plan([1, 2, 3], **fields)
        assert ex.value.status == 1 and word in str(ex.value), (word, str(ex.value))
    with pytest.raises(pkg.IbaError) as ex:
        pkg.sc_replay_plan([3, 0])
    assert "call 1 holds 0 descriptors" in str(ex.value)


class StatefulManager:
    """detectLoopClosureID's bookkeeping as the reference keeps it: a list of keys, a counter, a search set that is rebuilt on some calls"""

    def __init__(self, exclude, period):
        self.exclude, self.period, self.keys, self.counter, self.search_set = exclude, period, [], 0, []

    def add(self):
        self.keys.append(len(self.keys))

    def detect(self):
        if len(self.keys) < self.exclude + 1:
            return 0                                   # early return: nothing searched, the counter stays
        if self.counter % self.period == 0:
            self.search_set = self.keys[:len(self.keys) - self.exclude]
        self.counter = self.counter + 1
        return len(self.search_set)


@pytest.mark.parametrize("exclude,period", [(30, 30), (30, 7), (5, 1), (0, 3), (12, 50)])
def test_replay_plan_is_the_stateful_counter(pkg, exclude, period):
    rng = np.random.default_rng(exclude * 100 + period)
    for pattern in ("every keyframe", "some keyframes", "bursts"):
        m = StatefulManager(exclude, period)
        sizes, want = [], []
        for step in range(150):
            for _ in range(1 if pattern != "bursts" else int(rng.integers(1, 4))):
                m.add()
            if pattern == "every keyframe" or rng.random() < 0.7:
                sizes.append(len(m.keys)); want.append(m.detect())
        got = pkg.sc_replay_plan(sizes, num_exclude_recent=exclude, tree_period=period)
        assert got.dtype == np.int32 and got.tolist() == want, (pattern, exclude, period)
        assert SC.replay_plan(sizes, SC.options(num_exclude_recent=exclude, tree_period=period)).tolist() == want
        if (exclude, period) == (30, 30) and pattern == "every keyframe":
            assert want[:30] == [0] * 30 and want[30:60] == [1] * 30 and want[60:90] == [31] * 30 and want[90] == 61     # the 31-node threshold and three rebuilds


# ---- 2. the restatement against known answers ----
def _pt(ring, sector, z, frac=0.5):
    """a point in the middle of bin (ring, sector) (1-based) of the default 20 x 60 descriptor, on the ground plane z = 0 displaced to z"""
    rng_xy = (ring - frac) * 4.0
    a = np.deg2rad((sector - 0.5) * 6.0)
    return (rng_xy * np.cos(a), rng_xy * np.sin(a), z)


def test_one_point_per_chosen_bin():
    chosen = {(1, 1): 0.5, (3, 7): -1.25, (10, 30): 2.0, (20, 60): 0.75, (5, 16): -0.5, (12, 45): 1.5}
    pts = [_pt(r, s, z) for (r, s), z in chosen.items()]
    pts += [_pt(3, 7, -3.0), _pt(10, 30, 1.0)]                          # lower points of the same bins do not show (for ring 3 the 3-D norm still lies inside the ring)
    d, skipped = SC.descriptor(np.asarray(pts, np.float32), O)
    want = np.zeros((20, 60))
    for (r, s), z in chosen.items():
        want[r - 1, s - 1] = z
    assert skipped == 0 and d.dtype == np.float64 and np.array_equal(d, want)
    assert np.array_equal(SC.ring_key(d), want.sum(1) / 60.0) and np.array_equal(SC.sector_key(d), want.sum(0) / 20.0)   # one or two non-zeros per row / column: any order gives these sums


def test_range_is_the_3d_norm_and_the_sentinel_quirks():
    # beyond 80 m by the 3-D norm, inside by the xy range: skipped
    d, _ = SC.descriptor(np.asarray([(79.0, 1.0, 20.0), (10.0, 1.0, 0.5)], np.float32), O)
    assert np.count_nonzero(d) == 1 and d[2, 0] == 0.5
    # range exactly 80 is inside (the test is range > max_radius), ring 20; one float above is outside
    d, _ = SC.descriptor(np.asarray([(80.0, 0.0, 0.0), (0.0, 48.0, 64.0)], np.float32), O)
    assert d[19, 14] == 64.0 and np.count_nonzero(d) == 1                # (80, 0, 0) has z = 0: it enters but its bin reads 0
    up = np.nextafter(np.float32(80.0), np.float32(90.0))
    assert SC.bins(np.asarray([(up, 0.0, 1.0)], np.float32), O)[2].tolist() == [False]
    # z = -1000 and below never enter (strict '<' against the -1000 the matrix starts with); just above does
    far = SC.options(max_radius=2000.0)
    d, _ = SC.descriptor(np.asarray([(10.0, 1.0, -1000.0), (300.0, 1.0, -1000.5), (600.0, 1.0, -999.5)], np.float32), far)
    assert np.count_nonzero(d) == 1 and d[11, 0] == -999.5               # range 1166.1 / 2000 * 20 = 11.66 -> ring 12
    # ... and with a lidar_height the sentinel is met by z + lidar_height
    d, _ = SC.descriptor(np.asarray([(10.0, 1.0, -1002.0), (600.0, 1.0, -1001.5)], np.float32), SC.options(max_radius=2000.0, lidar_height=2.0))
    assert np.count_nonzero(d) == 1 and d[11, 0] == -999.5
    # non-finite points are skipped and counted
    d, skipped = SC.descriptor(np.asarray([(np.nan, 1.0, 1.0), (1.0, np.inf, 1.0), (1.0, 1.0, -np.inf), (10.0, 1.0, 0.25)], np.float32), O)
    assert skipped == 3 and np.count_nonzero(d) == 1
    d, skipped = SC.descriptor(np.zeros((0, 3), np.float32), O)
    assert skipped == 0 and not d.any()


def test_the_origin_column_and_the_x_axis():
    ring, sec, enters, a = SC.bins(np.asarray([(0.0, 0.0, 3.0), (-0.0, 0.0, 3.0), (0.0, -0.0, 2.0), (5.0, 0.0, 1.0), (5.0, -0.0, 1.0), (-5.0, 0.0, 1.0), (0.0, 5.0, 1.0), (5.0, -1e-30, 1.0)], np.float32), O)
    assert enters.all() and a["sector_arg"][:5].tolist() == [0.0] * 5 and a["exact_angle"][:5].all()
    assert sec.tolist() == [0, 0, 0, 0, 0, 29, 14, 59] and ring[:3].tolist() == [0, 0, 0]
    d, _ = SC.descriptor(np.asarray([(0.0, 0.0, 3.0), (0.0, 0.0, -1.0)], np.float32), O)
    assert d[0, 0] == 3.0 and np.count_nonzero(d) == 1
    # +0 orders above -0 in the bin key, and an empty bin is +0
    assert SC.z_key(np.float32(0.0)) > SC.z_key(np.float32(-0.0)) > SC.z_key(np.float32(-1e-30)) > 0
    z = np.asarray([-np.finfo(np.float32).max, -3.5, -0.0, 0.0, 1e-30, 7.25], np.float32)      # ascending, -0 before +0
    assert np.array_equal(SC.z_unkey(SC.z_key(z)).view(np.uint32), z.view(np.uint32)) and np.all(np.diff(SC.z_key(z).astype(np.int64)) > 0)


def _random_desc(seed, fill=0.6):
    rng = np.random.default_rng(seed)
    d = rng.uniform(-2.0, 6.0, (20, 60)).astype(np.float32).astype(np.float64)
    d[rng.random((20, 60)) > fill] = 0.0
    return d


@pytest.mark.parametrize("k", [0, 1, 3, 17, 30, 59])
def test_a_descriptor_rotated_by_k_sectors(k):
    d = _random_desc(5)
    turned = np.roll(d, -k, axis=1)                                      # circshift(turned, k) == d
    dist, shift = SC.distance(d, turned, O)
    assert shift == k and abs(dist) <= 60 * 2.0 ** -52, (dist, shift)    # 60 cosines of identical columns, each 1 within a few roundings
    assert SC.yaw(shift, O).dtype == np.float32 and SC.yaw(shift, O) == np.float32(math.radians(6.0 * k))
    assert SC.align(SC.sector_key(d), SC.sector_key(turned)) == k


def test_an_all_zero_column_and_no_common_column():
    d = _random_desc(6)
    d[:, 7] = 0.0
    e = d.copy(); e[:, 9] = 0.0
    n = SC.column_norms(d)
    assert n[7] == 0.0 and np.count_nonzero(n) == 59
    # columns 7 and 9 are left out of the mean: the other 58 are identical
    assert abs(SC.dist_direct(d, e)) <= 60 * 2.0 ** -52
    # no column that is non-zero in both: 0 / 0 = NaN, which never wins a '<' -> the initial 10000000 with shift 0, and never a loop
    a = np.zeros((20, 60)); b = np.zeros((20, 60))
    a[:, :30] = _random_desc(7)[:, :30] + 10.0; b[:, 30:] = _random_desc(8)[:, 30:] + 10.0
    assert np.isnan(SC.dist_direct(a, b))
    o_all = SC.options(search_ratio=0.0)                                 # radius 0: the one tried shift is the alignment's; here it is the NaN one
    al = SC.align(SC.sector_key(a), SC.sector_key(b))
    if np.isnan(SC.dist_direct(a, np.roll(b, al, axis=1))):
        assert SC.distance(a, b, o_all) == (SC.NO_WINNER, 0)
    z = np.zeros((20, 60))
    assert SC.distance(a, z, O) == (SC.NO_WINNER, 0) and SC.distance(z, z, O) == (SC.NO_WINNER, 0)
    db = dict(desc=np.stack([z, a, z]), ring_f=SC.ring_key(np.stack([z, a, z])).astype(np.float32))
    r = SC.detect(db, [(2, 2)], O)[0]
    assert r["loop_node"] == -1 and r["min_dist"] == SC.NO_WINNER and r["shift"] == 0 and r["cand_node"].tolist() == [0, 1, -1] and np.isnan(r["cand_dist"][2])


def test_the_window_and_the_radius():
    assert SC.search_radius(O) == 3 and SC.window(10, O) == [7, 8, 9, 10, 11, 12, 13]
    assert SC.window(1, O) == [0, 1, 2, 3, 4, 58, 59] and SC.window(59, O) == [0, 1, 2, 56, 57, 58, 59]       # sorted ascending after the wrap, as the reference sorts
    assert SC.window(2, SC.options(num_sector=7, search_ratio=1.0)) == list(range(7))                        # a window wider than the circle: every shift once
    assert SC.search_radius(SC.options(num_sector=256, search_ratio=0.05)) == 6 and SC.search_radius(SC.options(search_ratio=0.0)) == 0


def _plain_distance(sc1, sc2, opt):
    """the same definition written plainly: np.linalg.norm / np.dot, numpy's own summation order"""
    S = sc1.shape[1]
    vk1, vk2 = sc1.mean(0), sc2.mean(0)
    al = int(np.argmin([np.linalg.norm(vk1 - np.roll(vk2, s)) for s in range(S)]))
    best, arg = SC.NO_WINNER, 0
    for s in SC.window(al, opt):
        b = np.roll(sc2, s, axis=1)
        sims = [np.dot(sc1[:, c], b[:, c]) / (np.linalg.norm(sc1[:, c]) * np.linalg.norm(b[:, c])) for c in range(S) if np.linalg.norm(sc1[:, c]) != 0 and np.linalg.norm(b[:, c]) != 0]
        d = 1.0 - np.sum(sims) / len(sims)
        if d < best:
            best, arg = d, s
    return best, arg


def test_fixed_order_distance_against_a_plain_evaluation():
    """The two differ only in the order of f64 sums: per cosine a 20-term dot product and two 20-term norms (relative error <= about 20 u each, u = 2^-53), then a
    60-term mean of values <= 1: |gap| <= (3 * 20 + 60) u = 120 u = 1.3e-14 to first order; the bound is 4 times that, 5.4e-14. Measured on these inputs
    (profiles/sc_parity.md): 3.4e-16 at most."""
    worst = 0.0
    for seed in range(40):
        a, b = _random_desc(100 + seed, fill=0.3 + 0.015 * seed), np.roll(_random_desc(200 + seed), seed, axis=1)
        if seed % 3 == 0:
            b = np.roll(a, -seed, axis=1) + np.random.default_rng(seed).normal(0, 0.2, a.shape) * (a != 0)
        d0, s0 = SC.distance(a, b, O)
        d1, s1 = _plain_distance(a, b, O)
        assert s0 == s1, (seed, s0, s1)
        worst = max(worst, abs(d0 - d1))
    print("sc-figures fixed-order vs plain distance: worst gap %.3e over 40 pairs" % worst)
    assert worst <= 480 * 2.0 ** -53, worst


# ---- 3. the kd-tree pin ----
def test_brute_force_ring_key_rule_returns_nanoflanns_index_sets():
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sc_ringkey_nanoflann.npz"))
    keys, queries, idx = g["keys"], g["queries"], g["indices"]
    assert keys.dtype == np.float32 and queries.dtype == np.float32 and int(g["k"]) == 3 and int(g["leaf"]) == 10 and len(queries) >= 100
    both = np.concatenate([keys, queries])
    left_out = 0
    for i in range(len(queries)):
        d = keys.astype(np.float64) - queries[i].astype(np.float64)
        d2 = np.sort(SC.seq_sum(d * d, 1))
        if not (d2[3] - d2[2] > 1e-4 * d2[3]):                           # float accumulation moves a 20-term sum by about 20 * 2^-24 = 1.2e-6 relative: the gap is 80 times that
            left_out += 1
            continue
        got = SC.knn(both, len(keys) + i, len(keys), 3)
        assert sorted(got.tolist()) == sorted(idx[i].tolist()), (i, got, idx[i])
    assert left_out == 0

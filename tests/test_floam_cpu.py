"""CPU tier of the F-LOAM feature extraction (iba_floam_*, include/iba_mi355x.h): symbols, the struct layout and the ABI version through the ctypes
mirror, refusals that need no device, the numpy restatement tests/floam_ref.py against a second, literal transcription of the reference's loops
(python lists, a picked list searched with `in`, sorted with the tie rule) and against hand-computed answers, and the condition on every fixture of
the GPU tier: no kept point within 0.01 degrees of a ring boundary or within 1e-3 m of a distance limit."""
import ctypes as C
import re

import numpy as np
import pytest

import floam_ref as F

NAMES = ("iba_default_floam_options", "iba_floam_extract", "iba_floam_num", "iba_floam_n_edge", "iba_floam_n_surf", "iba_floam_edge_xyz", "iba_floam_edge_index", "iba_floam_surf_xyz",
         "iba_floam_surf_index", "iba_floam_stats", "iba_floam_free")
O = F.options()


@pytest.fixture(scope="module")
def floam(pkg):
    import importlib
    return importlib.import_module(pkg.__name__ + ".floam")


# ---- 1. the boundary: these fail before the feature exists ----
def test_floam_symbols_are_declared_and_exported_and_the_abi_is_still_4(pkg):
    pkg.build_extension()
    lib = pkg.load_library()
    hdr = open(pkg.HEADER_PATH).read()
    declared = set(re.findall(r"\b(iba_[a-z_0-9]+)\s*\(", hdr))
    for n in NAMES:
        assert n in declared, n
        assert getattr(lib, n) is not None, n
    assert int(re.search(r"#define IBA_ABI_VERSION (\d+)", hdr).group(1)) == pkg.ABI_VERSION == lib.iba_abi_version() == 4
    assert "typedef struct iba_floam_options {" in hdr and "#define IBA_FLOAM_MAX_RING_POINTS 8192" in hdr


def test_struct_layout_matches_the_header_and_the_defaults_are_the_references(pkg, abi, floam):
    o = abi.IbaFloamOptions
    assert C.sizeof(o) == 56 and [getattr(o, n).offset for n, _ in o._fields_] == [0, 4, 8, 16, 24, 28, 32, 36, 40, 48]
    body = re.search(r"typedef struct iba_floam_options \{(.*?)\} iba_floam_options;", open(pkg.HEADER_PATH).read(), re.S).group(1)
    assert re.findall(r"(?:int32_t|double)\s+(\w+);", body) == [n for n, _ in o._fields_]
    d = floam.floam_options()
    assert d.struct_size == 56 and {k: getattr(d, k) for k in F.DEFAULTS} == F.DEFAULTS
    assert abi.FLOAM_MAX_RING_POINTS == F.MAX_RING_POINTS == floam.MAX_RING_POINTS == 8192


def test_arguments_are_refused_without_a_device(pkg, floam):
    lib = floam._lib()
    err = lambda: lib.iba_last_error(None).decode()
    o = floam.floam_options()
    fr = np.zeros(2, np.int32)
    res = C.c_void_p(1)
    assert lib.iba_default_floam_options(None) == 1 and "NULL" in err()
    assert lib.iba_floam_extract(None, fr.ctypes.data, 2, C.byref(o), C.byref(res)) == 1 and "handle is NULL" in err()
    assert lib.iba_floam_num(None) == 0 and lib.iba_floam_n_edge(None, 0) == -1 and lib.iba_floam_n_surf(None, 0) == -1
    assert not lib.iba_floam_edge_xyz(None, 0) and not lib.iba_floam_surf_index(None, 0)
    assert lib.iba_floam_stats(None, 0, None, None, None, None) == 1 and "NULL" in err()
    lib.iba_floam_free(None)


# ---- 2. the restatement against a literal transcription of laserProcessingClass.cpp:68-211 ----
def literal_ring(p, opt):
    """one ring list (python list of float32 triples) -> (edge positions, surf positions), written like the reference: a cloudCurvature list of (id,
    value), a slice per sector, sorted by value (ties: the lower id first), a picked list searched linearly"""
    f32, f64 = np.float32, np.float64
    n = len(p)
    if n < opt["min_ring_points"]:
        return [], []
    cloud = []
    with np.errstate(all="ignore"):
        for j in range(5, n - 5):
            diff = []
            for a in range(3):
                s = p[j - 5][a] + p[j - 4][a] + p[j - 3][a] + p[j - 2][a] + p[j - 1][a] - f32(10) * p[j][a] + p[j + 1][a] + p[j + 2][a] + p[j + 3][a] + p[j + 4][a] + p[j + 5][a]
                assert type(s) is f32
                diff.append(f64(s))
            v = diff[0] * diff[0] + diff[1] * diff[1] + diff[2] * diff[2]
            cloud.append((j, float("inf") if v != v else float(v)))
    total = n - 10
    edges, surfs = [], []

    def gap(a, b):
        with np.errstate(all="ignore"):
            d = [f64(p[a][k] - p[b][k]) for k in range(3)]
            return d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    for s in range(opt["num_sectors"]):
        length = total // opt["num_sectors"]
        start, end = length * s, length * (s + 1) - 1
        if s == opt["num_sectors"] - 1:
            end = total - 1
        sub = sorted(cloud[start:end] if end > start else [], key=lambda c: (c[1], c[0]))
        picked, largest = [], 0
        for i in range(len(sub) - 1, -1, -1):
            ind = sub[i][0]
            if ind not in picked:
                if sub[i][1] <= opt["edge_curvature"]:
                    break
                largest += 1
                picked.append(ind)
                if largest <= opt["max_edges_per_sector"]:
                    edges.append(ind)
                else:
                    break
                for k in range(1, 6):
                    if gap(ind + k, ind + k - 1) > opt["neighbour_gap2"]:
                        break
                    picked.append(ind + k)
                for k in range(-1, -6, -1):
                    if gap(ind + k, ind + k + 1) > opt["neighbour_gap2"]:
                        break
                    picked.append(ind + k)
        for i in range(len(sub)):
            if sub[i][0] not in picked:
                surfs.append(sub[i][0])
    return edges, surfs


def random_ring(rng, k):
    """rings with runs of close neighbours, jumps, exact ties (a coarse dyadic lattice) and, every fourth, the lattice ring whose values sit exactly on 0.1
    and 0.05"""
    if k % 4 == 0:
        p = F.lattice_ring(n=int(rng.integers(300, 420)))[0]
        return p[::-1].copy() if k % 8 == 0 else p
    n = int(rng.integers(120, 400))
    if k % 4 == 1:                                                    # a lattice: many equal curvatures
        return (rng.integers(-3, 4, (n, 3)) / 8.0 + np.array([10.0, 0.0, -1.0])).astype(np.float32)
    az = np.linspace(-3.0, 3.0, n)
    t = 10.0 + rng.normal(0, 0.01, n) + 1.5 * (rng.uniform(size=n) < 0.05) + np.cumsum(rng.normal(0, 0.02, n))
    return np.stack([t * np.cos(az), t * np.sin(az), -0.1 * t], 1).astype(np.float32)


def test_the_restatement_equals_a_literal_transcription_on_200_random_rings():
    rng = np.random.default_rng(7)
    n_edges = n_tied = 0
    for k in range(200):
        p = random_ring(rng, k)
        opt = F.options(num_sectors=int(rng.choice([1, 3, 6, 7])), max_edges_per_sector=int(rng.choice([0, 2, 20])), min_ring_points=int(rng.choice([11, 131])))
        got = F.ring_features(p, opt)
        want = literal_ring([tuple(q) for q in p], opt)
        assert got == want, (k, opt)
        n_edges += len(got[0])
        v = F.curvature(p) if len(p) >= 11 else np.zeros(0)
        n_tied += len(v) - len(np.unique(v))
    assert n_edges > 500 and n_tied > 5000
    p, c1, g = F.lattice_ring()
    assert F.curvature(p)[c1 - 5] == 0.1 and F.gap2(p, g + 1, g) == 0.05       # exactly ON the thresholds: '<=' stops the walk, '>' does not stop the marks
    e, s = F.ring_features(p, O)
    v = F.curvature(p)
    at = [q for q in range(c1 + 2, c1 + 7) if v[q - 5] == 0.1]                 # ties exactly at 0.1 that no pick marks: surf, never edges
    assert len(at) == 5 and all(q in s and q not in e for q in at) and g in e and g + 1 not in s and g + 1 not in e


# ---- 3. hand-computed answers ----
def test_sectors_of_a_131_point_ring_and_nothing_from_130_points():
    assert F.sector_bounds(131, 6) == [(0, 19), (20, 39), (40, 59), (60, 79), (80, 99), (100, 120)]
    assert [hi - lo for lo, hi in F.sector_bounds(131, 6)] == [19, 19, 19, 19, 19, 20]
    rng = np.random.default_rng(0)
    p = (np.array([10.0, 0.0, -1.0]) + rng.normal(0, 1e-3, (131, 3))).astype(np.float32)      # smooth: everything is surf
    e, s = F.ring_features(p, O)
    assert e == [] and sorted(set(range(5, 126)) - set(s)) == [5 + q for q in (19, 39, 59, 79, 99, 120)]
    assert F.ring_features(p[:130], O) == ([], [])


def test_25_isolated_spikes_give_20_edges_and_the_21st_is_in_neither_list():
    p, info = F.quirk_ring()
    e, s = F.ring_features(p, O)
    spikes = info["spikes"]
    in_e = [q for q in spikes if q in e]
    neither = [q for q in spikes if q not in e and q not in s]
    assert len(in_e) == 20 and len(neither) == 1 and len([q for q in spikes if q in s]) == 4
    # the kink on the last entry of sector 0 is an edge; its marks reach into sector 1, whose entries are all in the output all the same
    k, ln = info["kink"], info["sector_len"]
    assert k in e and k == 5 + ln - 2 and (k + 1) not in e + s                # k + 1: the entry no sector owns
    assert all(q in e + s for q in range(k + 2, k + 6))
    assert all(q not in e + s for q in range(k - 5, k))                       # inside sector 0 the marks do remove


def test_ring_ids_at_the_centre_of_every_ring():
    for lines in (16, 32, 64):
        el = np.array([F.ring_centre(lines, r) for r in range(lines)])
        ring, cnt = F.classify(F.points_at(np.zeros(lines), np.full(lines, 10.0), el), F.options(num_lines=lines))
        assert ring.tolist() == list(range(lines)) and cnt == dict(n_nonfinite=0, n_out_of_range=0, n_no_ring=0)
    # the truncation towards zero and the edges of the fans
    pt = lambda e: F.points_at([0.0], [10.0], [e])
    assert F.classify(pt(-16.5), F.options(num_lines=16))[0][0] == 0 and F.classify(pt(-18.5), F.options(num_lines=16))[0][0] == -1
    assert F.classify(pt(16.5), F.options(num_lines=16))[0][0] == -1
    assert F.classify(pt(2.1), O)[0][0] == -1 and F.classify(pt(-24.4), O)[0][0] == -1 and F.classify(pt(-8.9), O)[0][0] == 32 and F.classify(pt(-8.7), O)[0][0] == 32


def test_every_gpu_fixture_keeps_its_distance_from_the_boundaries():
    for name, (scan, opt) in F.fixtures().items():
        am, dm = F.ring_margin(scan, opt)
        assert am >= 0.01 and dm >= 1e-3, (name, am, dm)
    s, want = F.poison_scan()
    got = F.extract(s, O)
    assert {k: got[k] for k in want} == want

"""Sim3 RANSAC, without a device (include/iba_mi355x.h, iba_sim3*): the symbols and struct layouts, every argument check through the C ABI, the host
restatement (iba_debug_sim3_host) against tests/sim3_ref.py byte for byte on the scene list, the helpers (the constructor's walk against an
object-style walk, Z6, iterate as a fold against a sequential iterate loop, the sets, the composition), the two CPU measurements and the stand-alone
sanitizer program. Every case a test names is first asserted on the REFERENCE restatement's own output."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import sim3_ref as R
import sim3_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
F, D = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sm():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".sim3")


@pytest.fixture(scope="module")
def fz():
    return importlib.import_module(PKG + ".fuse")


@pytest.fixture(scope="module")
def err():
    return importlib.import_module(PKG).IbaError


@pytest.fixture(scope="module")
def listed():
    sc = S.scene_list()
    return sc, S.ref_run(sc)


# ---- symbols, layouts, ABI ----

def test_symbols_layouts_defaults_and_rules(sm):
    L = sm._lib()
    names = ("iba_default_sim3_options", "iba_sim3_last_error", "iba_sim3_solve", "iba_sim3_free", "iba_sim3_n_jobs", "iba_sim3_read", "iba_sim3_counts", "iba_sim3_event",
             "iba_sim3_best", "iba_sim3_iterations", "iba_sim3_correspondences", "iba_sim3_sets", "iba_sim3_budget", "iba_sim3_iterate", "iba_sim3_compose",
             "iba_debug_sim3_host", "iba_debug_sim3_stage_ms", "iba_debug_sim3_chunks")
    pkg = importlib.import_module(PKG)
    hdr = "".join(open(p).read() for p in pkg.HEADER_PATHS)
    for name in names:
        getattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared"
    o = sm.sim3_options()
    assert (o.struct_size, o.probability, o.min_inliers, o.max_iterations, o.fix_scale, o.max_events, o.keep_stages) == (C.sizeof(sm.IbaSim3Options), 0.99, 20, 300, 0, 1, 0)
    assert C.sizeof(sm.IbaSim3Options) == 32 and sm.IbaSim3Options.probability.offset == 8 and sm.IbaSim3Options.keep_stages.offset == 28
    assert C.sizeof(sm.IbaSim3Job) == 96 and sm.IbaSim3Job.sets.offset == 48 and sm.IbaSim3Job.n.offset == 56 and sm.IbaSim3Job.fx1.offset == 64 and sm.IbaSim3Job.cy2.offset == 92
    assert C.sizeof(sm.IbaSim3Result) == 32 and sm.IbaSim3Result.best_it.offset == 20
    assert L.iba_sim3_last_error() is not None and L.iba_sim3_n_jobs(None) == 0
    for rule in ("Z1 thresholds", "Z2 preparation", "Z3 Horn", "Z4 rotation", "Z5 score", "Z6 budget", "Z7 the sequential rule", "Z8 status", "TRUNCATED",
                 "ties go to\n *                  the LATER iteration", "THE LOWEST KEYPOINT INDEX IS ITS GetIndexInKeyFrame", "raise max_events", "IBA_SIM3_COUNT_FORM",
                 "IBA_SIM3_BUDGET", "IBA_SIM3_TIMING", "SearchByBoW (it needs the vocabulary), SearchBySim3, OptimizeSim3, the covisibility consistency check, CorrectLoop"):
        assert rule in hdr, rule
    for k in range(1, 9):
        assert re.search(r"\bZ%d " % k, hdr)
    assert re.search(r"#define IBA_ABI_VERSION 4\b", hdr)
    for name, value in (("MAX_ITERATIONS", 4096), ("MAX_EVENTS", 16), ("TILE", 256)):
        assert re.search(r"#define IBA_SIM3_%s %d\b" % (name, value), hdr) and getattr(sm, name) == value
    for code, name in enumerate(("OK", "NO_MORE", "TOO_FEW")):
        assert re.search(r"IBA_SIM3_%s = %d\b" % (name, code), hdr) and getattr(sm, name) == code and getattr(R, name) == code


# ---- argument checks: all before the device is touched (device -1 would fail otherwise with another status) ----

def _expect(err, fn, text, status=1):
    with pytest.raises(err) as e:
        fn()
    assert e.value.status == status, str(e.value)
    assert text in str(e.value), str(e.value)


def test_argument_checks(sm, err):
    sc = S.scene([{"N": 30, "outliers": 0.2, "max_iterations": 10}], seed=2, max_iterations=10, min_inliers=5, probability=0.999999)
    j0 = sc["jobs"][0]

    def call(xyz=None, **kw):
        opts = {k: kw.pop(k) for k in list(kw) if k in dict(sm.IbaSim3Options._fields_)}
        j = dict(j0, **{k: np.array(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()})
        return S.lib_solve(sm, {"xyz": sc["xyz"] if xyz is None else xyz, "jobs": [j], "opts": dict(sc["opts"], **opts)}, device=-1)

    def edited(key, at, value):
        a = np.array(j0[key])
        a[at] = value
        return {key: a}

    # the good call reaches the device and fails there, with another status
    with pytest.raises(err) as e:
        call()
    assert e.value.status != 1, str(e.value)
    L, A = sm._lib(), C.addressof
    tb, lj, o, p = sm.table(sc["xyz"]), S.lib_job(sm, j0), sm.sim3_options(**sc["opts"]), C.c_void_p(None)
    good = [A(tb), A(lj), 1, A(o), -1, A(p)]
    for at, value, text in ((5, None, b"out is NULL"), (0, None, b"points is NULL"), (1, None, b"jobs is NULL"), (3, None, b"opt is NULL"), (2, 0, b"J < 1")):
        args = list(good)
        args[at] = value
        assert L.iba_sim3_solve(*args) == 1 and text in L.iba_sim3_last_error(), text
        host = args[:4] + args[5:]
        assert L.iba_debug_sim3_host(*host) == 1 and text in L.iba_sim3_last_error(), text
    for field in ("Tcw12_1", "Tcw12_2", "point1", "point2", "max_err1", "max_err2", "sets"):
        bad = sm.IbaSim3Job()
        C.memmove(A(bad), A(lj), C.sizeof(sm.IbaSim3Job))
        setattr(bad, field, None)
        assert L.iba_sim3_solve(A(tb), A(bad), 1, A(o), -1, A(p)) == 1 and b"NULL" in L.iba_sim3_last_error(), field
    _expect(err, lambda: call(struct_size=8), "struct_size")
    _expect(err, lambda: call(probability=1.0), "probability is outside (0, 1)")
    _expect(err, lambda: call(probability=0.0), "probability is outside (0, 1)")
    _expect(err, lambda: call(probability=float("nan")), "probability is outside (0, 1)")
    _expect(err, lambda: call(min_inliers=2), "min_inliers < 3")
    _expect(err, lambda: call(max_iterations=0), "max_iterations = 0 is outside 1..4096")
    _expect(err, lambda: call(max_iterations=4097), "max_iterations = 4097")
    _expect(err, lambda: call(max_events=0), "max_events = 0 is outside 1..16")
    _expect(err, lambda: call(max_events=17), "max_events = 17")
    _expect(err, lambda: call(**edited("point1", 3, len(sc["xyz"]))), "job 0: correspondence 3 names a point outside the table's 60")
    _expect(err, lambda: call(**edited("point2", 4, -1)), "correspondence 4 names a point outside")
    _expect(err, lambda: call(**edited("Tcw1", (1, 2), np.inf)), "a pose entry is not finite")
    _expect(err, lambda: call(**edited("Tcw2", (0, 3), np.nan)), "a pose entry is not finite")
    _expect(err, lambda: call(K1=(500.0, 500.0, np.nan, 240.0)), "an intrinsic is not finite")
    _expect(err, lambda: call(K2=(500.0, 0.0, 320.0, 240.0)), "fx or fy <= 0")
    _expect(err, lambda: call(K1=(-1.0, 500.0, 320.0, 240.0)), "fx or fy <= 0")
    _expect(err, lambda: call(**edited("max_err1", 7, np.nan)), "the threshold of correspondence 7 is not finite")
    _expect(err, lambda: call(**edited("max_err2", 0, np.inf)), "the threshold of correspondence 0 is not finite")
    xyz = sc["xyz"].copy()
    xyz[j0["point2"][2], 1] = np.nan
    _expect(err, lambda: call(xyz=xyz), "the table point of correspondence 2 is not finite")
    _expect(err, lambda: call(**edited("sets", (4, 1), 30)), "set 4 holds the index 30 outside [0, 30)")
    _expect(err, lambda: call(**edited("sets", (9, 0), -1)), "set 9 holds the index -1")
    s = np.array(j0["sets"])
    s[6] = (5, 9, 5)
    _expect(err, lambda: call(sets=s), "set 6 repeats an index")


def test_legal_too_few_and_accessor_checks(sm, err, listed):
    sc, refs = listed
    # a job with N < min_inliers is legal, needs no sets and gets a status; so does n == 0
    few = dict(sc["jobs"][2], sets=None)
    assert len(few["point1"]) == 12
    empty = dict(few, point1=np.zeros(0, np.int32), point2=np.zeros(0, np.int32), max_err1=np.zeros(0, F), max_err2=np.zeros(0, F))
    res = S.lib_solve(sm, dict(sc, jobs=[few, empty]), host=True)
    assert [res.read(b)["status"] for b in range(2)] == [R.TOO_FEW] * 2 and res.read(1)["n"] == 0 and res.iterate(0, 0, 5) == (0, -1, True)
    assert len(res.counts(0)) == 0 and res.best(0)["iteration"] == -1
    res.close()
    res = S.lib_solve(sm, sc, host=True, max_events=2)
    assert refs[0]["n_events"] > 2 and refs[1]["n_events"] == 0
    _expect(err, lambda: res.read(7), "job 7 is outside the result's 7 jobs")
    _expect(err, lambda: res.counts(-1), "job -1 is outside")
    _expect(err, lambda: res.event(0, 2), "event 2 is at or above max_events = 2: raise max_events")
    _expect(err, lambda: res.event(1, 0), "event 0 is outside the job's 0 events")
    _expect(err, lambda: res.event(0, -1), "negative")
    _expect(err, lambda: res.iterations(0), "the call did not ask for keep_stages")
    _expect(err, lambda: res.iterate(0, refs[0]["iterations"] + 1, 5), "from_it is outside")
    _expect(err, lambda: res.iterate(0, 0, -1), "n < 0")
    res.close()
    L = sm._lib()
    assert L.iba_sim3_read(None, 0, None) == 1 and b"the result is NULL" in L.iba_sim3_last_error()


# ---- the host restatement against the reference restatement ----

@pytest.mark.parametrize("keep", [1, 0])
def test_host_restatement_matches_the_reference_bytes(sm, listed, keep):
    sc, refs = listed
    assert [r["status"] for r in refs].count(R.OK) >= 3 and R.NO_MORE in [r["status"] for r in refs] and refs[2]["status"] == R.TOO_FEW
    assert len({r["n"] for r in refs}) > 3 and len({r["iterations"] for r in refs}) > 3
    assert refs[4]["n"] == 20 and refs[4]["iterations"] == 1                    # N == min_inliers: one iteration
    assert refs[6]["n_events"] == 3 and [e["iteration"] for e in refs[6]["events"]] == [4, 9, 17]
    res = S.lib_solve(sm, sc, host=True, keep_stages=keep, max_events=3)
    S.compare(res, refs, {"max_events": 3}, keep)
    assert res.n_chunks == 0
    res.close()


def test_host_edge_scenes(sm):
    """fix_scale, the degenerate triple and a point behind a camera through the host restatement"""
    sc = S.scene([{"N": 40, "outliers": 0.2, "max_iterations": 30}], seed=6, max_iterations=30, min_inliers=3, probability=0.999999, fix_scale=1)
    refs = S.ref_run(sc)
    assert (refs[0]["s"] == F(1.0)).all()
    S.compare(S.lib_solve(sm, sc, host=True, keep_stages=1), refs, sc["opts"], True)
    sc = S.scene([{"N": 30, "outliers": 0.2, "max_iterations": 8}], seed=3, max_iterations=8, min_inliers=3, probability=0.999999)
    j = sc["jobs"][0]
    sc["xyz"][j["point1"]], sc["xyz"][j["point2"]] = R.to_camera(j["Tcw1"], sc["xyz"][j["point1"]]), R.to_camera(j["Tcw2"], sc["xyz"][j["point2"]])
    j["Tcw1"], j["Tcw2"] = np.eye(3, 4, dtype=F), np.eye(3, 4, dtype=F)
    sc["xyz"][j["point1"][:3]], sc["xyz"][j["point2"][:3]] = (0.5, 0.25, 4.0), (0.25, -0.5, 3.0)
    sc["xyz"][j["point2"][9]] = (0.3, 0.2, -2.0)                                # behind camera 2
    j["sets"][:] = (29, 28, 27)
    j["sets"][0] = (0, 1, 2)
    refs = S.ref_run(sc)
    r = refs[0]
    assert np.isnan(r["s"][0]) and np.isnan(r["R"][0]).all() and r["counts"][0] == 0 and not r["inlier"][:, 9].any() and r["solver"].c2[9, 2] < 0
    S.compare(S.lib_solve(sm, sc, host=True, keep_stages=1), refs, sc["opts"], True)


# ---- iba_sim3_correspondences against an object-style walk ----

class _MapPoint:
    def __init__(self, pid, bad):
        self.id, self.bad, self.obs = pid, bad, {}

    def index_in(self, kf):
        return self.obs.get(kf, -1)


def _object_walk(holders, bad, matches12, octs, sigma2):
    """Sim3Solver's constructor on objects: holders[k] = keyframe k's mvpMapPoints as ids or -1"""
    pts = {}
    for k, h in enumerate(holders):
        for i, pid in enumerate(h):
            if pid >= 0:
                mp = pts.setdefault(pid, _MapPoint(pid, bool(bad[pid])))
                mp.obs.setdefault(k, i)                                          # the lowest keypoint index is its GetIndexInKeyFrame
    for pid in matches12:
        if pid >= 0:
            pts.setdefault(pid, _MapPoint(pid, bool(bad[pid])))
    out = {"index1": [], "point1": [], "point2": [], "max_err1": [], "max_err2": []}
    for i1, p2 in enumerate(matches12):
        if p2 < 0:
            continue
        p1 = holders[0][i1]
        if p1 < 0:
            continue
        mp1, mp2 = pts[p1], pts[p2]
        if mp1.bad or mp2.bad:
            continue
        a, b = mp1.index_in(0), mp2.index_in(1)
        if a < 0 or b < 0:
            continue
        out["index1"].append(i1)
        out["point1"].append(p1)
        out["point2"].append(p2)
        out["max_err1"].append(R.truncated_threshold(sigma2[octs[0][a]]))
        out["max_err2"].append(R.truncated_threshold(sigma2[octs[1][b]]))
    return {k: np.array(v, F if k.startswith("max") else np.int32) for k, v in out.items()}


def test_correspondences_walk(sm, fz, err):
    rng = np.random.default_rng(4)
    n1, n2, P = 40, 35, 120
    h1 = rng.permutation(60)[:n1].astype(np.int32)
    h2 = (60 + rng.permutation(60)[:n2]).astype(np.int32)
    h1[[3, 11]] = -1                                                           # keypoints without a point
    h1[20] = h1[5]                                                             # a point held twice in keyframe 1: keypoint 5 is its index
    h2[30] = h2[2]                                                             # and one in keyframe 2
    matches = np.full(n1, -1, np.int32)
    pick = rng.permutation(n1)[:28]
    matches[pick] = h2[rng.integers(0, n2, 28)]
    matches[0], matches[1], matches[5], matches[20] = 119, h2[2], h2[4], h2[4]  # 119: a point absent from keyframe 2
    bad = np.zeros(P, np.uint8)
    bad[h1[7]], bad[matches[1]] = 1, 1
    matches[7] = h2[0] if matches[7] < 0 else matches[7]
    o1, o2 = rng.integers(0, 8, n1).astype(np.int32), rng.integers(0, 8, n2).astype(np.int32)
    o1[5], o1[20], o2[2], o2[30] = 1, 6, 2, 7
    fmap = fz.FuseMap(np.array([0, n1, n1 + n2], np.int32), np.concatenate([h1, h2]), P, bad=bad)
    want = _object_walk([h1, h2], bad, matches, (o1, o2), S.LEVEL_SIGMA2)
    # the cases are in the input: a NULL match, a keypoint without a point, bad points on either side, an absent point, a point held twice
    assert (matches < 0).any() and 0 not in want["index1"] and 1 not in want["index1"] and 7 not in want["index1"] and 3 not in want["index1"]
    assert 5 in want["index1"] and 20 in want["index1"] and len(want["index1"]) > 10
    k5, k20 = list(want["index1"]).index(5), list(want["index1"]).index(20)
    assert want["max_err1"][k5] == want["max_err1"][k20] == F(13.0) and S.LEVEL_SIGMA2[1] == F(1.44)      # both from keypoint 5's octave 1: 13, not 13.26
    got = sm.correspondences(fmap, 0, 1, matches, o1, o2, S.LEVEL_SIGMA2, S.LEVEL_SIGMA2)
    for k in want:
        assert S.same_bytes(got[k], want[k]), k
    _expect(err, lambda: sm.correspondences(fmap, 0, 2, matches, o1, o2, S.LEVEL_SIGMA2, S.LEVEL_SIGMA2), "kf1 or kf2 is outside the map's 2 keyframes")
    m2 = matches.copy()
    m2[9] = P
    _expect(err, lambda: sm.correspondences(fmap, 0, 1, m2, o1, o2, S.LEVEL_SIGMA2, S.LEVEL_SIGMA2), "names a point outside the map's 120")
    _expect(err, lambda: sm.correspondences(fmap, 0, 1, matches, o1, o2, S.LEVEL_SIGMA2[:1], S.LEVEL_SIGMA2), "an octave is outside its level table")
    L = sm._lib()
    assert L.iba_sim3_correspondences(*([None] * 1 + [0, 1] + [None] * 5 + [1, 1] + [None] * 6)) == 1 and b"NULL" in L.iba_sim3_last_error()


def test_truncated_threshold_makes_an_outlier(sm):
    """a correspondence whose error lies between 13 and 13.26 is an outlier under the truncated bound of level 1"""
    assert R.truncated_threshold(1.44) == F(13.0) and 9.210 * 1.44 > 13.26
    sc = S.scene([{"N": 24, "outliers": 0.0, "noise_px": 0.0, "max_iterations": 4}], seed=8, max_iterations=4, min_inliers=3, probability=0.999999)
    j = sc["jobs"][0]
    j["max_err1"][:], j["max_err2"][:] = F(13.0), F(1e6)
    sv = R.Solver(sc["xyz"], j, min_inliers=3, max_iterations=4, probability=0.999999)
    h = sv.hypothesis(0)
    # move correspondence 10's point in camera 1 sideways until its error in image 1 lies between the two bounds
    T1 = j["Tcw1"].astype(D)
    for shift in np.linspace(0.0, 0.2, 4001):
        c1 = sv.c1[10].astype(D) + (shift, 0, 0)
        sc["xyz"][j["point1"][10]] = ((c1 - T1[:, 3]) @ T1[:, :3]).astype(F)
        s2 = R.Solver(sc["xyz"], j, min_inliers=3, max_iterations=4, probability=0.999999)
        e1 = R.reproject_err(h["T12"], np.asarray(j["K1"], F), s2.c2, s2.u1, s2.v1)[10]
        if e1 > 13.05:
            break
    assert 10 not in j["sets"][:4] and 13.0 < e1 < 13.26, e1
    refs = S.ref_run(sc)
    assert not refs[0]["inlier"][0, 10] and refs[0]["counts"][0] == 23
    j13 = dict(j, max_err1=np.full(24, F(13.26)))
    assert S.ref_run(dict(sc, jobs=[j13]))[0]["counts"][0] == 24                # under the untruncated bound it would be an inlier
    res = S.lib_solve(sm, sc, host=True, keep_stages=1)
    S.compare(res, refs, sc["opts"], True)
    res.close()


# ---- Z6, the sets, the composition ----

def test_budget(sm):
    assert sm.budget(20) == R.budget(20) == 1 and sm.budget(25) == R.budget(25) == 7 and sm.budget(100) == R.budget(100) == 300
    assert sm.budget(2 * 10 ** 9) == 300 and R.budget(2 * 10 ** 9) == 300                         # 1 - eps^3 == 1: the quotient is not finite
    assert 1.0 - float(F(20) / F(2 * 10 ** 9)) ** 3 == 1.0
    for N in list(range(20, 140)) + [500, 4097]:
        for kw in ({}, {"min_inliers": 3}, {"probability": 0.5, "max_iterations": 4096}, {"probability": 0.999999, "min_inliers": 19}):
            if N >= kw.get("min_inliers", 20):
                assert sm.budget(N, **kw) == R.budget(N, **kw), (N, kw)
    L = sm._lib()
    o = sm.sim3_options()
    it = C.c_int32(0)
    assert L.iba_sim3_budget(0, C.addressof(o), C.addressof(it)) == 1 and L.iba_sim3_budget(30, None, C.addressof(it)) == 1 and L.iba_sim3_budget(30, C.addressof(o), None) == 1


def test_sets(sm, err):
    s = sm.sets(40, 300, seed=3)
    assert s.shape == (300, 3) and s.min() >= 0 and s.max() < 40 and all(len(set(r)) == 3 for r in s.tolist())
    assert S.same_bytes(s, sm.sets(40, 300, seed=3)) and not S.same_bytes(s, sm.sets(40, 300, seed=4)) and len({tuple(r) for r in s.tolist()}) > 250
    assert sorted(sm.sets(3, 1)[0].tolist()) == [0, 1, 2]
    # the swap-with-back draw over splitmix64, restated
    def splitmix(state):
        state = (state + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z = state
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return state, z ^ (z >> 31)
    state, want = 3, []
    for _ in range(5):
        avail = list(range(40))
        for _ in range(3):
            state, z = splitmix(state)
            k = z % len(avail)
            want.append(avail[k])
            avail[k] = avail[-1]
            avail.pop()
    assert s[:5].reshape(-1).tolist() == want
    _expect(err, lambda: sm.sets(2, 10), "N = 2 is below 3")
    _expect(err, lambda: sm.sets(10, 0), "iterations = 0 is outside 1..4096")
    _expect(err, lambda: sm.sets(10, 4097), "iterations = 4097")


def test_compose(sm):
    rng = np.random.default_rng(1)
    Rcm, tcm, s = S.rot(0.2, -0.1, 0.4).astype(F), rng.normal(0, 1, 3).astype(F), F(1.3)
    Tmw = S.pose(-0.3, 0.2, 0.1, (0.5, -1.0, 2.0))
    so, Ro, to = sm.compose(s, Rcm, tcm, Tmw)
    assert so == float(s) and Ro.dtype == D
    assert np.max(np.abs(Ro - Rcm.astype(D) @ Tmw[:, :3].astype(D))) < 1e-15
    assert np.max(np.abs(to - (D(s) * (Rcm.astype(D) @ Tmw[:, 3].astype(D)) + tcm.astype(D)))) < 1e-15
    x = rng.normal(0, 1, 3)                                                    # Scw x = Scm (Tmw x)
    assert np.max(np.abs((so * Ro @ x + to) - (D(s) * Rcm.astype(D) @ (Tmw[:, :3].astype(D) @ x + Tmw[:, 3].astype(D)) + tcm.astype(D)))) < 1e-14
    L = sm._lib()
    assert L.iba_sim3_compose(C.c_float(1.0), None, None, None, None, None, None) == 1


# ---- iterate as a fold ----

def test_iterate_in_slices_of_five_replays_the_sequential_loop(sm):
    sc = S.three_event_scene()
    j = sc["jobs"][0]
    sv = R.Solver(sc["xyz"], j, **sc["opts"])
    want = []
    for _ in range(12):                                                        # the sequential loop: iterate(5) until nothing is left, and twice more
        e, no_more = sv.iterate(5)
        want.append((sv.n_iterations, -1 if e is None else len(sv.events) - 1, no_more))
    assert [w[1] for w in want if w[1] >= 0] == [0, 1, 2] and want[0] == (5, 0, False) and want[-1] == (30, -1, True) and [e["iteration"] for e in sv.events] == [4, 9, 17]
    assert (10, 1, False) in want and any(w[2] for w in want[:-2])
    for host_events in (3, 1):
        res = S.lib_solve(sm, sc, host=True, max_events=host_events)
        at, got = 0, []
        for _ in range(12):
            at, ev, nm = res.iterate(0, at, 5)
            got.append((at, ev, nm))
        assert got == want
        for k in range(host_events):
            assert res.event(0, k)["iteration"] == sv.events[k]["iteration"]
        assert res.iterate(0, 0, 300) == (5, 0, False) and res.iterate(0, 18, 300) == (30, -1, True) and res.iterate(0, 3, 0) == (3, -1, False)
        res.close()


# ---- the two CPU measurements (profiles/sim3_parity.md) ----

MEASURED_S, MEASURED_R, MEASURED_T = 4.59e-07, 9.23e-06, 4.58e-05    # the largest differences over the scene list, measured with tools/sim3_parity.py


def test_rules_beside_a_float64_solution(listed):
    """s, R, t of the rules beside numpy.linalg.eigh in float64 on the same triples: within 4 x the largest difference measured on the scene list"""
    sc, refs = listed
    ds, dR, dt = S.measure_float64(sc, refs)
    print("largest differences: s %.3e, R %.3e, t %.3e" % (ds, dR, dt))
    assert ds <= 4 * MEASURED_S and dR <= 4 * MEASURED_R and dt <= 4 * MEASURED_T


def test_rotation_beside_the_angle_axis_route(listed):
    """Z4 beside quaternion -> atan2 -> angle-axis -> Rodrigues in float64: the run reproduces the numbers profiles/sim3_parity.md records"""
    sc, refs = listed
    worst, differ, total = S.measure_angle_axis(sc, refs)
    print("largest entry difference %.3e, %d of %d verdicts differ" % (worst, differ, total))
    text = open(os.path.join(ROOT, "profiles", "sim3_parity.md")).read()
    m = re.search(r"\| inlier verdicts that differ \| (\d+) of (\d+) \|", text)
    assert m and (int(m.group(1)), int(m.group(2))) == (differ, total)
    m = re.search(r"\| largest entry difference of R \| ([0-9.e+-]+) \|", text)
    assert m and "%.3e" % worst == m.group(1)
    assert worst <= 2.0 ** -22                                                 # two float32 roundings of entries in [-1, 1] differ by an ulp or two at most


# ---- the sanitizer program ----

def test_selftest_program_builds_and_passes():
    """the stand-alone sanitizer program over the host half, the shared arithmetic and the helpers: plain g++, run on the CPU as a child process"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(importlib.import_module(PKG).__file__)), "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "san/sim3_selftest_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "san", "sim3_selftest_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "sim3_selftest ok" in r.stdout, r.stdout + r.stderr

"""New-map-point creation, without a device (include/iba_mi355x.h, iba_triangulate*): the symbols and struct layouts, every argument check, the host
restatement (iba_debug_triangulate_host) against tests/triangulate_ref.py byte for byte, R3's minimum against the literal walk, the median depth and
the known answer on noise-free geometry. Every case a test names is first asserted on the REFERENCE's own output.

Statuses the scenes cannot reach under the default options (tests/triangulate_scene.py says why): DEGENERATE and REPROJ2 occur under
triangulate_scene.OPEN and are asserted there; ZERO_DIST occurs in no call (z_i <= 0 comes first when x3D is a camera centre) and is reached by the
stand-alone self-test with a hand-made centre."""
import ctypes as C
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

import triangulate_ref as R
import triangulate_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
F = np.float32


@pytest.fixture(scope="module")
def tr():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".triangulate")


@pytest.fixture(scope="module")
def om():
    return importlib.import_module(PKG + ".orb_match")


@pytest.fixture(scope="module")
def err():
    return importlib.import_module(PKG).IbaError


@pytest.fixture(scope="module")
def hand():
    sc = S.hand_scene()
    return sc, R.run(sc["frames"], sc["keyframes"], sc["jobs"])


@pytest.fixture(scope="module")
def rand():
    sc = S.random_scene()
    return sc, R.run(sc["frames"], sc["keyframes"], sc["jobs"])


# ---- symbols, layouts, ABI ----

def test_symbols_and_layouts(tr):
    L = tr._lib()
    names = ("iba_default_triangulate_options", "iba_triangulate_last_error", "iba_triangulate", "iba_triangulation_free", "iba_triangulation_n_jobs", "iba_triangulation_job",
             "iba_triangulation_read", "iba_triangulation_points", "iba_triangulation_segments", "iba_triangulate_median_depth", "iba_debug_triangulate_host",
             "iba_debug_triangulate_chunks", "iba_debug_triangulate_stage_ms")
    pkg = importlib.import_module(PKG)
    hdr = "".join(open(p).read() for p in pkg.HEADER_PATHS)
    for name in names:
        getattr(L, name)
        assert re.search(r"\b%s\s*\(" % name, hdr), name + " is not declared"
    assert L.iba_abi_version() == 4 and re.search(r"#define\s+IBA_ABI_VERSION\s+4\b", hdr)
    o = tr.triangulate_options()
    assert (o.struct_size, o.th_low, o.keep_stages) == (C.sizeof(tr.IbaTriangulateOptions), 50, 0)
    assert (o.min_baseline_ratio, o.max_cos_parallax, o.epipole_gate, o.chi2_line, o.chi2_mono) == (F(0.01), F(0.9998), F(100.0), F(3.84), F(5.991))
    assert C.sizeof(tr.IbaTriangulateOptions) == 32 and tr.IbaTriangulateOptions.keep_stages.offset == 28
    assert C.sizeof(tr.IbaTriangulateKeyframe) == 48 and tr.IbaTriangulateKeyframe.median_depth.offset == 20 and tr.IbaTriangulateKeyframe.Tcw12.offset == 24
    assert tr.IbaTriangulateKeyframe.node.offset == 32 and tr.IbaTriangulateKeyframe.has_point.offset == 40
    assert C.sizeof(tr.IbaTriangulateJob) == 40 and tr.IbaTriangulateJob.scale_factor.offset == 12 and tr.IbaTriangulateJob.neighbours.offset == 16
    assert tr.IbaTriangulateJob.level_sigma2.offset == 32
    assert C.sizeof(tr.IbaTriangulateCounts) == 4 * 17 and tr.IbaTriangulateCounts.status.offset == 8 and tr.IbaTriangulateCounts.n_created.offset == 64
    assert re.search(r"#define\s+IBA_TRIANGULATE_BYTES_PER_SLOT\s+%dull" % tr.BYTES_PER_SLOT, hdr) and re.search(r"#define\s+IBA_TRIANGULATE_N_STATUS\s+14\b", hdr)
    assert L.iba_triangulate_last_error() is not None
    assert L.iba_triangulation_n_jobs(None) == 0 and L.iba_debug_triangulate_chunks(None) == 0
    for rule in ("R1 pair prologue", "R2 queries", "R3 pick", "R4 rays", "R5 triangulation", "R6 gates", "R7 first neighbour wins", "R8 the new point", "NOT PROVIDED",
                 "ORBmatcher matcher(0.6,false)", "never sets vbMatched2", "WHY THE WALK IS A MINIMUM", "IBA_TRIANGULATE_BUDGET", "SearchByBoW and SearchForTriangulation"):
        assert rule in hdr, rule
    for i, name in enumerate(R.NAMES):
        assert re.search(r"IBA_TRIANGULATE_%s = %d\b" % (name, i), hdr), name


# ---- argument checks: all before the device is touched (device -1 would fail otherwise with another status) ----

def _expect(err, fn, text):
    with pytest.raises(err) as e:
        fn()
    assert e.value.status == 1, str(e.value)
    assert text in str(e.value), str(e.value)


def test_argument_checks(tr, om, err, hand):
    sc, _ = hand
    fr, kf, jb = S.lib_args(tr, om, sc)
    k0, j0 = sc["keyframes"][0], sc["jobs"][0]
    call = lambda frames=fr, keyframes=kf, jobs=jb[:1], **kw: tr.triangulate(frames, keyframes, jobs, device=-1, **kw)
    keyframe = lambda **kw: tr.keyframe(**{**dict(frame=0, Tcw=k0["Tcw"], K=k0["K"], node=k0["node"], has_point=k0["has_point"], median_depth=5.0), **kw})
    job = lambda **kw: tr.job(**{**dict(current=0, neighbours=[1, 2], scale_factors=S.SF, level_sigma2=S.SIGMA2, scale_factor=1.2), **kw})
    L = tr._lib()
    o = tr.triangulate_options()
    p = C.c_void_p(None)
    fa, ka, ja = tr._array(om.IbaOrbFrame, fr), tr._array(tr.IbaTriangulateKeyframe, kf), tr._array(tr.IbaTriangulateJob, jb)
    A = C.addressof
    nF, nK = len(fr), len(kf)
    # NULLs and counts
    for args, text in (((A(fa), nF, A(ka), nK, A(ja), 1, A(o), -1, None), b"out is NULL"), ((None, nF, A(ka), nK, A(ja), 1, A(o), -1, A(p)), b"frames is NULL"),
                       ((A(fa), nF, None, nK, A(ja), 1, A(o), -1, A(p)), b"keyframes is NULL"), ((A(fa), nF, A(ka), nK, None, 1, A(o), -1, A(p)), b"jobs is NULL"),
                       ((A(fa), nF, A(ka), nK, A(ja), 1, None, -1, A(p)), b"opt is NULL"), ((A(fa), 0, A(ka), nK, A(ja), 1, A(o), -1, A(p)), b"F < 1"),
                       ((A(fa), nF, A(ka), 0, A(ja), 1, A(o), -1, A(p)), b"K < 1"), ((A(fa), nF, A(ka), nK, A(ja), 0, A(o), -1, A(p)), b"J < 1")):
        assert L.iba_triangulate(*args) == 1 and text in L.iba_triangulate_last_error(), text
    assert p.value is None and L.iba_default_triangulate_options(None) == 1
    # options
    _expect(err, lambda: call(struct_size=28), "struct_size")
    for v in (-1, 257):
        _expect(err, lambda: call(th_low=v), "th_low outside [0, 256]")
    for name in ("min_baseline_ratio", "max_cos_parallax", "epipole_gate", "chi2_line", "chi2_mono"):
        for v in (float("nan"), float("inf")):
            _expect(err, lambda: call(**{name: v}), name + " is not finite")
    # frames: what iba_orb_match refuses
    f0 = sc["frames"][0]
    _expect(err, lambda: call(frames=[om.frame(f0["xy"], f0["octave"], f0["angle"], f0["desc"], (0, 0, 0, 480))] + fr[1:]), "max <= min")
    big = 32768 + 1                                                    # IBA_ORB_MATCH_MAX_KEYPOINTS + 1
    _expect(err, lambda: call(frames=fr[:1] + [om.frame(np.zeros((big, 2), F), np.zeros(big, np.int32), np.zeros(big, F), np.zeros((big, 32), np.uint8), S.BOUNDS)] + fr[2:]), "frame 1: n outside [0, 32768]")
    # keyframes
    with_kf = lambda k: [k] + kf[1:]
    _expect(err, lambda: call(keyframes=with_kf(keyframe(frame=len(fr)))), "keyframe 0: a frame index outside")
    _expect(err, lambda: call(keyframes=with_kf(keyframe(frame=-1))), "a frame index outside")
    for k, v, why in ((5, np.nan, "not finite"), (11, np.inf, "not finite"), (3, -3e6, "above 1e6")):
        T = k0["Tcw"].copy(); T[k] = v
        _expect(err, lambda: call(keyframes=with_kf(keyframe(Tcw=T))), "keyframe 0: Tcw12")
        _expect(err, lambda: call(keyframes=with_kf(keyframe(Tcw=T))), why)
    _expect(err, lambda: call(keyframes=with_kf(keyframe(K=(512, np.nan, 320, 240)))), "an intrinsic")
    _expect(err, lambda: call(keyframes=with_kf(keyframe(K=(512, 512, 3e6, 240)))), "above 1e6")
    bad = keyframe(); bad.Tcw12 = None
    _expect(err, lambda: call(keyframes=with_kf(bad)), "Tcw12 is NULL")
    bad = keyframe(); bad.node = None
    _expect(err, lambda: call(keyframes=with_kf(bad)), "node is NULL")
    for v in (0.0, -1.0, np.nan, np.inf):
        ks = [kf[0], keyframe(frame=1, node=sc["keyframes"][1]["node"], has_point=None, median_depth=v)] + kf[2:]
        _expect(err, lambda: call(keyframes=ks), "neighbour 0: median_depth is not finite or <= 0")
    ks = [keyframe(median_depth=0.0)] + kf[1:]                       # of the current keyframe it is not read
    with pytest.raises(err) as e:
        call(keyframes=ks)
    assert e.value.status != 1
    # jobs
    _expect(err, lambda: call(jobs=[job(current=len(kf))]), "current outside the call's keyframes")
    _expect(err, lambda: call(jobs=[job(current=-1)]), "current outside the call's keyframes")
    _expect(err, lambda: call(jobs=[jb[0], job(neighbours=[1, len(kf)])]), "job 1: neighbour 1 outside the call's keyframes")
    _expect(err, lambda: call(jobs=[job(neighbours=[-1])]), "neighbour 0 outside")
    _expect(err, lambda: call(jobs=[job(neighbours=[1, 0])]), "neighbour 1 is the current keyframe")
    _expect(err, lambda: call(jobs=[job(neighbours=[1, 2, 1])]), "neighbour 2 is listed twice")
    bad = job(); bad.n_neighbours = -1
    _expect(err, lambda: call(jobs=[bad]), "n_neighbours < 0")
    bad = job(); bad.neighbours = None
    _expect(err, lambda: call(jobs=[bad]), "neighbours is NULL")
    bad = job(); bad.level_sigma2 = None
    _expect(err, lambda: call(jobs=[bad]), "scale_factors or level_sigma2 is NULL")
    _expect(err, lambda: call(jobs=[job(scale_factors=np.zeros(0, F), level_sigma2=np.zeros(0, F))]), "n_levels outside [1, 64]")
    _expect(err, lambda: call(jobs=[job(scale_factors=np.linspace(1, 2, 65), level_sigma2=np.ones(65))]), "n_levels outside [1, 64]")
    for sf in ([1.2, 1.44], [1.0, 1.2, 1.2], [1.0, 0.9]):
        _expect(err, lambda: call(jobs=[job(scale_factors=sf, level_sigma2=np.ones(len(sf)))]), "does not ascend from 1")
    _expect(err, lambda: call(jobs=[job(scale_factors=[1.0, np.nan], level_sigma2=[1.0, 1.0])]), "scale_factors")
    for v, why in ((np.nan, "level_sigma2"), (2e6, "level_sigma2"), (0.0, "level_sigma2 <= 0")):
        s2 = S.SIGMA2.copy(); s2[2] = v
        _expect(err, lambda: call(jobs=[job(level_sigma2=s2)]), why)
    for v, why in ((np.nan, "scale_factor: "), (0.0, "scale_factor <= 0")):
        _expect(err, lambda: call(jobs=[job(scale_factor=v)]), why)
    _expect(err, lambda: call(jobs=[job(scale_factors=S.SF[:5], level_sigma2=S.SIGMA2[:5])]), "of 5 levels")      # keyframe 1 holds an octave 7
    # the accessors on NULL, and the helper
    assert L.iba_triangulation_job(None, 0, None, None, None) == 1 and L.iba_triangulation_read(None, 0, *[None] * 4) == 1
    assert L.iba_triangulation_points(None, 0, *[None] * 8) == 1 and L.iba_triangulation_segments(None, 0, None) == 1
    assert L.iba_debug_triangulate_stage_ms(None, None) == 1
    L.iba_triangulation_free(None)
    _expect(err, lambda: tr.median_depth(np.eye(3, 4), np.zeros((0, 3))), "n < 1")
    _expect(err, lambda: tr.median_depth(np.eye(3, 4), np.zeros((3, 3)), q=0), "q < 1")


def test_legal_empties_pass_the_checks(tr, om, err, rand):
    """a job with no neighbours, an empty frame as a neighbour and as the current keyframe are legal: the call gets as far as the device (which
    device -1 is not), and the host restatement answers them"""
    sc, refs = rand
    fr, kf, jb = S.lib_args(tr, om, sc)
    assert refs[1]["n_neighbours"] == 0 and refs[3]["n_keypoints"] == 0 and len(sc["frames"][5]["octave"]) == 0 and 5 in sc["jobs"][2]["neighbours"]
    with pytest.raises(err) as e:
        tr.triangulate(fr, kf, [jb[1], jb[3], jb[2]], device=-1)
    assert e.value.status != 1, str(e.value)
    t = tr.triangulate_host(fr, kf, [jb[1], jb[3]])
    assert len(t) == 2 and t.counts(0)["n_created"] == 0 and t.read(1)["status"].shape == (2, 0) and len(t.points(0)["idx1"]) == 0
    t.close()


def test_accessor_checks(tr, om, err, hand):
    sc, refs = hand
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb)
    assert len(t) == len(jb) and t.n_chunks == 0 and not t.stage_ms.any()
    for bad in (-1, len(jb)):
        _expect(err, lambda: t.counts(bad), "outside the result's %d jobs" % len(jb))
        _expect(err, lambda: t.read(bad), "outside the result's")
        _expect(err, lambda: t.points(bad), "outside the result's")
    _expect(err, lambda: t.segments(0), "did not ask for keep_stages")
    assert tr._lib().iba_triangulation_job(t.p, 0, None, None, None) == 1
    S.assert_equal(t, refs, keep_stages=False)          # without keep_stages: the same results
    t.close()


# ---- the rules on the hand scene: every named case occurs in the reference's output, then the host restatement byte for byte ----

def test_hand_scene_limits(hand):
    sc, _ = hand
    assert len(sc["keyframes"]) < 10 and all(len(f["octave"]) <= 200 for f in sc["frames"])


def test_hand_scene_r1_r2(tr, om, hand):
    sc, refs = hand
    w, r, kfs = sc["where"], refs[0], sc["keyframes"]
    nb = sc["jobs"][0]["neighbours"].tolist()
    st = lambda name: r["status"][:, w[name]].tolist()
    # R1: keyframe 4 is skipped, keyframe 5 sits exactly at the ratio and is searched; the epipole of keyframe 1 is not finite
    earlier = (r["status"][:nb.index(4)] == R.CREATED).any(0)
    assert r["skipped"].tolist() == [k == 4 for k in nb] and np.array_equal(r["status"][nb.index(4)], np.where(earlier, R.SUPERSEDED, R.PAIR_SKIPPED))
    at = nb.index(5)
    assert R.div_f(r["baseline"][at], kfs[5]["median_depth"]) == F(0.01) and not r["skipped"][at] and st("at_ratio")[at] == R.CREATED
    assert R.div_f(r["baseline"][nb.index(4)], kfs[4]["median_depth"]) < F(0.01)
    assert R.prologue(R.camera(kfs[0]), R.camera(kfs[5]), np.nextafter(F(0.01), F(1)))[0]            # one ulp more of the option skips it
    ex1 = R.prologue(R.camera(kfs[0]), R.camera(kfs[1]), 0.01)[3:]
    ex2 = R.prologue(R.camera(kfs[0]), R.camera(kfs[2]), 0.01)[3:]
    assert not np.isfinite(ex1).all() and ex2 == (F(320.0), F(240.0))
    # R2: has_point on both sides, a node < 0, a node that occurs nowhere, and the segment lengths
    assert st("has_query") == [R.PAIR_SKIPPED if k == 4 else R.HAS_POINT for k in nb] and kfs[0]["has_point"][w["has_query"]]
    k, i2 = sc["cand"]["has_candidate"]["has"]
    assert kfs[k]["has_point"][i2] and r["n_has_point_walked"] >= 1 and r["match"][0, w["has_candidate"]] == sc["cand"]["has_candidate"]["free"][1]
    assert kfs[0]["node"][w["negative_node"]] < 0 and st("negative_node") == [R.PAIR_SKIPPED if k == 4 else R.NO_NODE for k in nb] and (kfs[1]["node"] < 0).any()
    assert st("segment0") == [R.PAIR_SKIPPED if k == 4 else R.NO_NODE for k in nb] and not r["seg_len"][:, w["segment0"]].any()
    for k, lengths in S.SEGMENTS.items():
        for n in lengths:
            name = "segment%d" % n
            assert r["seg_len"][nb.index(k), w[name]] == n and r["dist"][nb.index(k), w[name]] == 30 and r["match"][nb.index(k), w[name]] == sc["cand"][name]["late"][1], name
    assert {0, 1, 15, 16, 17, 63, 64, 65, 130} <= set(r["seg_len"].reshape(-1).tolist())
    # the node sets interleave: the reference's merge of the two feature vectors has to jump in BOTH directions (lower_bound on either side)
    a, b = sorted(set(kfs[0]["node"][kfs[0]["node"] >= 0].tolist())), sorted(set(kfs[1]["node"][kfs[1]["node"] >= 0].tolist()))
    i = j = jumps1 = jumps2 = shared = 0
    while i < len(a) and j < len(b):
        if a[i] == b[j]:
            shared, i, j = shared + 1, i + 1, j + 1
        elif a[i] < b[j]:
            jumps1, i = jumps1 + 1, int(np.searchsorted(a, b[j]))
        else:
            jumps2, j = jumps2 + 1, int(np.searchsorted(b, a[i]))
    assert jumps1 >= 2 and jumps2 >= 2 and shared >= 10
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb, keep_stages=1)
    S.assert_equal(t, refs)
    t.close()


def test_hand_scene_r3(tr, om, hand):
    sc, refs = hand
    w, c, r = sc["where"], sc["cand"], refs[0]
    m, d, st = (lambda name, pos=0: int(r["match"][pos, w[name]])), (lambda name, pos=0: int(r["dist"][pos, w[name]])), (lambda name, pos=0: int(r["status"][pos, w[name]]))
    # two candidates at equal least distance: the later wins
    assert c["tie"]["first"][1] < c["tie"]["later"][1] and (m("tie"), d("tie")) == (c["tie"]["later"][1], 25) and r["n_equal_replaced"] >= 1
    # exactly th_low is taken, th_low + 1 is not
    assert (m("at_th_low"), d("at_th_low"), st("at_th_low")) == (c["at_th_low"]["true"][1], 50, R.CREATED) and (m("above_th_low"), st("above_th_low")) == (-1, R.NO_MATCH)
    # a better candidate refused by the line test, and one refused by the epipole gate (keyframe 2, position 1)
    assert (m("line_refused"), d("line_refused")) == (c["line_refused"]["true"][1], 30) and r["n_line_refused"] >= 1
    assert (m("epipole_refused", 1), d("epipole_refused", 1)) == (c["epipole_refused"]["true"][1], 30) and r["n_epipole_refused"] >= 1
    k, i2 = c["epipole_refused"]["better"]
    p = sc["frames"][k]["xy"][i2]
    assert (p[0] - 320.0) ** 2 + (p[1] - 240.0) ** 2 < 100.0
    line = R.line_of(R.prologue(R.camera(sc["keyframes"][0]), R.camera(sc["keyframes"][2]), 0.01)[2], *sc["frames"][0]["xy"][w["epipole_refused"]])
    assert R.line_test(line, p[0], p[1], F(1.0), 3.84)[0]                                       # (it is the gate alone that refuses it)
    # den == 0: the query at the epipole of image 1
    assert st("den_zero", 1) == R.NO_MATCH and r["n_den_zero"] >= 1 and r["seg_len"][1, w["den_zero"]] == 1
    line = R.line_of(R.prologue(R.camera(sc["keyframes"][0]), R.camera(sc["keyframes"][2]), 0.01)[2], *sc["frames"][0]["xy"][w["den_zero"]])
    assert line[3] == 0
    # two queries take the same idx2
    assert m("same_idx2_a") == m("same_idx2_b") == c["same_idx2_a"]["true"][1] and st("same_idx2_a") == st("same_idx2_b") == R.CREATED
    # th_low of the options
    low = R.run(sc["frames"], sc["keyframes"], sc["jobs"], th_low=49)
    assert low[0]["status"][0, w["at_th_low"]] == R.NO_MATCH and low[0]["n_created"] == r["n_created"] - 1
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb, keep_stages=1, th_low=49)
    S.assert_equal(t, low)
    t.close()


def test_hand_scene_r4_to_r8(tr, om, hand):
    sc, refs = hand
    w, c, r = sc["where"], sc["cand"], refs[0]
    st = lambda name: r["status"][:, w[name]].tolist()
    nb = sc["jobs"][0]["neighbours"].tolist()
    assert st("parallax")[0] == R.PARALLAX and st("depth1")[0] == R.DEPTH1 and st("depth2")[1] == R.DEPTH2 and st("reproj1")[0] == R.REPROJ1 and st("scale")[0] == R.SCALE
    assert r["xyz"][0, w["parallax"]].tolist() == [0, 0, 0] and r["xyz"][0, w["depth1"], 2] < 0 and r["xyz"][0, w["scale"], 2] > 0
    # every status the default options can reach, and the two that OPEN reaches
    reached = {i for i in range(R.N_STATUS) if r["counts"][i] > 0}
    assert reached == set(range(R.N_STATUS)) - {R.DEGENERATE, R.REPROJ2, R.ZERO_DIST}, [R.NAMES[i] for i in reached]
    opened = R.run(sc["frames"], sc["keyframes"], sc["jobs"], **S.OPEN)
    assert st("degenerate_open")[0] == R.PARALLAX and opened[0]["status"][0, w["degenerate_open"]] == R.DEGENERATE and opened[0]["xyz"][0, w["degenerate_open"]].tolist() == [0, 0, 0]
    assert st("reproj2_open")[0] == R.NO_MATCH and opened[0]["status"][0, w["reproj2_open"]] == R.REPROJ2
    assert opened[0]["counts"][R.PARALLAX] == 0 and opened[0]["counts"][R.ZERO_DIST] == 0
    # R7: created at neighbours 0 and 2: the second is SUPERSEDED, its own outcome (the job with that neighbour alone) is CREATED
    alone = lambda name, pos: R.run_job(sc["frames"], sc["keyframes"], R.make_job(0, [nb[pos]], S.SF, S.SIGMA2, 1.2))["status"][0, w[name]]
    assert st("twice")[0] == R.CREATED and st("twice")[2] == R.SUPERSEDED and alone("twice", 2) == R.CREATED and r["match"][2, w["twice"]] == -1 and not r["xyz"][2, w["twice"]].any()
    assert refs[1]["status"][:, w["twice"]].tolist() == [R.CREATED, R.SUPERSEDED] and refs[1]["points"]["idx2"][refs[1]["points"]["idx1"] == w["twice"]] == [c["twice"]["at2"][1]]
    # refused at 0 and created at 1; a slot after a created one whose own outcome is NO_MATCH; one whose own outcome is PAIR_SKIPPED
    assert st("refused_then_created")[:3] == [R.DEPTH1, R.CREATED, R.SUPERSEDED]
    assert st("created_then_no_match")[:2] == [R.CREATED, R.SUPERSEDED] and alone("created_then_no_match", 1) == R.NO_MATCH
    assert st("lone")[nb.index(4)] == R.SUPERSEDED and alone("lone", nb.index(4)) == R.PAIR_SKIPPED
    # n_matches is the reference's nmatches of the round: SUPERSEDED slots were never searched
    assert r["n_matches"].tolist() == [int(np.sum(r["match"][p] >= 0)) for p in range(len(nb))] and r["n_matches"][0] > r["n_created_of"][0] > 0
    # R8: creation order is neighbour order first, ascending idx1 inside; the descriptor is the current keyframe's
    pts = r["points"]
    order = list(zip(pts["neighbour"].tolist(), pts["idx1"].tolist()))
    assert order == sorted(order) and len(set(pts["idx1"].tolist())) == len(order) == r["n_created"] and len(set(pts["neighbour"].tolist())) >= 4
    assert np.array_equal(pts["desc"], sc["frames"][0]["desc"][pts["idx1"]]) and np.all(pts["max_dist"] > pts["min_dist"]) and np.all(pts["min_dist"] > 0)
    assert np.allclose(np.linalg.norm(pts["normal"], axis=1), 1.0, atol=2e-2)
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb, keep_stages=1, **S.OPEN)
    S.assert_equal(t, opened)
    t.close()


def test_random_scene(tr, om, rand):
    sc, refs = rand
    slots = [r["n_keypoints"] * r["n_neighbours"] for r in refs]
    assert slots == [315 * 4, 0, 299 * 3, 0, 301] and all(s % 64 for s in slots if s)
    assert refs[0]["n_created"] > 50 and refs[0]["counts"][R.SUPERSEDED] > 50 and refs[0]["counts"][R.HAS_POINT] > 50 and refs[0]["counts"][R.NO_MATCH] > 50
    assert np.all(refs[0]["n_created_of"] > 0) and refs[2]["n_matches"].tolist()[1] == 0 and np.isin(refs[2]["status"][1], (R.HAS_POINT, R.NO_NODE, R.SUPERSEDED)).all()
    assert 1 in sc["jobs"][0]["neighbours"] and 1 in sc["jobs"][2]["neighbours"]            # one keyframe is a neighbour in two jobs
    assert sum(r["n_equal_replaced"] for r in refs) >= 0 and sum(r["n_line_refused"] for r in refs) > 0 and sum(r["n_has_point_walked"] for r in refs) > 0
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb, keep_stages=1)
    S.assert_equal(t, refs)
    t.close()


# ---- real frame sizes, many neighbours and more than 1024 blocks: the conditions on the reference, then the host restatement ----

@pytest.mark.parametrize("name", sorted(S.SIZES))
def test_sizes_on_the_host(tr, om, name):
    make, check = S.SIZES[name]
    sc = make()
    refs = R.run(sc["frames"], sc["keyframes"], sc["jobs"])
    check(sc, refs)
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb, keep_stages=1)
    S.assert_equal(t, refs)
    t.close()


def test_known_answer_on_noise_free_geometry(tr, om):
    """a loose sanity bound on exact inputs, not a parity gate: every CREATED point within 1e-3 relative of the true point"""
    sc = S.noise_free_scene()
    fr, kf, jb = S.lib_args(tr, om, sc)
    t = tr.triangulate_host(fr, kf, jb)
    total = 0
    for j, job in enumerate(sc["jobs"]):
        pts = t.points(j)
        own = sc["owner"][job["current"]] if job["current"] < 5 else np.zeros(0, np.int64)
        for k in range(len(pts["idx1"])):
            p = own[pts["idx1"][k]]
            assert sc["owner"][job["neighbours"][pts["neighbour"][k]]][pts["idx2"][k]] == p                  # exact descriptors: every match is a true one
            truth = sc["points"][p].astype(np.float64)
            assert np.linalg.norm(pts["xyz"][k] - truth) <= 1e-3 * np.linalg.norm(truth), (j, k, pts["xyz"][k], truth)
        total += len(pts["idx1"])
    t.close()
    assert total > 100


# ---- R3: the minimum of (distance, descending position) is the literal walk ----

def test_r3_minimum_is_the_sequential_walk():
    rng = np.random.default_rng(17)
    taken = ties = 0
    for _ in range(1000):
        n = int(rng.integers(0, 40))
        th_low = int(rng.integers(0, 60))
        dists = rng.integers(0, 70, n)
        ok = rng.uniform(size=n) < 0.6
        best, best_dist = R.walk(dists, lambda p: bool(ok[p]), th_low)
        eligible = [p for p in range(n) if dists[p] <= th_low and ok[p]]
        if not eligible:
            assert best == -1
            continue
        key = min((int(dists[p]) << 32) | (0xFFFFFFFF - p) for p in eligible)
        assert (best, best_dist) == (0xFFFFFFFF - (key & 0xFFFFFFFF), key >> 32)
        taken += 1
        ties += sum(dists[p] == best_dist for p in eligible) > 1
    assert taken > 500 and ties > 50


def test_median_depth(tr):
    rng = np.random.default_rng(3)
    T = S.pose(0.1, -0.2, 0.05, (0.3, -0.1, 0.7))
    for n in (1, 2, 3, 10, 257):
        X = rng.uniform(-5, 5, (n, 3)).astype(F)
        for q in (1, 2, 3):
            got = tr.median_depth(T, X, q)
            assert got.tobytes() == R.median_depth(T, X, q).tobytes(), (n, q)
    X = np.array([[0, 0, 5], [0, 0, 1], [0, 0, 9], [0, 0, 3]], F)
    assert tr.median_depth(np.eye(3, 4), X, 2) == F(3.0)


def test_selftest_program_builds_and_passes():
    """the stand-alone sanitizer program over the host half and the shared math text: plain g++, run on the CPU"""
    csrc = os.path.join(os.path.dirname(os.path.abspath(importlib.import_module(PKG).__file__)), "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "san/triangulate_selftest_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "san", "triangulate_selftest_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "triangulate_selftest ok" in r.stdout, r.stdout + r.stderr

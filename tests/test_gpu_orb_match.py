"""Windowed ORB matching on the device (include/iba_mi355x.h, iba_orb_match*): every stage and every output BYTE FOR BYTE against the numpy restatement
tests/orb_match_ref.py, with keep_stages = 1 so that a mismatch names its stage: the grid of every frame, the candidate lists with their order and
distances, match, dist and all counts. Hand-built cases carry their expected answers as well."""
import importlib

import numpy as np
import pytest

import orb_match_ref as R
import orb_match_scene as S
import orb_scene

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu
F = np.float32
BOUNDS = S.BOUNDS
flip = S.flip
BASE = np.arange(32, dtype=np.uint8) * 7 % 251


@pytest.fixture(scope="module")
def om():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".orb_match")


def lib_frames(om, frames):
    return [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in frames]


def lib_jobs(om, jobs):
    return [om.job(j["query_frame"], j["train_frame"], j["rule"], j["centre_xy"], j["radius"], j["level_range"], j["query_index"], j.get("valid")) for j in jobs]


def compare(m, grids, refs, stages=True):
    """the result m against the reference: 0 differing bytes, stage by stage"""
    assert len(m) == len(refs)
    if stages:
        for f, (off, lst) in enumerate(grids):
            g_off, g_lst = m.grid(f)
            assert np.array_equal(g_off, off), "grid offsets of frame %d" % f
            assert np.array_equal(g_lst, lst), "cell lists of frame %d" % f
    for j, r in enumerate(refs):
        c = m.counts(j)
        assert c["n_queries"] == r["n_queries"] and c["n_candidates"] == r["n_candidates"], "list lengths of job %d" % j
        if stages:
            off, idx, d = m.lists(j)
            assert np.array_equal(off, r["off"]), "list offsets of job %d" % j
            assert np.array_equal(idx, r["index"]), "candidate order of job %d" % j
            assert d.dtype == r["cdist"].dtype and np.array_equal(d, r["cdist"]), "distances of job %d" % j
        match, dist = m.read(j)
        assert np.array_equal(match, r["match"]), "match of job %d" % j
        assert np.array_equal(dist, r["dist"]), "dist of job %d" % j
        for k in ("n_matches", "n_displaced", "n_rot_removed"):
            assert c[k] == r[k], "%s of job %d" % (k, j)
        assert np.array_equal(c["hist"], r["hist"]) and np.array_equal(c["ind"], r["ind"]), "histogram of job %d" % j


def run_both(om, frames, jobs, **opts):
    """-> (the device result with keep_stages, the reference's grids, the reference's results), compared"""
    grids, refs = R.run(frames, jobs, **opts)
    m = om.match(lib_frames(om, frames), lib_jobs(om, jobs), keep_stages=1, **opts)
    compare(m, grids, refs)
    return m, grids, refs


def window_job(frames, a, b, rule, r, levels=(-1, -1), n=None):
    """every keypoint of frame a (or its first n) asks around its own position in frame b"""
    k = len(frames[a]["octave"]) if n is None else n
    return {"query_frame": a, "train_frame": b, "rule": rule, "centre_xy": frames[a]["xy"][:k].copy(), "radius": np.full(k, r, F),
            "level_range": np.tile(np.array(levels, np.int32), (k, 1)), "query_index": np.arange(k, dtype=np.int32), "valid": None}


def hand_job(q, t, rule, centres, radius, queries=None, levels=None, valid=None):
    k = len(centres)
    return {"query_frame": q, "train_frame": t, "rule": rule, "centre_xy": np.array(centres, F).reshape(k, 2), "radius": np.full(k, radius, F) if np.isscalar(radius) else np.array(radius, F),
            "level_range": np.tile(np.array([-1, -1], np.int32), (k, 1)) if levels is None else np.array(levels, np.int32).reshape(k, 2),
            "query_index": np.arange(k, dtype=np.int32) if queries is None else np.array(queries, np.int32), "valid": valid}


def test_frame_sizes_in_one_call(om):
    """n = 0, 1, 63, 64, 65 and 300 in ONE call; a keypoint outside the grid, two on a rounding tie, cells that hold several keypoints"""
    rng = np.random.default_rng(4)
    frames = []
    for n in (0, 1, 63, 64, 65, 300):
        xy = np.stack([rng.uniform(0, 630, n), rng.uniform(0, 470, n)], 1).astype(F)
        if n == 300:
            xy[0] = (900.0, 10.0)                         # outside the grid: in no cell
            xy[1] = xy[2] = (25.0, 35.0)                  # products 2.5 and 3.5: both round away from zero into cell (3, 4)
            xy[3] = (635.0, 100.0)                        # 63.5 rounds to 64: in no cell
            xy[10:40] = rng.uniform(200, 209.9, (30, 2))  # thirty keypoints over four cells
        frames.append(R.make_frame(xy, rng.integers(0, 3, n), rng.uniform(0, 360, n).astype(F), rng.integers(0, 256, (n, 32)), BOUNDS))
    jobs = []
    for t in range(6):
        jobs.append(window_job(frames, 5, t, R.CLAIM, 70.0))
        jobs.append(window_job(frames, 5, t, R.INIT, 90.0, n=131))
    jobs.append(window_job(frames, 0, 5, R.INIT, 50.0))   # a job without queries, from the frame without keypoints
    jobs.append(window_job(frames, 5, 5, R.CLAIM, 12.0, levels=(1, 2)))
    m, grids, refs = run_both(om, frames, jobs)
    off, lst = grids[5]
    assert lst[off[3 * 48 + 4]:off[3 * 48 + 5]].tolist() == [1, 2] and off[-1] == 298 and 0 not in lst and 3 not in lst
    assert max(np.diff(off)) >= 5 and m.n_chunks == 1
    assert refs[0]["n_candidates"] == 0 and refs[-2]["n_queries"] == 0 and refs[-1]["n_matches"] > 100
    plain = om.match(lib_frames(om, frames), lib_jobs(om, jobs))        # without keep_stages: the same results, and no stage accessor
    compare(plain, grids, refs, stages=False)
    with pytest.raises(importlib.import_module(PKG).IbaError, match="keep_stages"):
        plain.grid(5)
    with pytest.raises(importlib.import_module(PKG).IbaError, match="keep_stages"):
        plain.lists(0)
    plain.close()
    m.close()


def test_segment_lengths_windows_and_levels(om):
    """segments of 0, 1, 64, 65 and more than 128 entries in one job (the lanes' second and third trip); windows clipped by each image edge and wholly
    outside it; each level-range case of the truth table"""
    rng = np.random.default_rng(9)
    clusters = (((50, 50), 1), ((200, 100), 64), ((400, 100), 65), ((300, 300), 150), ((3, 240), 20), ((630, 240), 20), ((320, 3), 20), ((320, 470), 20))
    xy = np.concatenate([np.array(c, F) + rng.uniform(-2.9, 2.9, (k, 2)).astype(F) for c, k in clusters])
    n = len(xy)
    train = R.make_frame(xy, rng.integers(0, 5, n), rng.uniform(0, 360, n).astype(F), rng.integers(0, 256, (n, 32)), BOUNDS)
    query = R.make_frame(np.zeros((1, 2)), [0], [10.0], rng.integers(0, 256, (1, 32)), BOUNDS)
    centres = [(500, 400), (50, 50), (200, 100), (400, 100), (300, 300),                     # 0, 1, 64, 65, 150 entries
               (3, 240), (630, 240), (320, 3), (320, 470),                                   # clipped by the left, right, upper and lower edge
               (-100, 240), (800, 240), (320, -100), (320, 600),                             # wholly outside: M3's four early returns
               (300, 300), (300, 300), (300, 300), (300, 300)]                               # the level cases
    radius = [8.0] * 5 + [30.0] * 4 + [30.0] * 4 + [8.0] * 4
    levels = [(-1, -1)] * 13 + [(-1, -1), (0, 0), (2, -1), (-1, 3)]
    jobs = [hand_job(0, 1, rule, centres, radius, queries=[0] * len(centres), levels=levels) for rule in (R.INIT, R.CLAIM)]
    m, grids, refs = run_both(om, [query, train], jobs, th_low=256, th_high=256, nn_ratio=1.0, check_orientation=0)
    seg = np.diff(refs[0]["off"]).tolist()
    assert seg[:5] == [0, 1, 64, 65, 150] and seg[5:9] == [20] * 4 and seg[9:13] == [0] * 4
    o = train["octave"][130:280]
    assert seg[13:] == [150, int((o == 0).sum()), int((o >= 2).sum()), int((o <= 3).sum())] and 0 < seg[14] < seg[15] < seg[16] < 150
    assert refs[1]["n_matches"] >= 8                       # CLAIM at th_high = 256: every query with an unclaimed candidate below 256 takes one
    m.close()


def _tie_frames():
    # train 0: three keypoints in one window at distances 20, 20, 40 from BASE; train 1: two at 20 and 40; the query frame: BASE
    t0 = R.make_frame([[100, 100], [101, 100], [102, 100]], [0] * 3, [0] * 3, [flip(BASE, range(20)), flip(BASE, range(20, 40)), flip(BASE, range(40))], BOUNDS)
    t1 = R.make_frame([[100, 100], [101, 100]], [0] * 2, [0] * 2, [flip(BASE, range(20)), flip(BASE, range(40))], BOUNDS)
    return [R.make_frame([[100, 100]], [0], [0], [BASE], BOUNDS), t0, t1]


@pytest.mark.parametrize("opts,want", [
    ({}, [0, -1, 0, 0]),                         # CLAIM: the first of two equal least distances; INIT on t0: best == best2, the ratio rejects; on t1: 20 < 36
    ({"nn_ratio": 0.5}, [0, -1, 0, -1]),         # the ratio tie: 20 < 40 * 0.5 fails
    ({"th_low": 20, "th_high": 20}, [0, -1, 0, 0]),      # best == th_low and best == th_high are accepted
    ({"th_low": 19, "th_high": 19}, [-1, -1, -1, -1]),   # th + 1 is rejected
])
def test_distance_ties(om, opts, want):
    frames = _tie_frames()
    jobs = [hand_job(0, 1, R.CLAIM, [(100, 100)], 10.0), hand_job(0, 1, R.INIT, [(100, 100)], 10.0), hand_job(0, 2, R.CLAIM, [(100, 100)], 10.0), hand_job(0, 2, R.INIT, [(100, 100)], 10.0)]
    m, _, refs = run_both(om, frames, jobs, **opts)
    assert refs[0]["cdist"].tolist() == [20, 20, 40] and refs[2]["cdist"].tolist() == [20, 40]
    assert [int(m.read(j)[0][0]) for j in range(4)] == want
    assert [int(m.read(j)[1][0]) for j in range(4)] == [20 if w >= 0 else -1 for w in want]
    m.close()


def test_init_displacement_chain(om):
    """a later query displaces an earlier holder, which is displaced again; the displaced holder's bin still counts; a candidate skipped because
    held_dist <= dist changes another query's best2 and with it the ratio's verdict"""
    c2_bits = list(range(100, 140))
    train = R.make_frame([[100, 100], [400, 300], [402, 300]], [0] * 3, [0.0, 0.0, 0.0], [BASE, BASE, flip(BASE, c2_bits)], BOUNDS)
    qdesc = [flip(BASE, range(30)), flip(BASE, range(20)), flip(BASE, range(10)), flip(BASE, range(15)),      # to c0: 30, 20, 10, 15
             flip(BASE, range(5)),                                                                               # to c1: 5, to c2: 45
             flip(BASE, c2_bits[:21] + [0])]                                                                     # to c1: 22, to c2: 19 + 1 = 20
    qangle = [40.0, 100.0, 0.0, 0.0, 0.0, 0.0]             # bins 1, 3, 0, -, 0, 0
    query = R.make_frame(np.zeros((6, 2)), [0] * 6, qangle, qdesc, BOUNDS)
    centres = [(100, 100)] * 4 + [(401, 300)] * 2
    job = hand_job(0, 1, R.INIT, centres, 10.0)
    m, _, refs = run_both(om, [query, train], [job, dict(job, valid=np.array([1, 1, 1, 1, 0, 1], np.uint8))], check_orientation=0)
    assert refs[0]["match"].tolist() == [-1, -1, 0, -1, 1, 2] and refs[0]["dist"].tolist() == [-1, -1, 10, -1, 5, 20] and refs[0]["n_displaced"] == 2
    assert refs[1]["match"].tolist() == [-1, -1, 0, -1, -1, -1] and refs[1]["n_ratio_rejected"] == 1       # without query 4 nobody holds c1: 20 < 22 * 0.9 fails
    assert m.read(0)[0].tolist() == [-1, -1, 0, -1, 1, 2] and m.counts(0)["n_displaced"] == 2 and m.counts(0)["n_matches"] == 3
    m.close()
    m, _, refs = run_both(om, [query, train], [job])       # with the rotation check: bins 1 and 3 keep the displaced holders' counts
    assert refs[0]["hist"][:4].tolist() == [3, 1, 0, 1] and refs[0]["hist"].sum() == 5 and refs[0]["ind"].tolist() == [0, 1, 3] and refs[0]["n_rot_removed"] == 0
    assert m.counts(0)["hist"][:4].tolist() == [3, 1, 0, 1] and m.counts(0)["n_matches"] == 3
    m.close()


def test_claim_takes_the_second_or_nothing(om):
    train = R.make_frame([[100, 100], [101, 100]], [0] * 2, [0, 0], [BASE, flip(BASE, range(60, 90))], BOUNDS)
    query = R.make_frame(np.zeros((3, 2)), [0] * 3, [0] * 3, [flip(BASE, range(5)), flip(BASE, range(3)), BASE], BOUNDS)      # to c0: 5, 3, 0; to c1: 35, 33, 30
    m, _, refs = run_both(om, [query, train], [hand_job(0, 1, R.CLAIM, [(100, 100)] * 3, 10.0)])
    assert refs[0]["cdist"].tolist() == [5, 35, 3, 33, 0, 30]
    assert m.read(0)[0].tolist() == [0, 1, -1] and m.read(0)[1].tolist() == [5, 33, -1] and m.counts(0)["n_matches"] == 2
    m.close()


def _pairs_job(rots, rule, seed):
    """isolated pairs: query k sees train k alone, at a rotation difference of rots[k] degrees"""
    rng = np.random.default_rng(seed)
    n = len(rots)
    xy = np.stack([20 + 30.0 * (np.arange(n) % 20), 20 + 30.0 * (np.arange(n) // 20)], 1).astype(F)
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    train = R.make_frame(xy, [0] * n, np.full(n, 10.0, F), desc, BOUNDS)
    query = R.make_frame(xy, [0] * n, (np.array(rots, F) + F(10.0)) % F(360.0), desc, BOUNDS)
    return query, train, hand_job(0, 1, rule, xy, 5.0)


@pytest.mark.parametrize("rule", [R.INIT, R.CLAIM])
def test_rotation_check(om, rule):
    rots = [0.0] * 10 + [60.0] * 5 + [120.0] * 4 + [180.0] * 3 + [350.0] * 2          # bins 0, 2, 4, 6 and 350 - 360 .. 12
    query, train, job = _pairs_job(rots, rule, 1)
    m, _, refs = run_both(om, [query, train], [job])
    assert refs[0]["hist"][[0, 2, 4, 6, 12]].tolist() == [10, 5, 4, 3, 2] and refs[0]["ind"].tolist() == [0, 2, 4]
    assert m.counts(0)["n_rot_removed"] == 5 and m.counts(0)["n_matches"] == 19 and m.read(0)[0][19:].tolist() == [-1] * 5
    m.close()
    query, train, job = _pairs_job([0.0] * 20 + [60.0, 120.0], rule, 2)              # max2 = 1 < 0.1f * 20: ind2 and ind3 are dropped
    m, _, refs = run_both(om, [query, train], [job])
    assert refs[0]["ind"].tolist() == [0, -1, -1] and m.counts(0)["n_rot_removed"] == 2 and m.counts(0)["n_matches"] == 20
    m.close()
    query, train, job = _pairs_job([0.0] * 20 + [60.0, 60.0, 120.0], rule, 3)        # max2 = 2 stays, max3 = 1 < 2: only ind3 is dropped
    m, _, refs = run_both(om, [query, train], [job])
    assert refs[0]["ind"].tolist() == [0, 2, -1] and m.counts(0)["n_rot_removed"] == 1
    m.close()
    m, _, refs = run_both(om, [query, train], [job], check_orientation=0)
    assert m.counts(0)["n_matches"] == 23 and m.counts(0)["hist"].sum() == 0 and m.counts(0)["ind"].tolist() == [-1, -1, -1] and m.counts(0)["n_rot_removed"] == 0
    m.close()


def test_train_state_in_global_memory(om):
    """a train frame above IBA_ORB_MATCH_LDS_TRAIN keypoints keeps held_dist / holder in global memory; beside a small one in the same call"""
    rng = np.random.default_rng(12)
    n = 8200
    big = R.make_frame(np.stack([rng.uniform(0, 640, n), rng.uniform(0, 480, n)], 1), rng.integers(0, 3, n), rng.uniform(0, 360, n).astype(F), rng.integers(0, 256, (n, 32)), BOUNDS)
    small = S.sequence(2, 200, 3)
    q = R.make_frame(big["xy"][:120] + F(1.0), big["octave"][:120], big["angle"][:120], [flip(d, range(k % 7)) for k, d in enumerate(big["desc"][:120])], BOUNDS)
    q["xy"][1::4] = q["xy"][0::4]                            # several queries want the same train keypoint: displacements and taken claims
    q["desc"][1::4] = q["desc"][0::4]
    frames = [big, q] + small
    jobs = [window_job(frames, 1, 0, R.INIT, 25.0), S.init_job(frames, 2, 3), window_job(frames, 1, 0, R.CLAIM, 25.0), S.claim_job(frames, 2, 3)]
    m, _, refs = run_both(om, frames, jobs)
    assert refs[0]["n_matches"] > 30 and refs[2]["n_matches"] > 60 and refs[0]["max_segment"] > 64
    m.close()


def test_a_frame_at_the_declared_limit(om):
    """one CLAIM job into a frame of exactly IBA_ORB_MATCH_MAX_KEYPOINTS keypoints: the grid cell for cell (a cell that the ordered fill fills with
    two whole trips of 64 consecutive keypoints and a part of a third), claims up to the last index with the state in global memory"""
    sc = S.limit_scene()
    grids, refs = R.run(sc["frames"], sc["jobs"])
    S.check_limit(sc, grids, refs)
    m = om.match(lib_frames(om, sc["frames"]), lib_jobs(om, sc["jobs"]), keep_stages=1)
    compare(m, grids, refs)
    assert m.n_chunks == 1
    m.close()


NQ = (300, 257, 129, 64, 300)


@pytest.fixture(scope="module")
def scene():
    """6 frames of 300 keypoints, 5 INIT and 5 CLAIM jobs with ragged query counts, frames shared between jobs; the reference, computed once"""
    frames = S.sequence(6, 300, 2)
    jobs = [S.init_job(frames, k, k + 1, n_queries=NQ[k]) for k in range(5)]
    jobs += [S.claim_job(frames, k + 1 if k < 4 else 0, k if k < 4 else 5, n_queries=NQ[4 - k], seed=k) for k in range(5)]
    grids, refs = R.run(frames, jobs)
    return frames, jobs, grids, refs


def test_scene(om, scene):
    frames, jobs, grids, refs = scene
    # on the reference alone: the scene is not trivial
    for j, r in zip(jobs, refs):
        assert 4 * r["n_matches"] >= int(j["valid"].sum()) > 0
    assert sum(r["n_displaced"] for r in refs) >= 1 and sum(r["n_ratio_rejected"] for r in refs) >= 1
    assert sum(r["n_rot_removed"] for r in refs) >= 1 and max(r["max_segment"] for r in refs) > 64
    m = om.match(lib_frames(om, frames), lib_jobs(om, jobs), keep_stages=1)
    compare(m, grids, refs)
    assert m.n_chunks == 1
    m.close()


def test_chunking_changes_no_byte(om, scene, monkeypatch):
    frames, jobs, grids, refs = scene
    monkeypatch.setenv("IBA_ORB_MATCH_BUDGET", "1")          # less than one job: a chunk still holds one
    cut = om.match(lib_frames(om, frames), lib_jobs(om, jobs), keep_stages=1)
    monkeypatch.delenv("IBA_ORB_MATCH_BUDGET")
    assert cut.n_chunks == len(jobs)
    compare(cut, grids, refs)
    cut.close()
    monkeypatch.setenv("IBA_ORB_MATCH_BUDGET", str(6 * (refs[0]["n_candidates"] + refs[1]["n_candidates"])))
    some = om.match(lib_frames(om, frames), lib_jobs(om, jobs), keep_stages=1)
    monkeypatch.delenv("IBA_ORB_MATCH_BUDGET")
    assert 1 < some.n_chunks < len(jobs)
    compare(some, grids, refs)
    some.close()


def test_end_to_end_with_the_extraction(om):
    """two seeded mosaics, the second shifted by a few pixels: iba_orb_extract, iba_orb_match_init_queries, iba_orb_match, against the restatement on the
    same extracted features"""
    orb = importlib.import_module(PKG + ".orb")
    W, H = 320, 240
    wide = orb_scene.image(W + 8, H + 8, 5)
    images = [np.ascontiguousarray(wide[:H, :W]), np.ascontiguousarray(wide[3:H + 3, 5:W + 5])]
    feats = orb.extract(images, pattern=orb_scene.pattern(), n_features=500)
    got = [feats.read(i) for i in range(2)]
    feats.close()
    bounds = (0.0, float(W), 0.0, float(H))
    frames = [R.make_frame(g["xy"], g["octave"], g["angle"], g["desc"], bounds) for g in got]
    assert min(len(f["octave"]) for f in frames) > 100
    lf = lib_frames(om, frames)
    q = om.init_queries(lf[0], frames[0]["xy"], 100)
    want = R.init_queries(frames[0], frames[0]["xy"], 100)
    for k in want:
        assert np.array_equal(q[k], want[k]), k
    jobs = [dict(q, query_frame=0, train_frame=1, rule=R.INIT), dict(q, query_frame=0, train_frame=1, rule=R.CLAIM)]
    grids, refs = R.run(frames, jobs)
    m = om.match(lf, lib_jobs(om, jobs), keep_stages=1)
    compare(m, grids, refs)
    assert refs[0]["n_matches"] >= 10
    m.close()

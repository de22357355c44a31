"""Map-point fusion on the device (include/iba_mi355x.h, iba_fuse*): every output and kept stage of iba_fuse byte for byte against tests/fuse_ref.py
(the rules in numpy, F5 as the reference's walk) AND against the host restatement (iba_debug_fuse_host), on the scenes of tests/fuse_scene.py;
tests/test_fuse_cpu.py asserts on the reference's output that every named case occurs in them. Then the three pick widths, forced budgets (several
chunks, the same bytes), the changed options, and the chain from iba_triangulate through the recipe to the known answer, with the device calls."""
import importlib

import numpy as np
import pytest

import fuse_ref as R
import fuse_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fz():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".fuse")


@pytest.fixture(scope="module")
def mm():
    return importlib.import_module(PKG + ".map_match")


@pytest.fixture(scope="module")
def om():
    return importlib.import_module(PKG + ".orb_match")


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for name, make in (("hand", S.hand_scene), ("random", S.random_scene)):
        sc = make()
        out[name] = (sc, R.run(sc["frames"], sc["table"], sc["jobs"]))
    return out


@pytest.mark.parametrize("name", ["hand", "random"])
def test_device_against_ref_and_host(fz, mm, om, scenes, name):
    sc, refs = scenes[name]
    seg = np.concatenate([np.diff(r["off"]) for r in refs])
    if name == "hand":
        assert {0, 1, 7, 8, 9, 15, 16, 17, 63, 64, 65, 200} <= set(seg.tolist()) and all(c > 0 for c in refs[0]["counts"]) and refs[0]["n_gated_winner"] > 0
    else:
        assert [r["n_points"] for r in refs] == [300, 257, 257, 0, 1, 255, 258, 300] and sum(r["n_gated_winner"] for r in refs) > 0
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    dev = fz.fuse(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    host = fz.fuse_host(fr, tb, jb, keep_stages=1)
    S.same_results(dev, host, len(jb))
    host.close()
    dev.close()
    plain = fz.fuse(fr, tb, jb)                        # without keep_stages: the same results
    S.assert_equal(plain, refs, keep_stages=False)
    plain.close()


@pytest.mark.parametrize("lanes", [8, 16, 64])
def test_pick_widths_give_the_same_bytes(fz, mm, om, scenes, monkeypatch, lanes):
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    monkeypatch.setenv("IBA_FUSE_PICK_LANES", str(lanes))
    for name in ("hand", "random"):
        sc, refs = scenes[name]
        fr, tb, jb = S.lib_args(fz, mm, om, sc)
        dev = fz.fuse(fr, tb, jb, keep_stages=1)
        S.assert_equal(dev, refs)
        dev.close()


def planned_chunks(candidates, budget):
    """the cut of consecutive jobs under a byte budget (6 bytes per candidate, a chunk holds at least one job), restated"""
    n, at, held = 1, 0, 0
    for c in candidates:
        if held and (at > budget or 6 * c > budget - at):
            n, at, held = n + 1, 0, 0
        at, held = at + 6 * c, held + 1
    return n


def test_chunking_changes_no_byte(fz, mm, om, scenes, monkeypatch):
    sc, refs = scenes["random"]
    cand = [r["n_candidates"] for r in refs]
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    for budget in (1, 6 * (cand[0] + cand[1]), 6 * max(cand)):
        want = planned_chunks(cand, budget)
        monkeypatch.setenv("IBA_FUSE_BUDGET", str(budget))
        cut = fz.fuse(fr, tb, jb, keep_stages=1)
        monkeypatch.delenv("IBA_FUSE_BUDGET")
        assert cut.n_chunks == want and (budget > 1 or want == len(jb)) and (budget == 1 or 1 < want < len(jb)), (budget, cut.n_chunks, want)
        S.assert_equal(cut, refs)
        cut.close()


# ---- real frame sizes, the declared limit, many jobs (the scenes and their conditions: tests/fuse_scene.py, SIZES) ----

@pytest.fixture(scope="module")
def sizes():
    made = {}

    def get(name):
        if name not in made:
            make, check = S.SIZES[name]
            sc = make()
            refs = R.run(sc["frames"], sc["table"], sc["jobs"])
            check(sc, refs)
            made[name] = (sc, refs)
        return made[name]
    return get


@pytest.mark.parametrize("name", ["large", "limit"])
def test_real_sizes_and_the_limit(fz, mm, om, sizes, name):
    """2100 points over 2100 keypoints (9 frustum and pick blocks per job, every status); one frame of IBA_ORB_MATCH_MAX_KEYPOINTS keypoints with
    picks in its last 32"""
    sc, refs = sizes(name)
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    dev = fz.fuse(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    host = fz.fuse_host(fr, tb, jb, keep_stages=1)
    S.same_results(dev, host, len(jb))
    host.close()
    dev.close()


@pytest.mark.parametrize("lanes", [8, 16, 64])
def test_pick_widths_at_real_sizes(fz, mm, om, sizes, monkeypatch, lanes):
    sc, refs = sizes("large")
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    monkeypatch.setenv("IBA_FUSE_PICK_LANES", str(lanes))
    dev = fz.fuse(fr, tb, jb, keep_stages=1)
    S.assert_equal(dev, refs)
    dev.close()


def test_many_jobs_in_one_call_and_in_chunks(fz, mm, om, sizes, monkeypatch):
    """139 jobs: one chunk by default; a budget that cuts them into a few chunks and a budget of 1 (a chunk per job that has candidates) change no byte; a job alone
    gives the bytes of its slice"""
    sc, refs = sizes("many")
    cand = [r["n_candidates"] for r in refs]
    n = len(refs)
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    dev = fz.fuse(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    dev.close()
    monkeypatch.setenv("IBA_DEBUG_ENV", "1")
    for budget in (6 * sum(cand) // 7, 1):
        want = planned_chunks(cand, budget)
        assert (3 <= want < n) if budget > 1 else n // 2 < want <= n, (budget, want)          # (a job without candidates starts no chunk)
        monkeypatch.setenv("IBA_FUSE_BUDGET", str(budget))
        cut = fz.fuse(fr, tb, jb, keep_stages=1)
        monkeypatch.delenv("IBA_FUSE_BUDGET")
        assert cut.n_chunks == want, (budget, cut.n_chunks, want)
        S.assert_equal(cut, refs)
        cut.close()
    for j in (0, n // 2, n - 1):
        alone = fz.fuse(fr, tb, [jb[j]], keep_stages=1)
        S.assert_equal(alone, [refs[j]])
        alone.close()


def test_options_flip_the_recorded_cases(fz, mm, om, scenes):
    sc, refs = scenes["hand"]
    w, kp = sc["where"], sc["kp"]
    fr, tb, jb = S.lib_args(fz, mm, om, sc)
    low = R.run(sc["frames"], sc["table"], sc["jobs"], th_low=49)
    assert refs[0]["status"][w["pick_50"]] == R.PICKED and low[0]["status"][w["pick_50"]] == R.NO_MATCH
    sim3 = R.run(sc["frames"], sc["table"], sc["jobs"], check_reprojection=0)
    assert refs[0]["match"][w["gated_winner"]] == kp["gated_winner"][1] and sim3[0]["match"][w["gated_winner"]] == kp["gated_winner"][0]
    wide = R.run(sc["frames"], sc["table"], sc["jobs"], view_cos_limit=0.75, chi2_mono=0.5)
    assert wide[0]["status"][w["dot_at_limit"]] == R.ANGLE and wide[0]["status"][w["lone"]] == R.NO_MATCH
    for opts, want in (({"th_low": 49}, low), ({"check_reprojection": 0}, sim3), ({"view_cos_limit": 0.75, "chi2_mono": 0.5}, wide)):
        dev = fz.fuse(fr, tb, jb, keep_stages=1, **opts)
        S.assert_equal(dev, want)
        dev.close()


def test_fold_of_device_picks_on_the_map_scene(fz, mm, om):
    """the recipe with the device calls on the map scene that reaches every op, the object restatement beside it after every job"""
    sc = S.map_scene()
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in sc["frames"]]
    t = sc["table"]
    table = mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"])
    fmap, world = S.fuse_map(fz, sc["map"]), R.World(sc["map"])
    ops = S.recipe(fz, fz.fuse, frames, table, sc, fmap, world)
    assert set(np.concatenate([op for _, op in ops]).tolist()) == {R.OP_NONE, R.OP_ADD, R.OP_REPLACED_BY_HELD, R.OP_REPLACES_HELD, R.OP_HELD_BAD, R.OP_STALE_BAD, R.OP_STALE_IN_KEYFRAME}


def test_end_to_end_from_triangulation(fz, mm, om):
    """iba_triangulate -> the new points appended to a table that already holds those landmarks -> the recipe through iba_fuse -> the known answer"""
    S.check_end_to_end(fz, mm, om, importlib.import_module(PKG + ".triangulate"), host=False)

"""Local-map point matching on the device (include/iba_mi355x.h, iba_map_match*): every output and kept stage of iba_map_match byte for byte against
tests/map_match_ref.py (the rules in numpy, L4 as the reference's sequential scan) AND against the host restatement (iba_debug_map_match_host), on
the scenes of tests/map_match_scene.py; tests/test_map_match_cpu.py asserts on the reference's output that every named case occurs in them. Then
forced budgets (several chunks, the same bytes) and the chain to iba_pose_optimize."""
import importlib

import numpy as np
import pytest

import map_match_ref as R
import map_match_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mm():
    importlib.import_module(PKG)
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


def same_results(a, b, n_jobs):
    """two MapMatches byte for byte, the kept stages included"""
    for j in range(n_jobs):
        ca, cb = a.counts(j), b.counts(j)
        assert all(np.array_equal(ca[k], cb[k]) for k in ca), (j, ca, cb)
        ra, rb = a.read(j), b.read(j)
        assert all(S.same_bytes(ra[k], rb[k]) for k in ra), j
        assert S.same_bytes(a.keypoints(j), b.keypoints(j)) and all(S.same_bytes(x, y) for x, y in zip(a.lists(j), b.lists(j))), j


@pytest.mark.parametrize("name", ["hand", "random"])
def test_device_against_ref_and_host(mm, om, scenes, name):
    sc, refs = scenes[name]
    seg = np.concatenate([np.diff(r["off"]) for r in refs])
    if name == "hand":
        assert {0, 1, 63, 64, 65, 200} <= set(seg.tolist()) and all(c > 0 for c in refs[0]["counts"]) and refs[0]["n_ratio_refused"] > 0
    else:
        assert [r["n_points"] for r in refs] == [300, 257, 257, 257, 0, 1, 255, 256, 300] and sum(r["n_second_choice"] for r in refs) > 0
    fr, tb, jb = S.lib_args(mm, om, sc)
    dev = mm.match(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    host = mm.match_host(fr, tb, jb, keep_stages=1)
    same_results(dev, host, len(jb))
    host.close()
    dev.close()
    plain = mm.match(fr, tb, jb)                       # without keep_stages: the same results
    S.assert_equal(plain, refs, keep_stages=False)
    plain.close()


def test_options(mm, om, scenes):
    sc, _ = scenes["hand"]
    refs = R.run(sc["frames"], sc["table"], sc["jobs"], th_high=99, nn_ratio=0.5, view_cos_limit=0.75)
    w = sc["where"]
    assert refs[0]["match"][w["at_th_high"]] == -1 and refs[0]["match"][w["ratio_pass"]] == -1 and refs[0]["status"][w["cos_at_limit"]] == R.ANGLE
    fr, tb, jb = S.lib_args(mm, om, sc)
    dev = mm.match(fr, tb, jb, keep_stages=1, th_high=99, nn_ratio=0.5, view_cos_limit=0.75)
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


def test_chunking_changes_no_byte(mm, om, scenes, monkeypatch):
    sc, refs = scenes["random"]
    cand = [r["n_candidates"] for r in refs]
    fr, tb, jb = S.lib_args(mm, om, sc)
    for budget in (1, 6 * (cand[0] + cand[1]), 6 * max(cand)):
        want = planned_chunks(cand, budget)
        monkeypatch.setenv("IBA_MAP_MATCH_BUDGET", str(budget))
        cut = mm.match(fr, tb, jb, keep_stages=1)
        monkeypatch.delenv("IBA_MAP_MATCH_BUDGET")
        assert cut.n_chunks == want and (budget > 1 or want == len(jb)) and (budget == 1 or 1 < want < len(jb)), (budget, cut.n_chunks, want)
        S.assert_equal(cut, refs)
        cut.close()


# ---- real frame sizes, the declared limit, many jobs (the scenes and their conditions: tests/map_match_scene.py, SIZES) ----

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
def test_real_sizes_and_the_limit(mm, om, sizes, name):
    """2100 points over 2100 keypoints (9 blocks per job, a partial last bitmap word, claimed and occupied); one frame of IBA_ORB_MATCH_MAX_KEYPOINTS
    keypoints (the bitmap's last word, claimed and occupied)"""
    sc, refs = sizes(name)
    fr, tb, jb = S.lib_args(mm, om, sc)
    dev = mm.match(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    host = mm.match_host(fr, tb, jb, keep_stages=1)
    same_results(dev, host, len(jb))
    host.close()
    dev.close()


def test_many_jobs_in_one_call_and_in_chunks(mm, om, sizes, monkeypatch):
    """139 jobs: one chunk by default; a budget that cuts them into a few chunks and a budget of 1 (a chunk per job that has candidates) change no byte; a job alone
    gives the bytes of its slice"""
    sc, refs = sizes("many")
    cand = [r["n_candidates"] for r in refs]
    n = len(refs)
    fr, tb, jb = S.lib_args(mm, om, sc)
    dev = mm.match(fr, tb, jb, keep_stages=1)
    assert dev.n_chunks == 1
    S.assert_equal(dev, refs)
    dev.close()
    for budget in (6 * sum(cand) // 7, 1):
        want = planned_chunks(cand, budget)
        assert (3 <= want < n) if budget > 1 else n // 2 < want <= n, (budget, want)          # (a job without candidates starts no chunk)
        monkeypatch.setenv("IBA_MAP_MATCH_BUDGET", str(budget))
        cut = mm.match(fr, tb, jb, keep_stages=1)
        monkeypatch.delenv("IBA_MAP_MATCH_BUDGET")
        assert cut.n_chunks == want, (budget, cut.n_chunks, want)
        S.assert_equal(cut, refs)
        cut.close()
    for j in (0, n // 2, n - 1):
        alone = mm.match(fr, tb, [jb[j]], keep_stages=1)
        S.assert_equal(alone, [refs[j]])
        alone.close()


def test_end_to_end(mm, om):
    """iba_map_match -> iba_map_match_pose_edges -> iba_pose_optimize on the noise-free scene"""
    S.check_end_to_end(mm, om, importlib.import_module(PKG + ".pose"), host=False)

"""Two-view initialisation on the device (include/iba_mi355x.h, iba_twoview*): every output and every kept stage BYTE FOR BYTE against the numpy
restatement tests/twoview_ref.py, with keep_stages = 1 so that a mismatch names its stage; parallax_deg within one float32 ulp (acos is libm's).
The scene list runs in ONE call of 70 iterations (iterations is an option of the call, so the pair with 200 iterations' worth of sets is a call of
its own); the lane and wave edges of every kernel, repeated pairs, a hypothesis made singular on purpose, the host
restatement and the composition with iba_orb_match follow. The calls' default, keep_stages = 0, takes a kernel and a read-back of its own: the scene
list, the gather's block edge, the chunk cuts and a call of 73 pairs (more than one block of the one-lane-per-pair kernels) run that way too."""
import importlib

import numpy as np
import pytest

import orb_match_ref as MR
import orb_match_scene as MS
import twoview_ref as R
import twoview_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def tv():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".twoview")


@pytest.fixture(scope="module")
def err():
    return importlib.import_module(PKG).IbaError


def lib_pair(tv, p):
    return tv.pair(p["xy1"], p["xy2"], p["matches12"], p["K"], p.get("sets"))


def run_both(tv, pairs, iterations, refs=None, **opts):
    """the device result with keep_stages against the reference of every pair: 0 differing bytes in every output and stage -> (result, references)"""
    refs = [S.reference(p, iterations, **opts) for p in pairs] if refs is None else refs
    r = tv.init([lib_pair(tv, p) for p in pairs], iterations=iterations, keep_stages=1, **opts)
    assert len(r) == len(refs)
    for b, e in enumerate(refs):
        assert S.differences(r, b, e) == [], "pair %d (%s)" % (b, R_NAMES[e["status"]])
    assert r.sweep_cap_hits == sum(e["sweep_cap_hits"] for e in refs)
    return r, refs


R_NAMES = ("OK", "TOO_FEW_MATCHES", "NO_MODEL", "H_DEGENERATE", "NO_CLEAR_WINNER", "TOO_FEW_POINTS", "LOW_PARALLAX")


def exact_pair(N, seed, iterations, **kw):
    """a pair whose match list has exactly N entries"""
    p = S.with_sets(S.make_pair(seed, n=N, unmatched=0.0, **kw), iterations, 77 + N)
    assert S.n_matches(p) == N
    return p


def test_scene_list_in_one_call(tv):
    pairs, refs = S.scene_pairs(), S.scene_reference()
    assert len({len(p["xy1"]) for p in pairs}) > 4 and len({S.n_matches(p) for p in pairs}) > 4        # ragged n1 and N
    r, _ = run_both(tv, pairs, S.ITERATIONS, refs=refs)
    assert [r.read(b)["status"] for b in range(len(r))] == [st for _, st, _, _ in S.SCENES]
    r.close()


def test_two_hundred_iterations(tv):
    p = S.with_sets(S.make_pair(**S.SCENES[0][3]), 200, S.SETS_SEED)
    r, refs = run_both(tv, [p], 200)
    assert refs[0]["n_hyp"] == 4 and max(refs[0]["best_it_F"], refs[0]["best_it_H"]) > 64
    r.close()


@pytest.mark.parametrize("iterations", [1, 63, 64, 65])
def test_lane_and_wave_edges(tv, iterations):
    """iterations at the score kernel's wave edge; N = 8 (every set is all the matches), 9, 63, 64, 65 (the select walk's wave edge), 257 (the
    CheckRT block edge); 40 clean matches: n_good <= 50, position n_good - 1; 257: n_good >= 52, position 50"""
    pairs = [exact_pair(N, 20 + N, iterations, outliers=0.0, noise=0.1) for N in (8, 9, 63, 64, 65, 257, 40)]
    assert all(sorted(row) == list(range(8)) for row in pairs[0]["sets"].tolist())
    r, refs = run_both(tv, pairs, iterations)
    if iterations >= 63:
        best = [int(e["n_good"].max()) for e in refs]
        assert 0 < best[6] <= 50 and best[5] >= 52, best
    r.close()


def test_repeated_pairs_and_batch_slices(tv):
    five = [S.scene_pairs()[k] for k in (0, 1, 3, 6, 2)]
    refs = [S.scene_reference()[k] for k in (0, 1, 3, 6, 2)]
    r5, _ = run_both(tv, five, S.ITERATIONS, refs=refs)
    for b, p in enumerate(five):                        # B = 1 equals that pair's slice of the B = 5 call
        r1 = tv.init([lib_pair(tv, p)], iterations=S.ITERATIONS, keep_stages=1)
        assert S.differences(r1, 0, refs[b]) == []
        assert r1.read(0)["parallax_deg"].tobytes() == r5.read(b)["parallax_deg"].tobytes()
        r1.close()
    r5.close()
    r3 = tv.init([lib_pair(tv, five[1])] * 3, iterations=S.ITERATIONS, keep_stages=1)
    for b in range(3):
        assert S.differences(r3, b, refs[1]) == []
    r3.close()


def test_chunk_boundaries_change_no_byte(tv, monkeypatch):
    """the five pairs (ragged N; one below 8 matches) as one chunk, one chunk per pair and something between: the same bytes. The third budget is
    the documented cost (include/iba_mi355x_debug.h: 187 bytes per match + 148 per iteration) of the two smallest pairs, which are neighbours, plus
    2 KiB for the fixed records of each; every other pair of neighbours costs far more, so they share a chunk and no chunk holds three."""
    five = [S.scene_pairs()[k] for k in (0, 1, 3, 6, 2)]
    refs = [S.scene_reference()[k] for k in (0, 1, 3, 6, 2)]
    cost = sorted(187 * S.n_matches(p) + 148 * S.ITERATIONS for p in five)
    between = cost[0] + cost[1] + 2 * 2048
    assert between < sum(cost)
    parallax = None
    for budget, want in ((None, lambda c: c == 1), ("1", lambda c: c == 5), (str(between), lambda c: 1 < c < 5)):
        if budget is not None:
            monkeypatch.setenv("IBA_TWOVIEW_BUDGET", budget)
        r = tv.init([lib_pair(tv, p) for p in five], iterations=S.ITERATIONS, keep_stages=1)
        if budget is not None:
            monkeypatch.delenv("IBA_TWOVIEW_BUDGET")
        assert want(r.chunks), (budget, r.chunks)
        for b in range(5):
            assert S.differences(r, b, refs[b]) == [], (budget, b)
        got = [r.read(b)["parallax_deg"].tobytes() for b in range(5)]
        assert parallax is None or got == parallax, budget
        parallax = got
        r.close()


# ---- keep_stages left at its default of 0: tv_gather_kernel, the sel_* arrays at m_base offsets, and the branch of run_chunk that reads them ----
def run_plain(tv, pairs, iterations, refs):
    """the device result WITHOUT stages against the reference of every pair: 0 differing bytes in every output -> the result"""
    r = tv.init([lib_pair(tv, p) for p in pairs], iterations=iterations)
    assert len(r) == len(refs)
    for b, e in enumerate(refs):
        assert S.differences(r, b, e, stages=False) == [], "pair %d (%s)" % (b, R_NAMES[e["status"]])
    assert r.sweep_cap_hits == sum(e["sweep_cap_hits"] for e in refs)
    return r


def test_scene_list_without_stages(tv, err):
    pairs, refs = S.scene_pairs(), S.scene_reference()
    # the three ways through the branch: the gather runs (a candidate was named), the pair stopped before a candidate, the pair never reached the device
    assert any(e["status"] in (R.OK, R.LOW_PARALLAX) and e["chosen"] >= 0 for e in refs)
    assert any(e["status"] in (R.NO_CLEAR_WINNER, R.H_DEGENERATE, R.NO_MODEL) and e["chosen"] == -1 for e in refs)
    assert any(e["n_matches"] < 8 for e in refs)
    r = run_plain(tv, pairs, S.ITERATIONS, refs)
    kept = tv.init([lib_pair(tv, p) for p in pairs], iterations=S.ITERATIONS, keep_stages=1)
    for b in range(len(pairs)):
        assert S.output_bytes(r, b) == S.output_bytes(kept, b), b          # parallax_deg too: one libm on one machine
        for fn in (lambda: r.iterations_of(b), lambda: r.hypothesis(b, 0)):
            with pytest.raises(err, match="keep_stages"):
                fn()
    kept.close()
    r.close()


def test_gather_block_and_wave_edges_without_stages(tv):
    """the pairs of test_lane_and_wave_edges at 65 iterations: the N = 257 pair is accepted and its last match is a good point of the candidate, so the
    gather's second block of 256 lanes writes a point that is read; it is the sixth pair of the call, so its m_base is not 0"""
    sizes = (8, 9, 63, 64, 65, 257, 40)
    pairs = [exact_pair(N, 20 + N, 65, outliers=0.0, noise=0.1) for N in sizes]
    refs = [S.reference(p, 65) for p in pairs]
    big = refs[sizes.index(257)]
    assert sizes.index(257) > 0 and big["chosen"] >= 0 and big["status"] == R.OK and big["hyp_verdict"][big["chosen"]][256] == 6
    assert big["points"][big["list"][256, 0]].any() and big["triangulated"][big["list"][256, 0]] == 1
    assert sum(e["status"] == R.OK for e in refs) >= 3 and any(e["chosen"] == -1 for e in refs)
    run_plain(tv, pairs, 65, refs).close()


def test_chunk_boundaries_change_no_byte_without_stages(tv, monkeypatch):
    """test_chunk_boundaries_change_no_byte with keep_stages at its default; then a call all of whose pairs have fewer than 8 matches: every chunk
    returns before anything is queued"""
    five = [S.scene_pairs()[k] for k in (0, 1, 3, 6, 2)]
    refs = [S.scene_reference()[k] for k in (0, 1, 3, 6, 2)]
    cost = sorted(187 * S.n_matches(p) + 148 * S.ITERATIONS for p in five)
    between = cost[0] + cost[1] + 2 * 2048
    assert between < sum(cost)
    first = None
    for budget, want in ((None, lambda c: c == 1), ("1", lambda c: c == 5), (str(between), lambda c: 1 < c < 5)):
        if budget is not None:
            monkeypatch.setenv("IBA_TWOVIEW_BUDGET", budget)
        r = run_plain(tv, five, S.ITERATIONS, refs)
        if budget is not None:
            monkeypatch.delenv("IBA_TWOVIEW_BUDGET")
        print("chunks without stages at budget %s: %d" % (budget, r.chunks))
        assert want(r.chunks), (budget, r.chunks)
        got = [S.output_bytes(r, b) for b in range(5)]
        assert first is None or got == first, budget
        first = got
        r.close()
    few = [S.make_pair(6, n=9, unmatched=0.5, outliers=0.0), {"xy1": np.zeros((0, 2), F), "xy2": np.zeros((5, 2), F), "matches12": np.zeros(0, np.int32), "K": S.K4},
           S.make_pair(8, n=7, unmatched=0.0)]
    assert all(S.n_matches(p) < 8 for p in few) and S.n_matches(few[2]) == 7
    few_refs = [R.twoview(p["xy1"], p["xy2"], p["matches12"], p["K"], None, iterations=S.ITERATIONS) for p in few]
    assert all(e["status"] == R.TOO_FEW_MATCHES for e in few_refs)
    for budget in (None, "1"):
        if budget is not None:
            monkeypatch.setenv("IBA_TWOVIEW_BUDGET", budget)
        r = run_plain(tv, few, S.ITERATIONS, few_refs)
        if budget is not None:
            monkeypatch.delenv("IBA_TWOVIEW_BUDGET")
        assert r.chunks == (1 if budget is None else 3)
        r.close()


def test_more_pairs_than_one_block_of_lanes(tv):
    """73 pairs at 9 iterations: tv_motion_kernel and tv_accept_kernel give one lane to a pair in blocks of 64, so the second block runs with 9 of its
    lanes in use. The eight small pairs cycle and pair 0 comes once more as the last: an accepted pair, a pair refused by the acceptance and a pair
    below 8 matches stand on both sides of index 64"""
    S.check_small_reference()
    order = S.cycle_of_small(73)
    assert len(order) == 73 and order[72] == 0 and order[64:72] == list(range(8))
    small = [lib_pair(tv, p) for p in S.small_pairs()]
    refs = [S.small_reference()[k] for k in order]
    for keep in (1, 0):
        r = tv.init([small[k] for k in order], iterations=S.SMALL_ITERATIONS, keep_stages=keep)
        assert len(r) == 73 and r.chunks == 1
        for b, e in enumerate(refs):
            assert S.differences(r, b, e, stages=bool(keep)) == [], (keep, b, R_NAMES[e["status"]])
        assert r.sweep_cap_hits == sum(e["sweep_cap_hits"] for e in refs)
        assert S.output_bytes(r, 0) == S.output_bytes(r, 72)
        if keep:
            for k, x in r.iterations_of(0).items():
                assert x.tobytes() == r.iterations_of(72)[k].tobytes(), k
            for hyp in range(8):
                x, y = r.hypothesis(0, hyp), r.hypothesis(72, hyp)
                assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x), hyp
        r.close()


def test_singular_hypothesis_and_scattered_unmatched(tv):
    """set 0 is eight collinear points of frame 1: its homography is singular, H12i is not finite, and the score is whatever IEEE gives; a third of
    matches12 is -1"""
    p = S.make_pair(31, n=150, unmatched=0.33, outliers=0.1)
    lst = np.nonzero(p["matches12"] >= 0)[0]
    assert 0 < (p["matches12"] < 0).sum() and len(lst) > 60
    for k in range(8):
        p["xy1"][lst[5 * k]] = (100.0 + 40.0 * k, 50.0 + 20.0 * k)
    p = S.with_sets(p, 33, 9)
    p["sets"][0] = np.arange(8) * 5
    e = S.reference(p, 33)
    assert not np.isfinite(e["H12i"][0]).all() or abs(float(R.det33(e["Hi"][0]))) < 1e-6
    r, _ = run_both(tv, [p], 33, refs=[e])
    r.close()


def test_device_equals_host_restatement(tv):
    pairs = [lib_pair(tv, p) for p in S.scene_pairs()]
    d, h = tv.init(pairs, iterations=S.ITERATIONS, keep_stages=1), tv.init_host(pairs, iterations=S.ITERATIONS, keep_stages=1)
    assert d.sweep_cap_hits == h.sweep_cap_hits
    for b in range(len(pairs)):
        a, c = d.read(b), h.read(b)
        for k in a:
            assert np.asarray(a[k]).tobytes() == np.asarray(c[k]).tobytes(), (b, k)          # parallax_deg too: one libm on one machine
        for x, y in zip(d.matches(b) + d.points(b), h.matches(b) + h.points(b)):
            assert x.tobytes() == y.tobytes(), b
        for k, x in d.iterations_of(b).items():
            assert x.tobytes() == h.iterations_of(b)[k].tobytes(), (b, k)
        for hyp in range(8):
            x, y = d.hypothesis(b, hyp), h.hypothesis(b, hyp)
            assert all(np.asarray(x[k]).tobytes() == np.asarray(y[k]).tobytes() for k in x), (b, hyp)
    d.close()
    h.close()


def test_composition_with_orb_match(tv):
    """two synthetic frames through iba_orb_match (rule INIT); its match array is iba_twoview_init's matches12"""
    om = importlib.import_module(PKG + ".orb_match")
    frames = MS.sequence(2, 400, 5)
    job = MS.init_job(frames, 0, 1)
    m = om.match([om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in frames],
                 [om.job(job["query_frame"], job["train_frame"], job["rule"], job["centre_xy"], job["radius"], job["level_range"], job["query_index"], job.get("valid"))])
    match, _ = m.read(0)
    m.close()
    assert np.array_equal(match, MR.run(frames, [job])[1][0]["match"]) and (match >= 0).sum() >= 8
    p = S.with_sets({"xy1": frames[0]["xy"], "xy2": frames[1]["xy"], "matches12": match, "K": (500.0, 500.0, 320.0, 240.0)}, 40, 3)
    r, _ = run_both(tv, [p], 40)
    r.close()

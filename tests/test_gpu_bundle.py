"""Bundle adjustment on the device (include/iba_mi355x.h, iba_bundle*): iba_bundle_eval and iba_bundle_optimize BYTE FOR BYTE against the numpy
restatement tests/bundle_ref.py (with keep_stages, so a mismatch names its round) and against the host restatement iba_debug_bundle_host, at the
smallest shapes at which each rule can go wrong; the step and the sums under the project's gate against a long-double dense solve of the full damped
system; the same bytes alone, inside a ragged batch, split into chunks and on a second call; the composition with iba_twoview_init; every error.
The calls' default, keep_stages = 0 (stage tables of length 0, other chunk cuts), runs against the same references, and a call of 4105 tiny jobs takes
front_kernel and solve_kernel round their grid of 4096 workgroups a second time and back_kernel past its first block."""
import functools
import importlib

import numpy as np
import pytest

import bundle_ref as R
import bundle_scene as S
import twoview_scene as TS

PKG = "spatial-temporal-lidar-camera-calibration_amd"
pytestmark = pytest.mark.gpu
F = np.float32


@pytest.fixture(scope="module")
def bd():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".bundle")


@pytest.fixture(scope="module")
def err():
    return importlib.import_module(PKG).IbaError


@pytest.fixture()
def debug_env(monkeypatch):
    def set_(**kw):
        monkeypatch.setenv("IBA_DEBUG_ENV", "1")
        for k, v in kw.items():
            monkeypatch.setenv(k, str(v))
    return set_


def camera_counts_scene(seed):
    """free cameras with 0, 1, 63, 64, 65 and 129 edges (the lane rule and its tree) beside a fixed one that sees all 129 points"""
    counts = [129, 0, 1, 63, 64, 65, 129]
    vis = np.zeros((129, 7), bool)
    for c, k in enumerate(counts):
        vis[:k, c] = True
    return S.make(7, 129, seed, n_fixed=1, visibility=vis)


def losing_scene(seed):
    """a free camera and a point all of whose observations are gross (40..200 pixels, each its own direction): the classification after round 0 takes
    all their edges, and round 1 runs without them (a camera without a row, a point left out)"""
    sc = S.make(6, 60, seed, n_fixed=2, noise=0.5)
    g = np.random.default_rng(seed)
    hit = (sc["edge_camera"] == 4) | (sc["edge_point"] == 7)
    obs = sc["obs"].astype(np.float64)
    obs[hit] += (g.uniform(40, 200, (len(obs), 2)) * g.choice([-1, 1], (len(obs), 2)))[hit]
    sc["obs"], sc["hit"] = obs.astype(F), hit
    return sc


def ragged_scenes():
    """40 ragged jobs: every count of free cameras of the issue's list but the cap, the point counts 0, 1, 255, 256, 257, no edge, a point with no
    edge, a point seen by fixed cameras alone, a free camera with no edge, the point lists of 1, 2, 3 and 65, outliers"""
    no_edge_point = np.ones((20, 3), bool)
    no_edge_point[5] = False
    scs = [S.make(3, 40, 100, n_fixed=3), S.make(2, 60, 101), S.make(3, 50, 102, n_fixed=1), S.make(6, 40, 103, n_fixed=1, visibility=0.7),
           S.make(12, 30, 104, n_fixed=1, visibility=0.6), S.make(3, 30, 105, n_fixed=0), S.make(4, 0, 106), S.make(2, 1, 107), S.make(2, 255, 108, outliers=0.05),
           S.make(2, 256, 109), S.make(2, 257, 110, outliers=0.1), S.make(3, 25, 111, visibility=np.zeros((25, 3), bool)), S.make(3, 20, 112, visibility=no_edge_point),
           S.make(66, 6, 113, n_fixed=60, visibility=S.with_counts([1, 2, 3, 65, 66, 64], 66)), camera_counts_scene(114), losing_scene(115), S.make(0, 4, 116, n_fixed=0),
           S.exact_scene(4, 30, 117)]
    scs += [S.make(2 + k % 4, 10 + 7 * k, 200 + k, n_fixed=1 + k % 2, outliers=0.05 * (k % 3), visibility=None if k % 2 else 0.8) for k in range(40 - len(scs))]
    return scs


@pytest.fixture(scope="module")
def ragged():
    return ragged_references()[:2]


@functools.lru_cache(maxsize=None)
def ragged_references():
    """-> (the scenes, S.ref_of(sc)[0], S.ref_of(sc, stages=False)[0]) from ONE run of the reference per scene: the first is the second with the
    stages of the same run appended, which is all that S.ref_of does"""
    scs = ragged_scenes()
    plain = [S.ref_of(sc, stages=False) for sc in scs]
    return scs, [R.with_stages(out, extras) for out, extras in plain], [out for out, _ in plain]


@pytest.fixture(scope="module")
def ragged_plain():
    return ragged_references()[2]


def run_plain(bd, err, scs, opt, refs=None, kept=None):
    """keep_stages = 0, the calls' default, on the device and through the host restatement: every output against the reference without its stage
    entries, against the host, and against the entries of the same names of a call that kept the stages; iba_bundle_stage refuses"""
    refs = [S.ref_of(sc, stages=False, **opt)[0] for sc in scs] if refs is None else refs
    jobs = [S.lib_job(bd, sc) for sc in scs]
    o = S.lib_options(bd, opt, keep_stages=0)
    d, h = bd.optimize(jobs, o), bd.optimize_host(jobs, o)
    assert len(d) == len(scs) and d.big_steps == 0
    for j, e in enumerate(refs):
        got = d.everything(j)
        assert not any(k.startswith("stage") for k, _ in e) and R.differences(got, e) == [], j
        assert R.differences(got, h.everything(j)) == [], j
        if kept is not None:
            assert R.differences(got, S.without_stages(kept.everything(j))) == [], j
    for res in (d, h):
        with pytest.raises(err, match="keep_stages"):
            res.stage(0, 0)
    h.close()
    return d


def run_both(bd, scs, opt, refs=None):
    """device against reference and against the host restatement, every output and every stage"""
    refs = [S.ref_of(sc, **opt)[0] for sc in scs] if refs is None else refs
    jobs = [S.lib_job(bd, sc) for sc in scs]
    o = S.lib_options(bd, opt)
    d, h = bd.optimize(jobs, o), bd.optimize_host(jobs, o)
    assert len(d) == len(scs) and d.big_steps == 0
    for j, e in enumerate(refs):
        got = d.everything(j)
        assert R.differences(got, e) == [], j
        assert R.differences(got, h.everything(j)) == [], j
    h.close()
    return d


# ---- iba_bundle_eval ----
def test_eval_against_reference_and_long_double(bd):
    scs, masks = S.eval_cases()
    scs, masks = scs + [camera_counts_scene(5), S.make(12, 30, 6, n_fixed=1, visibility=0.6)], masks + [None, None]
    note = []
    for robust, lam, m in ((True, 1e-3, None), (False, 10.0, masks)):
        S.check_eval(bd, scs, m, robust, lam, False, note)
    print("eval (device): the largest share of the gate (4 x the restatement's own error + one ulp of the scale) used:", max(note))


def test_eval_huber_knee_depth_and_failed_inverse(bd):
    """the last information at or below the Huber knee and the first above it; a point behind a camera and one with p_z == 0 exactly (a chi2 that is
    not finite); lambda = 0 with a point whose informations are all zero (a 3 x 3 of zeros: the failed trial of B5)"""
    sc = S.make(3, 32, 11, n_fixed=1, outliers=0.5)
    q = S.ref_job(sc)
    ones = R.Job(sc["T_start"], sc["fixed"], sc["xyz"], sc["edge_point"], sc["edge_camera"], sc["obs"], np.ones(q.ne, F), sc["K"])
    r2, _ = R.edges(ones, ones.T, ones.X, jac=False)
    dsqr = np.float64(R.LOCAL_DELTA) * np.float64(R.LOCAL_DELTA)
    w = np.zeros(q.ne, F)
    for i, v in enumerate(r2):
        lo = F(dsqr / v)
        while np.float64(lo) * v > dsqr:
            lo = np.nextafter(lo, F(0))
        while np.float64(np.nextafter(lo, F(np.inf))) * v <= dsqr:
            lo = np.nextafter(lo, F(np.inf))
        w[i] = lo if i % 2 == 0 else np.nextafter(lo, F(np.inf))
    knee = dict(sc, inv_sigma2=w)
    c, _ = R.edges(S.ref_job(knee), q.T, q.X, jac=False)
    assert np.all(c[0::2] <= dsqr) and np.all(c[1::2] > dsqr)
    behind = dict(sc, xyz=sc["xyz"].copy())
    T1 = sc["T_start"][1]
    behind["xyz"][5] = (T1[:, :3].T @ (np.array([0.3, -0.2, -4.0]) - T1[:, 3])).astype(F)
    zero = S.exact_scene(3, 20, 3)
    zero["T_start"] = zero["T_true"].copy()
    zero["xyz"][7] = (1.0, 2.0, 0.0)                     # p_z == 0 exactly under the exact scene's translations
    once = S.make(3, 10, 12, n_fixed=1)
    once["inv_sigma2"] = np.where(once["edge_point"] == 9, F(0), once["inv_sigma2"]).astype(F)      # Hll of point 9 is exactly zero
    note = []
    S.check_eval(bd, [knee, behind, zero, once], None, True, 0.0, False, note)
    S.check_eval(bd, [knee, behind, zero, once], None, True, 2.0, False, note)
    got = bd.evaluate([S.lib_job(bd, zero), S.lib_job(bd, once)], lam=0.0)
    assert not np.isfinite(got[0]["chi2_edges"]).all() and got[1]["solved"] == 0


# ---- iba_bundle_optimize ----
def test_optimize_ragged_batch_in_one_call(bd, ragged):
    scs, refs = ragged
    d = run_both(bd, scs, R.LOCAL, refs)
    assert d.chunks == 1
    # the losing scene (job 15): after round 0 no edge of camera 4 and none of point 7 is active (the scene is chosen so), on the device as in the reference
    hit = scs[15]["hit"]
    _, extras = S.ref_of(scs[15])
    assert not extras["active"][hit].any() and extras["active"].sum() > 100
    assert d.read(15)["n_bad"][0] == int((~extras["active"]).sum()) >= int(hit.sum())
    d.close()


def test_optimize_the_cap_of_64_free_cameras(bd):
    """65 cameras, one fixed: a reduced system of 384; a handful of points each; and 11 free cameras: 66 unknowns"""
    scs = [S.make(65, 14, 300, n_fixed=1, visibility=0.5), S.make(12, 30, 301, n_fixed=1, visibility=0.6)]
    run_both(bd, scs, R.global_options(3, True)).close()


@pytest.mark.parametrize("opt", [R.global_options(20, True), R.global_options(10, False), dict(R.LOCAL, rounds=4, iterations=(1, 1, 2, 1), robust_rounds=2),
                                 dict(R.LOCAL, rounds=1, iterations=(1, 0, 0, 0))], ids=["global-robust", "global-plain", "four-rounds", "one-iteration"])
def test_optimize_other_schedules(bd, opt):
    scs = [S.make(2, 60, 400), S.make(5, 40, 401, n_fixed=2, outliers=0.1, visibility=0.7), S.make(3, 30, 402, n_fixed=0), losing_scene(403)]
    run_both(bd, scs, opt).close()


def test_optimize_all_outliers_non_finite_start_and_a_point_behind(bd):
    """a job every edge of which is an outlier (a threshold of 0: round 1 runs on nothing, one trial, rho == 0); a start whose chi2 is not finite
    (p_z == 0 exactly); a point behind a camera at the start, whose edges end up flagged"""
    gone = S.make(3, 40, 500)
    strict = dict(R.LOCAL, chi2_threshold=F(0))
    ref_gone, extras = S.ref_of(gone, **strict)
    assert dict(ref_gone)["n_bad"][0] == len(gone["obs"]) and not extras["active"].any() and dict(ref_gone)["trials"][1] == 1
    run_both(bd, [gone], strict, [ref_gone]).close()
    zero = S.exact_scene(3, 20, 3)
    zero["xyz"][7] = (1.0, 2.0, 0.0)
    zero["T_start"] = zero["T_true"].copy()
    behind = S.make(3, 40, 501, outliers=0.1)
    T1 = behind["T_start"][1]
    behind["xyz"][3] = (T1[:, :3].T @ (np.array([0.5, 0.1, -3.0]) - T1[:, 3])).astype(F)
    refs = [S.ref_of(sc)[0] for sc in (zero, behind)]
    assert not np.isfinite(dict(refs[0])["chi2"][0])
    assert dict(refs[1])["outlier"][np.flatnonzero(behind["edge_point"] == 3)].all()
    run_both(bd, [zero, behind], R.LOCAL, refs).close()


def test_optimize_trials_through_and_onto_the_camera_plane(bd):
    """the depth conditions at a TRIAL estimate, not the start. overshoot_scene: the first steps carry a point through the camera planes (p_z < 0 at
    trials whose chi2 is finite: rejected by rho, more trials than iterations). zero_depth_trial_scene: p_z == 0 EXACTLY at the first trial and
    nowhere before it; the trial's chi2 is NaN, the trial is rejected by the finite test and the iteration ends without a stop - beside the same job
    without that edge, which takes another path"""
    through = S.overshoot_scene(32)
    onto = S.zero_depth_trial_scene(41)
    plain = dict(onto, xyz=onto["xyz"][:-1], edge_point=onto["edge_point"][:-1], edge_camera=onto["edge_camera"][:-1], obs=onto["obs"][:-1], inv_sigma2=onto["inv_sigma2"][:-1])
    refs = [S.ref_of(sc) for sc in (through, onto, plain)]
    S.check_trial_scenes(refs)
    run_both(bd, [through, onto, plain], R.LOCAL, [r[0] for r in refs]).close()
    run_both(bd, [through, onto], R.global_options(10, False)).close()


def test_same_bytes_alone_in_a_batch_split_and_repeated(bd, ragged, debug_env):
    scs, refs = ragged
    alone = bd.optimize([S.lib_job(bd, scs[3])], S.lib_options(bd, R.LOCAL))
    assert R.differences(alone.everything(0), refs[3]) == []
    alone.close()
    debug_env(IBA_BUNDLE_BUDGET=1)                        # every job a chunk of its own
    a = run_both(bd, scs[:8], R.LOCAL, refs[:8])
    assert a.chunks == 8
    a.close()
    sizes = sorted(len(sc["edge_point"]) for sc in scs)
    debug_env(IBA_BUNDLE_BUDGET=3 * 260 * sizes[len(sizes) // 2])     # about three median jobs per chunk
    b = run_both(bd, scs, R.LOCAL, refs)
    assert 1 < b.chunks < len(scs)
    b.close()
    debug_env(IBA_BUNDLE_BUDGET=1 << 30)
    c = run_both(bd, scs, R.LOCAL, refs)                   # a second call
    assert c.chunks == 1
    c.close()


# ---- keep_stages = 0, the calls' default ----
def test_optimize_ragged_batch_without_stages(bd, err, ragged, ragged_plain):
    scs, _ = ragged
    kept = bd.optimize([S.lib_job(bd, sc) for sc in scs], S.lib_options(bd, R.LOCAL))
    d = run_plain(bd, err, scs, R.LOCAL, ragged_plain, kept)
    assert d.chunks == 1 and kept.chunks == 1
    d.close()
    kept.close()


def test_optimize_the_cap_of_64_free_cameras_without_stages(bd, err):
    scs = [S.make(65, 14, 300, n_fixed=1, visibility=0.5), S.make(12, 30, 301, n_fixed=1, visibility=0.6)]
    opt = R.global_options(3, True)
    kept = bd.optimize([S.lib_job(bd, sc) for sc in scs], S.lib_options(bd, opt))
    run_plain(bd, err, scs, opt, kept=kept).close()
    kept.close()


def test_same_bytes_split_into_chunks_without_stages(bd, err, ragged, ragged_plain, debug_env):
    """the budgets of test_same_bytes_alone_in_a_batch_split_and_repeated. Without the stage tables a job costs less, so the chunk cuts fall elsewhere;
    the middle budget is three median jobs at 222 bytes per edge, the edge term of job_bytes without them (4 x 5 + 12 + 1 + 1 + 4 + 8 x 23)"""
    scs, _ = ragged
    alone = bd.optimize([S.lib_job(bd, scs[3])], S.lib_options(bd, R.LOCAL, keep_stages=0))
    assert R.differences(alone.everything(0), ragged_plain[3]) == []
    alone.close()
    debug_env(IBA_BUNDLE_BUDGET=1)                        # every job a chunk of its own
    a = run_plain(bd, err, scs[:8], R.LOCAL, ragged_plain[:8])
    assert a.chunks == 8
    a.close()
    sizes = sorted(len(sc["edge_point"]) for sc in scs)
    debug_env(IBA_BUNDLE_BUDGET=3 * 222 * sizes[len(sizes) // 2])
    b = run_plain(bd, err, scs, R.LOCAL, ragged_plain)
    print("chunks of the 40 ragged jobs without stages at three median jobs a chunk:", b.chunks)
    assert 1 < b.chunks < len(scs)
    b.close()
    debug_env(IBA_BUNDLE_BUDGET=1 << 30)
    c = run_plain(bd, err, scs, R.LOCAL, ragged_plain)     # a second call
    assert c.chunks == 1
    c.close()


# ---- more jobs than workgroups ----
MAX_GRID = 4096      # kMaxGrid of csrc/iba_bundle_kernels.hpp
MANY = 4105          # front_kernel and solve_kernel run on min(n_jobs, 4096) workgroups: the first 9 take a second job; back_kernel: 17 blocks of 256 lanes


@pytest.mark.parametrize("shifted", [False, True], ids=["cycle", "shifted"])
def test_optimize_more_jobs_than_workgroups(bd, shifted):
    """4105 jobs under the local schedule, the eight tiny scenes in turn and scene 0 once more as the last job: all eight make the second trip of a
    workgroup (jobs 4096..4103). front_kernel and solve_kernel give job j to workgroup j % 4096, and 4096 is a multiple of 8, so in the plain cycle a
    workgroup's two jobs are one scene and finish at one step. The shifted order moves the scenes of the second trip on by three: there a workgroup's
    first job is done (kind == kDone, or no proposal for the solve) while its second still runs, and in another workgroup the other way round. Every
    output and stage of every job against the reference and the host restatement, then the same call without the stages"""
    S.check_tiny_reference()
    order = S.shifted_cycle_of_tiny(MANY, MAX_GRID) if shifted else S.cycle_of_tiny(MANY)
    assert len(order) == MANY > MAX_GRID and (MANY + 255) // 256 == 17 and MAX_GRID % 8 == 0 and order[:MAX_GRID] == S.cycle_of_tiny(MANY)[:MAX_GRID]
    S.check_second_trip(order, MAX_GRID, differ=shifted)
    tiny = [S.lib_job(bd, sc) for sc in S.tiny_scenes()]
    jobs = [tiny[k] for k in order]
    for keep, refs in zip((1, 0), S.tiny_reference()):
        o = S.lib_options(bd, R.LOCAL, keep_stages=keep)
        d, h = bd.optimize(jobs, o), bd.optimize_host(jobs, o)
        assert len(d) == MANY and d.big_steps == 0 and d.chunks == 1
        first = d.everything(0)
        assert len(first) == (15 if keep else 11)
        for j, k in enumerate(order):
            got = d.everything(j)
            assert R.differences(got, refs[k]) == [], (keep, j)
            assert R.differences(got, h.everything(j)) == [], (keep, j)
        assert R.differences(d.everything(MANY - 1), first) == []
        d.close()
        h.close()


def test_eval_more_jobs_than_workgroups(bd):
    """iba_bundle_eval goes through the same front_kernel and solve_kernel with o.eval set: 4105 jobs, the byte comparison of S.check_eval on every one.
    iba_bundle_eval reports no chunk count. The jobs run as ONE chunk, so that workgroups do take a second job: job_bytes of an evaluation is that of
    an optimisation without stages plus 8 bytes per edge (at most 36 edges: 288), less than the stage term of 4 x 8 x (12 cameras + 3 points) >= 768
    that test_optimize_more_jobs_than_workgroups pays for the same jobs, and that call asserts chunks == 1 under the same budget"""
    order = S.cycle_of_tiny(MANY)
    S.check_second_trip(order, MAX_GRID, differ=False)    # an evaluation has no early finish: a workgroup's two jobs may be one scene
    tiny = [S.lib_job(bd, sc) for sc in S.tiny_scenes()]
    for robust, lam in ((True, 1e-3), (False, 10.0)):
        own = [R.evaluate(S.ref_job(sc), None, robust, lam) for sc in S.tiny_scenes()]
        assert sum(e["solved"] for e in own) >= 6
        got = bd.evaluate([tiny[k] for k in order], robust=robust, lam=lam)
        assert len(got) == MANY
        for j, k in enumerate(order):
            assert S.eval_differences(bd, got[j], own[k]) == [], (robust, lam, j)


def test_composition_with_twoview_init(bd):
    """the result of iba_twoview_init on a twoview_scene pair as a two-camera job (the first camera fixed at the identity, the triangulated points,
    the matches as edges) through the global schedule of CreateInitialMapMonocular, device against restatement"""
    tv = importlib.import_module(PKG + ".twoview")
    p = TS.with_sets(TS.make_pair(seed=0, n=300), TS.ITERATIONS, TS.SETS_SEED)      # the scene list's "general_ok"
    r = tv.init([tv.pair(p["xy1"], p["xy2"], p["matches12"], p["K"], p["sets"])], iterations=TS.ITERATIONS)
    d = r.read(0)
    pts, tri = r.points(0)
    idx = np.flatnonzero(tri)
    assert len(idx) >= 50
    T = np.zeros((2, 3, 4))
    T[0, :, :3] = np.eye(3)
    T[1, :, :3], T[1, :, 3] = d["R21"].astype(np.float64), d["t21"].astype(np.float64)
    n = len(idx)
    sc = dict(T_start=T, fixed=np.array([1, 0], np.uint8), xyz=pts[idx], edge_point=np.concatenate([np.arange(n), np.arange(n)]).astype(np.int32),
              edge_camera=np.concatenate([np.zeros(n), np.ones(n)]).astype(np.int32), obs=np.concatenate([p["xy1"][idx], p["xy2"][p["matches12"][idx]]]).astype(F),
              inv_sigma2=np.ones(2 * n, F), K=p["K"])
    r.close()
    opt = R.global_options(20, True)
    res = run_both(bd, [sc], opt)
    out = res.read(0)
    first = R.evaluate(S.ref_job(sc), None, True, 0.0, delta=R.GLOBAL_DELTA)
    assert out["chi2"][0] <= first["chi2_robust"] and out["n_free"] == 1
    res.close()


def test_errors(bd, err):
    S.check_errors(bd, err, host=False)

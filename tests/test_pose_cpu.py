"""Motion-only pose optimisation without a device (include/iba_mi355x.h, iba_pose*): the numpy restatement tests/pose_ref.py against the truth of seeded
scenes, the Jacobian and the series of rule P6 against wider arithmetic, the host restatement behind iba_debug_pose_host BYTE FOR BYTE against pose_ref on
every output, iba_pose_edges_from_matches, every error by its message, and the stand-alone sanitizer self-test."""
import ctypes as C
import importlib
import math
import os
import subprocess

import numpy as np
import pytest

import pose_ref as R
import pose_scene as S

PKG = "spatial-temporal-lidar-camera-calibration_amd"
SIZES = (0, 1, 2, 3, 9, 10, 63, 64, 65, 255, 256, 257)


@pytest.fixture(scope="module")
def ps():
    importlib.import_module(PKG)
    return importlib.import_module(PKG + ".pose")


@pytest.fixture(scope="module")
def err():
    return importlib.import_module(PKG).IbaError


# ---- the reference against truth ----
def test_reference_recovers_a_noiseless_pose():
    sc = S.exact_scene(300, 1)
    e = S.ref_of(sc)
    assert e["rounds_run"] == 4 and e["n_inliers"] == 300 and not e["outlier"].any()
    assert np.abs(e["Tcw12"] - sc["T_true"]).max() < 1e-9
    assert e["chi2"][3] < 1e-12


def test_reference_flags_exactly_the_gross_outliers():
    sc = S.make(300, 4, noise=0.4, outliers=0.2)
    e = S.ref_of(sc)
    assert sc["is_outlier"].sum() == 60
    assert e["margin"] > 1e-6                         # no classified chi2 within 1e-6 relative of the threshold at any round
    assert np.array_equal(e["outlier"].astype(bool), sc["is_outlier"])
    assert e["n_inliers"] == 240 and e["rounds_run"] == 4
    assert np.abs(e["Tcw12"] - sc["T_true"]).max() < 0.02


def test_jacobian_against_central_differences():
    sc = S.make(40, 5)
    _, _, _, J = R.edge(sc["T_start"], sc["K"], sc["xyz"], sc["obs"], sc["inv_sigma2"])
    J = np.stack(J, 1).reshape(-1, 2, 6)
    worst = 0.0
    for i in range(40):
        Jn = R.jacobian_central(sc["T_start"], sc["K"], sc["xyz"][i], sc["obs"][i], h=1e-5).astype(np.float64)
        worst = max(worst, float(np.max(np.abs(J[i] - Jn) / (1.0 + np.abs(Jn)))))
    # central differences in long double with h = 1e-5: truncation h^2 |J'''| / 6 ~ 1e-10 relative, rounding 2^-64 / h ~ 1e-14
    assert worst < 1e-8, worst


def test_series_within_one_ulp_of_the_leading_term(ps):
    import mpmath as mp
    worst = [0.0, 0.0, 0.0]
    grid = np.concatenate([np.linspace(0.0, math.pi, 4001), np.linspace(3.0, math.pi, 1001), [1e-8, 1e-4, math.sqrt(R.PI2)]])
    for th in grid:
        s = min(float(th) * float(th), R.PI2)
        lib = ps.series(s)
        for off in (1, 2, 3):
            v = R.series(s, off)
            assert v == lib[off - 1]                  # the library's series is the reference's, bit for bit
            ulp = [2.0 ** -52, 2.0 ** -53, 2.0 ** -55][off - 1]          # one ulp of 1, 1/2, 1/6
            worst[off - 1] = max(worst[off - 1], float(abs(mp.mpf(v) - R.series_exact(s, off)) / ulp))
    print("series: worst error in ulp of the leading term:", worst)
    assert max(worst) <= 1.0, worst
    # the truncation: the first omitted term at theta = pi, relative to the leading one, is below 2^-53
    for off in (1, 2, 3):
        assert math.pi ** 28 / math.factorial(28 + off) * math.factorial(off) < 2.0 ** -53


# ---- the host restatement against the reference, byte for byte ----
@pytest.fixture(scope="module")
def ragged():
    return [S.make(n, 100 + n, outliers=0.2 if n >= 10 else 0.0) for n in SIZES]


def test_host_restatement_equals_reference(ps, ragged):
    jobs = [S.lib_job(ps, sc) for sc in ragged]
    h = ps.optimize_host(jobs, keep_stages=1)
    assert len(h) == len(SIZES)
    for j, sc in enumerate(ragged):
        assert S.differences(h, j, S.ref_of(sc)) == [], SIZES[j]
    assert h.big_steps == 0
    h.close()
    for j, sc in enumerate(ragged):                   # and one job per call
        h = ps.optimize_host([jobs[j]], keep_stages=1)
        assert S.differences(h, 0, S.ref_of(sc)) == [], SIZES[j]
        h.close()


def test_host_restatement_on_a_non_finite_trial(ps):
    sc = S.nonfinite_trial_scene()
    e = S.ref_of(sc)
    assert e["nonfinite_trials"] >= 1 and e["big_steps"] == 0
    h = ps.optimize_host([S.lib_job(ps, sc)], keep_stages=1)
    assert S.differences(h, 0, e) == []
    h.close()


def test_host_restatement_with_other_options(ps):
    sc = S.make(120, 7, outliers=0.25)
    for opt in (dict(rounds=2, iterations=3), dict(rounds=6, iterations=15, robust_rounds=1), dict(rounds=1, iterations=1, robust_rounds=0), dict(chi2_threshold=np.float32(9.21))):
        h = ps.optimize_host([S.lib_job(ps, sc)], keep_stages=1, **opt)
        assert S.differences(h, 0, S.ref_of(sc, **opt)) == [], opt
        h.close()


def test_host_eval_equals_reference(ps, ragged):
    g = np.random.default_rng(3)
    for robust in (True, False):
        masks = [None if len(sc["xyz"]) % 2 else (g.uniform(size=len(sc["xyz"])) < 0.7).astype(np.uint8) for sc in ragged]
        H, b, c, per = ps.evaluate([S.lib_job(ps, sc) for sc in ragged], active=masks, robust=robust, host=True)
        for j, sc in enumerate(ragged):
            eH, eb, ec, ep = R.eval_job(sc["T_start"], sc["K"], sc["xyz"], sc["obs"], sc["inv_sigma2"], masks[j], robust)
            assert H[j].tobytes() == eH.tobytes() and b[j].tobytes() == eb.tobytes() and c[j].tobytes() == np.float64(ec).tobytes() and per[j].tobytes() == ep.tobytes(), SIZES[j]


def test_exp_equals_reference(ps):
    g = np.random.default_rng(9)
    T = S.pose(g.normal(0, 0.4, 3), g.normal(0, 2, 3))
    for scale in (1e-9, 1e-3, 0.3, 1.7):
        dx = g.normal(0, 1, 6) * scale
        a, big = ps.exp_update(dx, T)
        e, ebig = R.exp_update(dx, T)
        assert big == ebig == 0 and a.tobytes() == e.tobytes()
        assert np.abs(a[:, :3] @ a[:, :3].T - np.eye(3)).max() < 1e-14
    a, big = ps.exp_update([0, 3.5, 0, 0, 0, 0], T)
    assert big == 1 and np.abs(a[:, :3] - S.rot([0, 3.5, 0]) @ T[:, :3]).max() < 1e-14


def test_edges_from_matches(ps):
    g = np.random.default_rng(21)
    n_last, n_cur = 60, 50
    world = g.normal(0, 5, (n_last, 3)).astype(np.float32)
    world[10] = world[11]                              # repeated world points
    world[20] = world[11]
    xy, octave = g.uniform(0, 600, (n_cur, 2)).astype(np.float32), g.integers(0, 8, n_cur)
    match = np.full(n_last, -1, np.int32)
    pick = g.choice(n_cur, 30, replace=False)
    match[g.choice(n_last, 30, replace=False)] = pick  # 20 keypoints of the current frame stay unmatched
    for qi in (None, g.permutation(n_last).astype(np.int32)):
        got = ps.edges_from_matches(match, qi, world, xy, octave, S.INV_LEVEL_SIGMA2)
        want = R.edges_from_matches(match, qi, world, xy, octave, S.INV_LEVEL_SIGMA2)
        assert len(got[3]) == 30 and np.all(np.diff(got[3]) > 0)
        for a, b in zip(got, want):
            assert a.tobytes() == b.tobytes()
    got = ps.edges_from_matches(np.zeros(0, np.int32), None, world, xy, octave, S.INV_LEVEL_SIGMA2)
    assert len(got[0]) == 0
    # two queries name the same keypoint: the later query overwrites, as the assignment mvpMapPoints[c] = pMP does
    twice = np.array([4, -1, 7, 4, 7, -1], np.int32)
    for qi in (None, np.array([9, 8, 7, 6, 5, 3], np.int32)):
        got = ps.edges_from_matches(twice, qi, world, xy, octave, S.INV_LEVEL_SIGMA2)
        assert list(got[3]) == [4, 7]
        assert got[0].tobytes() == world[[3, 4] if qi is None else [6, 5]].tobytes()
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, R.edges_from_matches(twice, qi, world, xy, octave, S.INV_LEVEL_SIGMA2)))


# ---- errors, by message ----
def test_errors(ps, err):
    sc = S.make(20, 8)

    def bad(msg, fn):
        with pytest.raises(err) as e:
            fn()
        assert msg in str(e.value), str(e.value)

    def with_(**kw):
        d = dict(sc)
        for k, v in kw.items():
            a = np.array(d[k], copy=True)
            a.reshape(-1)[v[0]] = v[1]
            d[k] = a
        return S.lib_job(ps, d)

    run = lambda jobs, **o: ps.optimize_host(jobs, **o)
    good = S.lib_job(ps, sc)
    bad("B = 0 < 1", lambda: run([]))
    bad("struct_size", lambda: run([good], struct_size=3))
    bad("rounds 0 is outside 1..8", lambda: run([good], rounds=0))
    bad("rounds 9 is outside 1..8", lambda: run([good], rounds=9))
    bad("iterations 101 is outside 1..100", lambda: run([good], iterations=101))
    bad("iterations 0 is outside 1..100", lambda: run([good], iterations=0))
    bad("chi2_threshold is not finite", lambda: run([good], chi2_threshold=float("nan")))
    bad("huber_delta is not finite or <= 0", lambda: run([good], huber_delta=0.0))
    bad("robust_rounds -1 is outside 0..8", lambda: run([good], robust_rounds=-1))
    bad("robust_rounds 9 is outside 0..8", lambda: run([good], robust_rounds=9))
    bad("chi2_threshold is not finite or < 0", lambda: run([good], chi2_threshold=-1.0))
    bad("job 1: edge 3: the point is not finite", lambda: run([good, with_(xyz=(9, np.nan))]))
    bad("job 0: edge 2: the observation is not finite", lambda: run([with_(obs=(5, np.inf))]))
    bad("job 0: edge 4: inv_sigma2 is not finite", lambda: run([with_(inv_sigma2=(4, np.nan))]))
    bad("job 0: edge 4: inv_sigma2 < 0", lambda: run([with_(inv_sigma2=(4, -1.0))]))
    bad("job 0: the pose is not finite", lambda: run([with_(T_start=(7, np.inf))]))
    for K, msg in (((0.0, 500, 1, 1), "fx or fy is not finite or <= 0"), ((500, -1.0, 1, 1), "fx or fy is not finite or <= 0"), ((500, 500, np.nan, 1), "cx or cy is not finite")):
        bad("job 0: " + msg, lambda K=K: run([ps.job(sc["T_start"], sc["xyz"], sc["obs"], sc["inv_sigma2"], K)]))
    q = S.lib_job(ps, sc)
    q.n = -1
    bad("n = -1 is outside 0..32768", lambda: run([q]))
    q.n = 32769
    bad("n = 32769 is outside 0..32768", lambda: run([q]))
    q = S.lib_job(ps, sc)
    q.obs = None
    bad("xyz, obs or inv_sigma2 is NULL", lambda: run([q]))
    q = S.lib_job(ps, sc)
    q.Tcw12 = None
    bad("Tcw12 is NULL", lambda: run([q]))
    L = ps._lib()
    assert L.iba_debug_pose_host(None, 1, C.addressof(ps.options()), C.addressof(C.c_void_p())) != 0 and b"jobs is NULL" in L.iba_pose_last_error()
    assert L.iba_debug_pose_host(None, 1, None, C.addressof(C.c_void_p())) != 0 and b"options is NULL" in L.iba_pose_last_error()
    assert L.iba_debug_pose_host(None, 1, None, None) != 0 and b"out is NULL" in L.iba_pose_last_error()
    assert L.iba_default_pose_options(None) != 0 and b"opt is NULL" in L.iba_pose_last_error()
    assert L.iba_pose_read(None, 0, None) != 0 and b"the result is NULL" in L.iba_pose_last_error()
    ja, z = ps._job_array([good]), np.zeros(36)
    for H, b, c in ((None, z, z), (z, None, z), (z, z, None)):
        for fn, dev in ((L.iba_pose_eval, [C.c_int(0)]), (L.iba_debug_pose_eval_host, [])):
            assert fn(C.addressof(ja), 1, None, 1, *dev, ps._p(H), ps._p(b), ps._p(c), None) != 0 and b"H, b or chi2_robust is NULL" in L.iba_pose_last_error()
    k = run([good], keep_stages=1)
    assert L.iba_pose_read(k.p, 0, None) != 0 and b"iba_pose_read: result is NULL" in L.iba_pose_last_error()
    assert L.iba_pose_stage(k.p, 0, 0, None) != 0 and b"iba_pose_stage: Tcw12 is NULL" in L.iba_pose_last_error()
    assert L.iba_pose_edges(None, 0, None, None) != 0 and b"iba_pose_edges: the result is NULL" in L.iba_pose_last_error()
    assert L.iba_pose_edges(k.p, 0, None, None) == 0                       # both outputs may be NULL
    k.close()
    # the same checks stand in front of the device entry points: nothing here reaches a device
    with pytest.raises(err) as e:
        ps.optimize([good], rounds=0)
    assert "iba_pose_optimize: rounds 0" in str(e.value)
    with pytest.raises(err) as e:
        ps.evaluate([with_(xyz=(0, np.inf))])
    assert "iba_pose_eval: job 0: edge 0: the point is not finite" in str(e.value)
    # accessors
    h = run([good, S.lib_job(ps, S.make(0, 1))])
    assert len(h) == 2 and h.read(1)["n"] == 0 and h.read(1)["n_inliers"] == 0     # n == 0 is legal
    bad("job 2 is outside the result's 2 jobs", lambda: h.read(2))
    bad("job -1 is outside the result's 2 jobs", lambda: h.edges(-1))
    bad("the call did not ask for keep_stages", lambda: h.stage(0, 0))
    h.close()
    h = run([good], keep_stages=1)
    bad("round 4 is outside the job's 4 rounds", lambda: h.stage(0, 4))
    h.close()
    bad("match 0 names keypoint 7 of 5", lambda: ps.edges_from_matches([7], None, np.zeros((3, 3)), np.zeros((5, 2)), np.zeros(5, np.int32), S.INV_LEVEL_SIGMA2))
    bad("query 0 names keypoint 9 of the last frame's 3", lambda: ps.edges_from_matches([1], [9], np.zeros((3, 3)), np.zeros((5, 2)), np.zeros(5, np.int32), S.INV_LEVEL_SIGMA2))
    bad("keypoint 1 has octave 8 of 8 levels", lambda: ps.edges_from_matches([1], None, np.zeros((3, 3)), np.zeros((5, 2)), np.full(5, 8, np.int32), S.INV_LEVEL_SIGMA2))
    bad("s is outside [0, pi^2]", lambda: ps.series(10.0))


def test_defaults_are_the_reference_constants(ps):
    o = ps.options()
    assert (o.rounds, o.iterations, o.robust_rounds, o.keep_stages) == (4, 10, 3, 0)
    assert np.float32(o.chi2_threshold) == np.float32(5.991) and np.float32(o.huber_delta) == np.float32(math.sqrt(5.991))
    assert C.sizeof(ps.IbaPoseResult) == 320 and C.sizeof(ps.IbaPoseOptions) == 28


def test_selftest_program_builds_and_passes():
    csrc = os.path.join(os.path.dirname(os.path.abspath(importlib.import_module(PKG).__file__)), "csrc")
    subprocess.check_call(["make", "-C", csrc, "-s", "san/pose_selftest_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "san", "pose_selftest_asan")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "0 failure(s)" in r.stdout, r.stdout + r.stderr

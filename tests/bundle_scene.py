"""Seeded scenes for the bundle adjustment's tests: cameras on an arc looking at a point cloud, float32 observations with pixel noise scaled by the
pyramid level, planted gross outliers, a chosen visibility pattern, and an "exact" variant in the manner of pose_scene.exact_scene."""
import functools

import numpy as np

import bundle_ref as R
from pose_scene import INV_LEVEL_SIGMA2, compose, pose

K = (718.856, 718.856, 607.1928, 185.2157)


def arc_cameras(n, g, radius=12.0, span=0.6):
    """n poses Tcw [n, 3, 4] on an arc of `span` radians around the origin, all looking at it from `radius` away"""
    T = np.zeros((n, 3, 4))
    for k, a in enumerate(np.linspace(-span / 2, span / 2, n) if n > 1 else [0.0][:n]):
        Rwc = pose([0.0, a, 0.0], [0, 0, 0])[:, :3]            # camera axes in the world
        centre = Rwc @ np.array([0.0, 0.0, -radius]) + g.normal(0, 0.05, 3)
        T[k, :, :3] = Rwc.T
        T[k, :, 3] = -Rwc.T @ centre
    return T


def project(T, X, Kk=K):
    p = X @ T[:, :3].T + T[:, 3]
    return np.stack([Kk[0] * p[:, 0] / p[:, 2] + Kk[2], Kk[1] * p[:, 1] / p[:, 2] + Kk[3]], 1)


def make(n_cameras, n_points, seed, n_fixed=1, noise=1.0, outliers=0.0, visibility=None, camera_motion=(0.01, 0.05), point_noise=0.05, shuffle=True):
    """-> dict: T_true, T_start [nc, 3, 4] f64, fixed [nc] u8 (the first n_fixed cameras), X_true [np, 3] f64, xyz [np, 3] f32 (the start), edge_point,
    edge_camera [ne] i32, obs [ne, 2] f32, inv_sigma2 [ne] f32, is_outlier [ne] bool, K. visibility: None (every camera sees every point), a float (the
    share of the pairs kept) or a bool array [np, nc]. The fixed cameras start at the truth; the edges are shuffled unless told otherwise."""
    g = np.random.default_rng(seed)
    T_true = arc_cameras(n_cameras, g)
    X_true = g.uniform(-3.0, 3.0, (n_points, 3)) * np.array([1.0, 0.4, 1.0])
    if visibility is None:
        vis = np.ones((n_points, n_cameras), bool)
    elif np.isscalar(visibility):
        vis = g.uniform(0, 1, (n_points, n_cameras)) < visibility
    else:
        vis = np.asarray(visibility, bool)
    ep, ec = np.nonzero(vis)
    if shuffle and len(ep):
        order = g.permutation(len(ep))
        ep, ec = ep[order], ec[order]
    ne = len(ep)
    octave = g.integers(0, 8, ne)
    obs = np.zeros((ne, 2))
    for c in range(n_cameras):
        m = ec == c
        obs[m] = project(T_true[c], X_true[ep[m]])
    obs += g.normal(0, 1.0, (ne, 2)) * (noise * 1.2 ** octave)[:, None]
    is_out = np.zeros(ne, bool)
    k = int(round(outliers * ne))
    if k:
        is_out[g.choice(ne, k, replace=False)] = True
        ang, r = g.uniform(0, 2 * np.pi, ne), g.uniform(30, 120, ne)
        obs[is_out] += (np.stack([np.cos(ang), np.sin(ang)], 1) * r[:, None])[is_out]
    fixed = np.zeros(n_cameras, np.uint8)
    fixed[:n_fixed] = 1
    T_start = T_true.copy()
    for c in range(n_fixed, n_cameras):
        T_start[c] = compose(pose(g.normal(0, 1, 3) * camera_motion[0] / np.sqrt(3), g.normal(0, 1, 3) * camera_motion[1] / np.sqrt(3)), T_true[c])
    xyz = (X_true + g.normal(0, point_noise, X_true.shape)).astype(np.float32)
    return dict(T_true=T_true, T_start=T_start, fixed=fixed, X_true=X_true, xyz=xyz, edge_point=ep.astype(np.int32), edge_camera=ec.astype(np.int32),
                obs=obs.astype(np.float32), inv_sigma2=INV_LEVEL_SIGMA2[octave], is_outlier=is_out, K=K)


def exact_scene(n_cameras, n_points, seed):
    """a scene every number of which float32 holds exactly, observations included: intrinsics 512 512 320 240, the true poses pure translations by
    multiples of 1/4, the points at depths that are powers of two behind every camera: the truth has residual 0, so the optimum is the truth
    itself. Cameras 0 and 1 are fixed (the gauge and the scale are pinned); the others start off the truth, the points at it."""
    g = np.random.default_rng(seed)
    Kk = (512.0, 512.0, 320.0, 240.0)
    T_true = np.zeros((n_cameras, 3, 4))
    T_true[:, :, :3] = np.eye(3)
    T_true[:, 0, 3] = np.arange(n_cameras) * 0.25
    z = 2.0 ** g.integers(2, 5, n_points)
    X = np.stack([g.integers(-16, 17, n_points) / 16.0 * z / 4.0, g.integers(-12, 13, n_points) / 16.0 * z / 4.0, z], 1)
    ep, ec = np.nonzero(np.ones((n_points, n_cameras), bool))
    p = X[ep] + T_true[ec, :, 3]
    obs = np.stack([512.0 * p[:, 0] / p[:, 2] + 320.0, 512.0 * p[:, 1] / p[:, 2] + 240.0], 1)
    assert np.array_equal(X.astype(np.float32), X) and np.array_equal(obs.astype(np.float32), obs)
    fixed = np.zeros(n_cameras, np.uint8)
    fixed[:2] = 1
    T_start = T_true.copy()
    for c in range(2, n_cameras):
        T_start[c] = compose(pose(g.normal(0, 1, 3) * 0.005, g.normal(0, 1, 3) * 0.02), T_true[c])
    octave = g.integers(0, 8, len(ep))
    return dict(T_true=T_true, T_start=T_start, fixed=fixed, X_true=X, xyz=X.astype(np.float32), edge_point=ep.astype(np.int32), edge_camera=ec.astype(np.int32),
                obs=obs.astype(np.float32), inv_sigma2=INV_LEVEL_SIGMA2[octave], is_outlier=np.zeros(len(ep), bool), K=Kk)


def overshoot_scene(seed, z_true=0.5, p=3):
    """the exact scene (every camera plane is z = 0) with the observations of point p replaced by those of a position at depth z_true, far nearer than
    its start (4 or 8 m): u = f x / z is so far from linear there that the first steps carry the point THROUGH the camera planes, p_z < 0 at those
    trials; their chi2 is finite and larger, so they are rejected (z_true > 0), or the point ends behind the cameras and the depth rule flags its
    edges (z_true < 0)"""
    sc = exact_scene(4, 20, seed)
    m = sc["edge_point"] == p
    pc = np.array([0.125, -0.0625, z_true])[None, :] + sc["T_true"][sc["edge_camera"][m], :, 3]
    obs = sc["obs"].copy()
    obs[m] = np.stack([512.0 * pc[:, 0] / pc[:, 2] + 320.0, 512.0 * pc[:, 1] / pc[:, 2] + 240.0], 1).astype(np.float32)
    return dict(sc, obs=obs, near=m)


def depth_at(T, X):
    """p_z of rule B1 in its own arithmetic: T [3, 4] f64, X [3] f32"""
    x, y, z = (np.float64(v) for v in np.asarray(X, np.float32))
    return ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]


def first_trial(sc, robust=True, delta=R.LOCAL_DELTA):
    """the estimates of the very first trial of a job (round 0, iteration 0) from the reference's own pieces -> (Tn [nc, 3, 4], Xn)"""
    q = ref_job(sc)
    act = np.ones(q.ne, bool)
    lin = R.linearise(q, q.T, q.X, act, robust, np.float64(delta))
    st = R.step(q, lin, act, 1e-5 * R.largest_diagonal(lin))
    Tn, Xn, _ = R.trial_estimates(q, lin, st, q.T, q.X)
    return Tn.reshape(-1, 3, 4), Xn


def zero_depth_trial_scene(seed, cam=1):
    """a job whose FIRST TRIAL puts a point at p_z == 0 EXACTLY before a free camera, while its start is finite and its factorisation succeeds. One
    point and one edge are appended to a seeded scene, the edge with information 0: every term it adds to a sum is a zero, its point's block is lambda I
    and its step is zero, so no other byte of the first trial changes and the point stays where it is put (both asserted). It is put where the trial
    pose Tn of `cam` (taken from the reference) has ((Tn20 X + Tn21 Y) + Tn22 Z) + Tn23 == 0: Z takes -Tn23 / Tn22 to float32, Y what is left of it, X
    what is left of that; each remainder is exact, and the last one is far below half an ulp of Tn23. There (fx p_x) / 0 is infinite and 0 x inf is
    NaN: the trial's chi2 is NaN, rho is NaN, the trial is rejected and the loop leaves the iteration without a stop (P5)."""
    F = np.float32
    base = make(3, 30, seed, n_fixed=1)
    Tn, _ = first_trial(base)
    a, b, c, d = Tn[cam, 2]
    X = None
    for dz in (0, 1, -1, 2, -2):
        Z = F(-d / c)
        for _ in range(abs(dz)):
            Z = np.nextafter(Z, F(np.inf) if dz > 0 else F(-np.inf))
        r1 = -d - c * np.float64(Z)
        Y = F(r1 / b)
        r2 = r1 - b * np.float64(Y)
        for x in (F(r2 / a), np.nextafter(F(r2 / a), F(np.inf)), np.nextafter(F(r2 / a), F(-np.inf))):
            if depth_at(Tn[cam], (x, Y, Z)) == 0.0:
                X = np.array([x, Y, Z], F)
                break
        if X is not None:
            break
    assert X is not None
    sc = dict(base, xyz=np.vstack([base["xyz"], X[None]]).astype(F), edge_point=np.append(base["edge_point"], len(base["xyz"])).astype(np.int32),
              edge_camera=np.append(base["edge_camera"], cam).astype(np.int32), obs=np.vstack([base["obs"], [[0, 0]]]).astype(F),
              inv_sigma2=np.append(base["inv_sigma2"], F(0)), is_outlier=np.append(base["is_outlier"], False), X_true=np.vstack([base["X_true"], X[None]]))
    again, Xn = first_trial(sc)
    assert again.tobytes() == Tn.tobytes() and Xn[-1].tobytes() == X.astype(np.float64).tobytes()     # the edge changed nothing but its own p_z
    assert depth_at(sc["T_start"][cam], X) != 0.0 and depth_at(again[cam], X) == 0.0
    return sc


def check_trial_scenes(refs):
    """what the reference itself must say of (overshoot_scene, zero_depth_trial_scene, the latter without its last edge) under the local schedule"""
    (through, ex_t), (onto, ex_o), (plain, ex_p) = refs
    assert ex_t["behind_trials"] >= 2 and ex_t["nonfinite_trials"] == 0 and dict(through)["trials"][0] > dict(through)["lm_iterations"][0]   # behind, finite, rejected
    assert ex_o["zero_depth_trials"] == 1 and ex_o["nonfinite_trials"] == 1 and ex_p["zero_depth_trials"] == 0 and ex_p["nonfinite_trials"] == 0
    assert dict(onto)["trials"][0] == dict(onto)["lm_iterations"][0] > 1                              # rejected, and the round went on without a stop
    assert dict(onto)["stage0_Tcw"].tobytes() != dict(plain)["stage0_Tcw"].tobytes()                    # the rejection changed the path


# ---- shared by the CPU and the GPU tests ----
def lib_job(bd, sc, T=None, xyz=None):
    return bd.job(sc["T_start"] if T is None else T, sc["fixed"], sc["xyz"] if xyz is None else xyz, sc["edge_point"], sc["edge_camera"], sc["obs"], sc["inv_sigma2"], sc["K"])


def ref_job(sc, T=None, xyz=None):
    return R.Job(sc["T_start"] if T is None else T, sc["fixed"], sc["xyz"] if xyz is None else xyz, sc["edge_point"], sc["edge_camera"], sc["obs"], sc["inv_sigma2"], sc["K"])


def ref_of(sc, stages=True, **opt):
    """the reference's outputs of a scene in the order of Bundle.everything()"""
    out, extras = R.optimize(ref_job(sc), **opt)
    return (R.with_stages(out, extras) if stages else out), extras


def lib_options(bd, opt, keep_stages=1):
    """an IbaBundleOptions from a dict in bundle_ref's form"""
    o = bd.options(rounds=opt["rounds"], iterations=opt["iterations"], robust_rounds=opt["robust_rounds"], keep_stages=keep_stages)
    o.chi2_threshold, o.huber_delta = float(opt["chi2_threshold"]), float(opt["huber_delta"])
    return o


def with_counts(vis_counts, n_cameras):
    """a visibility [np, nc] whose point p is seen by the first vis_counts[p] cameras"""
    vis = np.zeros((len(vis_counts), n_cameras), bool)
    for p, k in enumerate(vis_counts):
        vis[p, :k] = True
    return vis


def scenes():
    """small scenes that reach every rule: lanes and trees of the camera rule, point lists of 1, 2, 3 and 65, no free camera, no fixed camera, a
    sparse pattern, outliers, no edge at all"""
    return [make(2, 30, 1), make(5, 80, 2, n_fixed=2, outliers=0.05, visibility=0.7), make(3, 10, 3, n_fixed=0), make(3, 40, 4, n_fixed=3),
            make(66, 6, 5, n_fixed=60, visibility=with_counts([1, 2, 3, 65, 66, 64], 66)), make(2, 129, 6, outliers=0.1), make(4, 0, 7), make(0, 5, 8, n_fixed=0),
            make(12, 20, 9, n_fixed=1, visibility=0.5), exact_scene(4, 40, 10)]


# ---- eight tiny scenes for the calls of more jobs than workgroups: cheap references, and jobs that finish at different steps ----
TINY_TRIALS = ([5, 10], [5, 10], [7, 13], [5, 10], [5, 1], [5, 10], [1, 1], [5, 12])      # of the two rounds under R.LOCAL, from the reference


@functools.lru_cache(maxsize=None)
def tiny_scenes():
    return (make(2, 6, 900), make(3, 9, 901, n_fixed=1), make(2, 8, 902, outliers=0.3), make(4, 5, 903, n_fixed=2, visibility=0.7), make(2, 1, 904),
            make(3, 12, 905, n_fixed=0), make(2, 0, 906), make(5, 10, 907, n_fixed=1, visibility=0.6))


@functools.lru_cache(maxsize=None)
def tiny_reference():
    """the reference's outputs of tiny_scenes() under R.LOCAL -> (with the stages, without them): computed once, shared, never written to"""
    both = [R.optimize(ref_job(sc)) for sc in tiny_scenes()]
    return tuple(R.with_stages(out, extras) for out, extras in both), tuple(out for out, _ in both)


def check_tiny_reference():
    """the trial counts the reference itself must give: the eight jobs ask for different numbers of steps; scene 2 has rejected trials (more trials
    than iterations). Which two of them one workgroup takes is the order's business: check_second_trip"""
    plain = [dict(out) for out in tiny_reference()[1]]
    assert [d["trials"][:2].tolist() for d in plain] == [list(t) for t in TINY_TRIALS], [d["trials"][:2].tolist() for d in plain]
    assert plain[2]["lm_iterations"][:2].tolist() == [5, 8]
    assert len({sum(t) for t in TINY_TRIALS}) >= 5


def cycle_of_tiny(n):
    """the indices into tiny_scenes() of a call of n jobs: scene k % 8, and scene 0 again as the last. Where a grid of g workgroups (g a multiple of
    8) walks the jobs with a stride of g, a workgroup's second job is then the SAME scene as its first: both finish at one step"""
    return [k % 8 for k in range(n - 1)] + [0]


def shifted_cycle_of_tiny(n, grid, shift=3):
    """cycle_of_tiny with the scenes of the jobs from `grid` on moved on by `shift`: workgroup w of a grid of `grid` then takes scene w % 8 and, on its
    second trip, scene (w + shift) % 8, which asks for another number of steps; all eight scenes still make the second trip, and the last job is
    still scene 0"""
    return [(k % 8 if k < grid else (k + shift) % 8) for k in range(n - 1)] + [0]


def check_second_trip(order, grid, differ):
    """on the references: the jobs grid..grid + 7 are the eight scenes; differ: among the workgroups that take two jobs there is one whose first job
    needs fewer trials than its second (it is done while the second still runs) and one whose first needs more; else: each takes one scene twice"""
    total = [sum(t) for t in TINY_TRIALS]
    first, second = [total[order[w]] for w in range(len(order) - grid)], [total[k] for k in order[grid:]]
    assert sorted(order[grid:grid + 8]) == list(range(8)) and order[0] == order[-1] == 0
    if differ:
        assert any(a < b for a, b in zip(first, second)) and any(a > b for a, b in zip(first, second)), (first, second)
    else:
        assert order[grid:] == order[:len(order) - grid]


def without_stages(entries):
    """the entries of an everything() list that a call without keep_stages has too"""
    return [(k, v) for k, v in entries if not k.startswith("stage")]


# ---- the linear algebra against a long-double dense solve of the FULL damped system ----
def gate_share(dev, own, truth):
    """the gate of tests/test_gpu_pose.py and test_gpu_smooth.py: |device - truth| <= 4 |float64 restatement - truth| + one ulp of the output's scale
    (the largest magnitude of the truth over the array) -> the largest share of the gate used"""
    truth = np.asarray(truth, np.longdouble)
    d_dev, d_own = np.abs(np.asarray(dev, np.longdouble) - truth), np.abs(np.asarray(own, np.longdouble) - truth)
    ulp = (np.max(np.abs(truth)) if truth.size else np.longdouble(0)) * np.longdouble(2.0 ** -52)
    gate = 4 * d_own + ulp
    assert np.all(d_dev <= gate), (d_dev, gate)
    return float(np.max(np.where(gate > 0, d_dev / np.where(gate > 0, gate, 1), 0))) if truth.size else 0.0


def eval_differences(bd, got, own):
    """the names of the outputs of one job's iba_bundle_eval whose bytes differ from bundle_ref's"""
    return [k for k in bd.EVAL_FIELDS + ("chi2_robust", "n_reduced", "solved") if np.ascontiguousarray(got[k]).tobytes() != np.ascontiguousarray(own[k]).tobytes()]


def check_eval(bd, scs, masks, robust, lam, host, note):
    """iba_bundle_eval (host: iba_debug_bundle_eval_host) of the scenes against bundle_ref byte for byte, then under the gate against long double"""
    got = bd.evaluate([lib_job(bd, sc) for sc in scs], active=masks, robust=robust, lam=lam, host=host)
    for j, sc in enumerate(scs):
        q = ref_job(sc)
        m = None if masks is None else masks[j]
        own = R.evaluate(q, m, robust, lam)
        assert eval_differences(bd, got[j], own) == [], j
        if not all(np.isfinite(own[k]).all() for k in bd.EVAL_FIELDS) or not own["solved"]:
            continue                                      # this gate only; the bytes above were compared
        truth = R.full_system_longdouble(q, m, robust, lam)
        free = ~q.fixed
        for k, t in (("Hpp", truth["Hpp"][free]), ("bp", truth["bp"][free]), ("Hll", truth["Hll"]), ("bl", truth["bl"])):
            sel = free if k in ("Hpp", "bp") else slice(None)
            note.append(gate_share(got[j][k][sel], own[k][sel], t))
        note.append(gate_share([got[j]["chi2_robust"]], [own["chi2_robust"]], [truth["chi"]]))
        if truth["dp"] is not None:
            note.append(gate_share(got[j]["dp"], own["dp"], truth["dp"]))
            note.append(gate_share(got[j]["dl"], own["dl"], truth["dl"]))


def eval_cases():
    scs = scenes()
    g = np.random.default_rng(11)
    masks = [None if j % 2 else (g.uniform(0, 1, len(sc["edge_point"])) < 0.8).astype(np.uint8) for j, sc in enumerate(scs)]
    return scs, masks


def check_errors(bd, err, host, device=0):
    """every refusal of the argument checks, by its message: IBA_ERR_INVALID_ARG before any device is touched (host: through iba_debug_bundle_host)"""
    import ctypes as C
    import pytest
    sc = make(3, 12, 1)
    run = (lambda jobs, opt=None, **kw: bd.optimize_host(jobs, opt, **kw)) if host else (lambda jobs, opt=None, **kw: bd.optimize(jobs, opt, device=device, **kw))

    def changed(**kw):
        d = dict(sc)
        d.update(kw)
        return lib_job(bd, d)

    def refused(msg, fn):
        with pytest.raises(err, match=msg) as e:
            fn()
        assert e.value.status == 1                    # IBA_ERR_INVALID_ARG

    nan, inf = np.float32("nan"), np.float32("inf")
    T_bad, xyz_bad, obs_bad, w_nan, w_neg = sc["T_start"].copy(), sc["xyz"].copy(), sc["obs"].copy(), sc["inv_sigma2"].copy(), sc["inv_sigma2"].copy()
    T_bad[1, 2, 3], xyz_bad[4, 1], obs_bad[5, 0], w_nan[2], w_neg[3] = np.nan, inf, nan, nan, -1.0
    ep_bad, ec_bad, ep_dup = sc["edge_point"].copy(), sc["edge_camera"].copy(), sc["edge_point"].copy()
    ep_bad[0], ec_bad[1] = 12, -1
    first = int(np.flatnonzero((sc["edge_point"] == sc["edge_point"][0]) & (sc["edge_camera"] != sc["edge_camera"][0]))[0])
    ec_dup = sc["edge_camera"].copy()
    ec_dup[first] = sc["edge_camera"][0]
    refused("B = 0", lambda: run([]))
    refused("pose is not finite", lambda: run([changed(T_start=T_bad)]))
    refused("point 4 is not finite", lambda: run([changed(xyz=xyz_bad)]))
    refused("observation is not finite", lambda: run([changed(obs=obs_bad)]))
    refused("inv_sigma2 is not finite", lambda: run([changed(inv_sigma2=w_nan)]))
    refused("inv_sigma2 < 0", lambda: run([changed(inv_sigma2=w_neg)]))
    refused("fx or fy", lambda: run([changed(K=(0.0, 700.0, 1.0, 1.0))]))
    refused("cx or cy", lambda: run([changed(K=(700.0, 700.0, float("inf"), 1.0))]))
    refused("names point 12", lambda: run([changed(edge_point=ep_bad)]))
    refused("names camera -1", lambda: run([changed(edge_camera=ec_bad)]))
    refused("joined by two edges", lambda: run([lib_job(bd, sc), changed(edge_camera=ec_dup)]))
    many = make(66, 2, 2, n_fixed=1)
    refused("65 free cameras", lambda: run([lib_job(bd, many)]))
    q = lib_job(bd, sc)
    q.xyz = None
    refused("xyz is NULL", lambda: run([q]))
    for field, value, msg in (("rounds", 0, "rounds 0"), ("rounds", 5, "rounds 5"), ("robust_rounds", -1, "robust_rounds"), ("robust_rounds", 5, "robust_rounds"),
                              ("chi2_threshold", -1.0, "chi2_threshold"), ("huber_delta", 0.0, "huber_delta"), ("huber_delta", float("nan"), "huber_delta"),
                              ("struct_size", 8, "struct_size")):
        refused(msg, lambda: run([lib_job(bd, sc)], bd.options(**{field: value})))
    refused("iterations\\[1\\] = 0", lambda: run([lib_job(bd, sc)], bd.options(iterations=(5, 0))))
    refused("iterations\\[0\\] = 101", lambda: run([lib_job(bd, sc)], bd.options(iterations=(101, 10))))
    refused("n_iterations 0", lambda: bd.options_global(0, True))
    L = bd._lib()
    o, p = bd.options(), C.c_void_p(None)
    ja = bd._job_array([lib_job(bd, sc)])
    call = (lambda *a: L.iba_debug_bundle_host(*a)) if host else (lambda j, b, oo, out: L.iba_bundle_optimize(j, b, oo, C.c_int(device), out))
    assert call(None, C.c_int32(1), C.addressof(o), C.addressof(p)) == 1 and b"jobs is NULL" in L.iba_bundle_last_error()
    assert call(C.addressof(ja), C.c_int32(1), None, C.addressof(p)) == 1 and b"options is NULL" in L.iba_bundle_last_error()
    assert call(C.addressof(ja), C.c_int32(1), C.addressof(o), None) == 1 and b"out is NULL" in L.iba_bundle_last_error()
    assert L.iba_default_bundle_options(None) == 1 and L.iba_bundle_options_global(None, 5, 1) == 1
    refused("lambda", lambda: bd.evaluate([lib_job(bd, sc)], lam=-1.0, host=host, device=device))
    refused("names point 12", lambda: bd.evaluate([changed(edge_point=ep_bad)], host=host, device=device))
    res = run([lib_job(bd, sc)])
    for fn in (lambda: res.read(1), lambda: res.read(-1), lambda: res.edges(1), lambda: res.cameras(1), lambda: res.points(1)):
        refused("job", fn)
    refused("keep_stages", lambda: res.stage(0, 0))
    kept = run([lib_job(bd, sc)], keep_stages=1)
    refused("round 2 is outside", lambda: kept.stage(0, 2))
    refused("round -1 is outside", lambda: kept.stage(0, -1))
    assert L.iba_bundle_read(kept.p, C.c_int32(0), None) == 1 and L.iba_bundle_n_jobs(None) == 0

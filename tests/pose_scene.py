"""Seeded scenes for the pose optimisation's tests: a camera, points in front of it, pixel noise of about one pixel scaled by the pyramid level, a
share of gross outliers, and a start pose off the true one by a tracking-sized motion. Octaves 0-7 with informations 1.2^-2l."""
import numpy as np

import pose_ref as R

K = (718.856, 718.856, 607.1928, 185.2157)
WIDTH, HEIGHT = 1241.0, 376.0
INV_LEVEL_SIGMA2 = np.array([1.2 ** (-2 * l) for l in range(8)], np.float32)


def rot(w):
    """Rodrigues in float64"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    O = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + O
    return np.eye(3) + np.sin(th) / th * O + (1 - np.cos(th)) / th ** 2 * (O @ O)


def pose(w, t):
    T = np.zeros((3, 4))
    T[:, :3], T[:, 3] = rot(w), t
    return T


def compose(A, B):
    """A after B, both [3, 4]"""
    T = np.zeros((3, 4))
    T[:, :3] = A[:, :3] @ B[:, :3]
    T[:, 3] = A[:, :3] @ B[:, 3] + A[:, 3]
    return T


def make(n, seed, noise=1.0, outliers=0.0, motion=(0.02, 0.15)):
    """-> dict: T_true, T_start [3, 4] f64, xyz [n, 3] f32, obs [n, 2] f32, inv_sigma2 [n] f32, octave [n], is_outlier [n] bool, K.
    noise: pixels at level 0 (x 1.2^level); outliers: the share of observations moved by 30..120 pixels; motion: (radians, metres) of the start's offset"""
    g = np.random.default_rng(seed)
    T_true = pose(g.normal(0, 0.2, 3), g.normal(0, 1.0, 3))
    # points in the camera frame, inside the image, 4..40 m deep, then carried into the world
    z = g.uniform(4.0, 40.0, n)
    u, v = g.uniform(20, WIDTH - 20, n), g.uniform(20, HEIGHT - 20, n)
    pc = np.stack([(u - K[2]) / K[0] * z, (v - K[3]) / K[1] * z, z], 1)
    xyz = ((pc - T_true[:, 3]) @ T_true[:, :3]).astype(np.float32)
    octave = g.integers(0, 8, n)
    pw = xyz.astype(np.float64) @ T_true[:, :3].T + T_true[:, 3]
    obs = np.stack([K[0] * pw[:, 0] / pw[:, 2] + K[2], K[1] * pw[:, 1] / pw[:, 2] + K[3]], 1)
    obs += g.normal(0, 1.0, (n, 2)) * (noise * 1.2 ** octave)[:, None]
    is_out = np.zeros(n, bool)
    k = int(round(outliers * n))
    if k:
        is_out[g.choice(n, k, replace=False)] = True
        ang, r = g.uniform(0, 2 * np.pi, n), g.uniform(30, 120, n)
        obs[is_out] += (np.stack([np.cos(ang), np.sin(ang)], 1) * r[:, None])[is_out]
    d = pose(g.normal(0, 1, 3) * motion[0] / np.sqrt(3), g.normal(0, 1, 3) * motion[1] / np.sqrt(3))
    return dict(T_true=T_true, T_start=compose(d, T_true), xyz=xyz, obs=obs.astype(np.float32), inv_sigma2=INV_LEVEL_SIGMA2[octave], octave=octave, is_outlier=is_out, K=K)


def exact_scene(n, seed):
    """a scene every number of which float32 holds exactly, observations included: intrinsics 512 512 320 240, the true pose a pure translation by
    (1/2, -1/4, 1), depths behind it that are powers of two: the true pose has residual 0, so the optimum is the truth itself"""
    g = np.random.default_rng(seed)
    K = (512.0, 512.0, 320.0, 240.0)
    T_true = np.array([[1, 0, 0, 0.5], [0, 1, 0, -0.25], [0, 0, 1, 1.0]], np.float64)
    pz = 2.0 ** g.integers(2, 6, n)
    px, py = g.integers(-64, 65, n) / 16.0 * pz / 4.0, g.integers(-48, 49, n) / 16.0 * pz / 4.0
    xyz = np.stack([px - 0.5, py + 0.25, pz - 1.0], 1)
    obs = np.stack([512.0 * px / pz + 320.0, 512.0 * py / pz + 240.0], 1)
    assert np.array_equal(xyz.astype(np.float32), xyz) and np.array_equal(obs.astype(np.float32), obs)
    octave = g.integers(0, 8, n)
    d = pose(g.normal(0, 1, 3) * 0.02 / np.sqrt(3), g.normal(0, 1, 3) * 0.15 / np.sqrt(3))
    return dict(T_true=T_true, T_start=compose(d, T_true), xyz=xyz.astype(np.float32), obs=obs.astype(np.float32), inv_sigma2=INV_LEVEL_SIGMA2[octave], K=K)


# ---- shared by the CPU and the GPU tests ----
def lib_job(ps, sc, T=None):
    return ps.job(sc["T_start"] if T is None else T, sc["xyz"], sc["obs"], sc["inv_sigma2"], sc["K"])


def ref_of(sc, **opt):
    return R.optimize(sc["T_start"], sc["K"], sc["xyz"], sc["obs"], sc["inv_sigma2"], **opt)


def differences(res, j, e, stages=True):
    """the outputs of job j of a Pose result whose bytes differ from the reference dict e"""
    r, bad = res.read(j), []
    for k in ("n", "n_inliers", "rounds_run"):
        if r[k] != e[k]:
            bad.append(k)
    for k in ("Tcw12", "Tcw12f", "chi2", "n_bad", "lm_iterations", "trials"):
        if np.asarray(r[k]).tobytes() != np.asarray(e[k]).tobytes():
            bad.append(k)
    out, chi2 = res.edges(j)
    if out.tobytes() != e["outlier"].tobytes():
        bad.append("outlier")
    if chi2.tobytes() != e["chi2_edges"].tobytes():
        bad.append("chi2_edges")
    if stages:
        for rnd in range(e["rounds_run"]):
            if res.stage(j, rnd).tobytes() != e["stages"][rnd].tobytes():
                bad.append("stage %d" % rnd)
    return bad


def first_trial_pose(sc):
    """the pose of the very first trial of a job (round 0, iteration 0) from the reference's own pieces, or None where the factorisation fails"""
    s, _ = R.sums(sc["T_start"], sc["K"], sc["xyz"], sc["obs"], sc["inv_sigma2"], None, True, R.DEFAULT_DELTA)
    s = [float(v) for v in s]
    lam = 1e-5 * max(abs(s[R.hidx(k, k)]) for k in range(6))
    A = [[s[R.hidx(min(r, c), max(r, c))] + (lam if r == c else 0.0) for c in range(6)] for r in range(6)]
    dx = R.ldlt6(A, s[21:27])
    return None if dx is None else (R.exp_update(dx, sc["T_start"])[0], dx)


def nonfinite_trial_scene(groups=16, seed=0):
    """a job whose FIRST TRIAL has a chi2 sum that is not finite, while its start is finite and its factorisation succeeds. The camera looks down the
    world's z axis (rotation I, cx = cy = 0) and is 1/8 off in z alone. The points come in groups of four, (+-x, +-y, z) with one information, stored
    side by side: every sum that is odd in x or y cancels exactly inside its group of the tree of P3, so H's last row and column and b's first five
    entries are exact zeros and the first step is a pure translation along z: T' differs from T in Tz alone (asserted). The last edge has information
    0 (it adds +-0 to every sum), sits at (2^100, 0, 0), and row 2 of the start pose carries T20 = -Tz' 2^-100: too small to reach any other point's
    p_z (it is absorbed by their rounding), it puts the last edge's p_z at -Tz' 2^-100 2^100 + Tz' = 0 EXACTLY at the trial pose and nowhere else.
    There (fx p_x) / 0 is infinite and 0 x inf is NaN: the trial's chi2 sum is NaN, rho is NaN, the trial is rejected and the loop leaves the iteration
    without a stop (P5)."""
    g = np.random.default_rng(seed)
    K = (512.0, 512.0, 0.0, 0.0)
    z = 2.0 ** g.integers(2, 5, groups)
    x, y = g.integers(1, 33, groups) / 16.0 * z / 4.0, g.integers(1, 25, groups) / 16.0 * z / 4.0
    lvl = g.integers(0, 8, groups)
    sx, sy = np.array([1, 1, -1, -1.0]), np.array([1, -1, 1, -1.0])
    xyz = np.stack([np.outer(x, sx).ravel(), np.outer(y, sy).ravel(), np.repeat(z, 4)], 1)
    obs = np.stack([512.0 * xyz[:, 0] / xyz[:, 2], 512.0 * xyz[:, 1] / xyz[:, 2]], 1)
    assert np.array_equal(xyz.astype(np.float32), xyz) and np.array_equal(obs.astype(np.float32), obs)
    T = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.125]], np.float64)
    sc = dict(T_true=np.eye(3, 4), T_start=T, xyz=np.vstack([xyz, [[2.0 ** 100, 0, 0]]]).astype(np.float32), obs=np.vstack([obs, [[0, 0]]]).astype(np.float32),
              inv_sigma2=np.append(INV_LEVEL_SIGMA2[np.repeat(lvl, 4)], np.float32(0)), K=K)
    Tn, dx = first_trial_pose(sc)
    assert all(v == 0.0 for v in dx[:5]) and dx[5] != 0.0                   # a pure translation along z, exactly
    assert np.array_equal(Tn[:, :3], T[:, :3]) and Tn[0, 3] == 0 and Tn[1, 3] == 0
    sc["T_start"] = T.copy()
    sc["T_start"][2, 0] = -Tn[2, 3] * 2.0 ** -100
    again, _ = first_trial_pose(sc)
    assert again[2, 3] == Tn[2, 3] and again[2, 0] == sc["T_start"][2, 0]   # T20 changed nothing but the last edge's p_z
    return sc

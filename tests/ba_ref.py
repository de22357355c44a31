"""TEST INFRASTRUCTURE: an independent extended-precision reference of the ORB-only extrinsic BA linearisation, and the
inputs the edge-case tests share (tests/test_ba_cpu.py pins them on the CPU, tests/test_gpu_ba_edges.py runs them on the device).

The rules are those of include/iba_mi355x.h ("ORB-only extrinsic bundle adjustment") and of calibEdge (Optimizer.cc:65-205):
X_c0 = s Xw; X_l0 = T_cl^-1 X_c0; X_li = T_lw X_l0; X_ci = T_cl X_li; e = obs - project(X_ci); information invSigma2 * I;
Huber(sqrt(5.991)) the way g2o's BaseUnaryEdge::constructQuadraticForm applies it (rho' scales the information). Every
rotation is the angle-axis block of the edge: Rodrigues for theta > 0, p + w x p at theta == 0. Values and the 7 derivatives
travel together as a trailing axis of 8 in np.longdouble, vectorised over the edges. Two things differ from a double
evaluation on purpose: 1 - cos(theta) is taken as 2 sin^2(theta / 2) (the same number without the cancellation), and
theta == 0 is decided on the long-double norm, so an omega whose squares underflow in double takes the full branch here."""
import functools

import numpy as np
from scipy.spatial.transform import Rotation

LD = np.longdouble
if not np.finfo(LD).eps < 2e-19:
    raise ImportError("tests/ba_ref.py needs an extended-precision np.longdouble (eps < 2e-19, e.g. x87 80-bit); this platform's has eps = %g, "
                      "which is no reference for a double kernel" % float(np.finfo(LD).eps))

DELTA64 = np.sqrt(np.float64(5.991))          # deltaMono, held as a double by the robust kernel
DSQR64 = np.float64(DELTA64 * DELTA64)        # RobustKernelHuber::robustify: dsqr = delta * delta, in double
DELTA, DSQR = LD(DELTA64), LD(DSQR64)


# ---------------------------------------------------------------- duals: (..., 8) = value, d/dx[0..6] ----------------------------------------------------------------
def _const(a):
    a = np.asarray(a, LD)
    out = np.zeros(a.shape + (8,), LD)
    out[..., 0] = a
    return out


def _mul(f, g):
    f, g = np.broadcast_arrays(f, g)
    out = np.empty(f.shape, LD)
    out[..., 0] = f[..., 0] * g[..., 0]
    out[..., 1:] = f[..., :1] * g[..., 1:] + f[..., 1:] * g[..., :1]
    return out


def _div(f, g):
    f, g = np.broadcast_arrays(f, g)
    out = np.empty(f.shape, LD)
    out[..., 0] = f[..., 0] / g[..., 0]
    out[..., 1:] = (f[..., 1:] - out[..., :1] * g[..., 1:]) / g[..., :1]
    return out


def _fn(f, val, dval):
    out = np.empty(f.shape, LD)
    out[..., 0] = val
    out[..., 1:] = dval[..., None] * f[..., 1:]
    return out


def _cross(a, b):
    ax, ay, az = a[..., 0, :], a[..., 1, :], a[..., 2, :]
    bx, by, bz = b[..., 0, :], b[..., 1, :], b[..., 2, :]
    return np.stack([_mul(ay, bz) - _mul(az, by), _mul(az, bx) - _mul(ax, bz), _mul(ax, by) - _mul(ay, bx)], axis=-2)


def _dot(a, b):
    return _mul(a, b).sum(axis=-2)


def _rotate(w, p):
    """angle-axis rotation of p (..., 3, 8) by w (..., 3, 8)"""
    w, p = np.broadcast_arrays(w, p)
    th2 = _dot(w, w)
    full = th2[..., 0] > 0
    first = p + _cross(w, p)
    safe = np.where(full[..., None], th2, _const(1.0))
    th = np.sqrt(safe[..., 0])
    theta = _fn(safe, th, 1 / (2 * th))
    v = _div(w, theta[..., None, :])
    cth = _fn(theta, np.cos(th), -np.sin(th))
    sth = _fn(theta, np.sin(th), np.cos(th))
    omc = _fn(theta, 2 * np.sin(th / 2) ** 2, np.sin(th))
    out = _mul(p, cth[..., None, :]) + _mul(_cross(v, p), sth[..., None, :]) + _mul(v, _mul(_dot(v, p), omc)[..., None, :])
    return np.where(full[..., None, None], out, first)


def edges(prob, x):
    """residual duals (N, 2, 8) and X_ci (N, 3) of every edge at x"""
    c = np.zeros((7, 8), LD)
    c[:, 0] = np.asarray(x, np.float64)
    c[np.arange(7), 1 + np.arange(7)] = 1
    wcl, t, s = c[:3], c[3:6], c[6]
    f = prob.edge_frame
    Xc0 = _mul(s, _const(prob.edge_Xw))
    tlc = _rotate(-wcl, -t)
    Xl0 = _rotate(-wcl, Xc0) + tlc
    T6 = prob.frame_Tlw6.astype(LD)[f]
    Xli = _rotate(_const(T6[:, :3]), Xl0) + _const(T6[:, 3:])
    Xci = _rotate(wcl, Xli) + t
    intr = prob.frame_intr.astype(LD)[f]
    pre = np.stack([_mul(_const(intr[:, 0]), _div(Xci[:, 0], Xci[:, 2])) + _const(intr[:, 2]),
                    _mul(_const(intr[:, 1]), _div(Xci[:, 1], Xci[:, 2])) + _const(intr[:, 3])], axis=1)
    return _const(prob.edge_obs) - pre, Xci[:, :, 0]


class Lin:
    """one linearisation: H (7, 7), b (7), chi (robust chi2 of the active edges), chi2_edges (N), z (X_ci.z, N), above (N:
    which edges took the Huber branch), and the per-edge terms Hi (N, 7, 7), bi (N, 7), rho (N)"""


def linearise(prob, x, active=None, robust=True, above=None):
    """`above` forces the side of the Huber knee per edge (default: the reference's own chi2 > dsqr)"""
    with np.errstate(all="ignore"):
        e, Xci = edges(prob, x)
        r, J = e[:, :, 0], e[:, :, 1:]
        info = prob.edge_info.astype(LD)
        L = Lin()
        L.chi2_edges = info * (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1])
        L.z = Xci[:, 2]
        sel = np.ones(len(info), bool) if active is None else np.asarray(active) != 0
        rho0, rho1 = L.chi2_edges.copy(), np.ones(len(info), LD)
        L.above = np.zeros(len(info), bool)
        if robust:
            L.above = (L.chi2_edges > DSQR) if above is None else np.asarray(above, bool)
            sq = np.sqrt(L.chi2_edges[L.above])
            rho0[L.above], rho1[L.above] = 2 * sq * DELTA - DSQR, DELTA / sq
        w = rho1 * info
        L.Hi = w[:, None, None] * np.einsum("nrp,nrq->npq", J, J)
        L.bi = -w[:, None] * np.einsum("nrp,nr->np", J, r)
        L.rho = rho0
        L.H, L.b, L.chi = L.Hi[sel].sum(0), L.bi[sel].sum(0), rho0[sel].sum()
    return L


# ---------------------------------------------------------------- the project's gates, measured ----------------------------------------------------------------
FIGURES = {}    # (family, who) -> [chi2_edges as a fraction of its bound, robust chi2 rel, H / max|H|, b / max|b|, comparisons]


def check(family, who, got, ref, H=None, b=None, chi=None):
    """got = (H, b, chi, chi2_edges) of the device or the oracle against a Lin (H / b / chi override the reference's sums, for
    one-hot terms): per-edge chi2 at rtol 1e-11 / atol 1e-12, robust chi2 at 1e-11 relative, every entry of H and b within 1e-10 of
    the largest entry. Records the measured maxima under FIGURES[(family, who)] before it asserts."""
    gH, gb, gchi, gc2 = got
    rH, rb, rchi = (ref.H if H is None else H), (ref.b if b is None else b), (ref.chi if chi is None else chi)
    fig = FIGURES.setdefault((family, who), [0.0, 0.0, 0.0, 0.0, 0])
    fin = np.isfinite(ref.chi2_edges.astype(np.float64))
    if gc2 is not None:
        assert np.array_equal(np.isfinite(gc2), fin), (family, who, "non-finite chi2_edges elsewhere than the reference's")
        d = np.abs(gc2[fin].astype(LD) - ref.chi2_edges[fin]) / (LD(1e-12) + LD(1e-11) * np.abs(ref.chi2_edges[fin]))
        fig[0] = max(fig[0], float(d.max()) if d.size else 0.0)
    dchi = float(abs(LD(gchi) - rchi) / rchi) if rchi != 0 else (0.0 if gchi == 0 else np.inf)
    mH, mb = np.abs(rH).max(), np.abs(rb).max()
    dH = float(np.abs(gH.astype(LD) - rH).max() / mH) if mH != 0 else (0.0 if not gH.any() else np.inf)
    db = float(np.abs(gb.astype(LD) - rb).max() / mb) if mb != 0 else (0.0 if not gb.any() else np.inf)
    fig[1], fig[2], fig[3], fig[4] = max(fig[1], dchi), max(fig[2], dH), max(fig[3], db), fig[4] + 1
    assert fig[0] <= 1.0, (family, who, "chi2_edges beyond rtol 1e-11 / atol 1e-12 by a factor", fig[0])
    assert dchi <= 1e-11, (family, who, "robust chi2 relative", dchi)
    assert dH <= 1e-10 and db <= 1e-10, (family, who, "H, b as a fraction of the largest entry", dH, db)


def report(family):
    for (fam, who), f in sorted(FIGURES.items()):
        if fam == family:
            print("ba_parity %-9s %-7s vs long double: chi2_edges %.2e of its bound, chi2 %.2e rel, H %.2e, b %.2e of the largest entry (%d linearisations)"
                  % (fam, who, f[0], f[1], f[2], f[3], f[4]))


# ---------------------------------------------------------------- scenes ----------------------------------------------------------------
def make_scene(rotvec_cl, poses6, ba, t_cl=(0.05, -0.08, -0.27), scale=9.5, pts_per_frame=50, x_range=(-8.0, 8.0), y_range=(-2.0, 2.0),
               z_range=(4.0, 40.0), seed=0, pix_noise=0.5, outlier_frac=0.05):
    """Planted (R_cl = exp(rotvec_cl), t_cl, scale); poses6 (F, 6) goes to the edges verbatim as frame_Tlw6 (rotation vector and
    translation of world-lidar -> lidar_f). Every frame sees pts_per_frame points drawn in its own camera frame inside the ranges."""
    rng = np.random.default_rng(seed)
    poses6 = np.asarray(poses6, np.float64).reshape(-1, 6)
    Rcl, tcl = Rotation.from_rotvec(np.asarray(rotvec_cl, np.float64)).as_matrix(), np.asarray(t_cl, np.float64)
    F, P = len(poses6), pts_per_frame
    intr = np.tile([718.856, 718.856, 607.1928, 185.2157], (F, 1))
    sig2 = 1.44 ** -np.arange(8.0)
    ef, eX, eo, ei, es = [], [], [], [], []
    for f in range(F):
        Rlw = Rotation.from_rotvec(poses6[f, :3]).as_matrix()
        pc = np.stack([rng.uniform(*x_range, P), rng.uniform(*y_range, P), rng.uniform(*z_range, P)], 1)
        Xli = (pc - tcl) @ Rcl                        # camera_f -> lidar_f
        Xl0 = (Xli - poses6[f, 3:]) @ Rlw             # -> world lidar
        Xc0 = Xl0 @ Rcl.T + tcl                       # -> camera 0, metric
        eX.append((Xc0 / scale).astype(np.float32).astype(np.float64))
        uv = np.stack([intr[f, 0] * pc[:, 0] / pc[:, 2] + intr[f, 2], intr[f, 1] * pc[:, 1] / pc[:, 2] + intr[f, 3]], 1) + rng.normal(0, pix_noise, (P, 2))
        out = rng.random(P) < outlier_frac
        uv[out] += rng.normal(0, 40, (int(out.sum()), 2))
        eo.append(uv.astype(np.float32).astype(np.float64))
        ei.append(sig2[rng.integers(0, 8, P)].astype(np.float32).astype(np.float64))
        ef.append(np.full(P, f))
        es.append(np.arange(P))
    prob = ba.BaProblem(poses6, intr, np.concatenate(ef), np.concatenate(eX), np.concatenate(eo), np.concatenate(ei), np.concatenate(es))
    return prob, np.concatenate([np.asarray(rotvec_cl, np.float64), tcl, [scale]])


def subset(prob, idx, ba, info=None):
    idx = np.asarray(idx, np.int64)
    return ba.BaProblem(prob.frame_Tlw6, prob.frame_intr, prob.edge_frame[idx], prob.edge_Xw[idx], prob.edge_obs[idx],
                        prob.edge_info[idx] if info is None else info, prob.edge_slot[idx])


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


# frame poses with every rotation-vector edge: exactly 0 (with and without a translation), 1e-160-sized components (squares
# subnormal), components whose squares underflow, norm 3.1, and ordinary small ones
POSES = np.array([[0, 0, 0, 0, 0, 0],
                  [0, 0, 0, -1.0, 0.05, 0.02],
                  [1e-160, -2e-160, 1e-160, -2.1, -0.04, 0.03],
                  [0, 3e-170, 0, -2.9, 0.02, -0.05],
                  np.concatenate([3.1 * _unit([0.2, 0.9, -0.3]), [-4.0, 0.3, 0.1]]),
                  [0.02, -0.03, 0.01, -5.2, 0.1, -0.1],
                  [-0.05, 0.04, 0.03, -6.1, -0.2, 0.15],
                  [0.3, 0.2, -0.4, -7.0, 0.4, 0.2],
                  [0.01, 0.05, -0.02, -8.3, 0.1, 0.0]], np.float64)
OMEGA_G = np.array([1.21, -1.19, 1.22])      # lidar x-forward -> camera z-forward, roughly
DX = np.array([0.004, -0.006, 0.005, 0.03, -0.02, 0.04, 0.12])   # where the lane / ragged / small problems are linearised, off x_gt
Z_FLOOR = 1.0                                # every scene draws z in [4, 40] m and x stays near the planted one
LANES = (0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 127, 128, 255)
PAIRS = ((0, 63), (15, 16), (63, 64), (0, 255))
RAGGED = (0, 1, 2, 63, 64, 65, 255, 256, 257, 513)


class Case:
    def __init__(self, family, name, prob, x, active=None, robust=True, both_sides=False):
        self.family, self.name, self.prob, self.x, self.active, self.robust, self.both_sides = family, name, prob, np.asarray(x, np.float64), active, robust, both_sides


@functools.lru_cache(maxsize=None)
def scene_g(ba):
    """513 edges over the 9 special poses, generic planted rotation"""
    return make_scene(OMEGA_G, POSES, ba, pts_per_frame=57, seed=11)


@functools.lru_cache(maxsize=None)
def scene_i(ba):
    """the same poses with R_cl = I planted"""
    return make_scene(np.zeros(3), POSES, ba, pts_per_frame=57, seed=12)


@functools.lru_cache(maxsize=None)
def scene_l(ba):
    """520 edges over the poses other than the identity, generic planted rotation: an edge on the identity pose has
    X_ci = s Xw whatever x is, so its Jacobian is rounding noise and a one-edge H of it has no largest entry to gate against"""
    return make_scene(OMEGA_G, POSES[1:], ba, pts_per_frame=65, seed=13)


def mask80(n, seed):
    return (np.random.default_rng(seed).random(n) < 0.8).astype(np.uint8)


def lane_cases(ba):
    prob, x_gt = scene_l(ba)
    x = x_gt + DX
    p256, p257 = subset(prob, np.arange(256), ba), subset(prob, np.arange(257), ba)
    out = [Case("lane", "N=256", p256, x, None, rb, True) for rb in (True, False)] + [Case("lane", "N=257", p257, x, None, True, True)]
    for e in LANES + (256,):
        out += [Case("lane", "edge %d alone" % e, subset(p257, [e], ba), x, None, rb) for rb in (True, False)]
    return out


def ragged_cases(ba):
    prob, x_gt = scene_l(ba)
    out = []
    for n in RAGGED:
        p = subset(prob, np.arange(n), ba)
        out += [Case("ragged", "N=%d" % n, p, x_gt + DX, None, True, n >= 63), Case("ragged", "N=%d masked" % n, p, x_gt + DX, mask80(n, n), True, n >= 63),
                Case("ragged", "N=%d masked, no kernel" % n, p, x_gt + DX, mask80(n, n), False)]
    return out


def rotation_cases(ba):
    pi_, xi = scene_i(ba)
    pg, xg = scene_g(ba)
    off = np.array([0.02, -0.03, 0.05, 0.1])         # t and s off the planted ones: residuals and b are not at their minimum
    th = np.linalg.norm(OMEGA_G)
    omegas = [("omega = 0", pi_, np.zeros(3)), ("omega = (1e-170, 0, 0)", pi_, np.array([1e-170, 0, 0])),
              ("omega = (1e-160, -1e-160, 0)", pi_, np.array([1e-160, -1e-160, 0])), ("|omega| = 1e-9", pi_, 1e-9 * _unit([0.3, -0.5, 0.8])),
              ("planted + 2 pi", pg, OMEGA_G * ((th + 2 * np.pi) / th)), ("planted + 16 pi", pg, OMEGA_G * ((th + 16 * np.pi) / th))]
    out = []
    for name, p, w in omegas:
        x = np.concatenate([w, (xi if p is pi_ else xg)[3:] + off])
        out += [Case("rotation", name, p, x, None, True, True), Case("rotation", name + ", masked, no kernel", p, x, mask80(len(p.edge_frame), 5), False)]
    return out


def stride_base(ba):
    """the 25 x 200 scene the second-trip problem tiles (tests/ba_scene.py, untouched)"""
    import ba_scene
    prob, x_gt = ba_scene.make(n_frames=25, pts_per_frame=200, seed=5, ba=ba)
    return prob, x_gt + DX


STRIDE_N = 2048 * 256 + 77


def stride_problem(ba):
    """N = 2048 * 256 + 77 edges: the base scene's arrays tiled, the observations of every copy jittered afresh"""
    base, x = stride_base(ba)
    n0 = len(base.edge_frame)
    idx = np.arange(STRIDE_N) % n0
    obs = base.edge_obs[idx] + np.random.default_rng(77).normal(0, 0.3, (STRIDE_N, 2))
    return ba.BaProblem(base.frame_Tlw6, base.frame_intr, base.edge_frame[idx], base.edge_Xw[idx], obs, base.edge_info[idx], base.edge_slot[idx]), x


# ---- Huber knee ----
KNEE_STEPS = (0, 1, -1, 2, -2, 8, -8)        # ulps of dsqr = fl(fl(sqrt(5.991))^2) the chi2 of an edge is put at


def knee_base(ba):
    """64 edges of the lane scene with unit information: chi2_edges of one evaluation is e0^2 + e1^2 as the evaluator rounds it"""
    prob, x_gt = scene_l(ba)
    idx = np.arange(64) * 8
    return subset(prob, idx, ba, info=np.ones(64)), x_gt + DX


def knee_target(step):
    t = DSQR64
    for _ in range(abs(step)):
        t = np.nextafter(t, np.inf if step > 0 else -np.inf)
    return t


def knee_info(r2):
    """information per edge such that fl(info * r2) is dsqr + step ulps exactly; quotient taken in long double, then the
    doubles next to it tried. -> info (N,), step (N,) (cycling through KNEE_STEPS; an edge whose r2 cannot reach its step
    exactly takes the next one)"""
    info, steps = np.zeros(len(r2)), np.zeros(len(r2), np.int64)
    for i, r in enumerate(np.asarray(r2, np.float64)):
        for k in range(len(KNEE_STEPS)):
            st = KNEE_STEPS[(i + k) % len(KNEE_STEPS)]
            t = knee_target(st)
            g = np.float64(LD(t) / LD(r))
            cands = [g]
            for _ in range(3):
                cands += [np.nextafter(cands[-2] if len(cands) > 1 else g, np.inf), np.nextafter(cands[-1] if len(cands) > 1 else g, -np.inf)]
            hit = [c for c in cands if np.float64(c * r) == t]
            if hit:
                info[i], steps[i] = hit[0], st
                break
        else:
            raise AssertionError("no information puts edge %d on the knee" % i)
    return info, steps


# ---- poisoned edges behind a mask ----
def poison_problems(ba):
    """-> (poisoned, benign, x, active, bad): at x (omega = 0, t_z = 0) edge bad[0] sits on an all-zero pose with Xw.z = 0, so X_ci.z = 0
    exactly; edge bad[1] has a NaN Xw. `benign` holds ordinary edges at those two indices. Both are masked off."""
    poses = POSES.copy()
    prob, x_gt = make_scene(np.zeros(3), poses, ba, t_cl=(0.05, -0.08, 0.0), pts_per_frame=30, seed=21)
    x = x_gt + np.array([0, 0, 0, 0.03, -0.02, 0.0, 0.1])
    bad = (3, 200)                                   # edge 3 lies on frame 0 (all-zero pose)
    assert prob.edge_frame[bad[0]] == 0 and not prob.frame_Tlw6[0].any() and x[5] == 0.0 and not x[:3].any()
    Xw = prob.edge_Xw.copy()
    Xw[bad[0], 2] = 0.0
    Xw[bad[1], 1] = np.nan
    poisoned = ba.BaProblem(prob.frame_Tlw6, prob.frame_intr, prob.edge_frame, Xw, prob.edge_obs, prob.edge_info, prob.edge_slot)
    active = mask80(len(prob.edge_frame), 9)
    active[list(bad)] = 0
    return poisoned, prob, x, active, bad


# ---- small schedules ----
def small_problem(n, ba):
    """n edges spread over the frames of the generic scene (one per frame first), and the start of the schedule"""
    prob, x_gt = scene_l(ba)
    idx = (np.arange(n) % 8) * 65 + (np.arange(n) // 8) * 7 + 1
    return subset(prob, idx, ba), x_gt + np.array([0.004, -0.006, 0.005, 0.01, -0.01, 0.02, 0.1])


def cpu_cases(ba):
    """every linearisation of the device tests that the long-double route can afford (the tiled problem enters with its base scene)"""
    out = lane_cases(ba) + ragged_cases(ba) + rotation_cases(ba)
    base, x = stride_base(ba)
    out.append(Case("stride", "base scene, masked", base, x, mask80(len(base.edge_frame), 3), True, True))
    poisoned, benign, x, active, _ = poison_problems(ba)
    out += [Case("poison", "poisoned", poisoned, x, active, True, True), Case("poison", "benign", benign, x, active, True, True)]
    for n in (0, 1, 2, 3, 9, 10):
        p, x0 = small_problem(n, ba)
        out.append(Case("small", "N=%d at x0" % n, p, x0, None, True))
    return out


def knee_check(who, evaluator, ba):
    """The Huber-knee family for one evaluator (evaluator(prob) -> fn(x, active, robust) -> (H, b, chi, chi2_edges)): the
    information of 64 edges is rescaled so that the evaluator's own chi2 lands on dsqr and 1, 2, 8 ulps either side of it."""
    base, x = knee_base(ba)
    r2 = evaluator(base)(x, None, True)[3]                       # unit information: chi2 = e0^2 + e1^2 as this evaluator rounds it
    info, steps = knee_info(r2)
    assert set(steps.tolist()) == set(KNEE_STEPS), "a step of the knee ladder is left without an edge"
    prob = subset(base, np.arange(64), ba, info=info)
    ev = evaluator(prob)
    c2 = ev(x, None, True)[3]
    assert np.array_equal(c2, np.array([knee_target(s) for s in steps])), "the evaluator's own chi2_edges are not on the ladder"
    above = c2 > DSQR64                                           # the side this evaluator's chi2 fell on
    assert np.array_equal(above, steps > 0) and above.any() and (~above).any()
    ref = linearise(prob, x, None, True, above=above)
    ref_plain = linearise(prob, x, None, False)
    assert np.all(ref.z > Z_FLOOR)
    check("knee", who, ev(x, None, True), ref)
    for i in range(64):
        hot = np.zeros(64, np.uint8)
        hot[i] = 1
        rob, plain = ev(x, hot, True), ev(x, hot, False)
        check("knee", who, rob, ref, H=ref.Hi[i], b=ref.bi[i], chi=ref.rho[i])
        check("knee", who, plain, ref_plain, H=ref_plain.Hi[i], b=ref_plain.bi[i], chi=ref_plain.rho[i])
        same = np.array_equal(rob[0], plain[0]) and np.array_equal(rob[1], plain[1]) and rob[2] == plain[2]
        assert same == (not above[i]), ("edge %d at %+d ulp: kernel on and off %s" % (i, steps[i], "agree" if same else "differ"))
        if not above[i]:
            assert rob[2] == c2[i]
    return prob, x

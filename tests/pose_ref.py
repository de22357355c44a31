"""numpy restatement of the motion-only pose optimisation's rules P1-P9 (include/iba_mi355x.h, iba_pose*): float64, the same fixed sequences and the same
summation tree as csrc/iba_pose_math.hpp, written independently of it. Also the long-double / mpmath evaluations the parity gates compare with."""
import math

import numpy as np

LANES = 256
NSUMS = 28
PI2 = 9.869604401089358
DMAX = 1.7976931348623157e308
DEFAULT_DELTA = np.float32(math.sqrt(5.991))
NAN64 = np.frombuffer(np.uint64(0x7FF8000000000000).tobytes(), np.float64)[0]
NAN32 = np.frombuffer(np.uint32(0x7FC00000).tobytes(), np.float32)[0]
DEFAULTS = dict(rounds=4, iterations=10, chi2_threshold=np.float32(5.991), huber_delta=DEFAULT_DELTA, robust_rounds=3)


def canon(x):
    x = np.asarray(x)
    return np.where(np.isnan(x), NAN64 if x.dtype == np.float64 else NAN32, x).astype(x.dtype)


def hidx(p, q):
    return p * 6 - p * (p - 1) // 2 + (q - p)


# ---- P1 ----
def edge(T, K, xyz, obs, w, jac=True):
    """T [3, 4] f64, K = (fx, fy, cx, cy), xyz [n, 3], obs [n, 2], w [n] (float32 inputs are widened) -> ex, ey, chi2, J (list of 12 [n] arrays or None)"""
    T = np.asarray(T, np.float64).reshape(3, 4)
    fx, fy, cx, cy = (np.float64(np.float32(v)) for v in K)
    X, Y, Z = (np.asarray(xyz, np.float32).reshape(-1, 3)[:, k].astype(np.float64) for k in range(3))
    ox, oy = (np.asarray(obs, np.float32).reshape(-1, 2)[:, k].astype(np.float64) for k in range(2))
    w = np.asarray(w, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        px = ((T[0, 0] * X + T[0, 1] * Y) + T[0, 2] * Z) + T[0, 3]
        py = ((T[1, 0] * X + T[1, 1] * Y) + T[1, 2] * Z) + T[1, 3]
        pz = ((T[2, 0] * X + T[2, 1] * Y) + T[2, 2] * Z) + T[2, 3]
        ex = ox - ((fx * px) / pz + cx)
        ey = oy - ((fy * py) / pz + cy)
        chi2 = w * (ex * ex + ey * ey)
        if not jac:
            return ex, ey, chi2, None
        iz = 1.0 / pz
        iz2 = iz * iz
        zero = np.zeros_like(px)
        J = [((px * py) * iz2) * fx, (-(1.0 + (px * px) * iz2)) * fx, (py * iz) * fx, (-iz) * fx, zero, (px * iz2) * fx,
             (1.0 + (py * py) * iz2) * fy, (-((px * py) * iz2)) * fy, (-(px * iz)) * fy, zero, (-iz) * fy, (py * iz2) * fy]
    return ex, ey, chi2, J


# ---- P2 ----
def huber(chi2, robust, delta):
    delta = np.float64(delta)
    with np.errstate(all="ignore"):
        if not robust:
            return chi2, np.ones_like(chi2)
        dsqr = delta * delta
        over = chi2 > dsqr
        sq = np.sqrt(chi2)
        rho0 = np.where(over, (2.0 * sq) * delta - dsqr, chi2)
        rho1 = np.where(over, delta / sq, 1.0)
    return rho0, rho1


def edge_terms(T, K, xyz, obs, w, robust, delta, full=True):
    """-> terms [n, 28] (the b columns hold what is SUBTRACTED), chi2 [n]"""
    ex, ey, chi2, J = edge(T, K, xyz, obs, w, jac=full)
    rho0, rho1 = huber(chi2, robust, delta)
    t = np.zeros((len(chi2), NSUMS))
    with np.errstate(all="ignore"):
        if full:
            wr = rho1 * np.asarray(w, np.float32).astype(np.float64)
            at = 0
            for p in range(6):
                for q in range(p, 6):
                    t[:, at] = wr * (J[p] * J[q] + J[6 + p] * J[6 + q])
                    at += 1
            for p in range(6):
                t[:, 21 + p] = wr * (J[p] * ex + J[6 + p] * ey)
    t[:, 27] = rho0
    return t, chi2


# ---- P3 ----
def tree(v):
    """v [256, k] -> [k]: the balanced binary tree"""
    with np.errstate(all="ignore"):
        while len(v) > 1:
            v = v[0::2] + v[1::2]
    return v[0]


def lane_sums(terms, active):
    n = len(terms)
    rows = max(1, -(-n // LANES))
    pad = np.zeros((rows * LANES, NSUMS))
    act = np.ones(n, bool) if active is None else np.asarray(active).astype(bool)
    pad[:n] = np.where(act[:, None], terms, 0.0)
    acc = np.zeros((LANES, NSUMS))
    sign = np.ones(NSUMS)
    sign[21:27] = -1.0
    with np.errstate(all="ignore"):
        for j in range(rows):
            blk = pad[j * LANES:(j + 1) * LANES]
            acc = np.where(sign > 0, acc + blk, acc - blk)
    return acc


def sums(T, K, xyz, obs, w, active, robust, delta, full=True):
    """-> (sums [28], chi2 per edge [n])"""
    t, chi2 = edge_terms(T, K, xyz, obs, w, robust, delta, full)
    return tree(lane_sums(t, active)), chi2


def eval_job(T, K, xyz, obs, w, active=None, robust=True, delta=DEFAULT_DELTA):
    """what iba_pose_eval answers for one job -> H [6, 6], b [6], chi2_robust, chi2_edges [n]"""
    s, chi2 = sums(T, K, xyz, obs, w, active, robust, delta)
    H = np.zeros((6, 6))
    for r in range(6):
        for c in range(6):
            H[r, c] = s[hidx(min(r, c), max(r, c))]
    return canon(H), canon(s[21:27]), canon(s[27:28])[0], canon(chi2)


# ---- P4 ----
def ldlt6(A, b):
    """-> dx or None"""
    L = [[0.0] * 6 for _ in range(6)]
    d = [0.0] * 6
    for j in range(6):
        s = A[j][j]
        for k in range(j):
            s -= L[j][k] * L[j][k] * d[k]
        if not (s > 0.0) or not (s <= DMAX):
            return None
        d[j] = s
        for i in range(j + 1, 6):
            v = A[i][j]
            for k in range(j):
                v -= L[i][k] * L[j][k] * d[k]
            L[i][j] = fdiv(v, s)
    y = [0.0] * 6
    x = [0.0] * 6
    for i in range(6):
        v = b[i]
        for k in range(i):
            v -= L[i][k] * y[k]
        y[i] = v
    for i in range(5, -1, -1):
        v = fdiv(y[i], d[i])
        for k in range(i + 1, 6):
            v -= L[k][i] * x[k]
        x[i] = v
    return x


def fdiv(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


# ---- P6 ----
def two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def two_prod(a, b):
    p = a * b
    ca = 134217729.0 * a
    ah = ca - (ca - a)
    al = a - ah
    cb = 134217729.0 * b
    bh = cb - (cb - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def series_step(s, d, ah, al):
    p, e = two_prod(s, ah)
    e = e + s * al
    p, e = two_sum(p, e)
    q = p / d
    pp, ee = two_prod(q, d)
    r = ((p - pp) - ee) + e
    ql = r / d
    h, l = two_sum(1.0, -q)
    l = l - ql
    return two_sum(h, l)


def series(s, off):
    """off = 1: sin(th)/th, 2: (1 - cos(th))/th^2, 3: (th - sin(th))/th^3 at s = th^2 <= pi^2"""
    s = float(s)
    a = 1.0
    for k in range(13, 2, -1):
        a = 1.0 - (s / float((2 * k + off - 1) * (2 * k + off))) * a
    h, l = series_step(s, float((3 + off) * (4 + off)), a, 0.0)
    h, l = series_step(s, float((1 + off) * (2 + off)), h, l)
    return h * 0.5 if off == 2 else (h / 6.0 if off == 3 else h)


def exp_update(dx, T):
    """-> (Exp(dx) T as [3, 4], big)"""
    T = [float(v) for v in np.asarray(T, np.float64).reshape(12)]
    dx = [float(v) for v in dx]
    w0, w1, w2 = dx[:3]
    with np.errstate(all="ignore"):
        s = float((np.float64(w0) * w0 + np.float64(w1) * w1) + np.float64(w2) * w2)
    big = 0
    if s > PI2:
        th = math.sqrt(s) if math.isfinite(s) else s
        sn, cs = (math.sin(th), math.cos(th)) if math.isfinite(th) else (float("nan"), float("nan"))
        A, B, C = fdiv(sn, th), fdiv(1.0 - cs, s), fdiv(th - sn, fmul(s, th))
        big = 1
    elif s == s:
        A, B, C = series(s, 1), series(s, 2), series(s, 3)
    else:
        A = B = C = float("nan")
    O = np.array([0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0])
    with np.errstate(all="ignore"):
        f = np.float64
        O2 = np.array([-(f(w1) * w1 + f(w2) * w2), f(w0) * w1, f(w0) * w2, f(w0) * w1, -(f(w0) * w0 + f(w2) * w2), f(w1) * w2, f(w0) * w2, f(w1) * w2, -(f(w0) * w0 + f(w1) * w1)])
        I = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0])
        Re = (I + f(A) * O) + f(B) * O2
        V = (I + f(B) * O) + f(C) * O2
        Tn = np.zeros(12)
        Ta = np.array(T)
        u = np.array(dx[3:])
        for r in range(3):
            te = (V[3 * r] * u[0] + V[3 * r + 1] * u[1]) + V[3 * r + 2] * u[2]
            for c in range(3):
                Tn[4 * r + c] = (Re[3 * r] * Ta[c] + Re[3 * r + 1] * Ta[4 + c]) + Re[3 * r + 2] * Ta[8 + c]
            Tn[4 * r + 3] = ((Re[3 * r] * Ta[3] + Re[3 * r + 1] * Ta[7]) + Re[3 * r + 2] * Ta[11]) + te
    return Tn.reshape(3, 4), big


def fmul(a, b):
    with np.errstate(all="ignore"):
        return float(np.float64(a) * np.float64(b))


# ---- P4, P5, P7, P8: the whole schedule of one job ----
def finite(x):
    return -DMAX <= x <= DMAX


def optimize(T0, K, xyz, obs, w, **opt):
    """-> dict: Tcw12 [3, 4] f64, Tcw12f f32, n, n_inliers, rounds_run, chi2 [8], n_bad, lm_iterations, trials [8], outlier [n] u8, chi2_edges [n] f32,
    stages (a list of [3, 4] poses), big_steps, nonfinite_trials (trials whose factorisation succeeded and whose chi2 sum is not finite), margin (the least relative distance of a classified chi2 from the threshold, over all rounds)"""
    o = dict(DEFAULTS)
    o.update(opt)
    T0 = np.asarray(T0, np.float64).reshape(3, 4)
    xyz, obs, w = np.asarray(xyz, np.float32).reshape(-1, 3), np.asarray(obs, np.float32).reshape(-1, 2), np.asarray(w, np.float32).reshape(-1)
    n = len(w)
    res = dict(n=n, n_inliers=0, rounds_run=0, Tcw12=T0.copy(), Tcw12f=T0.astype(np.float32), chi2=np.zeros(8), n_bad=np.zeros(8, np.int32), lm_iterations=np.zeros(8, np.int32),
               trials=np.zeros(8, np.int32), outlier=np.zeros(n, np.uint8), chi2_edges=np.zeros(n, np.float32), stages=[], big_steps=0, margin=np.inf, nonfinite_trials=0)
    if n < 3:
        return res
    thr = np.float32(o["chi2_threshold"])
    delta = np.float64(np.float32(o["huber_delta"]))
    active = np.ones(n, bool)
    T = T0.copy()
    nbad = 0
    with np.errstate(all="ignore"):
        for rnd in range(o["rounds"]):
            robust = rnd < o["robust_rounds"]
            T = T0.copy()
            its = trials = 0
            lam = ni = current = 0.0
            for it in range(o["iterations"]):
                s, _ = sums(T, K, xyz, obs, w, active, robust, delta)
                s = [float(v) for v in s]
                current = s[27]
                if it == 0:
                    md = 0.0
                    for k in range(6):
                        d = abs(s[hidx(k, k)])
                        if d > md:
                            md = d
                    lam, ni = 1e-5 * md, 2.0
                its += 1
                qmax, stop = 0, False
                while True:
                    A = [[s[hidx(min(r, c), max(r, c))] + (lam if r == c else 0.0) for c in range(6)] for r in range(6)]
                    dx = ldlt6(A, s[21:27])
                    trials += 1
                    temp = DMAX
                    Tn = None
                    if dx is not None:
                        Tn, big = exp_update(dx, T)
                        res["big_steps"] += big
                        st, _ = sums(Tn, K, xyz, obs, w, active, robust, delta, full=False)
                        temp = float(st[27])
                        res["nonfinite_trials"] += 0 if finite(temp) else 1
                    rho = np.float64(current) - np.float64(temp)
                    scale = np.float64(1e-3)
                    if dx is not None:
                        for k in range(6):
                            scale = scale + np.float64(dx[k]) * (np.float64(lam) * dx[k] + s[21 + k])
                    rho = float(rho / scale)
                    if dx is not None and rho > 0.0 and finite(temp):
                        t = 2.0 * rho - 1.0
                        alpha = float(1.0 - (np.float64(t) * t) * t)
                        if 2.0 / 3.0 < alpha:
                            alpha = 2.0 / 3.0
                        if not (1.0 / 3.0 < alpha):
                            alpha = 1.0 / 3.0
                        lam, ni, current, T = lam * alpha, 2.0, temp, Tn
                    else:
                        lam = fmul(lam, ni)
                        ni = ni * 2.0
                        if not finite(lam):
                            stop = True
                            break
                    qmax += 1
                    if not (rho < 0.0 and qmax < 10):
                        stop = qmax == 10 or rho == 0.0
                        break
                if stop:
                    break
            _, _, chi2, _ = edge(T, K, xyz, obs, w, jac=False)
            c32 = chi2.astype(np.float32)
            bad = c32 > thr
            fin = np.isfinite(c32)
            if fin.any() and thr > 0:
                res["margin"] = min(res["margin"], float(np.min(np.abs(c32[fin].astype(np.float64) - np.float64(thr)) / np.float64(thr))))
            active = ~bad
            nbad = int(bad.sum())
            res["outlier"], res["chi2_edges"] = bad.astype(np.uint8), canon(c32)
            res["chi2"][rnd] = canon(np.float64(current))
            res["n_bad"][rnd], res["lm_iterations"][rnd], res["trials"][rnd] = nbad, its, trials
            res["stages"].append(np.array(T, np.float64).reshape(3, 4).copy())
            res["rounds_run"] = rnd + 1
            if n < 10:
                break
    res["Tcw12"] = np.array(T, np.float64).reshape(3, 4)
    res["Tcw12f"] = res["Tcw12"].astype(np.float32)
    res["n_inliers"] = n - nbad
    return res


# ---- P9 ----
def edges_from_matches(match, query_index, last_world_xyz, cur_xy, cur_octave, inv_level_sigma2):
    match = np.asarray(match, np.int32)
    qi = np.arange(len(match)) if query_index is None else np.asarray(query_index)
    point = {}
    for q, c in enumerate(match):
        if c >= 0:
            point[int(c)] = int(qi[q])
    keys = sorted(point)
    wx, xy = np.asarray(last_world_xyz, np.float32).reshape(-1, 3), np.asarray(cur_xy, np.float32).reshape(-1, 2)
    lv = np.asarray(inv_level_sigma2, np.float32)
    return (np.array([wx[point[c]] for c in keys], np.float32).reshape(-1, 3), np.array([xy[c] for c in keys], np.float32).reshape(-1, 2),
            np.array([lv[cur_octave[c]] for c in keys], np.float32), np.array(keys, np.int32))


# ---- the wider evaluations the gates compare with ----
def sums_longdouble(T, K, xyz, obs, w, active, robust, delta):
    """the 28 sums with every operation in long double and a plain sum -> (sums [28], the sums of the terms' magnitudes [28]) in long double"""
    ld = np.longdouble
    T = np.asarray(T, np.float64).reshape(3, 4).astype(ld)
    fx, fy, cx, cy = (ld(np.float32(v)) for v in K)
    P = np.asarray(xyz, np.float32).reshape(-1, 3).astype(ld)
    ob = np.asarray(obs, np.float32).reshape(-1, 2).astype(ld)
    w = np.asarray(w, np.float32).astype(ld)
    p = P @ T[:, :3].T + T[:, 3]
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    ex, ey = ob[:, 0] - (fx * px / pz + cx), ob[:, 1] - (fy * py / pz + cy)
    chi2 = w * (ex * ex + ey * ey)
    iz = 1 / pz
    iz2 = iz * iz
    z = np.zeros_like(px)
    J = [px * py * iz2 * fx, -(1 + px * px * iz2) * fx, py * iz * fx, -iz * fx, z, px * iz2 * fx, (1 + py * py * iz2) * fy, -px * py * iz2 * fy, -px * iz * fy, z, -iz * fy, py * iz2 * fy]
    d = ld(np.float64(np.float32(delta)))
    over = (chi2 > d * d) if robust else np.zeros(len(chi2), bool)
    sq = np.sqrt(chi2)
    rho0 = np.where(over, 2 * sq * d - d * d, chi2)
    wr = np.where(over, d / np.where(over, sq, 1), 1) * w
    act = np.ones(len(w), bool) if active is None else np.asarray(active).astype(bool)
    out, scale = np.zeros(NSUMS, ld), np.zeros(NSUMS, ld)
    terms = []
    for a in range(6):
        for b in range(a, 6):
            terms.append(wr * (J[a] * J[b] + J[6 + a] * J[6 + b]))
    for a in range(6):
        terms.append(-(wr * (J[a] * ex + J[6 + a] * ey)))
    terms.append(rho0)
    for k, t in enumerate(terms):
        out[k], scale[k] = np.sum(t[act]), np.sum(np.abs(t[act]))
    return out, scale


def jacobian_central(T, K, X, ob, h=1e-6):
    """d e / d dx at dx = 0 of e(Exp(dx) T) by central differences in long double (Exp by mpmath-free Rodrigues in long double) -> [2, 6]"""
    ld = np.longdouble
    T = np.asarray(T, np.float64).reshape(3, 4).astype(ld)
    fx, fy, cx, cy = (ld(np.float32(v)) for v in K)
    X = np.asarray(X, np.float32).astype(ld)
    ob = np.asarray(ob, np.float32).astype(ld)

    def err(dx):
        wv, u = dx[:3], dx[3:]
        th = np.sqrt(wv @ wv)
        O = np.array([[0, -wv[2], wv[1]], [wv[2], 0, -wv[0]], [-wv[1], wv[0], 0]], ld)
        if th > 0:
            A, B, C = np.sin(th) / th, (1 - np.cos(th)) / th ** 2, (th - np.sin(th)) / th ** 3
        else:
            A, B, C = ld(1), ld(0.5), ld(1) / 6
        R = np.eye(3, dtype=ld) + A * O + B * (O @ O)
        V = np.eye(3, dtype=ld) + B * O + C * (O @ O)
        p = R @ (T[:, :3] @ X + T[:, 3]) + V @ u
        return np.array([ob[0] - (fx * p[0] / p[2] + cx), ob[1] - (fy * p[1] / p[2] + cy)], ld)

    J = np.zeros((2, 6), ld)
    for k in range(6):
        d = np.zeros(6, ld)
        d[k] = ld(h)
        J[:, k] = (err(d) - err(-d)) / (2 * ld(h))
    return J


def series_exact(s, off):
    """the coefficient in mpmath at 200 bits"""
    import mpmath as mp
    with mp.workprec(200):
        s = mp.mpf(float(s))
        if s == 0:
            return mp.mpf(1) / [1, 2, 6][off - 1]
        th = mp.sqrt(s)
        return [mp.sin(th) / th, (1 - mp.cos(th)) / s, (th - mp.sin(th)) / (s * th)][off - 1]

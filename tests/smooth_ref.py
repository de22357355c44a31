"""Numpy restatement of the robust pose-graph smoother's contract (include/iba_mi355x.h, iba_smooth_*; rules S1-S5 as there): test infrastructure.
  * exp_se3 / log_se3 / jr_inv / ad_inv: rule S1 and the Jacobian pieces of S2 on stacks, in the dtype of their input; every coefficient has its
    series branch below SERIES_TH2 (theta^2), the closed form above it.
  * linearize(..., dtype): S2 and S3 over all factors at once, the node gather in ascending factor index; with dtype=np.longdouble the same rules in
    long double — the yardstick the parity gates measure both sides against.
  * dense_system / dense_solve: H as a dense 6N x 6N; ld=True refines the float64 solve with long-double residuals until it is the long-double answer.
  * sparse_system / sparse_solve / block_residual: the twins of tests/pgo_ref.py's, with the priors, for systems too large for the dense H.
  * optimize(g, opt, ld=None | "lin" | "solve"): rule S4 (rule 6 of iba_pgo_* on F); the two twins linearise, respectively solve, in long double.
    Every rho and every stopping comparison is recorded, check_margins asserts that none is a near-tie.
  * make_graph: a seeded chain with a prior on node 0, odometry factors, true loops and false loops (all loops robust).
"""
import numpy as np

import pgo_ref as P

EPS = P.EPS
SERIES_TH2 = 1e-2          # theta^2 below which the coefficients of Exp, Log and Jr^-1 are series in theta^2
SERIES_U2 = 2.5e-3         # (|v| / w)^2 of the quaternion below which atan(u) / u is a series (theta about 0.1)
STOP_NONE, STOP_RIGHT_TERM, STOP_INCREMENT, STOP_RESIDUAL_INCREMENT, STOP_RESIDUAL, STOP_MAX_ITERATION = 0, 1, 2, 3, 4, 5

DEFAULTS = dict(max_iteration=100, max_iteration_lm=20, min_relative_increment=1e-6, min_relative_residual_increment=1e-6, min_right_term=1e-6,
                min_residual=1e-6, upper_scale_factor=2.0 / 3.0, lower_scale_factor=1.0 / 3.0, segment=128)

# backend_opt.h:81-83
PRIOR_VAR = np.full(6, 1e-12)
ODOM_VAR = np.array([1e-6, 1e-6, 1e-6, 1e-4, 1e-4, 1e-4])
LOOP_VAR = np.full(6, 0.5)


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        if k not in o:
            raise KeyError(k)
    o.update(kw)
    return o


def _horner(x, cs):
    """cs[0] + x (cs[1] + x (...)), evaluated from the last coefficient"""
    v = x * 0 + cs[-1]
    for c in cs[-2::-1]:
        v = v * x + c
    return v


def _frac(dt, num, den):
    return dt(num) / dt(den)


def coeffs(th2):
    """th2 = theta^2 [n] -> dict of a = sin t / t, b = (1 - cos t) / t^2, c = (t - sin t) / t^3, e = (1 - (t / 2) cot(t / 2)) / t^2,
    c2 = (t^2 / 2 + cos t - 1) / t^4, k4 = (c2 + 3 (c - 1/6) / t^2) / 2"""
    dt = th2.dtype.type
    small = th2 < dt(SERIES_TH2)
    x = np.where(small, th2, dt(0))
    f = lambda n, d: _frac(dt, n, d)
    ser = dict(
        a=_horner(x, [dt(1), -f(1, 6), f(1, 120), -f(1, 5040), f(1, 362880), -f(1, 39916800)]),
        b=_horner(x, [f(1, 2), -f(1, 24), f(1, 720), -f(1, 40320), f(1, 3628800), -f(1, 479001600)]),
        c=_horner(x, [f(1, 6), -f(1, 120), f(1, 5040), -f(1, 362880), f(1, 39916800), -f(1, 6227020800)]),
        e=_horner(x, [f(1, 12), f(1, 720), f(1, 30240), f(1, 1209600), f(1, 47900160), f(691, 1307674368000)]),
        c2=_horner(x, [f(1, 24), -f(1, 720), f(1, 40320), -f(1, 3628800), f(1, 479001600)]),
        k4=_horner(x, [f(1, 120), -f(1, 2520), f(1, 120960), -f(1, 9979200), f(1, 1245404160)]))
    t2 = np.where(small, dt(1), th2)
    t = np.sqrt(t2)
    sh, ch = np.sin(t * dt(0.5)), np.cos(t * dt(0.5))
    s = dt(2) * sh * ch
    a = s / t
    b = dt(2) * sh * sh / t2
    c = (t - s) / (t2 * t)
    e = (dt(1) - (t * dt(0.5)) * ch / sh) / t2
    c2 = (dt(0.5) - b) / t2
    k4 = dt(0.5) * (c2 + dt(3) * (c - f(1, 6)) / t2)
    closed = dict(a=a, b=b, c=c, e=e, c2=c2, k4=k4)
    return {k: np.where(small, ser[k], closed[k]) for k in ser}


def hat(v):
    W = np.zeros(v.shape[:1] + (3, 3), v.dtype)
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 0], W[:, 1, 2], W[:, 2, 0], W[:, 2, 1] = -v[:, 2], v[:, 1], v[:, 2], -v[:, 0], -v[:, 1], v[:, 0]
    return W


def _mm(A, B):
    """3x3 stack product, sums in ascending k"""
    C = np.empty_like(A)
    for r in range(3):
        for c in range(3):
            C[:, r, c] = (A[:, r, 0] * B[:, 0, c] + A[:, r, 1] * B[:, 1, c]) + A[:, r, 2] * B[:, 2, c]
    return C


def _mv(A, v):
    o = np.empty_like(v)
    for r in range(3):
        o[:, r] = (A[:, r, 0] * v[:, 0] + A[:, r, 1] * v[:, 1]) + A[:, r, 2] * v[:, 2]
    return o


def _dot3(a, b):
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def exp_se3(xi):
    """S1: xi [n, 6] = [omega, upsilon] -> [n, 4, 4]: R = I + a W + b W^2, t = (I + b W + c W^2) upsilon"""
    xi = np.atleast_2d(xi)
    dt = xi.dtype.type
    om, up = xi[:, :3], xi[:, 3:]
    k = coeffs(_dot3(om, om))
    W = hat(om)
    W2 = _mm(W, W)
    I = np.eye(3, dtype=xi.dtype)[None]
    T = np.zeros((len(xi), 4, 4), xi.dtype)
    T[:, :3, :3] = I + k["a"][:, None, None] * W + k["b"][:, None, None] * W2
    T[:, :3, 3] = up + k["b"][:, None] * _mv(W, up) + k["c"][:, None] * _mv(W2, up)
    T[:, 3, 3] = dt(1)
    return T


def log_so3(M):
    """rotation part of a stack [n, >= 3, >= 3] -> omega [n, 3], through the quaternion (largest component first), theta = 2 atan2(|v|, w) in [0, pi]"""
    dt = M.dtype.type
    R = M
    tr = (R[:, 0, 0] + R[:, 1, 1]) + R[:, 2, 2]
    case = np.where(tr > 0, 0, np.where((R[:, 0, 0] > R[:, 1, 1]) & (R[:, 0, 0] > R[:, 2, 2]), 1, np.where(R[:, 1, 1] > R[:, 2, 2], 2, 3)))
    n = len(M)
    q = np.zeros((n, 4), M.dtype)   # w, x, y, z
    with np.errstate(invalid="ignore", divide="ignore"):
        S0 = np.sqrt(tr + dt(1)) * dt(2)
        S1 = np.sqrt(((dt(1) + R[:, 0, 0]) - R[:, 1, 1]) - R[:, 2, 2]) * dt(2)
        S2 = np.sqrt(((dt(1) + R[:, 1, 1]) - R[:, 0, 0]) - R[:, 2, 2]) * dt(2)
        S3 = np.sqrt(((dt(1) + R[:, 2, 2]) - R[:, 0, 0]) - R[:, 1, 1]) * dt(2)
        d21, d02, d10 = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
        s01, s02, s12 = R[:, 0, 1] + R[:, 1, 0], R[:, 0, 2] + R[:, 2, 0], R[:, 1, 2] + R[:, 2, 1]
        cand = [np.stack([S0 * dt(0.25), d21 / S0, d02 / S0, d10 / S0], 1), np.stack([d21 / S1, S1 * dt(0.25), s01 / S1, s02 / S1], 1),
                np.stack([d02 / S2, s01 / S2, S2 * dt(0.25), s12 / S2], 1), np.stack([d10 / S3, s02 / S3, s12 / S3, S3 * dt(0.25)], 1)]
    for c in range(4):
        q[case == c] = cand[c][case == c]
    q = np.where((q[:, 0] < 0)[:, None], -q, q)
    w, v = q[:, 0], q[:, 1:]
    s2 = _dot3(v, v)
    s = np.sqrt(s2)
    with np.errstate(invalid="ignore", divide="ignore"):
        u2 = s2 / (w * w)
        small = u2 < dt(SERIES_U2)
        x = np.where(small, u2, dt(0))
        f = lambda a, b: _frac(dt, a, b)
        ser = (dt(2) / np.where(small, w, dt(1))) * _horner(x, [dt(1), -f(1, 3), f(1, 5), -f(1, 7), f(1, 9), -f(1, 11)])
        closed = dt(2) * np.arctan2(s, w) / np.where(small, dt(1), s)
    k = np.where(small, ser, closed)
    return k[:, None] * v


def log_se3(M):
    """S1: [n, >= 3, 4] -> r [n, 6] = [omega, V(omega)^-1 t], V^-1 = I - W / 2 + e W^2"""
    dt = M.dtype.type
    om = log_so3(M)
    k = coeffs(_dot3(om, om))
    W = hat(om)
    t = M[:, :3, 3]
    Wt = _mv(W, t)
    up = (t - dt(0.5) * Wt) + k["e"][:, None] * _mv(W, Wt)
    return np.concatenate([om, up], 1)


def jr_inv(r):
    """S2: the derivative of Log(M Exp(eps)) in eps at eps = 0, r = Log(M): [[Ji, 0], [-Ji Q Ji, Ji]], Ji = I + W / 2 + e W^2 (W = [omega]x) and
    Q = -U / 2 + c (W U + U W + d W) - c2 (W W U + U W W + 3 d W) - 2 k4 d W W (U = [upsilon]x, d = omega . upsilon): Barfoot's Q at -r"""
    dt = r.dtype.type
    om, up = r[:, :3], r[:, 3:]
    k = coeffs(_dot3(om, om))
    W, U = hat(om), hat(up)
    d = _dot3(om, up)[:, None, None]
    W2 = _mm(W, W)
    WU = _mm(W, U)
    UW = np.transpose(WU, (0, 2, 1))
    WWU = _mm(W, WU)
    UWW = -np.transpose(WWU, (0, 2, 1))
    I = np.eye(3, dtype=r.dtype)[None]
    Ji = (I + dt(0.5) * W) + k["e"][:, None, None] * W2
    Q = ((dt(-0.5) * U + k["c"][:, None, None] * ((WU + UW) + d * W)) - k["c2"][:, None, None] * ((WWU + UWW) + dt(3) * d * W)) - (dt(2) * k["k4"][:, None, None]) * (d * W2)
    J = np.zeros((len(r), 6, 6), r.dtype)
    J[:, :3, :3] = Ji
    J[:, 3:, 3:] = Ji
    J[:, 3:, :3] = -_mm(_mm(Ji, Q), Ji)
    return J


def ad_inv(Pm):
    """Ad(P^-1) in [omega, upsilon] order: [[R^T, 0], [[t']x R^T, R^T]], t' = -R^T t"""
    Pi = P.inv12(Pm)
    Rt, tp = Pi[:, :3, :3], Pi[:, :3, 3]
    A = np.zeros((len(Pm), 6, 6), Pm.dtype)
    A[:, :3, :3] = Rt
    A[:, 3:, 3:] = Rt
    A[:, 3:, :3] = _mm(hat(tp), np.ascontiguousarray(Rt))
    return A


class Graph:
    """nodes [N, 4, 4]; factors in call order: fi [F] (-1: a prior), fj [F], Z [F, 4, 4], var [F, 6], robust [F] bool"""

    def __init__(self, nodes, factors=(), truth=None):
        self.nodes = np.ascontiguousarray(nodes, np.float64).reshape(-1, 4, 4)
        self.fi, self.fj, self.Z, self.var, self.robust = [], [], [], [], []
        self.truth = truth
        for f in factors:
            self.add(*f)

    def add(self, i, j, Z, var, robust=False):
        self.fi.append(int(i)); self.fj.append(int(j)); self.Z.append(np.asarray(Z, np.float64).reshape(4, 4)); self.var.append(np.asarray(var, np.float64).reshape(6))
        self.robust.append(bool(robust))

    @property
    def N(self):
        return len(self.nodes)

    @property
    def F(self):
        return len(self.fi)

    def arrays(self):
        F = self.F
        return (np.asarray(self.fi, np.int64).reshape(F), np.asarray(self.fj, np.int64).reshape(F), np.asarray(self.Z, np.float64).reshape(F, 4, 4),
                np.asarray(self.var, np.float64).reshape(F, 6), np.asarray(self.robust, bool).reshape(F))


def factor_terms(nodes, g, dtype=np.float64, want_j=True):
    """S2 per factor: r [F, 6], J [F, 6, 6] (with respect to delta_j), q = sum r_k^2 / var_k [F], scale [F] (|t| of everything M's translation is summed from)"""
    fi, fj, Z, var, _ = g.arrays()
    Pn = nodes.astype(dtype)
    Zi = P.inv12(Z.astype(dtype))
    Pj = Pn[fj]
    prior = fi < 0
    B = np.where(prior[:, None, None], Zi, P.mul12(Zi, P.inv12(Pn[np.where(prior, 0, fi)])))
    M = P.mul12(B, Pj)
    r = log_se3(M)
    iv = dtype(1) / var.astype(dtype)
    q = r[:, 0] * r[:, 0] * iv[:, 0]
    for k in range(1, 6):
        q = q + r[:, k] * r[:, k] * iv[:, k]
    J = None
    if want_j:
        Ji, Ad = jr_inv(r), ad_inv(Pj)
        J = np.zeros((g.F, 6, 6), dtype)
        for a in range(6):
            for c in range(6):
                v = Ji[:, a, 0] * Ad[:, 0, c]
                for k in range(1, 6):
                    v = v + Ji[:, a, k] * Ad[:, k, c]
                J[:, a, c] = v
    nrm = lambda T: np.sqrt(np.sum(T[:, :3, 3].astype(np.float64) ** 2, axis=1))
    scale = nrm(Z) + nrm(Pn[fj]) + np.where(prior, 0.0, nrm(Pn[np.where(prior, 0, fi)]))
    return r, J, q, scale


def linearize(nodes, g, dtype=np.float64):
    """-> dict(r, w, A [F, 6, 6], g [F, 6], D [N, 6, 6], b [N, 6], F, q, max_diag_between, terms): S2, S3; sums over a node's factors in ascending
    factor index. `terms`: per output the sum of the absolute values of the terms of its largest sum (for r: its largest entry), as tests/pgo_ref.py has it."""
    fi, fj, _, var, robust = g.arrays()
    nF, N = g.F, len(nodes)
    r, J, q, scale = factor_terms(nodes, g, dtype)
    iv = dtype(1) / var.astype(dtype)
    w = np.where(robust, dtype(1) / (dtype(1) + q), dtype(1))
    cost = np.where(robust, np.log1p(q), q)
    A = np.empty((nF, 6, 6), dtype)
    Aabs = np.zeros((nF, 6, 6))
    for k in range(6):
        for l in range(k, 6):
            a = J[:, 0, k] * iv[:, 0] * J[:, 0, l]
            t = np.abs(a)
            for m in range(1, 6):
                term = J[:, m, k] * iv[:, m] * J[:, m, l]
                a = a + term
                t = t + np.abs(term)
            A[:, k, l] = w * a
            A[:, l, k] = A[:, k, l]
            Aabs[:, k, l] = Aabs[:, l, k] = (w * t).astype(np.float64)
    gv = np.empty((nF, 6), dtype)
    gabs = np.zeros((nF, 6))
    for k in range(6):
        a = J[:, 0, k] * iv[:, 0] * r[:, 0]
        t = np.abs(a)
        for m in range(1, 6):
            term = J[:, m, k] * iv[:, m] * r[:, m]
            a = a + term
            t = t + np.abs(term)
        gv[:, k] = w * a
        gabs[:, k] = (w * t).astype(np.float64)
    D = np.zeros((N, 6, 6), dtype)
    Db = np.zeros((N, 6, 6), dtype)
    b = np.zeros((N, 6), dtype)
    babs = np.zeros((N, 6))
    Dabs = np.zeros((N, 6, 6))
    for f in range(nF):
        i, j = fi[f], fj[f]
        D[j] += A[f]; Dabs[j] += Aabs[f]
        b[j] += -gv[f]; babs[j] += gabs[f]
        if i >= 0:
            D[i] += A[f]; Dabs[i] += Aabs[f]
            b[i] += gv[f]; babs[i] += gabs[f]
            Db[i] += A[f]; Db[j] += A[f]
    Fv = dtype(0)
    for f in range(nF):
        Fv = Fv + cost[f]
    terms = dict(r=float(np.max(np.abs(r.astype(np.float64)))) if nF else 0.0, w=1.0, A=float(np.max(Aabs)) if nF else 0.0, D=float(np.max(Dabs)) if nF else 0.0,
                 b=float(np.max(babs)) if nF else 0.0, F=float(np.sum(np.abs(cost.astype(np.float64)))) if nF else 0.0)
    mdb = float(np.max(np.abs(np.stack([Db[:, k, k] for k in range(6)])))) if nF else 0.0
    return dict(r=r, w=w, A=A, g=gv, D=D, b=b, F=Fv, q=q, max_diag_between=mdb, terms=terms)


def dense_system(N, g, A, b):
    """H [6N, 6N]: a between factor adds A to H_ii, H_jj and -A to H_ij, H_ji; a prior adds A to H_jj. b stacked."""
    H = np.zeros((6 * N, 6 * N), np.asarray(A).dtype)
    for f in range(g.F):
        j = 6 * g.fj[f]
        H[j:j + 6, j:j + 6] += A[f]
        if g.fi[f] >= 0:
            i = 6 * g.fi[f]
            H[i:i + 6, i:i + 6] += A[f]
            H[i:i + 6, j:j + 6] -= A[f]; H[j:j + 6, i:i + 6] -= A[f]
    return H, np.asarray(b).reshape(-1)


def _factor_pairs(g):
    for f in range(g.F):
        i, j = g.fi[f], g.fj[f]
        yield j, j, 1.0, f
        if i >= 0:
            yield i, i, 1.0, f
            yield i, j, -1.0, f
            yield j, i, -1.0, f


def sparse_system(N, g, A):
    """the H of dense_system as a scipy.sparse CSC matrix, entry for entry: the twin of tests/pgo_ref.py's, with the priors"""
    return P.blocks_to_csc(N, *P.system_blocks(N, _factor_pairs(g), np.asarray(A, np.float64)))


sparse_solve = P.sparse_solve


def block_residual(N, g, A, b, lam, delta):
    """|(H + lam I) delta - b| / |b| in long double from H's 6x6 blocks, without forming H: _rel_residual's figure (see tests/pgo_ref.py)"""
    return P.blocks_residual(N, *P.system_blocks(N, _factor_pairs(g), np.asarray(A, np.float64).reshape(-1, 6, 6)), b, lam, delta)


def dense_solve(H, b, lam, ld=False):
    """(H + lam I)^-1 b; ld: refined with long-double residuals (the factorisation error of float64 at a 1e12 condition number is 1e-4: 5 rounds
    contract it below long double's rounding)"""
    M = H.astype(np.float64) + lam * np.eye(len(H))
    x = np.linalg.solve(M, b.astype(np.float64))
    if not ld:
        return x
    Ml, bl = H.astype(np.longdouble) + np.longdouble(lam) * np.eye(len(H), dtype=np.longdouble), b.astype(np.longdouble)
    xl = x.astype(np.longdouble)
    for _ in range(5):
        res = bl - Ml @ xl
        xl = xl + np.linalg.solve(M, res.astype(np.float64)).astype(np.longdouble)
    return xl.astype(np.float64)


def apply_delta(nodes, delta):
    """S4: Exp(delta_i) P_i"""
    return P.to44(P.mul12(exp_se3(np.asarray(delta, np.float64).reshape(-1, 6)), nodes))


def optimize(g, opt=None, ld=None, nodes=None):
    """S4 -> dict(nodes, weight, iterations, trials, stop, F, lam, lam0, trace, log, max_b [max |b| at the start and after every accepted step],
    iterates [the poses there])"""
    opt = options() if opt is None else opt
    dt = np.longdouble if ld == "lin" else np.float64
    N = g.N
    nodes = g.nodes.copy() if nodes is None else nodes.copy()
    log = dict(rho=[], cmp=[])

    def lin(nd):
        r = linearize(nd, g, dt)
        H, b = dense_system(N, g, r["A"].astype(np.float64), r["b"].astype(np.float64))
        return H, b, float(r["F"]), r["w"].astype(np.float64), r["max_diag_between"]

    def cmp(kind, lhs, rhs):
        log["cmp"].append((kind, float(lhs), float(rhs)))
        return lhs < rhs

    H, b, Fc, weight, mdb = lin(nodes)
    lam0 = lam = 1e-5 * mdb
    nu = 2.0
    stop, iterations, trials, trace = STOP_NONE, 0, 0, []
    max_b, iterates = [float(np.max(np.abs(b)))], [nodes.copy()]
    while stop == STOP_NONE:
        if cmp("right_term", float(np.max(np.abs(b))), opt["min_right_term"]):
            stop = STOP_RIGHT_TERM
            break
        if iterations >= opt["max_iteration"]:
            stop = STOP_MAX_ITERATION
            break
        x = P.vec6(nodes).reshape(-1)
        xnorm = float(np.sqrt(np.sum(x * x)))
        for _ in range(opt["max_iteration_lm"]):
            delta = dense_solve(H, b, lam, ld == "solve")
            trials += 1
            if cmp("increment", float(np.sqrt(np.sum(delta * delta))), opt["min_relative_increment"] * (xnorm + opt["min_relative_increment"])):
                stop = STOP_INCREMENT
                trace.append(2)
                break
            trial = apply_delta(nodes, delta)
            _, _, q, _ = factor_terms(trial, g, dt, want_j=False)
            cost = np.where(g.arrays()[4], np.log1p(q), q)
            acc = dt(0)
            for f in range(g.F):
                acc = acc + cost[f]
            F_new = float(acc)
            rho = (Fc - F_new) / (float(delta @ (lam * delta + b)) + 1e-3)
            log["rho"].append(rho)
            if rho > 0:
                t = 2.0 * rho - 1.0
                lam *= max(opt["lower_scale_factor"], min(1.0 - t * t * t, opt["upper_scale_factor"]))
                nu = 2.0
                trace.append(1)
                nodes = trial
                F_before = Fc
                H, b, Fc, weight, _ = lin(nodes)
                max_b.append(float(np.max(np.abs(b)))); iterates.append(nodes.copy())
                if cmp("residual_increment", F_before - F_new, opt["min_relative_residual_increment"] * F_before):
                    stop = STOP_RESIDUAL_INCREMENT
                break
            trace.append(0)
            lam *= nu
            nu *= 2.0
        iterations += 1
        if stop == STOP_NONE and cmp("residual", Fc, opt["min_residual"]):
            stop = STOP_RESIDUAL
    return dict(nodes=nodes, weight=weight, iterations=iterations, trials=trials, stop=stop, F=Fc, lam=lam, lam0=lam0, trace=trace, log=log, max_b=max_b,
                iterates=iterates)


def check_margins(res):
    """no decision of the run is a near-tie: every rho at least 1e-3 from 0, every comparison off its threshold by a factor >= 2"""
    for rho in res["log"]["rho"]:
        assert abs(rho) >= 1e-3, "rho = %g is within 1e-3 of 0" % rho
    for kind, lhs, rhs in res["log"]["cmp"]:
        assert lhs <= 0.5 * rhs or lhs >= 2.0 * rhs, "%s: %g against %g is within a factor 2" % (kind, lhs, rhs)


def max_b_at(nodes, g):
    """the reference's max |b| at given poses"""
    return float(np.max(np.abs(linearize(np.asarray(nodes, np.float64), g)["b"])))


def rel(a, b):
    """a^-1 b for two 4x4"""
    return P.to44(P.mul12(P.inv12(a[None]), b[None]))[0]


def make_graph(N, loops=2, false_loops=1, seed=0, prior_var=PRIOR_VAR, odom_var=ODOM_VAR, loop_var=LOOP_VAR, false_offset=5.0, min_gap=8, prior_node=0,
               rot_noise=1e-3, trans_noise=1e-2):
    """A smooth random trajectory (body -> world), the prior on prior_node at the raw pose, odometry factors between(raw_(i-1), raw_i) — at r = 0, as the
    back end builds them — from noisy integrated odometry, `loops` true loops (measured on the truth with small noise) and `false_loops` loops off
    by false_offset metres, all robust. Returns (Graph, list of loop factor indices, of which the last false_loops are false)."""
    rng = np.random.default_rng(seed)
    truth = np.zeros((N, 4, 4))
    truth[0] = np.eye(4)
    yaw = 0.0
    for i in range(1, N):
        yaw = 0.9 * yaw + rng.normal(0, 0.02)
        truth[i] = truth[i - 1] @ P.T_of(np.array([rng.normal(0, 0.003), rng.normal(0, 0.003), yaw, 1.0 + rng.normal(0, 0.05), rng.normal(0, 0.02), rng.normal(0, 0.01)]))[0]
    raw = np.zeros((N, 4, 4))
    raw[0] = truth[0]
    for i in range(1, N):
        step = rel(truth[i - 1], truth[i]) @ exp_se3(np.concatenate([rng.normal(0, rot_noise, 3), rng.normal(0, trans_noise, 3)]))[0]
        raw[i] = raw[i - 1] @ step
        raw[i, 3] = [0, 0, 0, 1]
    g = Graph(raw, truth=truth)
    g.add(-1, prior_node, raw[prior_node], prior_var)
    for i in range(1, N):
        g.add(i - 1, i, rel(raw[i - 1], raw[i]), odom_var)
    loop_ids, used = [], set()
    for k in range(loops + false_loops):
        while True:
            a, b = sorted(rng.integers(0, N, size=2).tolist())
            if b - a >= min(min_gap, max(N - 1, 1)) and (a, b) not in used:
                break
        used.add((a, b))
        Z = rel(truth[a], truth[b]) @ exp_se3(np.concatenate([rng.normal(0, rot_noise, 3), rng.normal(0, trans_noise, 3)]))[0]
        if k >= loops:
            d = rng.normal(size=3)
            Z = Z @ exp_se3(np.concatenate([np.zeros(3), false_offset * d / np.linalg.norm(d)]))[0]
        Z[3] = [0, 0, 0, 1]
        loop_ids.append(g.F)
        g.add(a, b, Z, loop_var, robust=True)
    return g, loop_ids


def case_graph(N, cross=(), seed=0, reverse=(), prior_node=0, prior_var=PRIOR_VAR, robust_chain=()):
    """The shapes of the linearise and solve tests: poses perturbed off a smooth trajectory (so no residual is zero), a prior on prior_node, the chain
    factors (i, i + 1) — stored (i + 1, i) for i in `reverse`, robust for i in `robust_chain` — then the cross factors as listed, robust, (i, j)
    kept in the order given (so j < i is a factor against the chain and a repeated pair a duplicate)."""
    base, _ = make_graph(N, loops=0, false_loops=0, seed=seed)
    truth = base.truth
    rng = np.random.default_rng(1000 + seed)
    noise = lambda r, t: exp_se3(np.concatenate([rng.normal(0, r, 3), rng.normal(0, t, 3)]))[0]
    nodes = truth.copy()
    for i in range(N):
        nodes[i] = nodes[i] @ noise(3e-3, 5e-2)
        nodes[i, 3] = [0, 0, 0, 1]
    g = Graph(nodes, truth=truth)
    g.add(-1, prior_node, truth[prior_node], prior_var)

    def add(i, j, var, robust):
        Z = rel(truth[i], truth[j]) @ noise(2e-3, 3e-2)
        Z[3] = [0, 0, 0, 1]
        g.add(i, j, Z, var, robust)

    for i in range(N - 1):
        add(*((i + 1, i) if i in reverse else (i, i + 1)), ODOM_VAR, i in robust_chain)
    for i, j in cross:
        add(i, j, LOOP_VAR, True)
    return g


def chain4(d, so2, sl2):
    """4 nodes on the x axis one metre apart, a tight prior on node 0, three odometry factors of one metre, one non-robust loop (0, 3) that
    measures 3 + d: a linear problem, every odometry factor absorbs d so2 / (3 so2 + sl2)"""
    T = lambda x: np.array([[1, 0, 0, x], [0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])
    g = Graph(np.stack([T(float(k)) for k in range(4)]))
    g.add(-1, 0, T(0.0), PRIOR_VAR)
    for k in range(3):
        g.add(k, k + 1, T(1.0), np.full(6, so2))
    g.add(0, 3, T(3.0 + d), np.full(6, sl2))
    return g


# stops that leave the run to the increment alone, at rounding level
NEVER = dict(min_relative_increment=1e-15, min_relative_residual_increment=0.0, min_right_term=0.0, min_residual=0.0, max_iteration=8)

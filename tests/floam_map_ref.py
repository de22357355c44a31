"""TEST INFRASTRUCTURE: the F-LOAM scan-to-map block (include/iba_mi355x.h, iba_floam_map_*: rules 1-8) restated in numpy. Imports nothing from the
product. Brute-force neighbours, numpy.linalg.eigh for the line fit, Householder QR for the plane fit, the trust-region loop of csrc/iba_lm.hpp on 6
parameters; a np.longdouble twin of the two fits is the yardstick of the records (rule 9 of the issue: the f64 evaluation against the same evaluation
in long double). The plane fit is the same QR in both; the line fit is eigh in f64, as the issue sets, and a cyclic Jacobi in long double, since numpy
has no long-double eigh: both are converged eigen solvers, so their difference is still the f64 rounding of the fit. Every association also reports its GATE MARGINS, the distance of every decision from its
threshold: |d5^2 - max_nn_dist2|, |l2 - ratio l1| / l2, min_j |plane_max_resid - |n . p_j + d||, ||r| - huber_delta|."""
import math
from fractions import Fraction

import numpy as np

LD = np.longdouble
NMOM = 34
NONE = 0xFFFFFFFF

DEFAULTS = dict(max_nn_dist2=1.0, edge_eig_ratio=3.0, edge_half_len=0.1, plane_max_resid=0.2, huber_delta=0.1, outer_passes=2, inner_iterations=4,
                min_map_edge=10, min_map_surf=50)
# LmOptions of csrc/iba_lm.hpp
LM = dict(function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16, min_radius=1e-32,
          min_relative_decrease=1e-3, min_lm_diagonal=1e-6, max_lm_diagonal=1e32)


def have_longdouble():
    """LDBL_MANT_DIG >= 64 (x87 80-bit or wider): the long-double twin says something about f64 only then"""
    return np.finfo(np.longdouble).nmant + 1 >= 64


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return o


# ---- rule 1: the query ----
if hasattr(math, "fma"):
    _fma = math.fma
else:
    def _fma(a, b, c):
        """correctly rounded a b + c (exact rational arithmetic, one rounding)"""
        return float(Fraction(a) * Fraction(b) + Fraction(c))


def transform(T, pts32):
    """lp_r = fma(T[r][2], z, fma(T[r][1], y, fma(T[r][0], x, T[r][3]))) on the widened float32 coordinates: the device's query to the bit"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x = np.asarray(pts32, np.float32).astype(np.float64).reshape(-1, 3)
    out = np.empty((len(x), 3))
    for i in range(len(x)):
        for r in range(3):
            out[i, r] = _fma(float(T[r, 2]), float(x[i, 2]), _fma(float(T[r, 1]), float(x[i, 1]), _fma(float(T[r, 0]), float(x[i, 0]), float(T[r, 3]))))
    return out


def transform_unfused(T, pts32):
    """the same rows with every operation rounded on its own (up to an ulp from the device's query: for sums, never for a decision)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x = np.asarray(pts32, np.float32).astype(np.float64).reshape(-1, 3)
    return ((x[:, 0:1] * T[:3, 0] + x[:, 1:2] * T[:3, 1]) + x[:, 2:3] * T[:3, 2]) + T[:3, 3]


# ---- rule 2: neighbours ----
def knn5(q, map32, max_nn_dist2):
    """brute force: the five map points of least (dx dx + dy dy) + dz dz, ascending by (d^2, index) -> idx [n, 5] int64, d2 [n, 5], ok [n]"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    m = np.asarray(map32, np.float32).astype(np.float64).reshape(-1, 3)
    n = len(q)
    idx = np.full((n, 5), -1, np.int64); d2 = np.full((n, 5), np.inf)
    if len(m) < 5 or n == 0:
        return idx, d2, np.zeros(n, bool)
    for i0 in range(0, n, 128):
        d = q[i0:i0 + 128, None, :] - m[None, :, :]
        dd = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        o = np.argsort(dd, axis=1, kind="stable")[:, :5]      # stable: equal distances keep ascending index order
        idx[i0:i0 + 128] = o
        d2[i0:i0 + 128] = np.take_along_axis(dd, o, axis=1)
    return idx, d2, d2[:, 4] < max_nn_dist2


# ---- rule 3: the line through five points ----
def _jacobi_eig3(Cm, dtype):
    """cyclic Jacobi on a batch of symmetric 3x3 in `dtype` -> eigenvalues [n, 3] (unsorted), eigenvectors as columns [n, 3, 3]"""
    A = np.array(Cm, dtype).copy()
    n = len(A)
    V = np.zeros((n, 3, 3), dtype); V[:, 0, 0] = V[:, 1, 1] = V[:, 2, 2] = 1
    one = dtype(1)
    for _ in range(12):
        for p, q_ in ((0, 1), (0, 2), (1, 2)):
            apq = A[:, p, q_]
            nz = apq != 0
            safe = np.where(nz, apq, one)
            with np.errstate(over="ignore"):   # (theta^2 may overflow beside a vanishing off-diagonal entry: t is then 0, as it should be)
                theta = (A[:, q_, q_] - A[:, p, p]) / (2 * safe)
                t = np.where(theta >= 0, one, -one) / (np.abs(theta) + np.sqrt(theta * theta + one))
            t = np.where(nz, t, 0 * one)
            c = one / np.sqrt(t * t + one); s = t * c
            G = np.zeros((n, 3, 3), dtype); G[:, 0, 0] = G[:, 1, 1] = G[:, 2, 2] = 1
            G[:, p, p] = c; G[:, q_, q_] = c; G[:, p, q_] = s; G[:, q_, p] = -s
            A = np.einsum("nji,njk,nkl->nil", G, A, G)
            A = (A + np.transpose(A, (0, 2, 1))) / 2
            V = np.einsum("nij,njk->nik", V, G)
    return np.stack([A[:, 0, 0], A[:, 1, 1], A[:, 2, 2]], axis=1), V


def fit_edge(P5, ratio, half_len, dtype=np.float64):
    """P5 [n, 5, 3] neighbours in order -> keep [n], a [n, 3], b [n, 3], lam [n, 3] ascending"""
    P = np.asarray(P5, np.float64).astype(dtype)
    n = len(P)
    if n == 0:
        return np.zeros(0, bool), np.zeros((0, 3), dtype), np.zeros((0, 3), dtype), np.zeros((0, 3), dtype)
    c = ((((P[:, 0] + P[:, 1]) + P[:, 2]) + P[:, 3]) + P[:, 4]) / dtype(5)
    E = P - c[:, None, :]
    Cm = np.zeros((n, 3, 3), dtype)
    for k in range(5):
        Cm = Cm + E[:, k, :, None] * E[:, k, None, :]
    if dtype == np.float64:
        lam, V = np.linalg.eigh(Cm)
    else:
        lam, V = _jacobi_eig3(Cm, dtype)
        o = np.argsort(lam, axis=1)
        lam = np.take_along_axis(lam, o, axis=1)
        V = np.take_along_axis(V, o[:, None, :], axis=2)
    u = V[:, :, 2]
    u = u / np.sqrt((u[:, 0:1] * u[:, 0:1] + u[:, 1:2] * u[:, 1:2]) + u[:, 2:3] * u[:, 2:3])
    keep = lam[:, 2] > dtype(ratio) * lam[:, 1]
    return keep, c + dtype(half_len) * u, c - dtype(half_len) * u, lam


# ---- rule 4: the plane through five points ----
def lstsq_qr(A, b, dtype=np.float64):
    """least squares by Householder QR of a batch of 5x3 systems (the device's steps) -> x [n, 3]; non-finite where rank deficient"""
    A = np.array(A, dtype).copy(); b = np.array(b, dtype).copy()
    n = len(A)
    diag = np.zeros((n, 3), dtype)
    with np.errstate(all="ignore"):
        for c in range(3):
            x = A[:, c:, c]
            nrm = np.sqrt((x * x).sum(axis=1))
            alpha = np.where(x[:, 0] >= 0, -nrm, nrm)
            v = x.copy(); v[:, 0] = v[:, 0] - alpha
            beta = (v * v).sum(axis=1)
            diag[:, c] = alpha
            for cc in range(c + 1, 3):
                f = 2 * (v * A[:, c:, cc]).sum(axis=1) / beta
                A[:, c:, cc] = A[:, c:, cc] - f[:, None] * v
            f = 2 * (v * b[:, c:]).sum(axis=1) / beta
            b[:, c:] = b[:, c:] - f[:, None] * v
        x2 = b[:, 2] / diag[:, 2]
        x1 = (b[:, 1] - A[:, 1, 2] * x2) / diag[:, 1]
        x0 = ((b[:, 0] - A[:, 0, 1] * x1) - A[:, 0, 2] * x2) / diag[:, 0]
    return np.stack([x0, x1, x2], axis=1)


def fit_surf(P5, max_resid, dtype=np.float64):
    """P5 [n, 5, 3] -> keep [n], n [n, 3], d [n], margin [n] = min_j |max_resid - |n . p_j + d||"""
    P = np.asarray(P5, np.float64).astype(dtype)
    n = len(P)
    if n == 0:
        return np.zeros(0, bool), np.zeros((0, 3), dtype), np.zeros(0, dtype), np.zeros(0, dtype)
    n0 = lstsq_qr(P, -np.ones((n, 5), dtype), dtype)
    with np.errstate(all="ignore"):
        nn = np.sqrt((n0[:, 0] * n0[:, 0] + n0[:, 1] * n0[:, 1]) + n0[:, 2] * n0[:, 2])
        d = 1 / nn
        nv = n0 / nn[:, None]
        res = np.abs(((nv[:, None, 0] * P[:, :, 0] + nv[:, None, 1] * P[:, :, 1]) + nv[:, None, 2] * P[:, :, 2]) + d[:, None])
        fine = (nn > 0) & np.isfinite(d) & np.all(np.isfinite(nv), axis=1)
        keep = fine & np.all(res <= dtype(max_resid), axis=1)
        margin = np.where(fine, np.min(np.abs(dtype(max_resid) - res), axis=1), np.inf)
    return keep, nv, d, margin


# ---- rules 2-4 and 7: the association of one pair ----
def associate(T, src_edge, src_surf, map_edge, map_surf, opt=None, dtype=np.float64):
    """-> dict(kind [n], tried [n], v [n, 7] (dtype), nn [n, 5] uint32, q [n, 3], d2 [n, 5], margins dict); the edge cloud's points first"""
    o = options(**(opt or {}))
    src_edge = np.asarray(src_edge, np.float32).reshape(-1, 3); src_surf = np.asarray(src_surf, np.float32).reshape(-1, 3)
    map_edge = np.asarray(map_edge, np.float32).reshape(-1, 3); map_surf = np.asarray(map_surf, np.float32).reshape(-1, 3)
    ne, ns = len(src_edge), len(src_surf)
    n = ne + ns
    kind = np.zeros(n, np.int32); tried = np.zeros(n, np.int32); v = np.zeros((n, 7), dtype)
    nn = np.full((n, 5), NONE, np.uint32); d2 = np.full((n, 5), np.inf)
    q = np.vstack([transform(T, src_edge), transform(T, src_surf)]) if n else np.zeros((0, 3))
    mg = dict(nn=np.inf, edge=np.inf, surf=np.inf)
    enabled = len(map_edge) > o["min_map_edge"] and len(map_surf) > o["min_map_surf"]
    if enabled:
        for lo, hi, mp, k in ((0, ne, map_edge, 1), (ne, n, map_surf, 2)):
            if hi == lo:
                continue
            idx, dd, ok = knn5(q[lo:hi], mp, o["max_nn_dist2"])
            d2[lo:hi] = dd
            if len(mp) >= 5:
                mg["nn"] = min(mg["nn"], float(np.min(np.abs(dd[:, 4] - o["max_nn_dist2"]))))
            sel = np.nonzero(ok)[0]
            tried[lo + sel] = 1
            nn[lo + sel] = idx[sel].astype(np.uint32)
            P5 = mp.astype(np.float64)[idx[sel]]
            if k == 1:
                keep, a, b, lam = fit_edge(P5, o["edge_eig_ratio"], o["edge_half_len"], dtype)
                if len(sel):
                    with np.errstate(all="ignore"):
                        mg["edge"] = min(mg["edge"], float(np.min(np.abs(lam[:, 2] - dtype(o["edge_eig_ratio"]) * lam[:, 1]) / lam[:, 2])))
                kk = lo + sel[keep]
                kind[kk] = 1; v[kk, 0:3] = a[keep]; v[kk, 3:6] = b[keep]
            else:
                keep, nv, d, margin = fit_surf(P5, o["plane_max_resid"], dtype)
                if len(sel):
                    mg["surf"] = min(mg["surf"], float(np.min(margin)))
                kk = lo + sel[keep]
                kind[kk] = 2; v[kk, 0:3] = nv[keep]; v[kk, 3] = d[keep]
    return dict(kind=kind, tried=tried, v=v, nn=nn, q=q, d2=d2, margins=mg, n_edge_pts=ne, enabled=enabled)


# ---- rules 3-6: residuals, Jacobians, sums ----
def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2], a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _norm(a):
    return np.sqrt((a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2])


def residuals(lp, kind, v):
    """lp [n, 3] transformed source points, records -> r [n], J [n, 6] (zero rows where kind == 0)"""
    lp = np.asarray(lp); dt = np.result_type(lp.dtype, np.asarray(v).dtype)
    lp = lp.astype(dt); v = np.asarray(v).astype(dt)
    n = len(lp)
    r = np.zeros(n, dt); g = np.zeros((n, 3), dt)
    e = np.nonzero(kind == 1)[0]
    if len(e):
        a, b, l = v[e, 0:3], v[e, 3:6], lp[e]
        nu = _cross(l - a, l - b); de = a - b
        den = _norm(de); nn = _norm(nu)
        r[e] = nn / den
        with np.errstate(all="ignore"):
            ge = _cross(de, nu / nn[:, None]) / den[:, None]
        g[e] = np.where(nn[:, None] > 0, ge, 0)
    s = np.nonzero(kind == 2)[0]
    if len(s):
        nv, l = v[s, 0:3], lp[s]
        r[s] = ((nv[:, 0] * l[:, 0] + nv[:, 1] * l[:, 1]) + nv[:, 2] * l[:, 2]) + v[s, 3]
        g[s] = nv
    return r, np.hstack([_cross(lp, g), g])


def moments(T, src_edge, src_surf, rec, huber_delta, dtype=np.float64):
    """the IBA_FLOAM_NMOM sums of one pair at T on the records `rec` (of associate) -> m [34], margin of the Huber knee"""
    src = np.vstack([np.asarray(src_edge, np.float32).reshape(-1, 3), np.asarray(src_surf, np.float32).reshape(-1, 3)])
    m = np.zeros(NMOM, dtype)
    if len(src) == 0:
        return m, np.inf
    lp = transform_unfused(T, src).astype(dtype)
    kind = rec["kind"]
    r, J = residuals(lp, kind, rec["v"])
    has = kind != 0
    delta = dtype(huber_delta)
    ar = np.abs(r)
    inl = ar <= delta
    with np.errstate(all="ignore"):
        w = np.where(inl, dtype(1), delta / ar)
    w = np.where(has, w, 0); rho = np.where(inl, r * r, 2 * delta * ar - delta * delta) * has
    ne = rec["n_edge_pts"]
    isE = np.arange(len(src)) < ne
    m[0] = rec["tried"][isE].sum(); m[1] = (kind[isE] == 1).sum(); m[2] = rec["tried"][~isE].sum(); m[3] = (kind[~isE] == 2).sum()
    wJ = w[:, None] * J
    o = 4
    for i in range(6):
        for j in range(i, 6):
            m[o] = (wJ[:, i] * J[:, j]).sum(); o += 1
    for i in range(6):
        m[25 + i] = (wJ[:, i] * r).sum()
    m[31] = rho.sum(); m[32] = (r * r)[has & isE].sum(); m[33] = (r * r)[has & ~isE].sum()
    margin = float(np.min(np.abs(ar[has] - delta))) if has.any() else np.inf
    return m, margin


def step(T, src_edge, src_surf, map_edge, map_surf, opt=None):
    """iba_floam_map_step of one pair -> moments [34], association dict (its margins gain 'huber')"""
    o = options(**(opt or {}))
    rec = associate(T, src_edge, src_surf, map_edge, map_surf, o)
    m, hm = moments(T, src_edge, src_surf, rec, o["huber_delta"])
    rec["margins"]["huber"] = hm
    return m, rec


# ---- rule 8 ----
def skew(w):
    return np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]], dtype=np.asarray(w).dtype)


def exp_se3(delta):
    """the reference's getTransformFromSe3 as a 4x4: the rotation of its quaternion, translation J(omega) upsilon"""
    d = np.asarray(delta, np.float64)
    om, up = d[:3], d[3:]
    theta = math.sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]); half = 0.5 * theta
    small = theta < 1e-10
    real = math.cos(half)
    if small:
        t2 = theta * theta; t4 = t2 * t2
        imag = 0.5 - 0.0208333 * t2 + 0.000260417 * t4
    else:
        imag = math.sin(half) / theta
    qw, qx, qy, qz = real, imag * om[0], imag * om[1], imag * om[2]
    tx, ty, tz = 2 * qx, 2 * qy, 2 * qz
    twx, twy, twz, txx, txy, txz, tyy, tyz, tzz = tx * qw, ty * qw, tz * qw, tx * qx, ty * qx, tz * qx, ty * qy, tz * qy, tz * qz
    R = np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    if small:
        Jm = R
    else:
        O = skew(om)
        Jm = np.eye(3) + (1 - math.cos(theta)) / (theta * theta) * O + (theta - math.sin(theta)) / (theta ** 3) * (O @ O)
    E = np.eye(4); E[:3, :3] = R; E[:3, 3] = Jm @ up
    return E


def plus(T, delta):
    """PoseSE3Parameterization::Plus: T <- Exp(delta) T"""
    Tn = exp_se3(delta) @ np.asarray(T, np.float64).reshape(4, 4)
    Tn[3] = [0, 0, 0, 1]
    return Tn


def _ldlt6(A, b):
    """A x = b by LDL^T without pivoting; None at a pivot that is not positive and finite"""
    L = np.zeros((6, 6)); d = np.zeros(6)
    for j in range(6):
        s = A[j, j] - (L[j, :j] * L[j, :j] * d[:j]).sum()
        if not (s > 0) or not np.isfinite(s):
            return None
        d[j] = s
        for i in range(j + 1, 6):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / s
    y = np.zeros(6)
    for i in range(6):
        y[i] = b[i] - (L[i, :i] * y[:i]).sum()
    x = np.zeros(6)
    for i in range(5, -1, -1):
        x[i] = y[i] / d[i] - (L[i + 1:, i] * x[i + 1:]).sum()
    return x if np.all(np.isfinite(x)) else None


def _unpack(m):
    H = np.zeros((6, 6)); o = 4
    for i in range(6):
        for j in range(i, 6):
            H[i, j] = H[j, i] = m[o]; o += 1
    return H, m[25:31].copy(), 0.5 * m[31]


def register(T0, src_edge, src_surf, map_edge, map_surf, opt=None):
    """iba_floam_map_register of one pair -> dict(T, initial_cost, final_cost, passes, iterations, evaluations, n_edge, n_surf, status)"""
    o = options(**(opt or {}))
    T = np.asarray(T0, np.float64).reshape(4, 4).copy()
    res = dict(T=T, initial_cost=0.0, final_cost=0.0, passes=0, iterations=0, evaluations=0, n_edge=0, n_surf=0, status=0)
    if not (len(map_edge) > o["min_map_edge"] and len(map_surf) > o["min_map_surf"]):
        res["status"] = 1
        return res
    for ps in range(o["outer_passes"]):
        rec = associate(T, src_edge, src_surf, map_edge, map_surf, o)
        m, _ = moments(T, src_edge, src_surf, rec, o["huber_delta"])
        H, g, cost = _unpack(m)
        res["passes"] += 1; res["evaluations"] += 1
        res["n_edge"], res["n_surf"] = int(m[1]), int(m[3])
        if ps == 0:
            res["initial_cost"] = cost
        res["final_cost"] = cost
        if m[1] + m[3] < 6:
            res["status"] = 1
            break
        radius, decrease = LM["initial_radius"], 2.0
        scale = 1.0 / (1.0 + np.sqrt(np.maximum(np.diag(H), 0.0)))
        stop = False
        for _ in range(o["inner_iterations"]):
            res["iterations"] += 1
            if np.max(np.abs(g)) <= LM["gradient_tolerance"]:
                break
            Hs = scale[:, None] * H * scale[None, :]; gs = scale * g
            A = Hs.copy()
            A[np.arange(6), np.arange(6)] += np.minimum(np.maximum(np.diag(Hs), LM["min_lm_diagonal"]), LM["max_lm_diagonal"]) / radius
            ds = _ldlt6(A, -gs)
            if ds is None:
                res["status"] = 1; stop = True
                break
            model = 0.0
            for i in range(6):
                model -= ds[i] * (gs[i] + 0.5 * float(Hs[i] @ ds))
            if not model > 0:
                radius = max(LM["min_radius"], radius / decrease); decrease *= 2
                if radius <= LM["min_radius"]:
                    break
                continue
            delta = scale * ds
            step2 = float((delta * delta).sum())
            xn2 = 1.0 + ((T[0, 3] * T[0, 3] + T[1, 3] * T[1, 3]) + T[2, 3] * T[2, 3])
            Tn = plus(T, delta)
            mn, _ = moments(Tn, src_edge, src_surf, rec, o["huber_delta"])
            Hn, gn, cn = _unpack(mn)
            res["evaluations"] += 1
            if math.sqrt(step2) <= LM["parameter_tolerance"] * (math.sqrt(xn2) + LM["parameter_tolerance"]):
                break
            if abs(cost - cn) <= LM["function_tolerance"] * cost:
                break
            rho = (cost - cn) / model
            if rho > LM["min_relative_decrease"]:
                T, H, g, cost = Tn, Hn, gn, cn
                t = 2.0 * rho - 1.0
                radius = min(LM["max_radius"], radius / max(1.0 / 3.0, 1.0 - t * t * t)); decrease = 2.0
            else:
                radius = max(LM["min_radius"], radius / decrease); decrease *= 2
                if radius <= LM["min_radius"]:
                    break
        res["final_cost"] = cost
        if stop:
            break
    res["T"] = T
    return res


# ---- rule 9 of the issue: the reference's own error, f64 against long double, per entry of the records ----
def record_yardstick(T, src_edge, src_surf, map_edge, map_surf, opt=None):
    """max over the kept records of |f64 entry - long-double entry| -> (edge yardstick over (a, b), surf yardstick over (n, d)); the kinds must agree"""
    a = associate(T, src_edge, src_surf, map_edge, map_surf, opt)
    b = associate(T, src_edge, src_surf, map_edge, map_surf, opt, dtype=LD)
    assert np.array_equal(a["kind"], b["kind"])
    return record_diff(a["kind"], a["v"], b["v"])


def record_diff(kind, v, w):
    """(edge, surf): the largest |v - w| over the entries of the records, the edges up to the swap of a and b"""
    v = np.asarray(v); w = np.asarray(w)
    dt = np.result_type(v.dtype, w.dtype)
    v = v.astype(dt); w = w.astype(dt)
    e = kind == 1; s = kind == 2
    de = 0.0
    if e.any():
        same = np.max(np.abs(v[e, :6] - w[e, :6]), axis=1)
        swap = np.max(np.abs(v[e, :6] - np.hstack([w[e, 3:6], w[e, 0:3]])), axis=1)
        de = float(np.max(np.minimum(same, swap)))
    ds = float(np.max(np.abs(v[s, :4] - w[s, :4]))) if s.any() else 0.0
    return de, ds


# ---- scenes ----
def rigid(w, t):
    """rotation vector w (rad), translation t -> 4x4"""
    T = np.eye(4)
    w = np.asarray(w, np.float64); th = float(np.linalg.norm(w))
    if th > 0:
        K = skew(w / th)
        T[:3, :3] = np.eye(3) + math.sin(th) * K + (1 - math.cos(th)) * (K @ K)
    T[:3, 3] = t
    return T


def _jgrid(rng, u0, u1, v0, v1, step):
    """a jittered grid on [u0, u1] x [v0, v1]"""
    us = np.arange(u0 + step / 2, u1, step); vs = np.arange(v0 + step / 2, v1, step)
    U, V = np.meshgrid(us, vs, indexing="ij")
    U = U + rng.uniform(-0.3, 0.3, U.shape) * step; V = V + rng.uniform(-0.3, 0.3, V.shape) * step
    return U.ravel(), V.ravel()


def room_clouds(rng, surf_step, pole_step, noise):
    """three walls, each at right angles to the next (x = 9, y = -7, x = -10: a room open towards +y), a floor z = -1.8 and four poles: planes along all
    three axes and vertical lines, so all six degrees of freedom are held -> (edge [n, 3], surf [n, 3]) f64"""
    surf = []
    u, v = _jgrid(rng, -7.0, 6.0, -1.8, 2.4, surf_step); surf.append(np.stack([np.full_like(u, 9.0), u, v], axis=1))       # wall x = 9
    u, v = _jgrid(rng, -10.0, 9.0, -1.8, 2.4, surf_step); surf.append(np.stack([u, np.full_like(u, -7.0), v], axis=1))     # wall y = -7
    u, v = _jgrid(rng, -7.0, 6.0, -1.8, 2.4, surf_step); surf.append(np.stack([np.full_like(u, -10.0), u, v], axis=1))     # wall x = -10
    u, v = _jgrid(rng, -10.0, 9.0, -7.0, 6.0, surf_step * 1.5); surf.append(np.stack([u, v, np.full_like(u, -1.8)], axis=1))   # floor
    surf = np.vstack(surf)
    edge = []
    for px, py in ((4.0, 2.0), (-5.0, 3.5), (-3.0, -4.0), (6.0, -3.0)):
        z = np.arange(-1.8 + pole_step / 2, 2.4, pole_step)
        z = z + rng.uniform(-0.3, 0.3, z.shape) * pole_step
        edge.append(np.stack([np.full_like(z, px), np.full_like(z, py), z], axis=1))
    edge = np.vstack(edge)
    return edge + rng.normal(0, noise, edge.shape), surf + rng.normal(0, noise, surf.shape)


def room_scene(seed, n_edge=300, n_surf=2000, noise=0.003):
    """-> dict(src_edge, src_surf, map_edge, map_surf float32; T_gt 4x4 scan -> map): the scan sees the same room from T_gt^-1, sampled on its own grids"""
    rng = np.random.default_rng(seed)
    map_edge, map_surf = room_clouds(rng, 0.28, 0.06, noise)
    T_gt = rigid([0.02, -0.015, 0.3], [1.2, -0.7, 0.15])
    se, ss = room_clouds(rng, 0.33, 0.05, 0.0)
    se = se[rng.permutation(len(se))[:n_edge]]; ss = ss[rng.permutation(len(ss))[:n_surf]]
    Ti = np.linalg.inv(T_gt)
    to_scan = lambda p: (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return dict(src_edge=to_scan(se), src_surf=to_scan(ss), map_edge=map_edge.astype(np.float32), map_surf=map_surf.astype(np.float32), T_gt=T_gt)


def perturbed(T_gt, seed, rot_deg=2.0, trans=0.2):
    """T_gt with a perturbation of exactly rot_deg degrees about a random axis and trans metres along a random direction"""
    rng = np.random.default_rng(seed)
    a = rng.normal(size=3); a /= np.linalg.norm(a)
    d = rng.normal(size=3); d /= np.linalg.norm(d)
    return rigid(a * math.radians(rot_deg), d * trans) @ T_gt


def pose_error(T, T_gt):
    """(rotation angle in rad, translation distance) of T T_gt^-1"""
    D = np.asarray(T) @ np.linalg.inv(T_gt)
    c = min(1.0, max(-1.0, (np.trace(D[:3, :3]) - 1) / 2))
    return math.acos(c), float(np.linalg.norm(D[:3, 3]))

"""TEST INFRASTRUCTURE: scaled point-to-point ICP as icp_calib.cpp runs it (Open3D RegistrationICP + TransformationEstimationPointToPoint(true)),
restated in numpy, f64, with two-pass centred moments — and a np.longdouble twin of the sums and of the 3x3 algebra. Imports nothing from the product.

Restated (Open3D and Eigen are not in the reference tree: parity with them is unpinned, see include/iba_mi355x.h):
  RegistrationICP                           evaluate at init; up to max_iter times: update = umeyama(q, p), T = update @ T, re-evaluate; stop when
                                            |d fitness| < relative_fitness and |d rmse| < relative_rmse
  GetRegistrationResultAndCorrespondences   nearest target per source point, kept when d^2 < r^2 (SearchHybrid = k-1 search + lower_bound: strict)
  Eigen::umeyama                            sigma = 1/n sum (p - mp)(q - mq)^T = U D V^T, S = diag(1, 1, -1) when det U det V < 0, R = U S V^T,
                                            c = tr(D S) / var_q, t = mp - c R mq
The composed T is applied to the ORIGINAL source points in every pass (the product's documented deviation from Open3D's cumulative copy).
Nearest neighbours: oracle.binding.geo_correspondences("oracle", ..) with an infinite gate (the kd search pinned to the reference's nanoflann), or
brute force on small clouds; d^2 is then re-formed as ((dx dx + dy dy) + dz dz) in f64 and the gate applied as d^2 < r^2."""
import numpy as np

LD = np.longdouble


def have_longdouble():
    """x87 80-bit (or wider): the long-double twin says something about f64 only then"""
    return np.finfo(np.longdouble).nmant >= 63


def transform(T, x):
    """q = T x in f64 (unfused; the kernel fuses three multiply-adds per row: up to an ulp apart)"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    x = np.asarray(x, np.float64).reshape(-1, 3)
    return ((x[:, 0:1] * T[:3, 0] + x[:, 1:2] * T[:3, 1]) + x[:, 2:3] * T[:3, 2]) + T[:3, 3]


def d2_of(q, p):
    d = q - p
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def nearest(q, tgt, brute=None):
    """index of the nearest target point per query (ties: lowest index) and its d^2. tgt: [m, 3] float32 values (any float dtype)."""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    tgt = np.asarray(tgt, np.float64).reshape(-1, 3)
    if len(q) == 0 or len(tgt) == 0:
        return np.zeros(len(q), np.int64) - (len(tgt) == 0), np.full(len(q), np.inf)
    if brute is None:
        brute = len(q) * len(tgt) <= 4_000_000
    if brute:
        idx = np.empty(len(q), np.int64)
        for i0 in range(0, len(q), 256):
            d = q[i0:i0 + 256, None, :] - tgt[None, :, :]
            idx[i0:i0 + 256] = np.argmin((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2], axis=1)
    else:
        from oracle import binding as ob
        s, t = ob.geo_correspondences("oracle", q, tgt, np.inf)
        assert len(s) == len(q) and np.array_equal(s, np.arange(len(q)))
        idx = t.astype(np.int64)
    return idx, d2_of(q, tgt[idx])


def second_gap(q, tgt):
    """per query: d^2 of the second nearest target minus d^2 of the nearest (scipy's kd tree picks the two, the values are re-formed here)"""
    from scipy.spatial import cKDTree
    tgt = np.asarray(tgt, np.float64)
    _, ii = cKDTree(tgt).query(q, k=2)
    a, b = d2_of(q, tgt[ii[:, 0]]), d2_of(q, tgt[ii[:, 1]])
    return np.abs(b - a)


def _jacobi_svd3(A):
    """one-sided Jacobi SVD of a 3x3 in the dtype of A (np.linalg has no long-double SVD) -> U, d, V with A = U diag(d) V^T, d descending"""
    dt = A.dtype.type
    U = A.copy(); V = np.eye(3, dtype=A.dtype)
    for _ in range(60):
        off = dt(0)
        for p in range(2):
            for q in range(p + 1, 3):
                al, be, ga = U[:, p] @ U[:, p], U[:, q] @ U[:, q], U[:, p] @ U[:, q]
                off = max(off, abs(ga) / (np.sqrt(al * be) + np.finfo(A.dtype).tiny))
                if ga == 0:
                    continue
                ze = (be - al) / (dt(2) * ga)
                t = (dt(1) if ze >= 0 else dt(-1)) / (abs(ze) + np.sqrt(dt(1) + ze * ze))
                c = dt(1) / np.sqrt(dt(1) + t * t); s = c * t
                up = U[:, p].copy(); U[:, p] = c * up - s * U[:, q]; U[:, q] = s * up + c * U[:, q]
                vp = V[:, p].copy(); V[:, p] = c * vp - s * V[:, q]; V[:, q] = s * vp + c * V[:, q]
        if off < np.finfo(A.dtype).eps:
            break
    d = np.sqrt((U * U).sum(0))
    order = np.argsort(-d)
    U, V, d = U[:, order], V[:, order], d[order]
    Un = np.zeros_like(U)
    for k in range(3):
        if d[k] > np.finfo(A.dtype).tiny:
            Un[:, k] = U[:, k] / d[k]
    if not d[2] > d[0] * np.finfo(A.dtype).eps:   # rank 2: complete the basis
        Un[:, 2] = np.cross(Un[:, 0], Un[:, 1]); Un[:, 2] /= np.sqrt(Un[:, 2] @ Un[:, 2])
    return Un, d, V


def _det3(M):
    return (M[0, 0] * (M[1, 1] * M[2, 2] - M[1, 2] * M[2, 1]) - M[0, 1] * (M[1, 0] * M[2, 2] - M[1, 2] * M[2, 0])
            + M[0, 2] * (M[1, 0] * M[2, 1] - M[1, 1] * M[2, 0]))


def umeyama(q, p, with_scaling=True, dtype=np.float64, info=None):
    """Eigen::umeyama(src = q, dst = p): 4x4 of `dtype` with upper-left c R. Two-pass centred moments. info (dict): receives 'reflect', 'c'."""
    q = np.asarray(q, dtype); p = np.asarray(p, dtype)
    n = dtype(len(q))
    mq, mp = q.sum(0) / n, p.sum(0) / n
    dq, dp = q - mq, p - mp
    var_q = (dq * dq).sum() / n
    sigma = (dp.T @ dq) / n
    if dtype is np.float64:
        U, d, Vt = np.linalg.svd(sigma); V = Vt.T
    else:
        U, d, V = _jacobi_svd3(sigma)
    S = np.ones(3, dtype)
    if _det3(U) * _det3(V) < 0:
        S[2] = -1
    R = (U * S) @ V.T
    c = (d * S).sum() / var_q if with_scaling else dtype(1)
    T = np.eye(4, dtype=dtype)
    T[:3, :3] = c * R
    T[:3, 3] = mp - c * (R @ mq)
    if info is not None:
        info["reflect"] = bool(S[2] < 0); info["c"] = float(c)
    return T


def moments(q, p, d2, pivot, dtype=np.float64):
    """the moment block of iba_icp_step (include/iba_mi355x.h) over the given kept pairs, sums in `dtype`"""
    q = np.asarray(q, np.float64); p = np.asarray(p, np.float64); v = np.asarray(pivot, np.float64)
    dq, dp = (q - v).astype(dtype), (p - v).astype(dtype)   # (the differences are formed in f64, as the kernel forms them)
    m = np.zeros(21, dtype)
    m[0] = len(q); m[1] = np.asarray(d2, np.float64).astype(dtype).sum()
    m[2:5] = dq.sum(0); m[5:8] = dp.sum(0)
    dqq = (np.asarray(q - v) ** 2)
    m[8] = ((dqq[:, 0] + dqq[:, 1]) + dqq[:, 2]).astype(dtype).sum()
    for i in range(3):
        for j in range(3):
            m[9 + 3 * i + j] = ((p - v)[:, i] * (q - v)[:, j]).astype(dtype).sum()   # each product rounded to f64 first, as on the device
    m[18:21] = v
    return m


def evaluate(T, src, tgt, gate, brute=None):
    """one pass: -> dict(idx, d2, keep, n, fitness, rmse, q)"""
    q = transform(T, src)
    idx, d2 = nearest(q, tgt, brute)
    keep = d2 < gate * gate
    n = int(keep.sum())
    return dict(q=q, idx=idx, d2=d2, keep=keep, n=n, fitness=n / max(len(src), 1), rmse=float(np.sqrt(d2[keep].sum() / n)) if n else 0.0)


def register(src, tgt, T_init, gate, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, with_scaling=True, dtype=np.float64, brute=None, trace=None, margins=False):
    """RegistrationICP. The SETS are always found in f64 from the f64 rounding of T (so that the f64 and the long-double run see the same pairs as
    long as no margin is touched); the moments, the Umeyama step and T = update @ T run in `dtype`.
    -> dict(T, n_corr, iterations, converged (1 criteria, 0 max_iter, -1 fewer than 3 pairs), fitness, rmse, counts [per evaluation],
            gate_margin, gap (over all evaluations, when margins=True))"""
    src = np.asarray(src, np.float64); tgtd = np.asarray(tgt, np.float64)
    T = np.asarray(T_init, dtype).reshape(4, 4).copy()
    out = dict(counts=[], gate_margin=np.inf, gap=np.inf)

    def ev(T):
        e = evaluate(np.asarray(T, np.float64), src, tgtd, gate, brute)
        out["counts"].append(e["n"])
        if margins:
            out["gate_margin"] = min(out["gate_margin"], float(np.min(np.abs(e["d2"] - gate * gate))))
            out["gap"] = min(out["gap"], float(np.min(second_gap(e["q"], tgtd))))
        if trace is not None:
            trace.append(e)
        return e

    e = ev(T)
    it, conv = 0, 0
    for _ in range(max_iter):
        if e["n"] < 3:
            conv = -1
            break
        k = e["keep"]
        U = umeyama(transform_any(T, src[k], dtype), tgtd[e["idx"][k]], with_scaling, dtype)
        T = U @ T
        e2 = ev(T)
        it += 1
        done = abs(e["fitness"] - e2["fitness"]) < rel_fitness and abs(e["rmse"] - e2["rmse"]) < rel_rmse
        e = e2
        if done:
            conv = 1
            break
    if conv == 0 and e["n"] < 3:
        conv = -1
    out.update(T=T, n_corr=e["n"], iterations=it, converged=conv, fitness=e["fitness"], rmse=e["rmse"])
    return out


def transform_any(T, x, dtype):
    T = np.asarray(T, dtype); x = np.asarray(x, dtype)
    return x @ T[:3, :3].T + T[:3, 3]


# ---- the conventions of icp_calib.cpp:55-71 ----
def init_from_sim3(rigid34, scale):
    """readSim3 form -> the init of the loop: (R^T, -R^T t), rotation times the scale"""
    R, t = np.asarray(rigid34, np.float64).reshape(3, 4)[:, :3], np.asarray(rigid34, np.float64).reshape(3, 4)[:, 3]
    T = np.eye(4); T[:3, :3] = R.T * scale; T[:3, 3] = -R.T @ t
    return T


def sim3_from_result(T):
    """the loop's result -> (rigid 3x4, scale) as writeSim3 takes them: scale = sqrt((A A^T)_00), A / scale, inverse"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    A = T[:3, :3]
    s = float(np.sqrt((A @ A.T)[0, 0]))
    R = A / s
    out = np.zeros((3, 4)); out[:, :3] = R.T; out[:, 3] = -R.T @ T[:3, 3]
    return out, s


# ---- the seeded scene of the loop tests: a street canyon (ground, two walls, a dozen boxes) ----
def canyon(seed, n_tgt=20000, n_src=3000, c=9.7, noise=0.02):
    """-> (tgt float32 [n_tgt, 3], src f64 [n_src, 3], T_planted 4x4 with T_planted @ src ~ tgt subset)"""
    rng = np.random.default_rng(seed)
    n_g, n_w = int(n_tgt * 0.4), int(n_tgt * 0.2)
    n_b = n_tgt - n_g - 2 * n_w
    g = np.c_[rng.uniform(-30, 30, n_g), rng.uniform(-8, 8, n_g), rng.normal(0, 0.01, n_g) - 1.7]
    w1 = np.c_[rng.uniform(-30, 30, n_w), np.full(n_w, 8.0) + rng.normal(0, 0.01, n_w), rng.uniform(-1.7, 6, n_w)]
    w2 = np.c_[rng.uniform(-30, 30, n_w), np.full(n_w, -8.0) + rng.normal(0, 0.01, n_w), rng.uniform(-1.7, 6, n_w)]
    boxes = []
    per = n_b // 12
    for k in range(12):
        m = per if k < 11 else n_b - 11 * per
        ctr = np.array([rng.uniform(-28, 28), rng.uniform(-6, 6), -1.7]); sz = rng.uniform(0.8, 2.5, 3)
        u = rng.uniform(-0.5, 0.5, (m, 3)); face = rng.integers(0, 3, m); sgn = rng.choice([-0.5, 0.5], m)
        u[np.arange(m), face] = sgn
        b = ctr + u * sz; b[:, 2] += sz[2] / 2
        boxes.append(b)
    tgt = np.concatenate([g, w1, w2] + boxes).astype(np.float32)
    pick = rng.choice(len(tgt), n_src, replace=False)
    near = tgt[pick].astype(np.float64) + rng.normal(0, noise, (n_src, 3))
    w = rng.normal(size=3); w *= 0.3 / np.linalg.norm(w)
    R = rotvec(w); t = rng.uniform(-1, 1, 3)
    Tp = np.eye(4); Tp[:3, :3] = c * R; Tp[:3, 3] = t
    src = (near - t) @ R / c   # = (c R)^-1 (near - t)
    return tgt, src, Tp


def rotvec(w):
    w = np.asarray(w, np.float64); th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th; K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def perturb(Tp, rng, rot=(2e-3, 2.5e-3), trans=(0.02, 0.04), scale=0.003):
    """a start rot rad, trans m and `scale` (relative) off the planted transform"""
    w = rng.normal(size=3); w *= rng.uniform(*rot) / np.linalg.norm(w)
    d = rng.normal(size=3); d *= rng.uniform(*trans) / np.linalg.norm(d)
    P = np.eye(4); P[:3, :3] = (1 + scale) * rotvec(w); P[:3, 3] = d
    return P @ Tp

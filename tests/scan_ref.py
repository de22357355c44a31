"""TEST INFRASTRUCTURE: scan-to-scan ICP edges (iba_scan_*, include/iba_mi355x.h) restated in numpy on top of tests/icp_ref.py — the point-to-plane
step, the information matrix and the one- / two-stage loop, in f64 and with an np.longdouble twin of the sums and of the 6x6 algebra. Imports
nothing from the product.

Restated (Open3D is not in the reference tree: parity with it is unpinned):
  TransformationEstimationPointToPlane   per kept pair (q = T x, target p, unit normal n): r = (q - p) . n, J = [q x n, n]; JtJ x = -Jtr by LDL^T;
                                         update = Rz(x2) Ry(x1) Rx(x0) with translation x[3:6]; T = update @ T
  GetInformationMatrixFromPointClouds    sum G^T G over the kept pairs, G = [-[t]x | I], t the target point
  RegistrationICP                        icp_ref.register's loop; coarse -> refine: the refine stage starts from the coarse stage's T
The product's rules, restated with it: a target point without a normal (has[i] False) keeps its pair in fitness / rmse and adds nothing to
JtJ / Jtr; an update needs at least 6 pairs with a normal and LDL^T pivots that are positive and, within the rotation and the translation block
each, not below 1e-12 of the block's largest."""
import numpy as np

import icp_ref as R

LD = np.longdouble
P2P, P2L, INFO = 0, 1, 2
NMOM = 32


def vec6_to_mat4(x, dtype=np.float64):
    """Open3D TransformVector6dToMatrix4d: Rz(x2) @ Ry(x1) @ Rx(x0), translation x[3:6]"""
    x = np.asarray(x, dtype)
    ca, sa, cb, sb, cg, sg = np.cos(x[0]), np.sin(x[0]), np.cos(x[1]), np.sin(x[1]), np.cos(x[2]), np.sin(x[2])
    U = np.eye(4, dtype=dtype)
    U[0, :3] = [cg * cb, cg * sb * sa - sg * ca, cg * sb * ca + sg * sa]
    U[1, :3] = [sg * cb, sg * sb * sa + cg * ca, sg * sb * ca - cg * sa]
    U[2, :3] = [-sb, cb * sa, cb * ca]
    U[:3, 3] = x[3:6]
    return U


def ldlt6_solve(A, b):
    """A x = b by LDL^T without pivoting in the dtype of A; None when the product's pivot rule calls the system singular"""
    dt = A.dtype.type
    n = 6
    L = np.zeros((n, n), A.dtype); d = np.zeros(n, A.dtype)
    for j in range(n):
        s = A[j, j] - (L[j, :j] * L[j, :j] * d[:j]).sum()
        if not (s > 0) or not np.isfinite(s):
            return None
        d[j] = s
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / s
    y = np.zeros(n, A.dtype)
    for i in range(n):
        y[i] = b[i] - (L[i, :i] * y[:i]).sum()
    x = np.zeros(n, A.dtype)
    for i in range(n - 1, -1, -1):
        x[i] = y[i] / d[i] - (L[i + 1:, i] * x[i + 1:]).sum()
    if not np.all(np.isfinite(x)):
        return None
    for blk in (slice(0, 3), slice(3, 6)):
        if not d[blk].min() > dt(1e-12) * d[blk].max():
            return None
    return x


def p2l_sums(q, p, n, has, d2, dtype=np.float64):
    """the point-to-plane sums of iba_scan_step over the given kept pairs (layout: include/iba_mi355x.h); products in f64 as on the device, sums in dtype"""
    q = np.asarray(q, np.float64); p = np.asarray(p, np.float64); n = np.asarray(n, np.float64); has = np.asarray(has, bool)
    m = np.zeros(NMOM, dtype)
    m[0] = len(q); m[1] = np.asarray(d2, np.float64).astype(dtype).sum(); m[2] = int(has.sum())
    q, p, n = q[has], p[has], n[has]
    d = q - p
    r = (d[:, 0] * n[:, 0] + d[:, 1] * n[:, 1]) + d[:, 2] * n[:, 2]
    J = np.c_[q[:, 1] * n[:, 2] - q[:, 2] * n[:, 1], q[:, 2] * n[:, 0] - q[:, 0] * n[:, 2], q[:, 0] * n[:, 1] - q[:, 1] * n[:, 0], n]
    o = 3
    for i in range(6):
        for j in range(i, 6):
            m[o] = (J[:, i] * J[:, j]).astype(dtype).sum(); o += 1
    for i in range(6):
        m[24 + i] = (J[:, i] * r).astype(dtype).sum()
    m[30] = (r * r).astype(dtype).sum()
    return m


def p2l_update(m):
    """the update of one point-to-plane step from its sums (in their dtype), or None"""
    if not m[2] >= 6:
        return None
    A = np.zeros((6, 6), m.dtype); o = 3
    for i in range(6):
        for j in range(i, 6):
            A[i, j] = A[j, i] = m[o]; o += 1
    if not np.all(np.isfinite(A)):
        return None
    x = ldlt6_solve(A, -m[24:30])
    return None if x is None else vec6_to_mat4(x, m.dtype.type)


def info_sums(t, dtype=np.float64):
    t = np.asarray(t, np.float64).reshape(-1, 3)
    m = np.zeros(NMOM, dtype)
    m[0] = len(t); m[1:4] = t.astype(dtype).sum(0)
    o = 4
    for i in range(3):
        for j in range(i, 3):
            m[o] = (t[:, i] * t[:, j]).astype(dtype).sum(); o += 1
    return m


def info_from_sums(s):
    n, tx, ty, tz, xx, xy, xz, yy, yz, zz = s[:10]
    z = s.dtype.type(0)
    return np.array([[yy + zz, -xy, -xz, z, -tz, ty], [-xy, xx + zz, -yz, tz, z, -tx], [-xz, -yz, xx + yy, -ty, tx, z],
                     [z, tz, -ty, n, z, z], [-tz, z, tx, z, n, z], [ty, -tx, z, z, z, n]], s.dtype)


def information(t, dtype=np.float64):
    """the definition itself: sum of G^T G, pair by pair"""
    I = np.zeros((6, 6), dtype)
    for tx, ty, tz in np.asarray(t, dtype).reshape(-1, 3):
        G = np.array([[0, tz, -ty, 1, 0, 0], [-tz, 0, tx, 0, 1, 0], [ty, -tx, 0, 0, 0, 1]], dtype)
        I += G.T @ G
    return I


def p2p_sums(q, p, d2, pivot, dtype=np.float64):
    m = np.zeros(NMOM, dtype)
    m[:21] = R.moments(q, p, d2, pivot, dtype)
    return m


def register(src, tgt, T_init, gate, estimation=P2P, normals=None, has=None, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6, dtype=np.float64, brute=None, margins=False):
    """one stage of RegistrationICP on an edge. Point-to-point: icp_ref.register without scaling. Point-to-plane: the same loop with p2l_update;
    the SETS are found in f64 from the f64 rounding of T, the sums, the solve and T = update @ T run in dtype.
    -> icp_ref.register's dict (+ n_planar under point-to-plane)"""
    if estimation == P2P:
        return R.register(src, tgt, T_init, gate, max_iter, rel_fitness, rel_rmse, False, dtype, brute, None, margins)
    src = np.asarray(src, np.float64); tgtd = np.asarray(tgt, np.float64)
    T = np.asarray(T_init, dtype).reshape(4, 4).copy()
    out = dict(counts=[], gate_margin=np.inf, gap=np.inf)

    def ev(T):
        e = R.evaluate(np.asarray(T, np.float64), src, tgtd, gate, brute)
        out["counts"].append(e["n"])
        if margins:
            out["gate_margin"] = min(out["gate_margin"], float(np.min(np.abs(e["d2"] - gate * gate))))
            out["gap"] = min(out["gap"], float(np.min(R.second_gap(e["q"], tgtd))))
        return e

    def sums(T, e):
        k = e["keep"]; idx = e["idx"][k]
        q = np.asarray(R.transform_any(T, src[k], dtype))
        # (the pair terms are products of f64 roundings on the device; the long-double twin keeps q in long double: it is the truth of the STEP)
        if dtype is np.float64:
            return p2l_sums(q, tgtd[idx], normals[idx], has[idx], e["d2"][k], dtype)
        return _p2l_sums_wide(q, tgtd[idx].astype(dtype), np.asarray(normals, np.float64)[idx].astype(dtype), np.asarray(has, bool)[idx], e["d2"][k], dtype)

    e = ev(T)
    it, conv = 0, 0
    m = sums(T, e)
    for _ in range(max_iter):
        U = p2l_update(m)
        if U is None:
            conv = -1
            break
        T = U @ T
        e2 = ev(T)
        m = sums(T, e2)
        it += 1
        done = abs(e["fitness"] - e2["fitness"]) < rel_fitness and abs(e["rmse"] - e2["rmse"]) < rel_rmse
        e = e2
        if done:
            conv = 1
            break
    if conv == 0 and e["n"] < 3:
        conv = -1
    out.update(T=T, n_corr=e["n"], iterations=it, converged=conv, fitness=e["fitness"], rmse=e["rmse"], n_planar=int(m[2]))
    return out


def _p2l_sums_wide(q, p, n, has, d2, dtype):
    m = np.zeros(NMOM, dtype)
    m[0] = len(q); m[1] = np.asarray(d2, dtype).sum(); m[2] = int(has.sum())
    q, p, n = q[has], p[has], n[has]
    r = ((q - p) * n).sum(1)
    J = np.concatenate([np.cross(q, n), n], axis=1)
    o = 3
    for i in range(6):
        for j in range(i, 6):
            m[o] = (J[:, i] * J[:, j]).sum(); o += 1
    for i in range(6):
        m[24 + i] = (J[:, i] * r).sum()
    m[30] = (r * r).sum()
    return m


def register_two_stage(src, tgt, T_init, coarse, refine, **kw):
    """coarse, refine: dict(gate, max_iter, rel_fitness, rel_rmse); the refine stage starts from the coarse stage's T -> the refine stage's dict"""
    a = register(src, tgt, T_init, coarse["gate"], max_iter=coarse["max_iter"], rel_fitness=coarse["rel_fitness"], rel_rmse=coarse["rel_rmse"], **kw)
    return register(src, tgt, a["T"], refine["gate"], max_iter=refine["max_iter"], rel_fitness=refine["rel_fitness"], rel_rmse=refine["rel_rmse"], **kw)


# ---- seeded scenes ----
def rigid(w, t):
    T = np.eye(4); T[:3, :3] = R.rotvec(w); T[:3, 3] = t
    return T


def perturb_rigid(T, rng, rot=(2e-3, 4e-3), trans=(0.02, 0.05)):
    """a start a few mrad and a few cm off T"""
    return R.perturb(T, rng, rot=rot, trans=trans, scale=0.0)


def _faces(seed):
    """(centre, u, v, half extent along u, along v) of the faces of a room seen from inside: floor, ceiling, four walls, three boxes"""
    rng = np.random.default_rng(seed)
    faces = [((0, 0, -1.5), (1, 0, 0), (0, 1, 0), 12, 8), ((0, 0, 2.5), (1, 0, 0), (0, 1, 0), 12, 8), ((0, 8, 0.5), (1, 0, 0), (0, 0, 1), 12, 2),
             ((0, -8, 0.5), (1, 0, 0), (0, 0, 1), 12, 2), ((12, 0, 0.5), (0, 1, 0), (0, 0, 1), 8, 2), ((-12, 0, 0.5), (0, 1, 0), (0, 0, 1), 8, 2)]
    for _ in range(3):
        c = np.array([rng.uniform(-9, 9), rng.uniform(-6, 6), -1.5]); s = rng.uniform(0.8, 2.0, 3)
        faces += [((c[0] + s[0], c[1], c[2] + s[2]), (0, 1, 0), (0, 0, 1), s[1], s[2]), ((c[0] - s[0], c[1], c[2] + s[2]), (0, 1, 0), (0, 0, 1), s[1], s[2]),
                  ((c[0], c[1] + s[1], c[2] + s[2]), (1, 0, 0), (0, 0, 1), s[0], s[2]), ((c[0], c[1] - s[1], c[2] + s[2]), (1, 0, 0), (0, 0, 1), s[0], s[2]),
                  ((c[0], c[1], c[2] + 2 * s[2]), (1, 0, 0), (0, 1, 0), s[0], s[1])]
    return faces


def room(seed, n=12000, noise=0.01, sampling=0):
    """`n` points on the faces of room `seed` (sampling: which independent sampling of them) -> (points [n, 3] f64, true unit normals [n, 3])"""
    faces = _faces(seed)
    rng = np.random.default_rng([seed, sampling, 7919])
    area = np.array([f[3] * f[4] for f in faces]); cnt = np.floor(n * area / area.sum()).astype(int); cnt[0] += n - cnt.sum()
    pts, nrm = [], []
    for (c, u, v, a, b), m in zip(faces, cnt):
        u = np.asarray(u, float); v = np.asarray(v, float); w = np.cross(u, v)
        pts.append(np.asarray(c, float) + rng.uniform(-a, a, (m, 1)) * u + rng.uniform(-b, b, (m, 1)) * v + rng.normal(0, noise, (m, 1)) * w)
        nrm.append(np.tile(w, (m, 1)))
    return np.concatenate(pts), np.concatenate(nrm)


def room_pair(seed, n=12000, noise=0.01, w=(0.01, -0.02, 0.03), t=(0.25, -0.1, 0.05)):
    """two scans of one room from two poses, the surfaces sampled independently (as two sweeps of a LiDAR do: no source point has an exact
    partner) -> (src float32 [n, 3], tgt float32 [n, 3], T_true 4x4 with T_true @ src on the target's surfaces)"""
    T = rigid(np.asarray(w, float), np.asarray(t, float))
    tgt = room(seed, n, noise, 0)[0].astype(np.float32)
    Ti = np.linalg.inv(T)
    src = (room(seed, n, noise, 1)[0] @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    return src, tgt, T


def pca_normals(pts, radius=0.6, max_pts=30, min_pts=5):
    """a plain restatement of the plane memo for CHOOSING test inputs on the CPU (never compared with the device): per point the unit eigenvector of the
    smallest eigenvalue of the covariance of its at most max_pts nearest neighbours inside radius (itself included) -> (normals [n, 3], has [n])"""
    from scipy.spatial import cKDTree
    pts = np.asarray(pts, np.float64)
    d, ii = cKDTree(pts).query(pts, k=min(max_pts, len(pts)), distance_upper_bound=radius)
    ok = np.isfinite(d) & (d * d < radius * radius)
    nrm = np.zeros((len(pts), 3)); has = ok.sum(1) >= max(min_pts, 3)
    for i in np.nonzero(has)[0]:
        nb = pts[ii[i][ok[i]]]
        c = nb - nb.mean(0)
        nrm[i] = np.linalg.eigh(c.T @ c)[1][:, 0]
    return nrm, has

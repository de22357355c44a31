"""The rules Z1-Z8 of the Sim3 RANSAC (include/iba_mi355x.h, iba_sim3*) restated in numpy, SEQUENTIALLY as the reference's Sim3Solver runs: the
constructor's preparation, then iterate() one iteration at a time with the best kept as state. float32 wherever the reference holds a float; a
cv::Mat operation is float64 on the widened entries with one rounding per element. Every scalar is an explicit numpy type, so no Python float
decides a precision."""
import math

import numpy as np

F, D = np.float32, np.float64
OK, NO_MORE, TOO_FEW = range(3)
MAX_SWEEPS = 30
PAIRS = ((0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3))
NAN = F(np.nan)


def canon(a):
    """NaNs as the one quiet NaN the library stores"""
    a = np.array(a, F)
    a[np.isnan(a)] = np.frombuffer(np.uint32(0x7FC00000).tobytes(), F)[0]
    return a


def dot3(a, b):
    return F((D(a[0]) * D(b[0]) + D(a[1]) * D(b[1])) + D(a[2]) * D(b[2]))


def to_camera(T, X):
    """Z2: T [3, 4] f32, X [N, 3] f32 -> [N, 3] f32, L1's order of sums in float32"""
    T, X = np.asarray(T, F).reshape(3, 4), np.asarray(X, F).reshape(-1, 3)
    return np.stack([((T[i, 0] * X[:, 0] + T[i, 1] * X[:, 1]) + T[i, 2] * X[:, 2]) + T[i, 3] for i in range(3)], axis=1).astype(F)


def to_image(K, c):
    """Z2: K = (fx, fy, cx, cy), c [N, 3] f32 -> u, v [N] f32; no test on z"""
    K = np.asarray(K, F)
    with np.errstate(all="ignore"):
        invz = (D(1.0) / c[:, 2].astype(D)).astype(F)
        return K[0] * (c[:, 0] * invz) + K[2], K[1] * (c[:, 1] * invz) + K[3]


def budget(N, probability=0.99, min_inliers=20, max_iterations=300):
    """Z6, with the host's libm through math"""
    if N == min_inliers:
        return 1
    eps = F(min_inliers) / F(N)
    try:
        q = math.log(1.0 - probability) / math.log(1.0 - math.pow(float(eps), 3))
    except (ZeroDivisionError, ValueError):
        return max_iterations
    if not math.isfinite(q):
        return max_iterations
    return max(1, min(int(math.ceil(q)), max_iterations)) if math.ceil(q) < 2 ** 31 else max_iterations


def truncated_threshold(sigma2):
    """Z1: (size_t)(9.210 * sigma2) as a float32"""
    return F(int(D(9.210) * D(F(sigma2))))


def jacobi_max_eigenvector(N4):
    """Z3: N4 = the 4 x 4 float32 matrix -> (the quaternion as 4 float32, the sweeps that rotated)"""
    A, V = np.array(N4, D), np.eye(4, dtype=D)
    sweep = 0
    with np.errstate(all="ignore"):
        while sweep < MAX_SWEEPS:
            rotated = 0
            for p, q in PAIRS:
                apq, app, aqq = A[p, q], A[p, p], A[q, q]
                if abs(apq) <= D(2.0 ** -53) * (abs(app) + abs(aqq)):
                    continue
                theta = (aqq - app) / (D(2.0) * apq)
                t = (D(1.0) if theta >= 0 else D(-1.0)) / (abs(theta) + np.sqrt(D(1.0) + theta * theta))
                c = D(1.0) / np.sqrt(D(1.0) + t * t)
                s = c * t
                for M in (A, V):
                    xp, xq = M[:, p].copy(), M[:, q].copy()
                    M[:, p], M[:, q] = c * xp - s * xq, s * xp + c * xq
                xp, xq = A[p, :].copy(), A[q, :].copy()
                A[p, :], A[q, :] = c * xp - s * xq, s * xp + c * xq
                A[p, q] = A[q, p] = D(0.0)
                rotated += 1
            if not rotated:
                break
            sweep += 1
    best = 0
    for c in range(1, 4):
        if A[c, c] > A[best, best]:
            best = c
    return V[:, best].astype(F), sweep


def rotation_from_quaternion(q):
    """Z4: q = (w, x, y, z) float32 -> (R [3, 3] f32, dead)"""
    w, x, y, z = (D(v) for v in q)
    with np.errstate(all="ignore"):
        vn = np.sqrt((x * x + y * y) + z * z)
        dead = not (vn > 0) or not np.isfinite(vn)
        n = ((w * w + x * x) + y * y) + z * z
        one, two = D(1.0), D(2.0)
        R = [one - two * (y * y + z * z) / n, two * (x * y - w * z) / n, two * (x * z + w * y) / n,
             two * (x * y + w * z) / n, one - two * (x * x + z * z) / n, two * (y * z - w * x) / n,
             two * (x * z - w * y) / n, two * (y * z + w * x) / n, one - two * (x * x + y * y) / n]
    return np.array(R, D).astype(F).reshape(3, 3), dead


def horn_matrix(P1, P2):
    """Z3 up to N: P1, P2 [3, 3] f32 with the points as COLUMNS -> (O1, O2, Pr1, Pr2, N4)"""
    P1, P2 = np.asarray(P1, F), np.asarray(P2, F)
    O, Pr = [], []
    for P in (P1, P2):
        s = np.array([F((D(P[r, 0]) + D(P[r, 1])) + D(P[r, 2])) for r in range(3)], F)
        o = (s.astype(D) / D(3.0)).astype(F)
        O.append(o)
        Pr.append((P - o[:, None]).astype(F))
    M = np.array([[dot3(Pr[1][i, :], Pr[0][j, :]) for j in range(3)] for i in range(3)], D)
    N11, N12, N13, N14 = (M[0, 0] + M[1, 1]) + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
    N22, N23, N24 = (M[0, 0] - M[1, 1]) - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
    N33, N34, N44 = (-M[0, 0] + M[1, 1]) - M[2, 2], M[1, 2] + M[2, 1], (-M[0, 0] - M[1, 1]) + M[2, 2]
    N4 = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]], D).astype(F)
    return O[0], O[1], Pr[0], Pr[1], N4


def horn(P1, P2, fix_scale=False, rotation=rotation_from_quaternion):
    """Z3 / Z4 -> dict: s f32, R [3, 3], t [3], T12, T21 [3, 4] f32 (NaNs canonical), sweeps"""
    O1, O2, Pr1, Pr2, N4 = horn_matrix(P1, P2)
    q, sweeps = jacobi_max_eigenvector(N4)
    R, dead = rotation(q)
    if dead:
        nan = canon(np.full(12, np.nan))
        return {"s": nan[0], "R": nan[:9].reshape(3, 3), "t": nan[:3], "T12": nan.reshape(3, 4), "T21": nan.reshape(3, 4).copy(), "sweeps": sweeps, "q": q}
    with np.errstate(all="ignore"):
        s = F(1.0)
        if not fix_scale:
            nom, den = D(0.0), D(0.0)
            for i in range(3):
                for j in range(3):
                    p3 = dot3(R[i, :], Pr2[:, j])
                    nom = nom + D(Pr1[i, j]) * D(p3)
                    den = den + D(F(p3 * p3))
            s = F(nom / den)
        sR = (s * R).astype(F)
        t = np.array([O1[i] - dot3(sR[i, :], O2) for i in range(3)], F)
        inv_s = D(1.0) / D(s)
        Ri = np.array([[F(inv_s * D(R[j, i])) for j in range(3)] for i in range(3)], F)
        ti = np.array([-dot3(Ri[i, :], t) for i in range(3)], F)
    return {"s": canon(s)[()], "R": canon(R), "t": canon(t), "T12": canon(np.concatenate([sR, t[:, None]], axis=1)), "T21": canon(np.concatenate([Ri, ti[:, None]], axis=1)),
            "sweeps": sweeps, "q": q}


def reproject_err(T, K, c, u0, v0):
    """Z5, one direction: T [3, 4], c [N, 3] the points in the other camera, (u0, v0) the image points here -> err [N] f32"""
    with np.errstate(all="ignore"):
        cd = c.astype(D)
        p = np.stack([((D(T[i, 0]) * cd[:, 0] + D(T[i, 1]) * cd[:, 1]) + D(T[i, 2]) * cd[:, 2]).astype(F) + T[i, 3] for i in range(3)], axis=1).astype(F)
        u, v = to_image(K, p)
        d0, d1 = (u0 - u).astype(D), (v0 - v).astype(D)
        return (d0 * d0 + d1 * d1).astype(F)


class Solver:
    """Sim3Solver over one job: the constructor (Z2), SetRansacParameters (Z6) and iterate (Z3-Z5, Z7) with the reference's state"""

    def __init__(self, xyz, job, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=0, rotation=rotation_from_quaternion):
        xyz = np.asarray(xyz, F).reshape(-1, 3)
        self.job, self.min_inliers, self.fix_scale, self.rotation = job, min_inliers, fix_scale, rotation
        self.N = len(job["point1"])
        self.c1, self.c2 = to_camera(job["Tcw1"], xyz[job["point1"]]), to_camera(job["Tcw2"], xyz[job["point2"]])
        self.u1, self.v1 = to_image(job["K1"], self.c1)
        self.u2, self.v2 = to_image(job["K2"], self.c2)
        self.e1, self.e2 = np.asarray(job["max_err1"], F), np.asarray(job["max_err2"], F)
        self.too_few = self.N < min_inliers
        self.max_its = 0 if self.too_few else budget(self.N, probability, min_inliers, max_iterations)
        self.n_iterations, self.best_inliers, self.best_it, self.best = 0, 0, -1, None
        self.counts, self.hyps, self.inliers, self.events = [], [], [], []

    def hypothesis(self, it):
        idx = np.asarray(self.job["sets"], np.int32).reshape(-1, 3)[it]
        return horn(self.c1[idx].T, self.c2[idx].T, self.fix_scale, self.rotation)

    def check_inliers(self, h):
        K1, K2 = np.asarray(self.job["K1"], F), np.asarray(self.job["K2"], F)
        err1 = reproject_err(h["T12"], K1, self.c2, self.u1, self.v1)
        err2 = reproject_err(h["T21"], K2, self.c1, self.u2, self.v2)
        with np.errstate(all="ignore"):
            return ((err1 < self.e1) & (err2 < self.e2)).astype(np.uint8)

    def iterate(self, n):
        """-> (event, no_more): event = None or the dict of the iteration that returned"""
        if self.too_few:
            return None, True
        current = 0
        while self.n_iterations < self.max_its and current < n:
            current += 1
            it = self.n_iterations
            self.n_iterations += 1
            h = self.hypothesis(it)
            inl = self.check_inliers(h)
            cnt = int(inl.sum())
            self.counts.append(cnt)
            self.hyps.append(h)
            self.inliers.append(inl)
            if cnt >= self.best_inliers:
                self.best_inliers, self.best_it, self.best = cnt, it, (h, inl)
                if cnt > self.min_inliers:
                    e = {"iteration": it, "n_inliers": cnt, "s": h["s"], "R": h["R"].reshape(-1), "t": h["t"], "inlier": inl}
                    self.events.append(e)
                    return e, False
        return None, self.n_iterations >= self.max_its


def run(xyz, job, probability=0.99, min_inliers=20, max_iterations=300, fix_scale=0, **_):
    """the whole job as the library reports it: the scan does not stop at an event (the caller calls iterate again with the best retained)"""
    sv = Solver(xyz, job, probability, min_inliers, max_iterations, fix_scale)
    while not sv.too_few and sv.n_iterations < sv.max_its:
        sv.iterate(sv.max_its)
    I, N = sv.max_its, sv.N
    out = {"status": TOO_FEW if sv.too_few else (OK if sv.events else NO_MORE), "n": N, "iterations": I, "n_events": len(sv.events), "events": sv.events,
           "best_it": sv.best_it, "best_inliers": sv.best_inliers, "counts": np.array(sv.counts, np.int32),
           "s": np.array([h["s"] for h in sv.hyps], F), "R": np.array([h["R"].reshape(-1) for h in sv.hyps], F).reshape(I, 9),
           "t": np.array([h["t"] for h in sv.hyps], F).reshape(I, 3), "inlier": np.array(sv.inliers, np.uint8).reshape(I, N),
           "sweep_cap_hits": sum(h["sweeps"] >= MAX_SWEEPS for h in sv.hyps), "solver": sv}
    if sv.best is not None:
        h, inl = sv.best
        out["best"] = {"iteration": sv.best_it, "n_inliers": sv.best_inliers, "s": h["s"], "R": h["R"].reshape(-1), "t": h["t"], "inlier": inl}
    return out

"""numpy restatement of the bundle adjustment's rules B1-B10 (include/iba_mi355x.h, iba_bundle*): float64, the same fixed sequences and summation
trees as csrc/iba_bundle_math.hpp, written independently of it (a plain LM loop per job, no sequencer; every sum vectorised over the items that
share a position in their lists). Also the long-double evaluations the parity gates compare with, and plain-Python restatements of the plan."""
import math

import numpy as np

from pose_ref import DMAX, canon, exp_update, finite, fmul, hidx, huber

WAVE, LANES = 64, 256
LOCAL_DELTA = np.float32(math.sqrt(5.991))
GLOBAL_DELTA = np.float32(math.sqrt(5.99))
LOCAL = dict(rounds=2, iterations=(5, 10, 0, 0), robust_rounds=1, chi2_threshold=np.float32(5.991), huber_delta=LOCAL_DELTA)


def global_options(n_iterations, robust):
    return dict(rounds=1, iterations=(n_iterations, 0, 0, 0), robust_rounds=1 if robust else 0, chi2_threshold=np.float32(5.991), huber_delta=GLOBAL_DELTA)


class Job:
    """the arrays of a job at the library's types, and its lists (B10): stable in edge index"""

    def __init__(self, Tcw, fixed, xyz, edge_point, edge_camera, obs, inv_sigma2, K):
        self.T = np.ascontiguousarray(Tcw, np.float64).reshape(-1, 12).copy()
        self.fixed = np.ascontiguousarray(fixed, np.uint8).reshape(-1).astype(bool)
        self.X = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3).astype(np.float64)
        self.ep = np.ascontiguousarray(edge_point, np.int64).reshape(-1)
        self.ec = np.ascontiguousarray(edge_camera, np.int64).reshape(-1)
        self.obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2).astype(np.float64)
        self.w = np.ascontiguousarray(inv_sigma2, np.float32).reshape(-1).astype(np.float64)
        self.K = tuple(np.float64(np.float32(v)) for v in K)
        self.nc, self.np, self.ne = len(self.T), len(self.X), len(self.ep)
        self.pos_in_point = position_in_group(self.ep, self.np)
        self.pos_in_camera = position_in_group(self.ec, self.nc)
        self.free = np.flatnonzero(~self.fixed)
        # the items of the reduced system: per pair of edges of one point with free cameras a <= b, in (a, b, point) order
        items = []
        order = np.argsort(self.ep, kind="stable")
        start = np.searchsorted(self.ep[order], np.arange(self.np + 1))
        for p in range(self.np):
            es = [int(e) for e in order[start[p]:start[p + 1]] if not self.fixed[self.ec[e]]]
            for i, ei in enumerate(es):
                for ek in es[i:]:
                    ea, eb = (ei, ek) if self.ec[ei] <= self.ec[ek] else (ek, ei)
                    items.append((int(self.ec[ea]), int(self.ec[eb]), p, ea, eb))
        items.sort(key=lambda t: t[:3])
        it = np.array(items, np.int64).reshape(-1, 5)
        self.it_a, self.it_b, self.it_p, self.it_ea, self.it_eb = (it[:, k] for k in range(5))
        key = self.it_a * (self.nc + 1) + self.it_b
        self.blocks, self.it_blk = np.unique(key, return_inverse=True)
        self.it_pos = position_in_group(self.it_blk, len(self.blocks))
        first = np.searchsorted(self.it_blk, np.arange(len(self.blocks)))
        self.blk_a, self.blk_b = self.it_a[first], self.it_b[first]


def position_in_group(group, n):
    """the rank of every item among the items of its group, in ascending item index"""
    order = np.argsort(group, kind="stable")
    start = np.searchsorted(group[order], np.arange(n + 1))
    pos = np.zeros(len(group), np.int64)
    pos[order] = np.arange(len(group)) - start[group[order]]
    return pos


def lane_sums(terms, group, pos, n_groups, active, lanes):
    """B3: item i is the pos[i]-th of group[i]'s list and belongs to lane pos % lanes; a lane adds its active items in ascending order onto +0.0; the
    lanes are combined by the balanced tree -> [n_groups, k]. (x - y is x + (-y) exactly, so what is subtracted comes negated.)"""
    acc = np.zeros((n_groups, lanes, terms.shape[1]))
    row, lane = pos // lanes, pos % lanes
    with np.errstate(all="ignore"):
        for r in range(int(row.max()) + 1 if len(row) else 0):
            sel = np.flatnonzero((row == r) & active)
            acc[group[sel], lane[sel]] += terms[sel]
        while acc.shape[1] > 1:
            acc = acc[:, 0::2] + acc[:, 1::2]
    return acc[:, 0]


def sequential_sums(terms, group, pos, n_groups, active):
    acc = np.zeros((n_groups, terms.shape[1]))
    with np.errstate(all="ignore"):
        for r in range(int(pos.max()) + 1 if len(pos) else 0):
            sel = np.flatnonzero((pos == r) & active)
            acc[group[sel]] += terms[sel]
    return acc


# ---- B1, B2 ----
def edges(q, T, X, jac=True):
    """-> chi2 [ne], p_z [ne] and, with jac, e [ne, 2], Jc [ne, 2, 6], Jl [ne, 2, 3]"""
    fx, fy, cx, cy = q.K
    Te, Xe = T[q.ec], X[q.ep]
    x, y, z = Xe[:, 0], Xe[:, 1], Xe[:, 2]
    with np.errstate(all="ignore"):
        px = ((Te[:, 0] * x + Te[:, 1] * y) + Te[:, 2] * z) + Te[:, 3]
        py = ((Te[:, 4] * x + Te[:, 5] * y) + Te[:, 6] * z) + Te[:, 7]
        pz = ((Te[:, 8] * x + Te[:, 9] * y) + Te[:, 10] * z) + Te[:, 11]
        ex = q.obs[:, 0] - ((fx * px) / pz + cx)
        ey = q.obs[:, 1] - ((fy * py) / pz + cy)
        chi2 = q.w * (ex * ex + ey * ey)
        if not jac:
            return chi2, pz
        iz = 1.0 / pz
        iz2 = iz * iz
        zero = np.zeros_like(px)
        Jc = np.stack([np.stack([((px * py) * iz2) * fx, (-(1.0 + (px * px) * iz2)) * fx, (py * iz) * fx, (-iz) * fx, zero, (px * iz2) * fx], 1),
                       np.stack([(1.0 + (py * py) * iz2) * fy, (-((px * py) * iz2)) * fy, (-(px * iz)) * fy, zero, (-iz) * fy, (py * iz2) * fy], 1)], 1)
        a, b = (-(fx * px)) * iz, (-(fy * py)) * iz
        Jl = np.stack([np.stack([(-iz) * (fx * Te[:, c] + a * Te[:, 8 + c]) for c in range(3)], 1),
                       np.stack([(-iz) * (fy * Te[:, 4 + c] + b * Te[:, 8 + c]) for c in range(3)], 1)], 1)
    return chi2, pz, np.stack([ex, ey], 1), Jc, Jl


def upper(J, wr):
    """w (J_0p J_0q + J_1p J_1q) for p <= q by rows -> [ne, k(k + 1) / 2]"""
    k = J.shape[2]
    with np.errstate(all="ignore"):
        return np.stack([wr * (J[:, 0, p] * J[:, 0, r] + J[:, 1, p] * J[:, 1, r]) for p in range(k) for r in range(p, k)], 1)


def gradient(J, e, wr):
    with np.errstate(all="ignore"):
        return np.stack([-(wr * (J[:, 0, p] * e[:, 0] + J[:, 1, p] * e[:, 1])) for p in range(J.shape[2])], 1)


def sym3(h):
    """[n, 6] upper triangles -> [n, 3, 3]"""
    return np.stack([np.stack([h[:, 0], h[:, 1], h[:, 2]], 1), np.stack([h[:, 1], h[:, 3], h[:, 4]], 1), np.stack([h[:, 2], h[:, 4], h[:, 5]], 1)], 1)


def job_chi2(q, rho, active, has):
    part = sequential_sums(rho[:, None], q.ep, q.pos_in_point, q.np, active)[:, 0]
    tot = lane_sums(part[:, None], np.zeros(q.np, np.int64), np.arange(q.np), 1, has, LANES)
    return float(tot[0, 0])


def linearise(q, T, X, active, robust, delta):
    """B1-B4 at the estimates -> dict of the sums and what the step needs"""
    chi2, _, e, Jc, Jl = edges(q, T, X)
    rho0, rho1 = huber(chi2, robust, delta)
    with np.errstate(all="ignore"):
        wr = rho1 * q.w
    cam = lane_sums(np.concatenate([upper(Jc, wr), gradient(Jc, e, wr)], 1), q.ec, q.pos_in_camera, q.nc, active, WAVE)
    pt = sequential_sums(np.concatenate([upper(Jl, wr), gradient(Jl, e, wr)], 1), q.ep, q.pos_in_point, q.np, active)
    cam_cnt = np.bincount(q.ec[active], minlength=q.nc)
    pt_cnt = np.bincount(q.ep[active], minlength=q.np)
    has_c, has_p = (~q.fixed) & (cam_cnt > 0), pt_cnt > 0
    with np.errstate(all="ignore"):
        W = wr[:, None, None] * (Jc[:, 0, :, None] * Jl[:, 0, None, :] + Jc[:, 1, :, None] * Jl[:, 1, None, :])
    return dict(chi2_edges=chi2, cam=cam, pt=pt, has_c=has_c, has_p=has_p, W=W, chi=job_chi2(q, rho0, active, has_p))


def largest_diagonal(lin):
    md = 0.0
    d = np.concatenate([np.abs(lin["pt"][lin["has_p"]][:, [0, 3, 5]]).ravel(), np.abs(lin["cam"][lin["has_c"]][:, [hidx(k, k) for k in range(6)]]).ravel()])
    for v in d:
        if v > md:
            md = float(v)
    return md


def reduced_solve(S, b):
    """B7 -> dp or None. The trailing update subtracts column k's products from every later entry: per entry, k ascending, one at a time."""
    n = len(b)
    L, v = S.copy(), b.copy()
    with np.errstate(all="ignore"):
        for k in range(n):
            d = L[k, k]
            if not (d > 0.0 and d <= DMAX):
                return None
            l = np.sqrt(d)
            L[k, k] = l
            L[k + 1:, k] = L[k + 1:, k] / l
            c = L[k + 1:, k]
            L[k + 1:, k + 1:] -= np.tril(c[:, None] * c[None, :])
        y = np.zeros(n)
        for k in range(n):
            y[k] = v[k] / L[k, k]
            v[k + 1:] = v[k + 1:] - L[k + 1:, k] * y[k]
        x, v = np.zeros(n), y.copy()
        for k in range(n - 1, -1, -1):
            x[k] = v[k] / L[k, k]
            v[:k] = v[:k] - L[k, :k] * x[k]
    return x


def step(q, lin, active, lam):
    """B5-B7 -> None (a failed trial) or dict: dp [nc, 6], dl [np, 3], S, bs, rank"""
    has_c, has_p = lin["has_c"], lin["has_p"]
    h = lin["pt"]
    with np.errstate(all="ignore"):
        a00, a01, a02, a11, a12, a22 = h[:, 0] + lam, h[:, 1], h[:, 2], h[:, 3] + lam, h[:, 4], h[:, 5] + lam
        c00, c01, c02 = a11 * a22 - a12 * a12, a02 * a12 - a01 * a22, a01 * a12 - a02 * a11
        c11, c12, c22 = a00 * a22 - a02 * a02, a01 * a02 - a00 * a12, a00 * a11 - a01 * a01
        det = (a00 * c00 + a01 * c01) + a02 * c02
        if np.any(has_p & ~((det > 0.0) & (det <= DMAX))):
            return None
        idet = 1.0 / det
        A = sym3(np.stack([c00 * idet, c01 * idet, c02 * idet, c11 * idet, c12 * idet, c22 * idet], 1))
    rank = np.full(q.nc, -1, np.int64)
    rank[has_c] = np.arange(int(has_c.sum()))
    n = 6 * int(has_c.sum())
    S, bs = np.zeros((n, n)), np.zeros(n)
    blk = np.arange(n) // 6
    S[blk[:, None] > blk[None, :]] = -0.0           # a block without a live item is minus its sum of +0.0
    W, bl = lin["W"], h[:, 6:9]
    live = active[q.it_ea] & active[q.it_eb] if len(q.it_ea) else np.zeros(0, bool)
    with np.errstate(all="ignore"):
        Wa, Wb, Ai = W[q.it_ea], W[q.it_eb], A[q.it_p]
        Y = (Wa[:, :, 0, None] * Ai[:, None, 0, :] + Wa[:, :, 1, None] * Ai[:, None, 1, :]) + Wa[:, :, 2, None] * Ai[:, None, 2, :]
        G = (Y[:, :, None, 0] * Wb[:, None, :, 0] + Y[:, :, None, 1] * Wb[:, None, :, 1]) + Y[:, :, None, 2] * Wb[:, None, :, 2]
        bi = bl[q.it_p]
        g = (Y[:, :, 0] * bi[:, None, 0] + Y[:, :, 1] * bi[:, None, 1]) + Y[:, :, 2] * bi[:, None, 2]
        sums = lane_sums(np.concatenate([G.reshape(-1, 36), g], 1), q.it_blk, q.it_pos, len(q.blocks), live, WAVE)
        for k in range(len(q.blocks)):
            a, b = int(q.blk_a[k]), int(q.blk_b[k])
            if rank[a] < 0 or rank[b] < 0:
                continue
            ra, rb, Gs = 6 * rank[a], 6 * rank[b], sums[k, :36].reshape(6, 6)
            if a == b:
                Hpp = np.array([[lin["cam"][a, hidx(min(r, s), max(r, s))] + (lam if r == s else 0.0) for s in range(6)] for r in range(6)])
                S[ra:ra + 6, ra:ra + 6] = np.tril(Hpp - Gs)
                bs[ra:ra + 6] = lin["cam"][a, 21:27] - sums[k, 36:42]
            else:
                S[rb:rb + 6, ra:ra + 6] = -Gs.T
    dp_red = reduced_solve(S, bs)
    if dp_red is None:
        return None
    dp = np.zeros((q.nc, 6))
    dp[has_c] = dp_red.reshape(-1, 6)
    v = bl.copy()
    use = active & (rank[q.ec] >= 0)
    with np.errstate(all="ignore"):
        for r in range(int(q.pos_in_point.max()) + 1 if q.ne else 0):
            sel = np.flatnonzero((q.pos_in_point == r) & use)
            Ws, d = W[sel], dp[q.ec[sel]]
            t = Ws[:, 0, :] * d[:, 0, None] + Ws[:, 1, :] * d[:, 1, None]
            for k in range(2, 6):
                t = t + Ws[:, k, :] * d[:, k, None]
            v[q.ep[sel]] -= t
        dl = (A[:, :, 0] * v[:, 0, None] + A[:, :, 1] * v[:, 1, None]) + A[:, :, 2] * v[:, 2, None]
    dl[~has_p] = 0.0
    Sfull = S.copy()
    iu = np.triu_indices(n, 1)
    Sfull[iu] = S.T[iu]
    bs6 = np.zeros((q.nc, 6))
    bs6[has_c] = bs.reshape(-1, 6)
    return dict(dp=dp, dl=dl, S=Sfull, bs=bs6, rank=rank)


def scale_of(lin, st, lam):
    """B8: one running sum, cameras ascending then points ascending"""
    s = 1e-3
    with np.errstate(all="ignore"):
        for c in np.flatnonzero(lin["has_c"]):
            for k in range(6):
                d = np.float64(st["dp"][c, k])
                s = s + d * (np.float64(lam) * d + lin["cam"][c, 21 + k])
        for p in np.flatnonzero(lin["has_p"]):
            for k in range(3):
                d = np.float64(st["dl"][p, k])
                s = s + d * (np.float64(lam) * d + lin["pt"][p, 6 + k])
    return np.float64(s)


def trial_estimates(q, lin, st, T, X):
    Tn, big = T.copy(), 0
    for c in np.flatnonzero(st["rank"] >= 0):
        t, g = exp_update(st["dp"][c], T[c])
        Tn[c], big = t.reshape(12), big + g
    with np.errstate(all="ignore"):
        Xn = np.where(lin["has_p"][:, None], X + st["dl"], X)
    return Tn, Xn, big


def evaluate(q, active=None, robust=True, lam=0.0, delta=LOCAL_DELTA):
    """what iba_bundle_eval answers for one job"""
    act = np.ones(q.ne, bool) if active is None else np.asarray(active).astype(bool)
    lin = linearise(q, q.T, q.X, act, robust, np.float64(delta))
    st = step(q, lin, act, float(lam))
    hc, hp = lin["has_c"], lin["has_p"]
    Hpp = np.array([[[lin["cam"][c, hidx(min(r, s), max(r, s))] for s in range(6)] for r in range(6)] for c in range(q.nc)]).reshape(q.nc, 6, 6)
    out = dict(Hpp=canon(np.where(hc[:, None, None], Hpp, 0.0)), bp=canon(np.where(hc[:, None], lin["cam"][:, 21:27], 0.0)),
               Hll=canon(np.where(hp[:, None, None], sym3(lin["pt"][:, :6]), 0.0)), bl=canon(np.where(hp[:, None], lin["pt"][:, 6:9], 0.0)),
               chi2_edges=canon(lin["chi2_edges"]), chi2_robust=canon(np.float64(lin["chi"])), n_reduced=6 * int(hc.sum()), solved=0 if st is None else 1)
    n = out["n_reduced"]
    if st is None:
        out.update(S=np.zeros((n, n)), bs=np.zeros((q.nc, 6)), dp=np.zeros((q.nc, 6)), dl=np.zeros((q.np, 3)))
    else:
        out.update(S=canon(st["S"]), bs=canon(st["bs"]), dp=canon(st["dp"]), dl=canon(st["dl"]))
    return out


# ---- B8, B9: the whole schedule of one job ----
def optimize(q, **opt):
    """-> a list of (name, array) in the order of Bundle.everything(), stages included, and a dict of extras"""
    o = dict(LOCAL)
    o.update(opt)
    thr, delta = np.float32(o["chi2_threshold"]), np.float64(np.float32(o["huber_delta"]))
    rounds = o["rounds"]
    T, X = q.T.copy(), q.X.copy()
    active = np.ones(q.ne, bool)
    chi2s, n_bad, its_, trials_ = np.zeros(4), np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    stages, big_steps, n_dead = [], 0, 0
    nonfinite_trials = behind_trials = zero_depth_trials = 0      # trials with a good factorisation whose chi2 is not finite; with an active edge at p_z <= 0; at p_z == 0
    outlier, c32 = np.zeros(q.ne, np.uint8), np.zeros(q.ne, np.float32)
    with np.errstate(all="ignore"):
        for rnd in range(rounds):
            robust = rnd < o["robust_rounds"]
            its = trials = 0
            lam = ni = current = 0.0
            for it in range(o["iterations"][rnd]):
                lin = linearise(q, T, X, active, robust, delta)
                current = lin["chi"]
                if it == 0:
                    lam, ni = 1e-5 * largest_diagonal(lin), 2.0
                its += 1
                qmax, stop = 0, False
                while True:
                    st = step(q, lin, active, lam)
                    trials += 1
                    temp = DMAX
                    scale = np.float64(1e-3)
                    if st is not None:
                        Tn, Xn, big = trial_estimates(q, lin, st, T, X)
                        big_steps += big
                        c2, pz = edges(q, Tn, Xn, jac=False)
                        temp = job_chi2(q, huber(c2, robust, delta)[0], active, lin["has_p"])
                        nonfinite_trials += 0 if finite(temp) else 1
                        behind_trials += 1 if np.any(active & ~(pz > 0.0)) else 0
                        zero_depth_trials += 1 if np.any(active & (pz == 0.0)) else 0
                        scale = scale_of(lin, st, lam)
                    rho = float((np.float64(current) - np.float64(temp)) / scale)
                    if st is not None and rho > 0.0 and finite(temp):
                        t = 2.0 * rho - 1.0
                        alpha = float(1.0 - (np.float64(t) * t) * t)
                        if 2.0 / 3.0 < alpha:
                            alpha = 2.0 / 3.0
                        if not (1.0 / 3.0 < alpha):
                            alpha = 1.0 / 3.0
                        lam, ni, current, T, X = lam * alpha, 2.0, temp, Tn, Xn
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
            c2, pz = edges(q, T, X, jac=False)
            bad = (c2.astype(np.float32) > thr) | ~(pz > 0.0)
            if rnd == rounds - 1:
                outlier, c32 = bad.astype(np.uint8), canon(c2.astype(np.float32))
                n_bad[rnd] = int(bad.sum())
            else:
                n_dead += int((bad & active).sum())
                active = active & ~bad
                n_bad[rnd] = n_dead
            chi2s[rnd] = canon(np.float64(current))
            its_[rnd], trials_[rnd] = its, trials
            stages.append((canon(T.reshape(-1, 3, 4).copy()), canon(X.copy())))
    T, X = canon(T.reshape(-1, 3, 4)), canon(X)
    out = [("counts", np.array([q.nc, q.np, q.ne, len(q.free), int(n_bad[rounds - 1]), rounds], np.int32)), ("chi2", chi2s), ("n_bad", n_bad), ("lm_iterations", its_),
           ("trials", trials_), ("Tcw", T), ("Tcwf", T.astype(np.float32)), ("xyz", X), ("xyzf", X.astype(np.float32)), ("outlier", outlier), ("edge_chi2", c32)]
    return out, dict(stages=stages, big_steps=big_steps, active=active, final_chi2=float(chi2s[rounds - 1]), nonfinite_trials=nonfinite_trials, behind_trials=behind_trials,
                     zero_depth_trials=zero_depth_trials)


def with_stages(out, extras):
    res = list(out)
    for k, (T, X) in enumerate(extras["stages"]):
        res += [("stage%d_Tcw" % k, T), ("stage%d_xyz" % k, X)]
    return res


def differences(got, want):
    """the names of the outputs whose bytes differ"""
    bad = [a for (a, x), (b, y) in zip(got, want) if a != b or np.ascontiguousarray(x).tobytes() != np.ascontiguousarray(y).tobytes()]
    return bad + (["length"] if len(got) != len(want) else [])


# ---- the truth of the parity gates: the FULL damped system, edge by edge in long double, solved densely in long double ----
def full_system_longdouble(q, active, robust, lam, delta=LOCAL_DELTA):
    """-> dict of long-double Hpp [nc, 6, 6], bp, Hll, bl, chi, and dp [nc, 6], dl [np, 3] of the dense solve over the participating unknowns (None
    where no edge is active)"""
    ld = np.longdouble
    act = np.ones(q.ne, bool) if active is None else np.asarray(active).astype(bool)
    fx, fy, cx, cy = (ld(v) for v in q.K)
    Hpp, bp, Hll, bl = np.zeros((q.nc, 6, 6), ld), np.zeros((q.nc, 6), ld), np.zeros((q.np, 3, 3), ld), np.zeros((q.np, 3), ld)
    Hpl = {}
    chi, delta = ld(0), ld(np.float64(delta))
    for e in np.flatnonzero(act):
        c, p = int(q.ec[e]), int(q.ep[e])
        T = q.T[c].astype(ld).reshape(3, 4)
        P = T[:, :3] @ q.X[p].astype(ld) + T[:, 3]
        x, y, z = P
        err = np.array([ld(q.obs[e, 0]) - (fx * x / z + cx), ld(q.obs[e, 1]) - (fy * y / z + cy)], ld)
        w = ld(q.w[e])
        c2 = w * (err @ err)
        rho0, rho1 = c2, ld(1)
        if robust and c2 > delta * delta:
            rho0, rho1 = 2 * np.sqrt(c2) * delta - delta * delta, delta / np.sqrt(c2)
        chi += rho0
        Jc = np.array([[x * y / z ** 2 * fx, -(1 + x * x / z ** 2) * fx, y / z * fx, -fx / z, 0, x / z ** 2 * fx],
                       [(1 + y * y / z ** 2) * fy, -x * y / z ** 2 * fy, -x / z * fy, 0, -fy / z, y / z ** 2 * fy]], ld)
        Jl = -(1 / z) * (np.array([[fx, 0, -fx * x / z], [0, fy, -fy * y / z]], ld) @ T[:, :3])
        wr = rho1 * w
        Hll[p] += wr * Jl.T @ Jl
        bl[p] -= wr * Jl.T @ err
        if not q.fixed[c]:
            Hpp[c] += wr * Jc.T @ Jc
            bp[c] -= wr * Jc.T @ err
            Hpl[(c, p)] = wr * Jc.T @ Jl
    cams = [c for c in range(q.nc) if not q.fixed[c] and np.any(act & (q.ec == c))]
    pts = [p for p in range(q.np) if np.any(act & (q.ep == p))]
    n = 6 * len(cams) + 3 * len(pts)
    out = dict(Hpp=Hpp, bp=bp, Hll=Hll, bl=bl, chi=chi, dp=None, dl=None)
    if n == 0:
        return out
    A, b = np.zeros((n, n), ld), np.zeros(n, ld)
    ci, pi = {c: 6 * k for k, c in enumerate(cams)}, {p: 6 * len(cams) + 3 * k for k, p in enumerate(pts)}
    for c in cams:
        A[ci[c]:ci[c] + 6, ci[c]:ci[c] + 6] = Hpp[c] + ld(lam) * np.eye(6, dtype=ld)
        b[ci[c]:ci[c] + 6] = bp[c]
    for p in pts:
        A[pi[p]:pi[p] + 3, pi[p]:pi[p] + 3] = Hll[p] + ld(lam) * np.eye(3, dtype=ld)
        b[pi[p]:pi[p] + 3] = bl[p]
    for (c, p), Wm in Hpl.items():
        A[ci[c]:ci[c] + 6, pi[p]:pi[p] + 3] = Wm
        A[pi[p]:pi[p] + 3, ci[c]:ci[c] + 6] = Wm.T
    x = solve_longdouble(A, b)
    dp, dl = np.zeros((q.nc, 6), ld), np.zeros((q.np, 3), ld)
    for c in cams:
        dp[c] = x[ci[c]:ci[c] + 6]
    for p in pts:
        dl[p] = x[pi[p]:pi[p] + 3]
    out.update(dp=dp, dl=dl)
    return out


def solve_longdouble(A, b):
    """Gaussian elimination with partial pivoting in long double (numpy's solvers do not take the type)"""
    A, b = A.copy(), b.copy()
    n = len(b)
    for k in range(n):
        piv = k + int(np.argmax(np.abs(A[k:, k])))
        if piv != k:
            A[[k, piv]], b[[k, piv]] = A[[piv, k]], b[[piv, k]]
        f = A[k + 1:, k] / A[k, k]
        A[k + 1:, k:] -= f[:, None] * A[k, k:][None, :]
        b[k + 1:] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for k in range(n - 1, -1, -1):
        x[k] = (b[k] - A[k, k + 1:] @ x[k + 1:]) / A[k, k]
    return x


# ---- the plan in plain Python (B6, B10) ----
def plan_plain(fixed, edge_point, edge_camera, n_points):
    nc = len(fixed)
    pt = [[e for e in range(len(edge_point)) if edge_point[e] == p] for p in range(n_points)]
    cam = [[e for e in range(len(edge_camera)) if edge_camera[e] == c] for c in range(nc)]
    free = [c for c in range(nc) if not fixed[c]]
    blocks = [(a, b) for a in free for b in free if a <= b]
    items = {k: [] for k in blocks}
    for p in range(n_points):
        es = [e for e in pt[p] if not fixed[edge_camera[e]]]
        for i, ei in enumerate(es):
            for ek in es[i:]:
                ea, eb = (ei, ek) if edge_camera[ei] <= edge_camera[ek] else (ek, ei)
                items[(edge_camera[ea], edge_camera[eb])].append((p, ea, eb))
    return pt, cam, blocks, items

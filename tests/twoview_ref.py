"""numpy restatement of the two-view initialisation's rules T1-T11 (include/iba_mi355x.h, iba_twoview*): the reference the library's host
restatement and its kernels are compared with, byte for byte. Wherever the order of a float sum is part of a rule the sum is an explicit loop (never
np.sum on a float32 sequence); the vectorisation is across hypotheses, or across (motion hypothesis, match), which are independent. float32
arithmetic is numpy float32 arrays (every operation rounded), the cv::Mat operations are float64 on the widened entries, rounded once per element."""
import math

import numpy as np

f32, f64 = np.float32, np.float64
OK, TOO_FEW_MATCHES, NO_MODEL, H_DEGENERATE, NO_CLEAR_WINNER, TOO_FEW_POINTS, LOW_PARALLAX = range(7)
MAX_SWEEPS = 30
TWO_M104 = 2.0 ** -104


def canon(x):
    """a NaN that is stored into an output is 0x7FC00000"""
    x = np.array(x, f32, copy=True)
    x.view(np.uint32)[np.isnan(x)] = 0x7FC00000
    return x


# ---- T1 ----
def normalize(xy):
    xy = np.ascontiguousarray(xy, f32).reshape(-1, 2)
    n = len(xy)
    with np.errstate(all="ignore"):
        mean = np.zeros(2, f32)
        for i in range(n):
            mean = mean + xy[i]
        mean = mean / f32(n)
        out = xy - mean
        dev = np.zeros(2, f32)
        for i in range(n):
            dev = dev + np.abs(out[i])
        dev = dev / f32(n)
        s = (f64(1.0) / dev.astype(f64)).astype(f32)
        out = out * s
        T = np.zeros((3, 3), f32)
        T[0, 0], T[1, 1], T[2, 2] = s[0], s[1], 1
        T[0, 2], T[1, 2] = -mean[0] * s[0], -mean[1] * s[1]
    return out.astype(f32), T


# ---- the sets ----
M64 = (1 << 64) - 1


def make_sets(N, iterations, seed):
    s = seed & M64
    out = np.zeros((iterations, 8), np.int32)
    for it in range(iterations):
        avail = list(range(N))
        for j in range(8):
            s = (s + 0x9E3779B97F4A7C15) & M64
            z = s
            z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
            z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
            z = z ^ (z >> 31)
            r = z % len(avail)
            out[it, j] = avail[r]
            avail[r] = avail[-1]
            avail.pop()
    return out


# ---- T2, batched over the leading axis ----
def jacobi(A):
    """A [B, M, N] float32 -> (G, V, sweeps that rotated)"""
    G = np.array(A, f64, copy=True)
    B, M, N = G.shape
    V = np.broadcast_to(np.eye(N), (B, N, N)).copy()
    fro = np.zeros(B)
    for i in range(M):
        for j in range(N):
            fro = fro + G[:, i, j] * G[:, i, j]
    tiny = fro * TWO_M104
    sweeps = np.zeros(B, np.int64)
    for _ in range(MAX_SWEEPS):
        rotated = np.zeros(B, bool)
        for p in range(N - 1):
            for q in range(p + 1, N):
                gp, gq = G[:, :, p].copy(), G[:, :, q].copy()
                a, b, g = np.zeros(B), np.zeros(B), np.zeros(B)
                for r in range(M):
                    a = a + gp[:, r] * gp[:, r]
                    b = b + gq[:, r] * gq[:, r]
                    g = g + gp[:, r] * gq[:, r]
                rot = ~((g * g <= a * b * TWO_M104) | (a <= tiny) | (b <= tiny))
                if not rot.any():
                    continue
                zeta = (b - a) / (2.0 * g)
                t = np.where(zeta >= 0.0, 1.0, -1.0) / (np.abs(zeta) + np.sqrt(1.0 + zeta * zeta))
                c = 1.0 / np.sqrt(1.0 + t * t)
                s = c * t
                c, s, m = c[:, None], s[:, None], rot[:, None]
                G[:, :, p] = np.where(m, c * gp - s * gq, gp)
                G[:, :, q] = np.where(m, s * gp + c * gq, gq)
                vp, vq = V[:, :, p].copy(), V[:, :, q].copy()
                V[:, :, p] = np.where(m, c * vp - s * vq, vp)
                V[:, :, q] = np.where(m, s * vp + c * vq, vq)
                rotated |= rot
        sweeps += rotated
        if not rotated.any():
            break
    return G, V, sweeps


def col_norms2(G):
    n = np.zeros((G.shape[0], G.shape[2]))
    for r in range(G.shape[1]):
        n = n + G[:, r, :] * G[:, r, :]
    return n


def null_vector(A):
    """A [B, M, N] float32 -> (v [B, N] float32, sweeps [B])"""
    with np.errstate(all="ignore"):
        G, V, sw = jacobi(A)
        n = col_norms2(G)
        best, bn = np.zeros(len(G), np.int64), n[:, 0].copy()
        for c in range(1, n.shape[1]):
            m = n[:, c] < bn
            bn = np.where(m, n[:, c], bn)
            best = np.where(m, c, best)
        return V[np.arange(len(G)), :, best].astype(f32), sw


def svd33(A):
    """A [3, 3] float32 -> (U, w, Vt) float32, sweeps"""
    with np.errstate(all="ignore"):
        G, V, sw = jacobi(np.asarray(A, f32)[None])
        G, V = G[0], V[0]
        n = col_norms2(G[None])[0]
        o = [0, 1, 2]
        if n[o[1]] > n[o[0]]:
            o[0], o[1] = o[1], o[0]
        if n[o[2]] > n[o[1]]:
            o[1], o[2] = o[2], o[1]
            if n[o[1]] > n[o[0]]:
                o[0], o[1] = o[1], o[0]
        wd = np.sqrt(n[o])
        ud = G[:, o] / wd[None, :]
        Vt = V[:, o].T.astype(f32)
        if wd[2] <= 2.0 ** -23 * wd[0]:
            u1, u2 = ud[:, 0], ud[:, 1]
            ud[:, 2] = [u1[1] * u2[2] - u1[2] * u2[1], u1[2] * u2[0] - u1[0] * u2[2], u1[0] * u2[1] - u1[1] * u2[0]]
        return ud.astype(f32), wd.astype(f32), np.ascontiguousarray(Vt), int(sw[0])


# ---- the cv::Mat operations; the trailing two axes are the matrix ----
def mul33(A, B):
    A, B = np.asarray(A, f32).astype(f64), np.asarray(B, f32).astype(f64)
    with np.errstate(all="ignore"):
        return ((A[..., :, 0, None] * B[..., None, 0, :] + A[..., :, 1, None] * B[..., None, 1, :]) + A[..., :, 2, None] * B[..., None, 2, :]).astype(f32)


def mul331(A, x):
    A, x = np.asarray(A, f32).astype(f64), np.asarray(x, f32).astype(f64)
    return ((A[..., :, 0] * x[..., None, 0] + A[..., :, 1] * x[..., None, 1]) + A[..., :, 2] * x[..., None, 2]).astype(f32)


def _cof(M):
    M = np.asarray(M, f32).astype(f64)
    a, b, c, d, e, f, g, h, i = (M[..., r, k] for r in range(3) for k in range(3))
    det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g)
    return det, (e * i - f * h, c * h - b * i, b * f - c * e, f * g - d * i, a * i - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d)


def det33(M):
    return _cof(M)[0]


def inv33(M):
    with np.errstate(all="ignore"):
        det, cof = _cof(M)
        return np.stack([(x / det).astype(f32) for x in cof], -1).reshape(np.shape(M))


def norm3(x):
    x = np.asarray(x, f32).astype(f64)
    return np.sqrt((x[..., 0] * x[..., 0] + x[..., 1] * x[..., 1]) + x[..., 2] * x[..., 2])


def inv_affine_diag(T):
    T = np.asarray(T, f32).astype(f64)
    Ti = np.zeros((3, 3), f32)
    with np.errstate(all="ignore"):
        Ti[0, 0], Ti[1, 1], Ti[2, 2] = f32(1.0 / T[0, 0]), f32(1.0 / T[1, 1]), 1
        Ti[0, 2], Ti[1, 2] = f32(-T[0, 2] / T[0, 0]), f32(-T[1, 2] / T[1, 1])
    return Ti


def make_K(fx, fy, cx, cy):
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], f32)


# ---- T3 / T4 over all iterations of a pair: pn [I, 8, 4] float32 ----
def design_h(pn):
    u1, v1, u2, v2 = (pn[:, :, k] for k in range(4))
    z, one = np.zeros_like(u1), np.ones_like(u1)
    r0 = np.stack([z, z, z, -u1, -v1, -one, v2 * u1, v2 * v1, v2], -1)
    r1 = np.stack([u1, v1, one, z, z, z, -u2 * u1, -u2 * v1, -u2], -1)
    return np.stack([r0, r1], 2).reshape(len(pn), 16, 9).astype(f32)


def design_f(pn):
    u1, v1, u2, v2 = (pn[:, :, k] for k in range(4))
    return np.stack([u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, np.ones_like(u1)], -1).astype(f32)


def h_hypotheses(pn, T1, T2inv):
    with np.errstate(all="ignore"):
        Hn, sw = null_vector(design_h(pn))
        H21 = mul33(mul33(T2inv[None], Hn.reshape(-1, 3, 3)), T1[None])
        return H21, inv33(H21), sw


def f_hypotheses(pn, T1, T2t):
    with np.errstate(all="ignore"):
        Fpre, sw = null_vector(design_f(pn))
        Fpre = Fpre.reshape(-1, 3, 3)
        v3, sw2 = null_vector(Fpre)
        F64, v64 = Fpre.astype(f64), v3.astype(f64)
        y = (F64[:, :, 0] * v64[:, None, 0] + F64[:, :, 1] * v64[:, None, 1]) + F64[:, :, 2] * v64[:, None, 2]
        Fn = (F64 - y[:, :, None] * v64[:, None, :]).astype(f32)
        return mul33(mul33(T2t[None], Fn), T1[None]), np.maximum(sw, sw2)


# ---- T5 over all iterations: the walk over the matches is the loop, in list order ----
def _recip(x):
    return (f64(1.0) / x.astype(f64)).astype(f32)


def inv_sigma_square(sigma):
    s = f32(sigma)
    return f32(f64(1.0) / f64(s * s))


def score_h(H, Hi, mxy, invs):
    """H, Hi [I, 3, 3] float32, mxy [N, 4] -> (score [I], bIn [I, N])"""
    th = f32(5.991)
    h, hi = H.reshape(-1, 9), Hi.reshape(-1, 9)
    score, flags = np.zeros(len(h), f32), np.zeros((len(h), len(mxy)), bool)
    with np.errstate(all="ignore"):
        for i, (u1, v1, u2, v2) in enumerate(mxy.astype(f32)):
            w = _recip(hi[:, 6] * u2 + hi[:, 7] * v2 + hi[:, 8])
            x = (hi[:, 0] * u2 + hi[:, 1] * v2 + hi[:, 2]) * w
            y = (hi[:, 3] * u2 + hi[:, 4] * v2 + hi[:, 5]) * w
            chi1 = ((u1 - x) * (u1 - x) + (v1 - y) * (v1 - y)) * invs
            out1 = chi1 > th
            score = np.where(out1, score, score + (th - chi1))
            w = _recip(h[:, 6] * u1 + h[:, 7] * v1 + h[:, 8])
            x = (h[:, 0] * u1 + h[:, 1] * v1 + h[:, 2]) * w
            y = (h[:, 3] * u1 + h[:, 4] * v1 + h[:, 5]) * w
            chi2 = ((u2 - x) * (u2 - x) + (v2 - y) * (v2 - y)) * invs
            out2 = chi2 > th
            score = np.where(out2, score, score + (th - chi2))
            flags[:, i] = ~out1 & ~out2
    return score.astype(f32), flags


def score_f(F, mxy, invs):
    th, thScore = f32(3.841), f32(5.991)
    f = F.reshape(-1, 9)
    score, flags = np.zeros(len(f), f32), np.zeros((len(f), len(mxy)), bool)
    with np.errstate(all="ignore"):
        for i, (u1, v1, u2, v2) in enumerate(mxy.astype(f32)):
            a2 = f[:, 0] * u1 + f[:, 1] * v1 + f[:, 2]
            b2 = f[:, 3] * u1 + f[:, 4] * v1 + f[:, 5]
            c2 = f[:, 6] * u1 + f[:, 7] * v1 + f[:, 8]
            num2 = a2 * u2 + b2 * v2 + c2
            chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * invs
            out1 = chi1 > th
            score = np.where(out1, score, score + (thScore - chi1))
            a1 = f[:, 0] * u2 + f[:, 3] * v2 + f[:, 6]
            b1 = f[:, 1] * u2 + f[:, 4] * v2 + f[:, 7]
            c1 = f[:, 2] * u2 + f[:, 5] * v2 + f[:, 8]
            num1 = a1 * u1 + b1 * v1 + c1
            chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * invs
            out2 = chi2 > th
            score = np.where(out2, score, score + (thScore - chi2))
            flags[:, i] = ~out1 & ~out2
    return score.astype(f32), flags


def select_best(s):
    best, it = f32(0.0), -1
    for k, v in enumerate(s):
        if v > best:
            best, it = v, k
    return it, f32(best)


# ---- T7 / T8 ----
def motions_from_f(F, K):
    E = mul33(mul33(K.T.copy(), F), K)
    U, w, Vt, sw = svd33(E)
    u3 = U[:, 2].copy()
    t = (u3.astype(f64) / norm3(u3)).astype(f32)
    W = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], f32)
    R1 = mul33(mul33(U, W), Vt)
    if det33(R1) < 0:
        R1 = -R1
    R2 = mul33(mul33(U, W.T.copy()), Vt)
    if det33(R2) < 0:
        R2 = -R2
    return np.stack([R1, R2, R1, R2]), np.stack([t, t, -t, -t]), sw


def motions_from_h(H21, K):
    """-> (R [8, 3, 3], t [8, 3], sweeps) or (None, None, sweeps) on the early refusal"""
    A = mul33(mul33(inv33(K), H21), K)
    U, w, Vt, sw = svd33(A)
    with np.errstate(all="ignore"):
        s = f32(det33(U) * det33(Vt))
        d1, d2, d3 = w
        if float(d1 / d2) < 1.00001 or float(d2 / d3) < 1.00001:
            return None, None, sw
        aux1 = np.sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3))
        aux3 = np.sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3))
        x1, x3 = [aux1, aux1, -aux1, -aux1], [aux3, -aux3, aux3, -aux3]
        aux_stheta = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2)
        ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2)
        stheta = [aux_stheta, -aux_stheta, -aux_stheta, aux_stheta]
        aux_sphi = np.sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2)
        cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2)
        sphi = [aux_sphi, -aux_sphi, -aux_sphi, aux_sphi]
        sU = (s * U).astype(f32)
        R, t = np.zeros((8, 3, 3), f32), np.zeros((8, 3), f32)
        for k in range(8):
            i = k & 3
            Rp = np.eye(3, dtype=f32)
            if k < 4:
                Rp[0, 0], Rp[0, 2], Rp[2, 0], Rp[2, 2] = ctheta, -stheta[i], stheta[i], ctheta
                tp = np.array([x1[i], 0, -x3[i]], f32) * f32(d1 - d3)
            else:
                Rp[0, 0], Rp[0, 2], Rp[1, 1], Rp[2, 0], Rp[2, 2] = cphi, sphi[i], -1, sphi[i], -cphi
                tp = np.array([x1[i], 0, x3[i]], f32) * f32(d1 + d3)
            R[k] = mul33(mul33(sU, Rp), Vt)
            tk = mul331(U, tp)
            t[k] = (tk.astype(f64) / norm3(tk)).astype(f32)
    return R, t, sw


# ---- T9 for one motion hypothesis over the inlier matches m [n, 4] ----
def check_rt(R, t, K, m, th2):
    """-> (verdict [n] uint8 in 1..6, p [n, 3] float32, cos [n] float32, sweeps [n])"""
    fx, fy, cx, cy = K[0, 0], K[1, 1], K[0, 2], K[1, 2]
    n = len(m)
    with np.errstate(all="ignore"):
        P1 = np.zeros((3, 4), f32)
        P1[:, :3] = K
        Rt = np.concatenate([R, t[:, None]], 1).astype(f64)
        K64 = K.astype(f64)
        P2 = ((K64[:, 0, None] * Rt[None, 0, :] + K64[:, 1, None] * Rt[None, 1, :]) + K64[:, 2, None] * Rt[None, 2, :]).astype(f32)
        R64, t64 = R.astype(f64), t.astype(f64)
        O2 = (-((R64[0, :] * t64[0] + R64[1, :] * t64[1]) + R64[2, :] * t64[2])).astype(f32)
        u1, v1, u2, v2 = (m[:, k].astype(f32)[:, None] for k in range(4))
        A = np.stack([u1 * P1[None, 2] - P1[None, 0], v1 * P1[None, 2] - P1[None, 1], u2 * P2[None, 2] - P2[None, 0], v2 * P2[None, 2] - P2[None, 1]], 1).astype(f32)
        x, sw = null_vector(A)
        p = (x[:, :3] / x[:, 3:4]).astype(f32)
        verdict = np.zeros(n, np.uint8)
        bad = ~np.isfinite(p).all(1)
        verdict[bad] = 1
        p[bad] = 0
        dist1 = norm3(p).astype(f32)
        n2 = (p - O2[None]).astype(f32)
        dist2 = norm3(n2).astype(f32)
        p64, n64 = p.astype(f64), n2.astype(f64)
        dot = (p64[:, 0] * n64[:, 0] + p64[:, 1] * n64[:, 1]) + p64[:, 2] * n64[:, 2]
        cos = (dot / (dist1 * dist2).astype(f64)).astype(f32)
        cos[bad] = 0
        low = cos.astype(f64) < 0.99998
        todo = verdict == 0
        hit = todo & (p[:, 2] <= 0) & low
        verdict[hit] = 2
        p2 = (((R64[None, :, 0] * p64[:, None, 0] + R64[None, :, 1] * p64[:, None, 1]) + R64[None, :, 2] * p64[:, None, 2]) + t64[None]).astype(f32)
        hit = (verdict == 0) & (p2[:, 2] <= 0) & low
        verdict[hit] = 3
        invZ1 = _recip(p[:, 2])
        im1x, im1y = fx * p[:, 0] * invZ1 + cx, fy * p[:, 1] * invZ1 + cy
        e1 = (im1x - u1[:, 0]) * (im1x - u1[:, 0]) + (im1y - v1[:, 0]) * (im1y - v1[:, 0])
        verdict[(verdict == 0) & (e1 > th2)] = 4
        invZ2 = _recip(p2[:, 2])
        im2x, im2y = fx * p2[:, 0] * invZ2 + cx, fy * p2[:, 1] * invZ2 + cy
        e2 = (im2x - u2[:, 0]) * (im2x - u2[:, 0]) + (im2y - v2[:, 0]) * (im2y - v2[:, 0])
        verdict[(verdict == 0) & (e2 > th2)] = 5
        verdict[verdict == 0] = 6
    return verdict, p, canon(cos), sw


# ---- T10 up to the parallax test ----
def accept_f(n_good, N, min_tri):
    maxGood = max(n_good[:4])
    nMinGood = max(int(0.9 * N), min_tri)
    nsimilar = sum(1 for k in range(4) if n_good[k] > 0.7 * maxGood)
    if maxGood < nMinGood:
        return -1, TOO_FEW_POINTS, 0
    if nsimilar > 1:
        return -1, NO_CLEAR_WINNER, 0
    return [k for k in range(4) if n_good[k] == maxGood][0], 0, 0


def accept_h(n_good, N, min_tri):
    best, second, idx = 0, 0, -1
    for k in range(8):
        if n_good[k] > best:
            second, best, idx = best, n_good[k], k
        elif n_good[k] > second:
            second = n_good[k]
    if not second < 0.75 * best:
        return -1, NO_CLEAR_WINNER, 0
    return idx, 0, (0 if (best > min_tri and best > 0.9 * N) else TOO_FEW_POINTS)


def parallax_deg(c):
    """a 51st cosine may round to the float32 above 1: acos is NaN there, as libm's is in the library, where math.acos would raise"""
    c = float(c)
    return f32(math.acos(c) * 180 / math.pi) if -1.0 <= c <= 1.0 else f32(np.nan)


# ---- the whole of one pair ----
def twoview(xy1, xy2, matches12, K4, sets, sigma=1.0, iterations=200, min_parallax_deg=1.0, min_triangulated=50, rh_threshold=0.40):
    """-> dict with every field of iba_twoview_result, list, inlier, points, triangulated, the kept stages (Hi, H12i, Fi, score_H, score_F, and
    per motion hypothesis hyp_R, hyp_t, hyp_points, hyp_verdict), and sweep_cap_hits"""
    xy1, xy2 = np.ascontiguousarray(xy1, f32).reshape(-1, 2), np.ascontiguousarray(xy2, f32).reshape(-1, 2)
    m12 = np.ascontiguousarray(matches12, np.int32).reshape(-1)
    n1, I = len(xy1), int(iterations)
    first = np.nonzero(m12 >= 0)[0].astype(np.int32)
    lst = np.stack([first, m12[first]], 1).astype(np.int32) if len(first) else np.zeros((0, 2), np.int32)
    N = len(lst)
    z9, z3 = np.zeros((3, 3), f32), np.zeros(3, f32)
    r = {"status": OK, "n_matches": N, "model": 0, "n_hyp": 0, "chosen": -1, "best_it_H": -1, "best_it_F": -1, "n_inliers_H": 0, "n_inliers_F": 0,
         "SH": f32(0), "SF": f32(0), "RH": f32(0), "H21": z9.copy(), "F21": z9.copy(), "n_good": np.zeros(8, np.int32), "cos_parallax": np.zeros(8, f32),
         "parallax_deg": np.zeros(8, f32), "R21": z9.copy(), "t21": z3.copy(), "list": lst, "inlier": np.zeros(N, np.uint8),
         "points": np.zeros((n1, 3), f32), "triangulated": np.zeros(n1, np.uint8),
         "Hi": np.zeros((I, 3, 3), f32), "H12i": np.zeros((I, 3, 3), f32), "Fi": np.zeros((I, 3, 3), f32), "score_H": np.zeros(I, f32), "score_F": np.zeros(I, f32),
         "hyp_R": np.zeros((8, 3, 3), f32), "hyp_t": np.zeros((8, 3), f32), "hyp_points": np.zeros((8, N, 3), f32), "hyp_verdict": np.zeros((8, N), np.uint8),
         "sweep_cap_hits": 0}
    if N < 8:
        r["status"] = TOO_FEW_MATCHES
        return r
    sets = np.ascontiguousarray(sets, np.int32).reshape(I, 8)
    sigma = f32(sigma)
    pn1, T1 = normalize(xy1)
    pn2, T2 = normalize(xy2)
    T2inv, T2t = inv_affine_diag(T2), T2.T.copy()
    mxy = np.concatenate([xy1[lst[:, 0]], xy2[lst[:, 1]]], 1).astype(f32)
    mn = np.concatenate([pn1[lst[:, 0]], pn2[lst[:, 1]]], 1).astype(f32)
    pn = mn[sets]                                          # [I, 8, 4]
    invs = inv_sigma_square(sigma)
    H, Hinv, swH = h_hypotheses(pn, T1, T2inv)
    F, swF = f_hypotheses(pn, T1, T2t)
    H, Hinv, F = canon(H), canon(Hinv), canon(F)
    hits = int((swH == MAX_SWEEPS).sum() + (swF == MAX_SWEEPS).sum())
    sH, inH = score_h(H, Hinv, mxy, invs)
    sF, inF = score_f(F, mxy, invs)
    sH, sF = canon(sH), canon(sF)
    r.update(Hi=H, H12i=Hinv, Fi=F, score_H=sH, score_F=sF)
    r["best_it_H"], r["SH"] = select_best(sH)
    r["best_it_F"], r["SF"] = select_best(sF)
    flagsH = flagsF = np.zeros(N, bool)
    if r["best_it_H"] >= 0:
        r["H21"], flagsH = H[r["best_it_H"]].copy(), inH[r["best_it_H"]]
    if r["best_it_F"] >= 0:
        r["F21"], flagsF = F[r["best_it_F"]].copy(), inF[r["best_it_F"]]
    r["n_inliers_H"], r["n_inliers_F"] = int(flagsH.sum()), int(flagsF.sum())
    SH, SF = r["SH"], r["SF"]
    r["RH"] = f32(SH / f32(SH + SF)) if f32(SH + SF) > 0 else f32(0)
    r["model"] = 1 if r["RH"] > f32(rh_threshold) else 0
    inl = flagsH if r["model"] else flagsF
    r["inlier"] = inl.astype(np.uint8)
    K = make_K(*K4)
    if (r["best_it_H"] if r["model"] else r["best_it_F"]) < 0:
        r["status"] = NO_MODEL
    elif r["model"] == 0:
        R, t, sw = motions_from_f(r["F21"], K)
        hits += sw == MAX_SWEEPS
        r["n_hyp"] = 4
    else:
        R, t, sw = motions_from_h(r["H21"], K)
        hits += sw == MAX_SWEEPS
        if R is None:
            r["status"] = H_DEGENERATE
        else:
            r["n_hyp"] = 8
    r["sweep_cap_hits"] = int(hits)
    if r["status"]:
        return r
    nh = r["n_hyp"]
    r["hyp_R"][:nh], r["hyp_t"][:nh] = R, t
    th2 = f32(f64(4.0) * f64(sigma * sigma))
    idx = np.nonzero(inl)[0]
    cosv = np.zeros((8, N), f32)
    for k in range(nh):
        r["cos_parallax"][k] = 1
        if not len(idx):
            continue
        verdict, p, cos, sw = check_rt(R[k], t[k], K, mxy[idx], th2)
        r["sweep_cap_hits"] += int((sw == MAX_SWEEPS).sum())
        r["hyp_verdict"][k, idx], r["hyp_points"][k, idx], cosv[k, idx] = verdict, p, cos
        good = np.sort(cos[verdict == 6])
        r["n_good"][k] = len(good)
        if len(good):
            r["cos_parallax"][k] = good[min(50, len(good) - 1)]
    r["cos_parallax"] = canon(r["cos_parallax"])
    n_inl = r["n_inliers_H"] if r["model"] else r["n_inliers_F"]
    cand, before, after = (accept_h if r["model"] else accept_f)([int(v) for v in r["n_good"]], n_inl, int(min_triangulated))
    for k in range(nh):
        r["parallax_deg"][k] = parallax_deg(r["cos_parallax"][k])
    if before:
        r["status"] = before
        return r
    r["chosen"] = cand
    par = r["parallax_deg"][cand]
    enough = par >= f32(min_parallax_deg) if r["model"] else par > f32(min_parallax_deg)
    r["status"] = LOW_PARALLAX if not enough else (after if after else OK)
    if r["status"] == OK:
        r["R21"], r["t21"] = R[cand].copy(), t[cand].copy()
        good = r["hyp_verdict"][cand] == 6
        r["points"][lst[good, 0]] = r["hyp_points"][cand, good]
        r["triangulated"][lst[good & (cosv[cand].astype(f64) < 0.99998), 0]] = 1
    return r

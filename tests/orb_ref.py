"""Numpy restatement of the ORB extraction rules O1-O10 of include/iba_mi355x.h, written from the rules and sharing no code with the library. Every
float32 step is rounded on its own (constants are wrapped in F()), integers are numpy integers, and the f64 sine / cosine mirrors the library's fixed
operation sequence in Python floats. extract() returns every stage and the statistics the tests assert on."""
import math

import numpy as np

F = np.float32
MINB, EDGE, HALF = 16, 19, 15
CIRCLE = [(0, -3), (1, -3), (2, -2), (3, -1), (3, 0), (3, 1), (2, 2), (1, 3), (0, 3), (-1, 3), (-2, 2), (-3, 1), (-3, 0), (-3, -1), (-2, -2), (-1, -3)]
BLUR_W = np.array([18, 34, 49, 54, 49, 34, 18], np.int64)


def _round_half_away(r):
    n = int(r)
    return n + 1 if float(r) - n >= 0.5 else n


def umax_table():
    vmax = int(np.floor(F(F(F(HALF) * np.sqrt(F(2))) / F(2)) + F(1)))
    vmin = int(np.ceil(F(F(HALF) * np.sqrt(F(2))) / F(2)))
    um = [0] * 17
    for v in range(vmax + 1):
        um[v] = int(np.rint(math.sqrt(HALF * HALF - v * v)))
    v0 = 0
    for v in range(HALF, vmin - 1, -1):
        while um[v0] == um[v0 + 1]:
            v0 += 1
        um[v] = v0
        v0 += 1
    return um[:16]


def plan(W, H, n_features=2000, scale_factor=1.2, n_levels=8):
    """O1, O3 and the start nodes of O6 -> dict like the library's plan, plus sf"""
    scale = F(scale_factor)
    sf = [F(1)]
    for _ in range(1, n_levels):
        sf.append(F(sf[-1] * scale))
    factor = F(F(1) / scale)
    d = F(F(F(n_features) * F(F(1) - factor)) / F(F(1) - F(math.pow(float(factor), float(n_levels)))))
    feats, total = [], 0
    for l in range(n_levels - 1):
        feats.append(int(np.rint(d)))
        total += feats[-1]
        d = F(d * factor)
    feats.append(max(n_features - total, 0))
    wh, cells, n_ini = [], [], []
    for l in range(n_levels):
        inv = F(F(1) / sf[l])
        Wl, Hl = int(np.rint(F(F(W) * inv))), int(np.rint(F(F(H) * inv)))
        if Wl < 1 or Hl < 1:
            Wl = Hl = 0
        wh.append((Wl, Hl))
        width, height = Wl - 2 * MINB, Hl - 2 * MINB
        nC, nR = (width // 30, height // 30) if width > 0 and height > 0 else (0, 0)
        if nC < 1 or nR < 1:
            cells.append((0, 0, 0, 0))
            n_ini.append(0)
            continue
        cells.append((nC, nR, int(np.ceil(F(F(width) / F(nC)))), int(np.ceil(F(F(height) / F(nR))))))
        n_ini.append(_round_half_away(F(F(width) / F(height))))
    return {"level_wh": np.array(wh, np.int32), "features_per_level": np.array(feats, np.int32), "cells": np.array(cells, np.int32),
            "n_ini": np.array(n_ini, np.int32), "umax": np.array(umax_table(), np.int32), "sf": sf}


def cell_regions(Wl, Hl, cell):
    """the tested regions [(i, j, x0, x1, y0, y1)] of a level's cells in order (i, then j), empty ones left out"""
    nC, nR, wC, hC = (int(c) for c in cell)
    out = []
    maxBX, maxBY = Wl - MINB, Hl - MINB
    for i in range(nR):
        iniY = MINB + i * hC
        maxY = min(iniY + hC + 6, maxBY)
        if iniY >= maxBY - 3:
            continue
        for j in range(nC):
            iniX = MINB + j * wC
            maxX = min(iniX + wC + 6, maxBX)
            if iniX >= maxBX - 6:
                continue
            if iniX + 3 < maxX - 3 and iniY + 3 < maxY - 3:
                out.append((i, j, iniX + 3, maxX - 3, iniY + 3, maxY - 3))
    return out


def _axis_table(src, dst):
    scale = float(src) / float(dst)
    f = ((np.arange(dst, dtype=np.float64) + 0.5) * scale - 0.5).astype(F)
    s = np.floor(f)
    f = (f - s).astype(F)
    s = s.astype(np.int64)
    lo, hi = s < 0, s >= src - 1
    s[lo], f[lo] = 0, 0
    s[hi], f[hi] = src - 1, 0
    c1 = np.rint(f * F(2048)).astype(np.int64)
    return s, np.minimum(s + 1, src - 1), 2048 - c1, c1


def resize(src, Wd, Hd):
    """O2"""
    Hs, Ws = src.shape
    xs, xs1, a0, a1 = _axis_table(Ws, Wd)
    ys, ys1, b0, b1 = _axis_table(Hs, Hd)
    p = src.astype(np.int64)
    S = p[:, xs] * a0[None, :] + p[:, xs1] * a1[None, :]
    S0, S1 = S[ys, :], S[ys1, :]
    out = (((b0[:, None] * (S0 >> 4)) >> 16) + ((b1[:, None] * (S1 >> 4)) >> 16) + 2) >> 2
    return out.astype(np.uint8)


def fast_scores(img, min_th):
    """O4 -> uint8 map, 0 where the score is below min_th and within 3 pixels of the edge"""
    H, W = img.shape
    out = np.zeros((H, W), np.uint8)
    if H < 7 or W < 7:
        return out
    p = img.astype(np.int32)
    c = p[3:H - 3, 3:W - 3]
    d = [p[3 + dy:H - 3 + dy, 3 + dx:W - 3 + dx] - c for dx, dy in CIRCLE]
    best = np.full(c.shape, -1000, np.int32)
    for k in range(16):
        arc = [d[(k + j) % 16] for j in range(9)]
        bright = np.minimum.reduce(arc)
        dark = np.minimum.reduce([-a for a in arc])
        best = np.maximum(best, np.maximum(bright, dark))
    score = best - 1
    out[3:H - 3, 3:W - 3] = np.where(score >= min_th, score, 0).astype(np.uint8)
    return out


def _suppress(region, t):
    """O5 on a cell's tested region at threshold t -> (kept mask, ties)"""
    z = np.where(region >= t, region, 0).astype(np.int32)
    q = np.pad(z, 1)
    h, w = z.shape
    nb = [q[1 + dy:1 + dy + h, 1 + dx:1 + dx + w] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy, dx) != (0, 0)]
    m = np.maximum.reduce(nb)
    return (z > 0) & (z > m), int(np.sum((z > 0) & (z == m)))


def cell_candidates(scores, cell, ini_th, min_th):
    """O5 for a level -> xy [n, 2] relative to MINB, score [n], fallback cells, suppression ties"""
    H, W = scores.shape
    xy, sc, n_fb, ties = [], [], 0, 0
    for _, _, x0, x1, y0, y1 in cell_regions(W, H, cell):
        region = scores[y0:y1, x0:x1]
        keep, t = _suppress(region, ini_th)
        if not keep.any():
            n_fb += 1
            keep, t = _suppress(region, min_th)
        ties += t
        ys, xs = np.nonzero(keep)            # row-major: row, then column
        for y, x in zip(ys, xs):
            xy.append((x0 + x - MINB, y0 + y - MINB))
            sc.append(int(region[y, x]))
    return np.array(xy, np.int32).reshape(-1, 2), np.array(sc, np.int32), n_fb, ties


class _Node:
    __slots__ = ("UL", "UR", "BL", "BR", "keys", "no_more", "seq")

    def __init__(self, UL, UR, BL, BR, seq):
        self.UL, self.UR, self.BL, self.BR, self.keys, self.no_more, self.seq = UL, UR, BL, BR, [], False, seq


def distribute(xy, score, width, height, N):
    """O6 -> (chosen indices in node-list order, {"phase2": bool, "size_tie": bool})"""
    stats = {"phase2": False, "size_tie": False}
    n = len(score)
    n_ini = _round_half_away(F(F(width) / F(height)))
    if n_ini < 1 or n < 1:
        return np.zeros(0, np.int32), stats
    hX = F(F(width) / F(n_ini))
    counter = [0]

    def new_node(UL, UR, BL, BR):
        nd = _Node(UL, UR, BL, BR, counter[0])
        counter[0] += 1
        return nd

    nodes = []
    for i in range(n_ini):
        ulx, urx = int(F(hX * F(i))), int(F(hX * F(i + 1)))
        nodes.append(new_node((ulx, 0), (urx, 0), (ulx, height), (urx, height)))
    start = list(nodes)
    for k in range(n):
        start[int(F(F(xy[k][0]) / hX))].keys.append(k)
    kept = []
    for nd in nodes:
        if len(nd.keys) == 1:
            nd.no_more = True
        if nd.keys:
            kept.append(nd)
    nodes = kept

    def divide(nd):
        halfX = int(np.ceil(F(F(nd.UR[0] - nd.UL[0]) / F(2))))
        halfY = int(np.ceil(F(F(nd.BR[1] - nd.UL[1]) / F(2))))
        n1 = new_node(nd.UL, (nd.UL[0] + halfX, nd.UL[1]), (nd.UL[0], nd.UL[1] + halfY), (nd.UL[0] + halfX, nd.UL[1] + halfY))
        n2 = new_node(n1.UR, nd.UR, n1.BR, (nd.UR[0], nd.UL[1] + halfY))
        n3 = new_node(n1.BL, n1.BR, nd.BL, (n1.BR[0], nd.BL[1]))
        n4 = new_node(n3.UR, n2.BR, n3.BR, nd.BR)
        for k in nd.keys:
            x, y = int(xy[k][0]), int(xy[k][1])
            if x < n1.UR[0]:
                (n1 if y < n1.BR[1] else n3).keys.append(k)
            else:
                (n2 if y < n1.BR[1] else n4).keys.append(k)
        for c in (n1, n2, n3, n4):
            c.no_more = len(c.keys) == 1
        return [n1, n2, n3, n4]

    def push_children(nd, record):
        added = 0
        for c in divide(nd):
            if c.keys:
                nodes.insert(0, c)
                if len(c.keys) > 1:
                    added += 1
                    record.append(c)
        return added

    finish = False
    while not finish:
        prev, n_expand, record = len(nodes), 0, []
        for nd in list(nodes):               # children go to the front and are not visited in this pass
            if nd.no_more:
                continue
            n_expand += push_children(nd, record)
            nodes.remove(nd)
        if len(nodes) >= N or len(nodes) == prev:
            finish = True
        elif len(nodes) + n_expand * 3 > N:
            stats["phase2"] = True
            while not finish:
                prev = len(nodes)
                todo = sorted(record, key=lambda c: (len(c.keys), c.seq))   # the library's own tie rule: equal sizes, the later node first
                if any(len(todo[j].keys) == len(todo[j - 1].keys) for j in range(1, len(todo))):
                    stats["size_tie"] = True
                record = []
                for nd in reversed(todo):
                    push_children(nd, record)
                    nodes.remove(nd)
                    if len(nodes) >= N:
                        break
                if len(nodes) >= N or len(nodes) == prev:
                    finish = True
    chosen = []
    for nd in nodes:
        best = nd.keys[0]
        for k in nd.keys[1:]:
            if score[k] > score[best]:
                best = k
        chosen.append(best)
    return np.array(chosen, np.int32), stats


_K = F(180.0 / math.pi)
_P1, _P3, _P5, _P7 = F(F(0.9997878412794807) * _K), F(F(-0.3258083974640975) * _K), F(F(0.1555786518463281) * _K), F(F(-0.04432655554792128) * _K)
_EPS = F(2.220446049250313e-16)


def atan2_deg(y, x):
    """O7's polynomial on float32 scalars"""
    y, x = F(y), F(x)
    ax, ay = F(abs(x)), F(abs(y))
    if ax >= ay:
        c = F(ay / F(ax + _EPS))
        c2 = F(c * c)
        a = F(F(F(F(F(F(F(_P7 * c2) + _P5) * c2) + _P3) * c2) + _P1) * c)
    else:
        c = F(ax / F(ay + _EPS))
        c2 = F(c * c)
        a = F(F(90) - F(F(F(F(F(F(F(_P7 * c2) + _P5) * c2) + _P3) * c2) + _P1) * c))
    if x < 0:
        a = F(F(180) - a)
    if y < 0:
        a = F(F(360) - a)
    return a


def sincos(x):
    """O9's f64 pair (cos, sin) of x radians: scalars or float64 arrays, the library's operation sequence"""
    x = np.asarray(x, np.float64)
    two_over_pi, pio2_hi, pio2_lo = 6.36619772367581382433e-01, 1.57079632673412561417e+00, 6.07710050650619224932e-11
    q = np.floor(x * two_over_pi + 0.5)
    r = (x - q * pio2_hi) - q * pio2_lo
    z = r * r
    S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04, 2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
    Cc = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05, -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)
    ps = S[0] + z * (S[1] + z * (S[2] + z * (S[3] + z * (S[4] + z * S[5]))))
    pc = Cc[0] + z * (Cc[1] + z * (Cc[2] + z * (Cc[3] + z * (Cc[4] + z * Cc[5]))))
    s = r + (r * z) * ps
    c = (1.0 - 0.5 * z) + (z * z) * pc
    k = q.astype(np.int64) & 3
    return np.choose(k, [c, -s, -c, s]), np.choose(k, [s, c, -s, -c])


def angle_ab(angle_deg):
    """(a, b) = (cos, sin) as float32 of float32 degrees (scalars or arrays)"""
    a_rad = (np.asarray(angle_deg, F) * F(math.pi / 180.0)).astype(F)
    c, s = sincos(a_rad.astype(np.float64))
    return c.astype(F), s.astype(F)


def orientation(img, x, y, umax):
    m10 = m01 = 0
    for v in range(-HALF, HALF + 1):
        lim = int(umax[abs(v)])
        row = img[y + v, x - lim:x + lim + 1].astype(np.int64)
        m10 += int(np.sum(np.arange(-lim, lim + 1) * row))
        m01 += v * int(np.sum(row))
    return atan2_deg(F(m01), F(m10))


def blur(img):
    """O8"""
    p = np.pad(img.astype(np.int64), 3, mode="reflect")
    H, W = img.shape
    hs = sum(BLUR_W[q] * p[:, q:q + W] for q in range(7))
    assert hs.max() < 65536
    vs = sum(BLUR_W[q] * hs[q:q + H, :] for q in range(7))
    return ((vs + 32768) >> 16).astype(np.uint8)


def describe(blurred, x, y, angle, pattern, stats=None):
    """O9 for one keypoint -> 32 bytes"""
    a, b = angle_ab(angle)
    pat = np.asarray(pattern, np.int8).reshape(256, 4).astype(F)
    vals = []
    for ox, oy in ((0, 1), (2, 3)):
        px, py = pat[:, ox], pat[:, oy]
        fr = ((px * b).astype(F) + (py * a).astype(F)).astype(F)
        fc = ((px * a).astype(F) - (py * b).astype(F)).astype(F)
        if stats is not None:
            stats["rint_ties"] = stats.get("rint_ties", 0) + int(np.sum(np.abs(fr - np.trunc(fr)) == 0.5) + np.sum(np.abs(fc - np.trunc(fc)) == 0.5))
        vals.append(blurred[y + np.rint(fr).astype(np.int64), x + np.rint(fc).astype(np.int64)].astype(np.int32))
    bits = (vals[0] < vals[1]).astype(np.uint8).reshape(32, 8)
    return np.sum(bits << np.arange(8, dtype=np.uint8)[None, :], axis=1).astype(np.uint8)


def extract(img, pattern, n_features=2000, scale_factor=1.2, n_levels=8, ini_th_fast=20, min_th_fast=7):
    """O1-O10 for one image -> dict of every stage, the outputs and the statistics"""
    img = np.ascontiguousarray(img, np.uint8)
    H, W = img.shape
    pl = plan(W, H, n_features, scale_factor, n_levels)
    out = {"plan": pl, "levels": [], "scores": [], "cand_xy": [], "cand_score": [], "blurred": [], "per_level": [], "candidates_per_level": [],
           "fallback_cells_per_level": [], "stats": {"fallback_cells": 0, "suppression_ties": 0, "phase2": False, "size_tie": False}}
    kp = {"xy": [], "angle": [], "response": [], "octave": [], "size": [], "desc": []}
    for l in range(n_levels):
        Wl, Hl = (int(v) for v in pl["level_wh"][l])
        if Wl < 1:
            lvl = np.zeros((0, 0), np.uint8)
        else:
            lvl = img if l == 0 else resize(out["levels"][l - 1], Wl, Hl)
        out["levels"].append(lvl)
        sc = fast_scores(lvl, min_th_fast) if Wl >= 1 else lvl
        out["scores"].append(sc)
        cxy, csc, n_fb, ties = cell_candidates(sc, pl["cells"][l], ini_th_fast, min_th_fast) if pl["cells"][l][0] else (np.zeros((0, 2), np.int32), np.zeros(0, np.int32), 0, 0)
        out["cand_xy"].append(cxy)
        out["cand_score"].append(csc)
        out["candidates_per_level"].append(len(csc))
        out["fallback_cells_per_level"].append(n_fb)
        out["stats"]["fallback_cells"] += n_fb
        out["stats"]["suppression_ties"] += ties
        chosen = np.zeros(0, np.int32)
        if pl["cells"][l][0]:
            chosen, st = distribute(cxy, csc, Wl - 2 * MINB, Hl - 2 * MINB, int(pl["features_per_level"][l]))
            out["stats"]["phase2"] |= st["phase2"]
            out["stats"]["size_tie"] |= st["size_tie"]
        out["per_level"].append(len(chosen))
        bl = blur(lvl) if len(chosen) else np.zeros_like(lvl)
        out["blurred"].append(bl)
        sf = pl["sf"][l]
        for c in chosen:
            x, y = int(cxy[c][0]) + MINB, int(cxy[c][1]) + MINB
            ang = orientation(lvl, x, y, pl["umax"])
            kp["xy"].append((F(F(x) * sf), F(F(y) * sf)))
            kp["angle"].append(ang)
            kp["response"].append(F(csc[c]))
            kp["octave"].append(l)
            kp["size"].append(F(int(F(F(31) * sf))))
            kp["desc"].append(describe(bl, x, y, ang, pattern))
    n = len(kp["octave"])
    out.update(xy=np.array(kp["xy"], F).reshape(n, 2), angle=np.array(kp["angle"], F), response=np.array(kp["response"], F), octave=np.array(kp["octave"], np.int32),
               size=np.array(kp["size"], F), desc=np.array(kp["desc"], np.uint8).reshape(n, 32), n_keypoints=n)
    return out

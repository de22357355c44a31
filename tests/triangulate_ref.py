"""The new-map-point creation restated in numpy from the rules R1-R8 of include/iba_mi355x.h, SEQUENTIALLY AS THE REFERENCE IS WRITTEN: neighbour after
neighbour, with a has_point array of the current keyframe that is updated after each neighbour's search and triangulation, and R3 as the literal
walk with bestDist (NOT as the key minimum the library computes, nor as the independent outcomes plus R7 the device computes), so a comparison checks
both arguments independently. float32 scalars and arrays throughout (every operation rounded, left to right), float64 where the rules say double;
the 3 x 3 operations and the Jacobi null vector are twoview_ref's. The matching walk is scalar per query; R4-R6 are vectorised over the matches of
one neighbour, which are independent. A keyframe is a dict (frame, Tcw [12] f32, K = (fx, fy, cx, cy), node [n] i32, has_point [n] u8 or None,
median_depth); a job a dict (current, neighbours, scale_factors, level_sigma2, scale_factor)."""
import numpy as np

import map_match_ref as L
import orb_match_ref as M
import twoview_ref as TV

F, D = np.float32, np.float64
(CREATED, HAS_POINT, NO_NODE, PAIR_SKIPPED, NO_MATCH, PARALLAX, DEGENERATE, DEPTH1, DEPTH2, REPROJ1, REPROJ2, ZERO_DIST, SCALE, SUPERSEDED) = range(14)
N_STATUS = 14
NAMES = ("CREATED", "HAS_POINT", "NO_NODE", "PAIR_SKIPPED", "NO_MATCH", "PARALLAX", "DEGENERATE", "DEPTH1", "DEPTH2", "REPROJ1", "REPROJ2", "ZERO_DIST", "SCALE", "SUPERSEDED")
DEFAULTS = dict(th_low=50, min_baseline_ratio=0.01, max_cos_parallax=0.9998, epipole_gate=100.0, chi2_line=3.84, chi2_mono=5.991)


def make_keyframe(frame, Tcw, K, node, has_point=None, median_depth=1.0):
    return {"frame": int(frame), "Tcw": np.ascontiguousarray(np.asarray(Tcw, F).reshape(-1)[:12]), "K": tuple(F(v) for v in K), "node": np.ascontiguousarray(node, np.int32).reshape(-1),
            "has_point": None if has_point is None else np.ascontiguousarray(has_point, np.uint8).reshape(-1), "median_depth": F(median_depth)}


def make_job(current, neighbours, scale_factors, level_sigma2, scale_factor):
    return {"current": int(current), "neighbours": np.ascontiguousarray(neighbours, np.int32).reshape(-1), "scale_factors": np.ascontiguousarray(scale_factors, F).reshape(-1),
            "level_sigma2": np.ascontiguousarray(level_sigma2, F).reshape(-1), "scale_factor": F(scale_factor)}


def div_f(a, b):
    """the correctly rounded float32 quotient"""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F).astype(D) / np.asarray(b, F).astype(D)).astype(F)


def camera(kf):
    T = kf["Tcw"]
    fx, fy, cx, cy = kf["K"]
    return {"T": T.reshape(3, 4), "R": np.ascontiguousarray(T.reshape(3, 4)[:, :3]), "t": np.ascontiguousarray(T.reshape(3, 4)[:, 3]), "Ow": np.array(L.camera_centre(T), F),
            "fx": fx, "fy": fy, "cx": cx, "cy": cy, "invfx": F(div_f(F(1), fx)), "invfy": F(div_f(F(1), fy)), "median_depth": kf["median_depth"]}


def prologue(c1, c2, min_baseline_ratio):
    """R1 -> (skipped, baseline, F12 [3, 3] f32, ex, ey)"""
    with np.errstate(all="ignore"):
        b = (c2["Ow"] - c1["Ow"]).astype(F)
        baseline = F(TV.norm3(b))
        skipped = bool(D(div_f(baseline, c2["median_depth"])) < D(F(min_baseline_ratio)))
        R12 = TV.mul33(c1["R"], np.ascontiguousarray(c2["R"].T))
        v = TV.mul331(R12, c2["t"])
        t12 = (-v + c1["t"]).astype(F)
        z = F(0)
        tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], F)
        K1, K2 = TV.make_K(c1["fx"], c1["fy"], c1["cx"], c1["cy"]), TV.make_K(c2["fx"], c2["fy"], c2["cx"], c2["cy"])
        F12 = TV.mul33(TV.mul33(TV.mul33(TV.inv33(np.ascontiguousarray(K1.T)), tx), R12), TV.inv33(K2))
        C2 = (TV.mul331(c2["R"], c1["Ow"]) + c2["t"]).astype(F)
        invz = F(div_f(F(1), C2[2]))
        ex = F(F(F(c2["fx"] * C2[0]) * invz) + c2["cx"])
        ey = F(F(F(c2["fy"] * C2[1]) * invz) + c2["cy"])
    return skipped, baseline, F12, ex, ey


def line_of(F12, x1, y1):
    with np.errstate(all="ignore"):
        a = F(F(F(x1 * F12[0, 0]) + F(y1 * F12[1, 0])) + F12[2, 0])
        b = F(F(F(x1 * F12[0, 1]) + F(y1 * F12[1, 1])) + F12[2, 1])
        c = F(F(F(x1 * F12[0, 2]) + F(y1 * F12[1, 2])) + F12[2, 2])
        den = F(F(a * a) + F(b * b))
    return a, b, c, den


def inside_epipole_gate(ex, ey, x2, y2, sf2, gate):
    with np.errstate(all="ignore"):
        dx, dy = F(ex - x2), F(ey - y2)
        return bool(F(F(dx * dx) + F(dy * dy)) < F(F(gate) * sf2))


def line_test(line, x2, y2, s2, chi2_line):
    a, b, c, den = line
    with np.errstate(all="ignore"):
        num = F(F(F(a * x2) + F(b * y2)) + c)
        if den == 0:
            return False, True
        dsqr = F(div_f(F(num * num), den))
        return bool(D(dsqr) < D(F(chi2_line)) * D(s2)), False


def walk(dists, passes, th_low):
    """R3's literal walk over one segment: dists [n] int, passes(pos) -> bool (the two checks of the candidate at pos; called only where the
    reference would evaluate them) -> (position or -1, distance)"""
    best_dist, best = int(th_low), -1
    for pos, d in enumerate(dists):
        d = int(d)
        if d > th_low or d > best_dist:
            continue
        if passes(pos):
            best, best_dist = pos, d
    return best, best_dist


def row_dot(T, r, x):
    """(float)(((R_r0 X + R_r1 Y) + R_r2 Z) + t_r) in double, for x [B, 3]"""
    Td, xd = T.astype(D), x.astype(D)
    with np.errstate(all="ignore"):
        return (((Td[r, 0] * xd[:, 0] + Td[r, 1] * xd[:, 1]) + Td[r, 2] * xd[:, 2]) + Td[r, 3]).astype(F)


def reprojection_fails(c, x, z, u, v, s2, chi2_mono):
    with np.errstate(all="ignore"):
        xc, yc = row_dot(c["T"], 0, x), row_dot(c["T"], 1, x)
        invz = (D(1.0) / z.astype(D)).astype(F)
        pu = ((c["fx"] * xc).astype(F) * invz).astype(F) + c["cx"]
        pv = ((c["fy"] * yc).astype(F) * invz).astype(F) + c["cy"]
        e0, e1 = (pu - u).astype(F), (pv - v).astype(F)
        err2 = ((e0 * e0).astype(F) + (e1 * e1).astype(F)).astype(F)
        return err2.astype(D) > D(F(chi2_mono)) * s2.astype(D)


def triangulate(c1, c2, sf, sigma2, scale_factor, u1, v1, o1, u2, v2, o2, max_cos_parallax, chi2_mono):
    """R4-R6 for B matches -> (status [B], x [B, 3] f32, zeros where no point was formed)"""
    B = len(u1)
    status, xyz = np.full(B, -1, np.int32), np.zeros((B, 3), F)
    if not B:
        return status, xyz
    one = np.ones(B, F)
    with np.errstate(all="ignore"):
        xn1 = np.stack([((u1 - c1["cx"]).astype(F) * c1["invfx"]).astype(F), ((v1 - c1["cy"]).astype(F) * c1["invfy"]).astype(F), one], 1)
        xn2 = np.stack([((u2 - c2["cx"]).astype(F) * c2["invfx"]).astype(F), ((v2 - c2["cy"]).astype(F) * c2["invfy"]).astype(F), one], 1)
        ray1, ray2 = TV.mul331(np.ascontiguousarray(c1["R"].T), xn1), TV.mul331(np.ascontiguousarray(c2["R"].T), xn2)
        r1, r2 = ray1.astype(D), ray2.astype(D)
        dot = (r1[:, 0] * r2[:, 0] + r1[:, 1] * r2[:, 1]) + r1[:, 2] * r2[:, 2]
        cos = (dot / (TV.norm3(ray1) * TV.norm3(ray2))).astype(F)
        tri = (cos > 0) & (cos.astype(D) < D(F(max_cos_parallax)))
        status[~tri] = PARALLAX
        T1, T2 = c1["T"], c2["T"]
        A = np.zeros((B, 4, 4), F)
        A[:, 0] = (xn1[:, 0, None] * T1[2][None, :]).astype(F) - T1[0][None, :]
        A[:, 1] = (xn1[:, 1, None] * T1[2][None, :]).astype(F) - T1[1][None, :]
        A[:, 2] = (xn2[:, 0, None] * T2[2][None, :]).astype(F) - T2[0][None, :]
        A[:, 3] = (xn2[:, 1, None] * T2[2][None, :]).astype(F) - T2[1][None, :]
        h, _ = TV.null_vector(A)
        x = (h[:, :3].astype(D) / h[:, 3:4].astype(D)).astype(F)
        deg = (h[:, 3] == 0) | ~np.isfinite(x).all(1)
        status[tri & deg] = DEGENERATE
        live = tri & ~deg
        x = np.where(live[:, None], x, F(0)).astype(F)
        xyz[:] = x
        z1, z2 = row_dot(T1, 2, x), row_dot(T2, 2, x)
        n1, n2 = (x - c1["Ow"][None, :]).astype(F), (x - c2["Ow"][None, :]).astype(F)
        dist1, dist2 = TV.norm3(n1).astype(F), TV.norm3(n2).astype(F)
        ratio_dist, ratio_octave, ratio_factor = div_f(dist2, dist1), div_f(sf[o1], sf[o2]), F(F(1.5) * scale_factor)
        gates = ((DEPTH1, z1 <= 0), (DEPTH2, z2 <= 0), (REPROJ1, reprojection_fails(c1, x, z1, u1, v1, sigma2[o1], chi2_mono)),
                 (REPROJ2, reprojection_fails(c2, x, z2, u2, v2, sigma2[o2], chi2_mono)), (ZERO_DIST, (dist1 == 0) | (dist2 == 0)),
                 (SCALE, ((ratio_dist * ratio_factor).astype(F) < ratio_octave) | (ratio_dist > (ratio_octave * ratio_factor).astype(F))))
        for code, refused in gates:                      # the reference's order: the first gate that refuses names the status
            status[live & (status < 0) & refused] = code
        status[live & (status < 0)] = CREATED
    return status, xyz


def new_points(c1, c2, sf, x, o1):
    """R8 for B created points -> (normal [B, 3], min_dist [B], max_dist [B])"""
    with np.errstate(all="ignore"):
        d1, d2 = (x - c1["Ow"][None, :]).astype(F), (x - c2["Ow"][None, :]).astype(F)
        l1, l2 = TV.norm3(d1), TV.norm3(d2)
        a, b = (d1.astype(D) / l1[:, None]).astype(F), (d2.astype(D) / l2[:, None]).astype(F)
        normal = TV.canon(((a + b).astype(F) * F(0.5)).astype(F))
        max_d = (l1.astype(F) * sf[o1]).astype(F)
        min_d = div_f(max_d, sf[-1])
    return normal.reshape(-1, 3), min_d, max_d


def run_job(frames, keyframes, job, **opts):
    """R1-R8 for one job -> dict: status, match, dist [n_nb, n], xyz [n_nb, n, 3], seg_len [n_nb, n], counts [14], n_matches, n_created_of [n_nb], points,
    and for the tests' conditions on a scene: baseline, skipped [n_nb], n_equal_replaced, n_epipole_refused, n_line_refused, n_den_zero (a refusal
    of a candidate that would otherwise have been taken), n_has_point_walked"""
    o = {**DEFAULTS, **opts}
    kf1 = keyframes[job["current"]]
    f1 = frames[kf1["frame"]]
    c1 = camera(kf1)
    sf, sigma2 = job["scale_factors"], job["level_sigma2"]
    n, n_nb = len(f1["octave"]), len(job["neighbours"])
    given = np.zeros(n, bool) if kf1["has_point"] is None else kf1["has_point"].astype(bool)
    has_point = given.copy()                               # mpCurrentKeyFrame's map points, as the job goes on
    out = {"status": np.zeros((n_nb, n), np.uint8), "match": np.full((n_nb, n), -1, np.int32), "dist": np.full((n_nb, n), -1, np.int32), "xyz": np.zeros((n_nb, n, 3), F),
           "seg_len": np.zeros((n_nb, n), np.int32), "n_matches": np.zeros(n_nb, np.int32), "n_created_of": np.zeros(n_nb, np.int32), "baseline": np.zeros(n_nb, F),
           "skipped": np.zeros(n_nb, bool)}
    diag = {"n_equal_replaced": 0, "n_epipole_refused": 0, "n_line_refused": 0, "n_den_zero": 0, "n_has_point_walked": 0}
    pts = {"idx1": [], "neighbour": [], "idx2": [], "xyz": [], "normal": [], "min_dist": [], "max_dist": [], "desc": []}
    for pos, nb in enumerate(job["neighbours"]):
        kf2 = keyframes[nb]
        f2 = frames[kf2["frame"]]
        c2 = camera(kf2)
        has2 = np.zeros(len(f2["octave"]), bool) if kf2["has_point"] is None else kf2["has_point"].astype(bool)
        skipped, baseline, F12, ex, ey = prologue(c1, c2, o["min_baseline_ratio"])
        out["baseline"][pos], out["skipped"][pos] = baseline, skipped
        by_node = {}
        for i2, v in enumerate(kf2["node"]):
            if v >= 0:
                by_node.setdefault(int(v), []).append(i2)
        st = out["status"][pos]
        matched = []
        for i in range(n):
            cand = by_node.get(int(kf1["node"][i]), []) if kf1["node"][i] >= 0 else []
            if not skipped and not given[i]:
                out["seg_len"][pos, i] = len(cand)
            if has_point[i] and not given[i]:
                st[i] = SUPERSEDED                         # the point an earlier neighbour of this job gave it
            elif skipped:
                st[i] = PAIR_SKIPPED
            elif has_point[i]:
                st[i] = HAS_POINT
            elif not cand:
                st[i] = NO_NODE
            else:
                x1, y1 = f1["xy"][i]
                line = line_of(F12, x1, y1)
                dists = M.hamming(f1["desc"][i], f2["desc"][cand])
                seen = {"last": None}

                def passes(p, cand=cand, line=line, dists=dists, seen=seen):
                    i2 = cand[p]
                    o2 = f2["octave"][i2]
                    x2, y2 = f2["xy"][i2]
                    if inside_epipole_gate(ex, ey, x2, y2, sf[o2], o["epipole_gate"]):
                        diag["n_epipole_refused"] += 1
                        return False
                    ok, den_zero = line_test(line, x2, y2, sigma2[o2], o["chi2_line"])
                    diag["n_den_zero"] += int(den_zero)
                    diag["n_line_refused"] += int(not ok and not den_zero)
                    if ok and seen["last"] is not None and int(dists[p]) == seen["last"]:
                        diag["n_equal_replaced"] += 1
                    if ok:
                        seen["last"] = int(dists[p])
                    return ok

                free = [p for p in range(len(cand)) if not has2[cand[p]]]
                diag["n_has_point_walked"] += len(cand) - len(free)
                best, best_dist = walk([dists[p] for p in free], lambda q: passes(free[q]), o["th_low"])
                if best < 0:
                    st[i] = NO_MATCH
                else:
                    out["match"][pos, i], out["dist"][pos, i] = cand[free[best]], best_dist
                    matched.append(i)
        # ---- the reference's nmatches, then R4-R6 on every match ----
        out["n_matches"][pos] = len(matched)
        m1 = np.array(matched, np.int64)
        m2 = out["match"][pos, m1].astype(np.int64)
        status, xyz = triangulate(c1, c2, sf, sigma2, job["scale_factor"], f1["xy"][m1, 0], f1["xy"][m1, 1], f1["octave"][m1], f2["xy"][m2, 0], f2["xy"][m2, 1], f2["octave"][m2],
                                  o["max_cos_parallax"], o["chi2_mono"])
        st[m1] = status
        out["xyz"][pos, m1] = xyz
        made = m1[status == CREATED]
        if len(made):
            normal, min_d, max_d = new_points(c1, c2, sf, out["xyz"][pos, made], f1["octave"][made])
            pts["idx1"].extend(made.tolist()); pts["neighbour"].extend([pos] * len(made)); pts["idx2"].extend(out["match"][pos, made].tolist())
            pts["xyz"].extend(out["xyz"][pos, made]); pts["normal"].extend(normal); pts["min_dist"].extend(min_d); pts["max_dist"].extend(max_d)
            pts["desc"].extend(f1["desc"][made])
            has_point[made] = True                         # mpCurrentKeyFrame->AddMapPoint, after the neighbour's whole search
        out["n_created_of"][pos] = len(made)
    out["counts"] = np.bincount(out["status"].reshape(-1), minlength=N_STATUS).astype(np.int32)
    out["n_created"] = int(out["counts"][CREATED])
    out["points"] = {"idx1": np.array(pts["idx1"], np.int32), "neighbour": np.array(pts["neighbour"], np.int32), "idx2": np.array(pts["idx2"], np.int32),
                     "xyz": np.array(pts["xyz"], F).reshape(-1, 3), "normal": np.array(pts["normal"], F).reshape(-1, 3), "min_dist": np.array(pts["min_dist"], F),
                     "max_dist": np.array(pts["max_dist"], F), "desc": np.array(pts["desc"], np.uint8).reshape(-1, 32)}
    out.update(diag)
    out["n_keypoints"], out["n_neighbours"] = n, n_nb
    return out


def run(frames, keyframes, jobs, **opts):
    return [run_job(frames, keyframes, j, **opts) for j in jobs]


def median_depth(Tcw, xyz, q=2):
    """KeyFrame::ComputeSceneMedianDepth(q)"""
    T = np.asarray(Tcw, F).reshape(-1)[:12].astype(D)
    X = np.asarray(xyz, F).reshape(-1, 3).astype(D)
    z = (((T[8] * X[:, 0] + T[9] * X[:, 1]) + T[10] * X[:, 2]).astype(F) + F(T[11])).astype(F)
    return np.sort(z)[(len(z) - 1) // q]

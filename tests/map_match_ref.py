"""The local-map point matching restated in numpy / plain Python from the rules L1-L6 of include/iba_mi355x.h, with float32 scalars throughout
(every operation rounded, left to right) and float64 where the rules say double. L4 is written as the reference's sequential scan (strict `<`, then
`else if <`), NOT as the two lexicographic minima the library computes, so a comparison checks that argument independently. The grid, the area
query and the descriptor distance are those of orb_match_ref (rules M2-M4). A table is a dict (xyz, normal [P, 3] f32, min_dist, max_dist [P] f32,
desc [P, 32] u8); a job is a dict (frame, Tcw [12] f32, K = (fx, fy, cx, cy), scale_factors f32, th, points or None, skip or None, occupied or None)."""
import math

import numpy as np

import orb_match_ref as M

F, D = np.float32, np.float64
IN_VIEW, SKIPPED, DEPTH, NOT_FINITE, BOUNDS, DISTANCE, ANGLE = range(7)
N_STATUS = 7


def make_table(xyz, normal, min_dist, max_dist, desc):
    return {"xyz": np.ascontiguousarray(xyz, F).reshape(-1, 3), "normal": np.ascontiguousarray(normal, F).reshape(-1, 3), "min_dist": np.ascontiguousarray(min_dist, F).reshape(-1),
            "max_dist": np.ascontiguousarray(max_dist, F).reshape(-1), "desc": np.ascontiguousarray(desc, np.uint8).reshape(-1, 32)}


def make_job(frame, Tcw, K, scale_factors, th, points=None, skip=None, occupied=None):
    return {"frame": int(frame), "Tcw": np.ascontiguousarray(np.asarray(Tcw, F).reshape(-1)[:12]), "K": tuple(F(v) for v in K), "scale_factors": np.ascontiguousarray(scale_factors, F).reshape(-1),
            "th": F(th), "points": None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1), "skip": None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1),
            "occupied": None if occupied is None else np.ascontiguousarray(occupied, np.uint8).reshape(-1)}


def camera_centre(T):
    """L1: Ow_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2)"""
    return [F(-F(F(F(T[i] * T[3]) + F(T[4 + i] * T[7])) + F(T[8 + i] * T[11]))) for i in range(3)]


def frustum(T, Ow, K, bounds, sf, limit, P, n, min_dist, max_dist):
    """L1 for one point that is not skipped -> (status, u, v, view_cos, level, ratio); the last is for the libm diagnostic"""
    fx, fy, cx, cy = K
    min_x, max_x, min_y, max_y = bounds
    X, Y, Z = (F(v) for v in P)
    with np.errstate(all="ignore"):
        pc = [F(F(F(F(T[4 * i] * X) + F(T[4 * i + 1] * Y)) + F(T[4 * i + 2] * Z)) + T[4 * i + 3]) for i in range(3)]
        if pc[2] < F(0.0):
            return DEPTH, F(0), F(0), F(0), 0, None
        invz = F(D(1.0) / D(pc[2]))
        u = F(F(F(fx * pc[0]) * invz) + cx)
        v = F(F(F(fy * pc[1]) * invz) + cy)
        if not (np.isfinite(u) and np.isfinite(v)):
            return NOT_FINITE, F(0), F(0), F(0), 0, None
        if u < min_x or u > max_x or v < min_y or v > max_y:
            return BOUNDS, F(0), F(0), F(0), 0, None
        po = [F(F(P[k]) - Ow[k]) for k in range(3)]
        dist = F(np.sqrt(D(D(D(po[0]) * D(po[0]) + D(po[1]) * D(po[1])) + D(po[2]) * D(po[2]))))
        if dist < F(F(0.8) * F(min_dist)) or dist > F(F(1.2) * F(max_dist)):
            return DISTANCE, F(0), F(0), F(0), 0, None
        view_cos = F(D(D(D(po[0]) * D(n[0]) + D(po[1]) * D(n[1])) + D(po[2]) * D(n[2])) / D(dist))
        if not np.isfinite(view_cos) or view_cos < F(limit):
            return ANGLE, F(0), F(0), F(0), 0, None
        ratio = F(F(max_dist) / dist)
    level = len(sf) - 1
    for k in range(len(sf)):
        if ratio <= sf[k]:
            level = k
            break
    return IN_VIEW, u, v, view_cos, level, ratio


def libm_level(ratio, sf):
    """the reference's own expression (MapPoint::PredictScale), a diagnostic only: ceil(log(ratio) / mfLogScaleFactor) clamped, with mfLogScaleFactor =
    log(mfScaleFactor) in float32 as Frame keeps it and the quotient of a float by a float in float32"""
    log_sf = F(math.log(float(sf[1]))) if len(sf) > 1 else F(1)
    with np.errstate(all="ignore"):
        q = F(F(np.log(F(ratio))) / log_sf)
    if not np.isfinite(q):
        return 0 if q < 0 else len(sf) - 1
    return min(max(int(math.ceil(float(q))), 0), len(sf) - 1)


def query_radius(view_cos, th, sf_level):
    """L2"""
    r = F(2.5) if D(view_cos) > D(0.998) else F(4.0)
    if th != F(1.0):
        r = F(r * th)
    return F(r * sf_level)


def run_job(frames, table, job, grids=None, th_high=100, nn_ratio=0.8, view_cos_limit=0.5):
    """L1-L5 for one job -> dict with the L5 outputs, the lists (off, index, cdist) and, for the tests' conditions on a scene: n_ratio_refused,
    n_th_refused, n_second_choice (accepted although the overall least candidate was claimed or occupied), n_nothing_left (every candidate below 256
    was claimed or occupied), n_libm_differs"""
    f = frames[job["frame"]]
    g = grids[job["frame"]] if grids is not None else M.grid(f)
    T, sf, th = job["Tcw"], job["scale_factors"], job["th"]
    Ow = camera_centre(T)
    nn_ratio = F(nn_ratio)
    pts = job["points"] if job["points"] is not None else np.arange(len(table["min_dist"]), dtype=np.int32)
    n, nk = len(pts), len(f["octave"])
    out = {"status": np.zeros(n, np.uint8), "u": np.zeros(n, F), "v": np.zeros(n, F), "view_cos": np.zeros(n, F), "level": np.zeros(n, np.int32), "radius": np.zeros(n, F),
           "match": np.full(n, -1, np.int32), "dist": np.full(n, -1, np.int32), "point_of": np.full(nk, -1, np.int32)}
    counts = np.zeros(N_STATUS, np.int32)
    has_point = np.zeros(nk, bool) if job["occupied"] is None else job["occupied"].astype(bool).copy()      # mvpMapPoints[idx] && Observations() > 0
    off, index, cdist = np.zeros(n + 1, np.int32), [], []
    n_matches = n_ratio_refused = n_th_refused = n_second_choice = n_nothing_left = n_libm_differs = 0
    for k in range(n):
        off[k + 1] = off[k]
        if job["skip"] is not None and job["skip"][k]:
            out["status"][k] = SKIPPED
            counts[SKIPPED] += 1
            continue
        p = int(pts[k])
        st, u, v, vc, level, ratio = frustum(T, Ow, job["K"], f["bounds"], sf, view_cos_limit, table["xyz"][p], table["normal"][p], table["min_dist"][p], table["max_dist"][p])
        out["status"][k] = st
        counts[st] += 1
        if st != IN_VIEW:
            continue
        n_libm_differs += int(libm_level(ratio, sf) != level)
        r = query_radius(vc, th, sf[level])
        out["u"][k], out["v"][k], out["view_cos"][k], out["level"][k], out["radius"][k] = u, v, vc, level, r
        cand = M.area(f, g, u, v, r, level - 1, level)
        d = M.hamming(table["desc"][p], f["desc"][cand]) if len(cand) else np.zeros(0, np.int32)
        off[k + 1] += len(cand)
        index.extend(int(c) for c in cand)
        cdist.extend(int(x) for x in d)
        # the reference's scan
        best_dist, best_level, best_dist2, best_level2, best_idx = 256, -1, 256, -1, -1
        for c, dc in zip(cand, d):
            if has_point[c]:
                continue
            if dc < best_dist:
                best_dist2, best_level2 = best_dist, best_level
                best_dist, best_level, best_idx = int(dc), int(f["octave"][c]), int(c)
            elif dc < best_dist2:
                best_level2, best_dist2 = int(f["octave"][c]), int(dc)
        if best_idx < 0:
            n_nothing_left += int(len(d) > 0 and int(d.min()) < 256)
            continue
        if not best_dist <= th_high:
            n_th_refused += 1
            continue
        if best_level == best_level2 and F(best_dist) > F(nn_ratio * F(best_dist2)):
            n_ratio_refused += 1
            continue
        if len(d) and int(d.min()) < best_dist:
            n_second_choice += 1
        has_point[best_idx] = True
        out["match"][k], out["dist"][k], out["point_of"][best_idx] = best_idx, best_dist, k
        n_matches += 1
    out.update({"n_points": n, "counts": counts, "n_candidates": int(off[n]), "n_matches": n_matches, "off": off, "index": np.array(index, np.int32), "cdist": np.array(cdist, np.uint16),
                "n_ratio_refused": n_ratio_refused, "n_th_refused": n_th_refused, "n_second_choice": n_second_choice, "n_nothing_left": n_nothing_left, "n_libm_differs": n_libm_differs})
    return out


def run(frames, table, jobs, **opts):
    """a call: every frame's grid once, then every job -> a list of results"""
    grids = [M.grid(f) for f in frames]
    return [run_job(frames, table, j, grids, **opts) for j in jobs]


def pose_edges(prior_point, point_of, points, table_xyz, xy, octave, inv_level_sigma2):
    """L6 -> (xyz, obs, inv_sigma2, keypoint_index)"""
    xyz, obs, w, idx = [], [], [], []
    for c in range(len(octave)):
        p = -1 if prior_point is None else int(prior_point[c])
        k = -1 if point_of is None else int(point_of[c])
        if k >= 0:
            p = int(points[k]) if points is not None else k
        if p < 0:
            continue
        xyz.append(table_xyz[p]); obs.append(xy[c]); w.append(inv_level_sigma2[octave[c]]); idx.append(c)
    return np.array(xyz, F).reshape(-1, 3), np.array(obs, F).reshape(-1, 2), np.array(w, F), np.array(idx, np.int32)

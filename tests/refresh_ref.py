"""The map-point refresh restated in numpy / plain Python from the rules S1-S7 of include/iba_mi355x.h, AS THE REFERENCE IS WRITTEN: the full N x N
matrix of distances, np.sort of each row, the element at int(0.5 * (N - 1)), and the walk with `median < BestMedian` from INT_MAX - not the rank
form the library evaluates. Float work uses float32 scalars throughout (every operation rounded, left to right) and float64 where the rules say
double. A scene is a dict: frames (orb_match_ref.make_frame), keyframes (make_keyframe), table (map_match_ref.make_table), point_bad [P] u8 or
None, ref_keyframe [P] i32, obs_off [P + 1], obs_keyframe, obs_keypoint i32, list (i32 or None)."""
import numpy as np

import map_match_ref as L1
import orb_match_ref as M

F, D = np.float32, np.float64
REFRESHED, BAD, EMPTY = range(3)
DESC_NONE, DESC_PICKED, DESC_KEPT = range(3)
GEO_NONE, GEO_UPDATED, GEO_NO_REF, GEO_DEGENERATE = range(4)
INT_MAX = 2 ** 31 - 1

make_table = L1.make_table
camera_centre = L1.camera_centre


def make_keyframe(frame, Tcw, scale_factors, bad=False):
    return {"frame": int(frame), "Tcw": np.ascontiguousarray(np.asarray(Tcw, F).reshape(-1)[:12]), "scale_factors": np.ascontiguousarray(scale_factors, F).reshape(-1), "bad": bool(bad)}


def distance_matrix(descs):
    """Distances[i][j] of ComputeDistinctiveDescriptors: every pair, the diagonal 0"""
    d = np.ascontiguousarray(descs, np.uint8).reshape(-1, 32)
    return M.POP[d[:, None, :] ^ d[None, :, :]].sum(2).astype(np.int32)


def distinctive(descs):
    """S3 as the reference walks it -> (BestIdx, BestMedian, the median of every row)"""
    N = len(descs)
    dist = distance_matrix(descs)
    best_median, best_idx, medians = INT_MAX, 0, []
    for i in range(N):
        v = np.sort(dist[i])
        median = int(v[int(0.5 * (N - 1))])
        medians.append(median)
        if median < best_median:
            best_median, best_idx = median, i
    return best_idx, best_median, medians


def po_and_length(X, Ow):
    po = [F(F(X[c]) - F(Ow[c])) for c in range(3)]
    return po, np.sqrt(D(D(D(po[0]) * D(po[0])) + D(D(po[1]) * D(po[1]))) + D(D(po[2]) * D(po[2])))


def refresh_point(sc, centres, p, keep_stages=False):
    """S1-S6 for one point -> dict of S7's outputs (medians: one per observation of the full list, -1 for a bad keyframe's)"""
    t = sc["table"]
    e0, e1 = int(sc["obs_off"][p]), int(sc["obs_off"][p + 1])
    out = {"status": EMPTY, "desc_state": DESC_NONE, "geo_state": GEO_NONE, "best_obs": -1, "best_median": -1, "n_desc": 0, "normal": t["normal"][p].copy(),
           "min_dist": t["min_dist"][p], "max_dist": t["max_dist"][p], "desc": t["desc"][p].copy(), "medians": []}
    if sc["point_bad"] is not None and sc["point_bad"][p]:
        out["status"] = BAD
        return out
    if e1 == e0:
        return out
    out["status"] = REFRESHED
    kfs, kps = sc["obs_keyframe"][e0:e1], sc["obs_keypoint"][e0:e1]
    # ComputeDistinctiveDescriptors
    rows = [k for k in range(e1 - e0) if not sc["keyframes"][kfs[k]]["bad"]]
    out["n_desc"] = len(rows)
    out["medians"] = [-1] * (e1 - e0)
    if rows:
        descs = np.stack([sc["frames"][sc["keyframes"][kfs[k]]["frame"]]["desc"][kps[k]] for k in rows])
        best_idx, best_median, medians = distinctive(descs)
        out["desc_state"], out["best_obs"], out["best_median"], out["desc"] = DESC_PICKED, rows[best_idx], best_median, descs[best_idx].copy()
        for k, m in zip(rows, medians):
            out["medians"][k] = m
    else:
        out["desc_state"] = DESC_KEPT
    # UpdateNormalAndDepth
    X = t["xyz"][p]
    total, n, degenerate, kref = [F(0.0)] * 3, e1 - e0, False, -1
    for k in range(n):
        po, length = po_and_length(X, centres[kfs[k]])
        if length == 0.0:
            degenerate = True
            continue
        total = [F(total[c] + F(D(po[c]) / length)) for c in range(3)]
        if kref < 0 and kfs[k] == sc["ref_keyframe"][p]:
            kref = k
    if degenerate:
        out["geo_state"] = GEO_DEGENERATE
        return out
    out["normal"] = np.array([F(D(total[c]) / D(n)) for c in range(3)], F)
    if kref < 0:
        out["geo_state"] = GEO_NO_REF
        return out
    ref = sc["keyframes"][kfs[kref]]
    _, length = po_and_length(X, centres[kfs[kref]])
    level = int(sc["frames"][ref["frame"]]["octave"][kps[kref]])
    sf = ref["scale_factors"]
    out["max_dist"] = F(F(length) * sf[level])
    out["min_dist"] = F(D(out["max_dist"]) / D(sf[len(sf) - 1]))
    out["geo_state"] = GEO_UPDATED
    return out


def run(sc, keep_stages=True):
    """a call -> dict of arrays per listed point, the counts and the kept medians (off, median)"""
    P = len(sc["table"]["min_dist"])
    pts = np.arange(P, dtype=np.int32) if sc["list"] is None else np.asarray(sc["list"], np.int32)
    centres = [camera_centre(k["Tcw"]) for k in sc["keyframes"]]
    cache, rows = {}, []
    for p in pts.tolist():
        if p not in cache:
            cache[p] = refresh_point(sc, centres, p)
        rows.append(cache[p])
    n = len(rows)
    res = {"status": np.array([r["status"] for r in rows], np.uint8), "desc_state": np.array([r["desc_state"] for r in rows], np.uint8),
           "geo_state": np.array([r["geo_state"] for r in rows], np.uint8), "best_obs": np.array([r["best_obs"] for r in rows], np.int32),
           "best_median": np.array([r["best_median"] for r in rows], np.int32), "n_desc": np.array([r["n_desc"] for r in rows], np.int32),
           "normal": np.array([r["normal"] for r in rows], F).reshape(n, 3), "min_dist": np.array([r["min_dist"] for r in rows], F), "max_dist": np.array([r["max_dist"] for r in rows], F),
           "desc": np.array([r["desc"] for r in rows], np.uint8).reshape(n, 32), "point": pts}
    res["counts"] = {"n_points": n, "status": np.bincount(res["status"], minlength=3).astype(np.int32), "desc_state": np.bincount(res["desc_state"], minlength=3).astype(np.int32),
                     "geo_state": np.bincount(res["geo_state"], minlength=4).astype(np.int32),
                     "n_desc_changed": int(sum(1 for r, p in zip(rows, pts) if r["desc_state"] == DESC_PICKED and not np.array_equal(r["desc"], sc["table"]["desc"][p])))}
    res["med_off"] = np.concatenate([[0], np.cumsum([len(r["medians"]) for r in rows])]).astype(np.int32)
    res["median"] = np.array([m for r in rows for m in r["medians"]], np.int32)
    return res

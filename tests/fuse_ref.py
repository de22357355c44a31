"""The map-point fusion restated in numpy / plain Python from the rules F1-F6 and U1-U5 of include/iba_mi355x.h. The device rules use float32
scalars throughout (every operation rounded, left to right) and float64 where the rules say double; F5 is written as the reference's walk (bestDist,
bestIdx, strict `<`), NOT as the lexicographic minimum the library computes. The grid, the area query and the descriptor distance are those of
orb_match_ref (rules M2-M4). The fold is a LITERAL OBJECT RESTATEMENT: MapPoint objects with an observation dict, KeyFrame objects with a holder
list, and Replace / AddObservation / IsInKeyFrame as the reference writes them, so the library's array state is checked against something that is
not itself. A table is map_match_ref's dict; a job is a dict (frame, Tcw [12] f32, K, scale_factors, inv_level_sigma2 f32, th, points or None,
skip or None)."""
import math

import numpy as np

import map_match_ref as L1
import orb_match_ref as M

F, D = np.float32, np.float64
PICKED, SKIPPED, DEPTH, NOT_FINITE, BOUNDS, DISTANCE, ANGLE, NO_CANDIDATE, NO_MATCH = range(9)
N_STATUS = 9
LOCAL, LOOP = 0, 1
OP_NONE, OP_ADD, OP_REPLACED_BY_HELD, OP_REPLACES_HELD, OP_HELD_BAD, OP_RECORD, OP_STALE_BAD, OP_STALE_IN_KEYFRAME = range(8)

make_table = L1.make_table
camera_centre = L1.camera_centre
libm_level = L1.libm_level


def make_job(frame, Tcw, K, scale_factors, inv_level_sigma2, th, points=None, skip=None):
    return {"frame": int(frame), "Tcw": np.ascontiguousarray(np.asarray(Tcw, F).reshape(-1)[:12]), "K": tuple(F(v) for v in K), "scale_factors": np.ascontiguousarray(scale_factors, F).reshape(-1),
            "inv_level_sigma2": np.ascontiguousarray(inv_level_sigma2, F).reshape(-1), "th": F(th), "points": None if points is None else np.ascontiguousarray(points, np.int32).reshape(-1),
            "skip": None if skip is None else np.ascontiguousarray(skip, np.uint8).reshape(-1)}


def frustum(T, Ow, K, bounds, sf, limit, th, P, n, min_dist, max_dist):
    """F2-F4 for one point that is not skipped -> (status, u, v, level, radius, ratio); PICKED stands for "in view"; ratio is for the libm diagnostic"""
    fx, fy, cx, cy = K
    min_x, max_x, min_y, max_y = (F(b) for b in bounds)
    X, Y, Z = (F(v) for v in P)
    out = lambda st: (st, F(0), F(0), 0, F(0), None)
    with np.errstate(all="ignore"):
        pc = [F(F(F(F(T[4 * i] * X) + F(T[4 * i + 1] * Y)) + F(T[4 * i + 2] * Z)) + T[4 * i + 3]) for i in range(3)]
        if pc[2] < F(0.0):
            return out(DEPTH)
        invz = F(D(1.0) / D(pc[2]))
        x, y = F(pc[0] * invz), F(pc[1] * invz)
        u, v = F(F(fx * x) + cx), F(F(fy * y) + cy)
        if not (np.isfinite(u) and np.isfinite(v)):
            return out(NOT_FINITE)
        if not (u >= min_x and u < max_x and v >= min_y and v < max_y):            # KeyFrame::IsInImage
            return out(BOUNDS)
        po = [F(F(P[k]) - Ow[k]) for k in range(3)]
        dist = F(np.sqrt(D(D(D(po[0]) * D(po[0]) + D(po[1]) * D(po[1])) + D(po[2]) * D(po[2]))))
        if dist < F(F(0.8) * F(min_dist)) or dist > F(F(1.2) * F(max_dist)):
            return out(DISTANCE)
        dot = D(D(D(po[0]) * D(n[0]) + D(po[1]) * D(n[1])) + D(po[2]) * D(n[2]))
        if dot < D(D(F(limit)) * D(dist)):
            return out(ANGLE)
        ratio = F(D(F(max_dist)) / D(dist))
    level = len(sf) - 1
    for k in range(len(sf)):
        if ratio <= sf[k]:
            level = k
            break
    return PICKED, u, v, level, F(F(th) * sf[level]), ratio


def walk(f, cand, dists, u, v, lv, chi2_mono, check_reprojection):
    """F5 as the reference writes it -> (bestDist, bestIdx, n_gated: candidates the gate refused)"""
    best_dist, best_idx, n_gated = 256, -1, 0
    for c, dc in zip(cand, dists):
        if check_reprojection:
            ex, ey = F(u - f["xy"][c, 0]), F(v - f["xy"][c, 1])
            e2 = F(F(ex * ex) + F(ey * ey))
            if D(F(e2 * lv[f["octave"][c]])) > D(F(chi2_mono)):
                n_gated += 1
                continue
        if dc < best_dist:
            best_dist, best_idx = int(dc), int(c)
    return best_dist, best_idx, n_gated


def run_job(frames, table, job, grids=None, th_low=50, view_cos_limit=0.5, chi2_mono=5.99, check_reprojection=1, desc=None):
    """F1-F6 for one job -> dict with the F6 outputs, the lists (off, index, cdist) and, for the tests' conditions: n_gated_winner (the least-distance
    candidate was refused by the gate), n_libm_differs. desc overrides the table's descriptors (the deviation count)."""
    f = frames[job["frame"]]
    g = grids[job["frame"]] if grids is not None else M.grid(f)
    T, sf, th, lv = job["Tcw"], job["scale_factors"], job["th"], job["inv_level_sigma2"]
    Ow = camera_centre(T)
    tdesc = table["desc"] if desc is None else desc
    pts = job["points"] if job["points"] is not None else np.arange(len(table["min_dist"]), dtype=np.int32)
    n = len(pts)
    out = {"status": np.zeros(n, np.uint8), "u": np.zeros(n, F), "v": np.zeros(n, F), "level": np.zeros(n, np.int32), "radius": np.zeros(n, F), "match": np.full(n, -1, np.int32),
           "dist": np.full(n, -1, np.int32)}
    counts = np.zeros(N_STATUS, np.int32)
    off, index, cdist = np.zeros(n + 1, np.int32), [], []
    n_gated_winner = n_libm_differs = 0
    for k in range(n):
        off[k + 1] = off[k]
        p = int(pts[k])
        if p < 0 or (job["skip"] is not None and job["skip"][k]):
            st = SKIPPED
        else:
            st, u, v, level, r, ratio = frustum(T, Ow, job["K"], f["bounds"], sf, view_cos_limit, th, table["xyz"][p], table["normal"][p], table["min_dist"][p], table["max_dist"][p])
        if st == PICKED:
            n_libm_differs += int(libm_level(ratio, sf) != level)
            out["u"][k], out["v"][k], out["level"][k], out["radius"][k] = u, v, level, r
            cand = M.area(f, g, u, v, r, level - 1, level)
            d = M.hamming(tdesc[p], f["desc"][cand]) if len(cand) else np.zeros(0, np.int32)
            off[k + 1] += len(cand)
            index.extend(int(c) for c in cand)
            cdist.extend(int(x) for x in d)
            if len(cand) == 0:
                st = NO_CANDIDATE
            else:
                best_dist, best_idx, n_gated = walk(f, cand, d, u, v, lv, chi2_mono, check_reprojection)
                if n_gated and int(d.min()) < best_dist:
                    n_gated_winner += 1
                if best_dist <= th_low and best_idx >= 0:
                    out["match"][k], out["dist"][k] = best_idx, best_dist
                else:
                    st = NO_MATCH
        out["status"][k] = st
        counts[st] += 1
    out.update({"n_points": n, "points": pts.copy(), "counts": counts, "n_candidates": int(off[n]), "n_picked": int(counts[PICKED]), "off": off, "index": np.array(index, np.int32),
                "cdist": np.array(cdist, np.uint16), "n_gated_winner": n_gated_winner, "n_libm_differs": n_libm_differs})
    return out


def run(frames, table, jobs, **opts):
    """a call: every frame's grid once, then every job -> a list of results"""
    grids = [M.grid(f) for f in frames]
    return [run_job(frames, table, j, grids, **opts) for j in jobs]


# ---- the fold as objects ----

class KeyFrame:
    def __init__(self, kid, n):
        self.id, self.mvpMapPoints = kid, [None] * n

    def GetMapPoint(self, idx):
        return self.mvpMapPoints[idx]

    def AddMapPoint(self, pMP, idx):
        self.mvpMapPoints[idx] = pMP

    def ReplaceMapPointMatch(self, idx, pMP):
        self.mvpMapPoints[idx] = pMP

    def EraseMapPointMatch(self, idx):
        self.mvpMapPoints[idx] = None


class MapPoint:
    def __init__(self, pid, world):
        self.id, self.world = pid, world
        self.mObservations = {}             # KeyFrame -> idx; iterated in keyframe-id order where an order matters
        self.mbBad, self.mpReplaced, self.mnFound, self.mnVisible, self.stale = False, None, 0, 0, False

    def isBad(self):
        return self.mbBad

    def Observations(self):
        return len(self.mObservations)

    def IsInKeyFrame(self, pKF):
        return pKF in self.mObservations

    def AddObservation(self, pKF, idx):
        if pKF in self.mObservations:
            return
        self.mObservations[pKF] = idx

    def Replace(self, pMP):
        if pMP.id == self.id:
            return
        obs = self.mObservations
        self.mObservations = {}
        self.mbBad = True
        nvisible, nfound = self.mnVisible, self.mnFound
        self.mpReplaced = pMP
        for pKF, idx in sorted(obs.items(), key=lambda kv: kv[0].id):
            if not pMP.IsInKeyFrame(pKF):
                pKF.ReplaceMapPointMatch(idx, pMP)
                pMP.AddObservation(pKF, idx)
            else:
                pKF.EraseMapPointMatch(idx)
        pMP.mnFound += nfound
        pMP.mnVisible += nvisible
        pMP.stale = True
        self.world.on_replace(pMP)


class World:
    """the map as objects, built from the arrays of a map dict (kp_off, holder, P, bad, replaced_by, found, visible); arrays() gives them back.
    refresh = (frames_of_keyframe, desc) performs ComputeDistinctiveDescriptors after every Replace, into desc [P, 32] in place."""

    def __init__(self, m, refresh=None):
        self.kfs = [KeyFrame(k, int(m["kp_off"][k + 1] - m["kp_off"][k])) for k in range(len(m["kp_off"]) - 1)]
        self.pts = [MapPoint(p, self) for p in range(m["P"])]
        self.refresh, self.n_refreshed = refresh, 0
        for p, mp in enumerate(self.pts):
            mp.mbBad, mp.mnFound, mp.mnVisible = bool(m["bad"][p]), int(m["found"][p]), int(m["visible"][p])
            mp.mpReplaced = None if m["replaced_by"][p] < 0 else self.pts[int(m["replaced_by"][p])]
        for k, kf in enumerate(self.kfs):
            for i in range(len(kf.mvpMapPoints)):
                p = int(m["holder"][m["kp_off"][k] + i])
                if p >= 0:
                    kf.mvpMapPoints[i] = self.pts[p]
                    self.pts[p].mObservations[kf] = i

    def on_replace(self, pMP):
        if self.refresh is not None:
            kf_frames, desc = self.refresh
            desc[pMP.id] = distinctive_descriptor([kf_frames[kf.id]["desc"][idx] for kf, idx in sorted(pMP.mObservations.items(), key=lambda kv: kv[0].id)])
            self.n_refreshed += 1

    def arrays(self):
        holder = np.array([-1 if mp is None else mp.id for kf in self.kfs for mp in kf.mvpMapPoints], np.int32)
        return {"holder": holder, "bad": np.array([mp.mbBad for mp in self.pts], np.uint8), "replaced_by": np.array([-1 if mp.mpReplaced is None else mp.mpReplaced.id for mp in self.pts], np.int32),
                "found": np.array([mp.mnFound for mp in self.pts], np.int32), "visible": np.array([mp.mnVisible for mp in self.pts], np.int32),
                "descriptor_stale": np.array([mp.stale for mp in self.pts], np.uint8)}

    def fold(self, keyframe, points, status, match, mode=LOCAL):
        """the tail of Fuse over a job's picks, list position after list position -> (op, other, nFused)"""
        pKF = self.kfs[keyframe]
        n = len(points)
        op, other, nFused = np.zeros(n, np.int32), np.full(n, -1, np.int32), 0
        for i in range(n):
            if status[i] != PICKED:
                continue
            pMP = self.pts[int(points[i])]
            if pMP.isBad():
                op[i] = OP_STALE_BAD
                continue
            if pMP.IsInKeyFrame(pKF):
                op[i] = OP_STALE_IN_KEYFRAME
                continue
            bestIdx = int(match[i])
            pMPinKF = pKF.GetMapPoint(bestIdx)
            if pMPinKF is not None:
                other[i] = pMPinKF.id
                if not pMPinKF.isBad():
                    if mode == LOOP:
                        op[i] = OP_RECORD
                    elif pMPinKF.Observations() > pMP.Observations():
                        op[i] = OP_REPLACED_BY_HELD
                        pMP.Replace(pMPinKF)
                    else:
                        op[i] = OP_REPLACES_HELD
                        pMPinKF.Replace(pMP)
                else:
                    op[i] = OP_HELD_BAD
            else:
                op[i] = OP_ADD
                pMP.AddObservation(pKF, bestIdx)
                pKF.AddMapPoint(pMP, bestIdx)
            nFused += 1
        return op, other, nFused

    def skip(self, keyframe, points):
        pKF = self.kfs[keyframe]
        return np.array([1 if (p < 0 or self.pts[p].isBad() or self.pts[p].IsInKeyFrame(pKF)) else 0 for p in (int(x) for x in points)], np.uint8)

    def candidates(self, targets):
        """vpFuseCandidates"""
        out, mark = [], set()
        for t in targets:
            for pMP in self.kfs[int(t)].mvpMapPoints:
                if pMP is None:
                    continue
                if pMP.isBad() or pMP.id in mark:
                    continue
                mark.add(pMP.id)
                out.append(pMP.id)
        return np.array(out, np.int32)


def distinctive_descriptor(descs):
    """MapPoint::ComputeDistinctiveDescriptors: the descriptor with the least median of distances to the others (the first at a tie)"""
    n = len(descs)
    A = np.array(descs, np.uint8).reshape(n, 32)
    dist = np.array([[int(M.hamming(A[i], A[j:j + 1])[0]) for j in range(n)] for i in range(n)])
    best_median, best_idx = 2 ** 31 - 1, 0
    for i in range(n):
        med = sorted(dist[i].tolist())[int(0.5 * (n - 1))]
        if med < best_median:
            best_median, best_idx = med, i
    return A[best_idx].copy()


def make_map(kp_n, P, holder=None):
    """a map dict over K keyframes with kp_n[k] keypoints"""
    kp_off = np.concatenate([[0], np.cumsum(kp_n)]).astype(np.int32)
    return {"kp_off": kp_off, "holder": np.full(int(kp_off[-1]), -1, np.int32) if holder is None else np.ascontiguousarray(holder, np.int32).copy(), "P": int(P),
            "bad": np.zeros(P, np.uint8), "replaced_by": np.full(P, -1, np.int32), "found": np.zeros(P, np.int32), "visible": np.zeros(P, np.int32)}

"""The windowed ORB matching restated in numpy / plain Python from the rules M1-M9 of include/iba_mi355x.h and the two query builders, with float32
scalars throughout (every operation rounded, left to right). The device results are compared with this byte for byte. A frame is a dict
(xy [n, 2] f32, octave [n] i32, angle [n] f32, desc [n, 32] u8, bounds = (min_x, max_x, min_y, max_y)); a job is a dict (query_frame, train_frame,
rule, centre_xy, radius, level_range, query_index, valid or None)."""
import numpy as np

F = np.float32
COLS, ROWS, CELLS, HISTO = 64, 48, 3072, 30
INIT, CLAIM = 0, 1
INT_MAX = 2 ** 31 - 1
POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def make_frame(xy, octave, angle, desc, bounds):
    return {"xy": np.ascontiguousarray(xy, F).reshape(-1, 2), "octave": np.ascontiguousarray(octave, np.int32).reshape(-1),
            "angle": np.ascontiguousarray(angle, F).reshape(-1), "desc": np.ascontiguousarray(desc, np.uint8).reshape(-1, 32),
            "bounds": tuple(F(v) for v in bounds)}


def roundf(p):
    """C's roundf: half away from zero (p - trunc(p) is exact)"""
    p = F(p)
    t = np.trunc(p)
    if abs(p - t) >= F(0.5):
        t = t + (F(1) if p > 0 else F(-1))
    return F(t)


def inv_wh(frame):
    min_x, max_x, min_y, max_y = frame["bounds"]
    return F(64.0) / F(max_x - min_x), F(48.0) / F(max_y - min_y)


def cell_of(x, lo, inv, n):
    """M2 along one axis: the cell or -1"""
    p = roundf(F(F(x) - lo) * inv)
    return int(p) if (p >= 0 and p < n) else -1


def pos_in_grid(frame, x, y):
    """M2: (px, py), either -1 where the keypoint is in no cell"""
    iw, ih = inv_wh(frame)
    return cell_of(x, frame["bounds"][0], iw, COLS), cell_of(y, frame["bounds"][2], ih, ROWS)


def grid(frame):
    """M2 for a frame -> (cell_off [3073] with cell = px * 48 + py, list): a cell's keypoints in ascending index"""
    cells = [[] for _ in range(CELLS)]
    for i, (x, y) in enumerate(frame["xy"]):
        px, py = pos_in_grid(frame, x, y)
        if px >= 0 and py >= 0:
            cells[px * ROWS + py].append(i)
    off = np.zeros(CELLS + 1, np.int32)
    off[1:] = np.cumsum([len(c) for c in cells])
    lst = np.array([i for c in cells for i in c], np.int32)
    return off, lst


def window(u, lo, r, inv, n):
    """M3 along one axis -> (first, last) or None where the list is empty"""
    with np.errstate(all="ignore"):
        a = np.floor(F(F(F(u) - lo) - F(r)) * inv)
        b = np.ceil(F(F(F(u) - lo) + F(r)) * inv)
    first = (0 if a < 0 else int(a)) if a < n else n
    if first >= n:
        return None
    last = (n - 1 if b > n - 1 else int(b)) if b >= 0 else -1
    if last < 0:
        return None
    return first, last


def area(frame, g, u, v, r, min_level, max_level):
    """M3: the indices in the list's order"""
    u, v, r = F(u), F(v), F(r)
    iw, ih = inv_wh(frame)
    wx, wy = window(u, frame["bounds"][0], r, iw, COLS), window(v, frame["bounds"][2], r, ih, ROWS)
    if wx is None or wy is None:
        return np.zeros(0, np.int32)
    off, lst = g
    check = min_level > 0 or max_level >= 0
    out = []
    for ix in range(wx[0], wx[1] + 1):         # (with cell = px * 48 + py the cells iy = first .. last of a column are one run of the list)
        idx = lst[off[ix * ROWS + wy[0]]:off[ix * ROWS + wy[1] + 1]]
        keep = np.ones(len(idx), bool)
        if check:
            keep &= ~(frame["octave"][idx] < min_level)
            if max_level >= 0:
                keep &= ~(frame["octave"][idx] > max_level)
        keep &= (np.abs(frame["xy"][idx, 0] - u) < r) & (np.abs(frame["xy"][idx, 1] - v) < r)
        out.append(idx[keep])
    return np.concatenate(out).astype(np.int32)


def hamming(d, D):
    """M4: one descriptor against rows of descriptors"""
    return POP[np.bitwise_xor(np.asarray(D, np.uint8).reshape(-1, 32), np.asarray(d, np.uint8).reshape(1, 32))].sum(1).astype(np.int32)


def rot_bin(angle_q, angle_c):
    """M8's bin"""
    rot = F(F(angle_q) - F(angle_c))
    if rot < F(0.0):
        rot = F(rot + F(360.0))
    b = int(roundf(F(rot * F(F(1.0) / F(HISTO)))))
    return 0 if b == HISTO else b


def three_maxima(hist):
    """ComputeThreeMaxima -> [ind1, ind2, ind3]"""
    max1 = max2 = max3 = 0
    i1 = i2 = i3 = -1
    for i, s in enumerate(int(v) for v in hist):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            i3, i2, i1 = i2, i1, i
        elif s > max2:
            max3, max2 = max2, s
            i3, i2 = i2, i
        elif s > max3:
            max3, i3 = s, i
    if F(max2) < F(F(0.1) * F(max1)):
        i2 = i3 = -1
    elif F(max3) < F(F(0.1) * F(max1)):
        i3 = -1
    return [i1, i2, i3]


def run_job(frames, job, grids=None, th_low=50, th_high=100, nn_ratio=0.9, check_orientation=1):
    """M5-M9 for one job -> dict with the M9 outputs, the lists (off, index, cdist) and, for the tests' conditions on a scene, n_ratio_rejected and
    max_segment"""
    qf, tf = frames[job["query_frame"]], frames[job["train_frame"]]
    g = grids[job["train_frame"]] if grids is not None else grid(tf)
    nq, nt = len(job["radius"]), len(tf["octave"])
    rule, nn_ratio = job["rule"], F(nn_ratio)
    match, dist = np.full(nq, -1, np.int32), np.full(nq, -1, np.int32)
    held, holder = np.full(nt, INT_MAX, np.int64), np.full(nt, -1, np.int64)    # CLAIM: held 0 = claimed
    hist, entry_bin = np.zeros(HISTO, np.int32), np.full(nq, -1, np.int32)
    off, index, cdist = np.zeros(nq + 1, np.int32), [], []
    n_matches = n_displaced = n_ratio_rejected = 0
    for q in range(nq):
        off[q + 1] = off[q]
        if job.get("valid") is not None and not job["valid"][q]:
            continue
        k = int(job["query_index"][q])
        cand = area(tf, g, job["centre_xy"][q][0], job["centre_xy"][q][1], job["radius"][q], int(job["level_range"][q][0]), int(job["level_range"][q][1]))
        d = hamming(qf["desc"][k], tf["desc"][cand]) if len(cand) else np.zeros(0, np.int32)
        off[q + 1] += len(cand)
        index.extend(int(c) for c in cand)
        cdist.extend(int(v) for v in d)
        best, best2, best_c = (INT_MAX if rule == INIT else 256), INT_MAX, -1
        for c, dc in zip(cand, d):
            if rule == INIT and held[c] <= dc:
                continue
            if rule == CLAIM and held[c] == 0:
                continue
            if dc < best:
                best2, best, best_c = best, int(dc), int(c)
            elif rule == INIT and dc < best2:
                best2 = int(dc)
        if best_c < 0:
            continue
        if rule == INIT:
            if not best <= th_low:
                continue
            if not F(best) < F(F(best2) * nn_ratio):
                n_ratio_rejected += 1
                continue
            if holder[best_c] >= 0:
                match[holder[best_c]] = dist[holder[best_c]] = -1
                n_matches -= 1
                n_displaced += 1
            holder[best_c], held[best_c] = q, best
        else:
            if not best <= th_high:
                continue
            held[best_c] = 0
        match[q], dist[q] = best_c, best
        n_matches += 1
        if check_orientation:
            entry_bin[q] = rot_bin(qf["angle"][k], tf["angle"][best_c])
            hist[entry_bin[q]] += 1
    ind, n_rot_removed = [-1, -1, -1], 0
    if check_orientation:
        ind = three_maxima(hist)
        for q in range(nq):
            if entry_bin[q] >= 0 and entry_bin[q] not in ind and match[q] >= 0:
                match[q] = dist[q] = -1
                n_matches -= 1
                n_rot_removed += 1
    seg = np.diff(off)
    return {"match": match, "dist": dist, "n_queries": nq, "n_matches": n_matches, "n_candidates": int(off[nq]), "n_displaced": n_displaced, "n_rot_removed": n_rot_removed,
            "hist": hist, "ind": np.array(ind, np.int32), "off": off, "index": np.array(index, np.int32), "cdist": np.array(cdist, np.uint16),
            "n_ratio_rejected": n_ratio_rejected, "max_segment": int(seg.max()) if nq else 0}


def run(frames, jobs, **opts):
    """a call: every frame's grid once, then every job -> (grids, results)"""
    grids = [grid(f) for f in frames]
    return grids, [run_job(frames, j, grids, **opts) for j in jobs]


def init_queries(frame, prev_matched_xy, window_size):
    n = len(frame["octave"])
    return {"centre_xy": np.ascontiguousarray(prev_matched_xy, F).reshape(n, 2).copy(), "radius": np.full(n, F(window_size), F), "level_range": np.zeros((n, 2), np.int32),
            "query_index": np.arange(n, dtype=np.int32), "valid": (frame["octave"] == 0).astype(np.uint8)}


def motion_queries(frame, has_point, outlier, world_xyz, Tcw, fx, fy, cx, cy, bounds, scale_factors, th):
    n = len(frame["octave"])
    T = np.asarray(Tcw, F).reshape(-1)[:12]
    fx, fy, cx, cy, th = F(fx), F(fy), F(cx), F(cy), F(th)
    min_x, max_x, min_y, max_y = (F(v) for v in bounds)
    out = {"centre_xy": np.zeros((n, 2), F), "radius": np.zeros(n, F), "level_range": np.zeros((n, 2), np.int32), "query_index": np.arange(n, dtype=np.int32),
           "valid": np.zeros(n, np.uint8)}
    for i in range(n):
        if not has_point[i] or outlier[i]:
            continue
        X, Y, Z = (F(v) for v in np.asarray(world_xyz, F).reshape(n, 3)[i])
        with np.errstate(all="ignore"):
            xc = F(F(F(T[0] * X) + F(T[1] * Y)) + F(T[2] * Z)) + T[3]
            yc = F(F(F(T[4] * X) + F(T[5] * Y)) + F(T[6] * Z)) + T[7]
            zc = F(F(F(T[8] * X) + F(T[9] * Y)) + F(T[10] * Z)) + T[11]
            invzc = F(np.float64(1.0) / np.float64(zc))
            if invzc < 0:
                continue
            u = F(F(F(fx * xc) * invzc) + cx)
            v = F(F(F(fy * yc) * invzc) + cy)
        if not (np.isfinite(u) and np.isfinite(v)):
            continue
        if u < min_x or u > max_x or v < min_y or v > max_y:
            continue
        o = int(frame["octave"][i])
        out["centre_xy"][i] = (u, v)
        out["radius"][i] = F(th * F(scale_factors[o]))
        out["level_range"][i] = (o - 1, o + 1)
        out["valid"][i] = 1
    return out

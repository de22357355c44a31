"""numpy restatement of the Scan Context rules of include/iba_mi355x.h (iba_sc_describe / iba_sc_distance / iba_sc_detect / iba_sc_replay_plan):
descriptor, ring and sector keys, the shift-aligned column-cosine distance, the brute-force ring-key search and the replay of the reference's
stateful detection. Every sum is taken in the header's fixed order with separately rounded f64 operations (numpy has no fma), so the device
result is compared with this file byte for byte. Nothing here is tuned to a device result."""
import math

import numpy as np

DEFAULTS = dict(num_ring=20, num_sector=60, max_radius=80.0, lidar_height=0.0, num_exclude_recent=30, num_candidates=3, search_ratio=0.1,
                tree_period=30, dist_thres=0.2)
NO_WINNER = 10000000.0       # the reference's initial minimum: what comes back when no shift / no candidate wins a '<'
RAD2DEG = 180.0 / math.pi


def options(**kw):
    o = dict(DEFAULTS)
    for k in kw:
        if k not in o:
            raise KeyError(k)
    o.update(kw)
    return o


# ---- rule 1 / 2: the point, its ring and sector ----
def bin_arguments(scan, opt):
    """-> dict over the FINITE points of a float32 scan: z32 (float32 z), zz (z + lidar_height), rng, ring_arg, sector_arg (the arguments of the two
    ceils), exact_angle (the angle is 0 by the rules alone: y == 0 with x > 0, or the origin column); n_skipped = points with a non-finite coordinate"""
    p = np.asarray(scan, np.float32).reshape(-1, 3)
    fin = np.isfinite(p).all(axis=1)
    q = p[fin].astype(np.float64)
    x, y = q[:, 0], q[:, 1]
    zz = q[:, 2] + float(opt["lidar_height"])
    rng = np.sqrt((x * x + y * y) + zz * zz)
    ang = np.arctan2(y, x) * RAD2DEG
    ang = np.where(ang < 0.0, ang + 360.0, ang)
    origin = (x == 0.0) & (y == 0.0)
    ang = np.where(origin, 0.0, ang)
    return dict(z32=p[fin, 2].copy(), zz=zz, rng=rng, ring_arg=rng / float(opt["max_radius"]) * int(opt["num_ring"]), sector_arg=ang / 360.0 * int(opt["num_sector"]),
                exact_angle=origin | ((y == 0.0) & (x > 0.0)), n_skipped=int((~fin).sum()))


def bins(scan, opt):
    """-> (ring index 0-based, sector index 0-based, enters, args): enters = inside max_radius by the 3-D norm and z + lidar_height above the -1000 sentinel"""
    a = bin_arguments(scan, opt)
    R, S = int(opt["num_ring"]), int(opt["num_sector"])
    ring = np.maximum(np.minimum(R, np.ceil(a["ring_arg"]).astype(np.int64)), 1) - 1
    sec = np.maximum(np.minimum(S, np.ceil(a["sector_arg"]).astype(np.int64)), 1) - 1
    enters = ~(a["rng"] > float(opt["max_radius"])) & (a["zz"] > -1000.0)
    return ring, sec, enters, a


def non_decisive(scan, opt, eps=1e-9):
    """mask over the finite points: a ceil argument or the range (in ring units) closer than eps to its boundary"""
    a = bin_arguments(scan, opt)
    near = lambda v: np.abs(v - np.round(v)) <= eps
    return near(a["ring_arg"]) | near(a["sector_arg"]) | (np.abs(a["ring_arg"] - int(opt["num_ring"])) <= eps)


def z_key(z32):
    """the order-preserving 32-bit key of a float32 (what the device's integer atomic max orders by); 0 is below every finite value"""
    b = np.asarray(z32, np.float32).view(np.uint32)
    return np.where(b >> 31, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def z_unkey(k):
    k = np.asarray(k, np.uint32)
    return np.where(k >> 31, k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(np.float32)


# ---- rule 3 / 4: descriptor and keys ----
def descriptor(scan, opt):
    """-> (desc [R, S] f64, n_skipped): the bin keeps the largest float32 z (by key), widened, + lidar_height; an empty bin is 0"""
    R, S = int(opt["num_ring"]), int(opt["num_sector"])
    ring, sec, enters, a = bins(scan, opt)
    key = np.zeros(R * S, np.uint32)
    np.maximum.at(key, (ring * S + sec)[enters], z_key(a["z32"][enters]))
    val = z_unkey(key).astype(np.float64) + float(opt["lidar_height"])
    return np.where(key == 0, 0.0, val).reshape(R, S), a["n_skipped"]


def seq_sum(m, axis):
    """the sum along an axis taken sequentially from index 0, every add rounded on its own"""
    m = np.moveaxis(np.asarray(m, np.float64), axis, 0)
    acc = np.zeros(m.shape[1:], np.float64)
    for k in range(m.shape[0]):
        acc = acc + m[k]
    return acc


def ring_key(desc):
    return seq_sum(desc, -1) / float(desc.shape[-1])         # row means, columns ascending


def sector_key(desc):
    return seq_sum(desc, -2) / float(desc.shape[-2])         # column means, rows ascending


def column_norms(desc):
    return np.sqrt(seq_sum(desc * desc, -2))


def describe(scans, opt):
    """-> dict(desc [n, R, S], ring [n, R], ring_f [n, R] float32, sector [n, S], skipped [n] int64)"""
    ds, sk = zip(*(descriptor(s, opt) for s in scans))
    d = np.stack(ds)
    rk = ring_key(d)
    return dict(desc=d, ring=rk, ring_f=rk.astype(np.float32), sector=sector_key(d), skipped=np.asarray(sk, np.int64))


# ---- distance ----
def search_radius(opt):
    return int(math.floor(0.5 * float(opt["search_ratio"]) * int(opt["num_sector"]) + 0.5))     # C round() of a non-negative value


def window(argmin, opt):
    """the shifts tried around the sector-key argmin, ascending (duplicates of a window wider than the circle removed: they cannot win a '<')"""
    S, rad = int(opt["num_sector"]), search_radius(opt)
    return sorted(set((argmin + d) % S for d in range(-rad, rad + 1)))


def align(vk1, vk2):
    """fastAlignUsingVkey: the first shift that minimises |vk1 - circshift(vk2, shift)|, the squares added columns ascending"""
    S = len(vk1)
    best, arg = NO_WINNER, 0
    for sh in range(S):
        d = vk1 - np.roll(vk2, sh)
        n = float(np.sqrt(seq_sum(d * d, 0)))
        if n < best:
            best, arg = n, sh
    return arg


def dist_direct(sc1, sc2, n1=None, n2=None):
    """distDirectSC: 1 - mean over the columns where both norms are non-zero of the column cosine; NaN without such a column"""
    n1 = column_norms(sc1) if n1 is None else n1
    n2 = column_norms(sc2) if n2 is None else n2
    dots = seq_sum(sc1 * sc2, 0)
    s, cnt = 0.0, 0
    for c in range(sc1.shape[1]):
        if n1[c] == 0.0 or n2[c] == 0.0:
            continue
        s = s + float(dots[c]) / (float(n1[c]) * float(n2[c]))
        cnt += 1
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(1.0 - np.float64(s) / np.float64(cnt))


def distance(sc1, sc2, opt):
    """distanceBtnScanContext -> (distance, shift); (NO_WINNER, 0) when every tried shift gives NaN"""
    a = align(sector_key(sc1), sector_key(sc2))
    n1, n2 = column_norms(sc1), column_norms(sc2)
    best, arg = NO_WINNER, 0
    for sh in window(a, opt):
        d = dist_direct(sc1, np.roll(sc2, sh, axis=1), n1, np.roll(n2, sh))
        if d < best:
            best, arg = d, sh
    return best, arg


def distances(desc, pairs, opt):
    out = [distance(desc[a], desc[b], opt) for a, b in pairs]
    return np.array([d for d, _ in out], np.float64), np.array([s for _, s in out], np.int32)


# ---- search and detection ----
def knn(ring_f, node, db_end, k):
    """exact brute force over [0, db_end) on the float keys: f64 distances, rows ascending; equal distances to the lower node; -1 fills"""
    out = np.full(k, -1, np.int32)
    if db_end > 0:
        q = ring_f[node].astype(np.float64)
        d = ring_f[:db_end].astype(np.float64) - q[None, :]
        d2 = seq_sum(d * d, 1)
        order = np.lexsort((np.arange(db_end), d2))[:k]
        out[:len(order)] = order
    return out


def yaw(shift, opt):
    return np.float32(shift * (360.0 / int(opt["num_sector"])) * math.pi / 180.0)


def detect(db, queries, opt):
    """db = describe(...); queries = [(node, db_end)] -> list of dict(loop_node, min_dist, shift, yaw_rad, cand_node [k], cand_dist [k], cand_shift [k])"""
    k = int(opt["num_candidates"])
    res = []
    for node, db_end in queries:
        cand = knn(db["ring_f"], node, db_end, k)
        cd, cs = np.full(k, np.nan), np.full(k, -1, np.int32)
        best, arg, nn = NO_WINNER, 0, -1
        for i, c in enumerate(cand):
            if c < 0:
                continue
            cd[i], cs[i] = distance(db["desc"][node], db["desc"][c], opt)
            if cd[i] < best:
                best, arg, nn = cd[i], int(cs[i]), int(c)
        res.append(dict(loop_node=nn if best < float(opt["dist_thres"]) else -1, min_dist=float(best), shift=arg, yaw_rad=yaw(arg, opt), cand_node=cand, cand_dist=cd, cand_shift=cs))
    return res


def replay_plan(sizes_at_call, opt):
    """detectLoopClosureID's statefulness as a pure function: db_end per call (0: the early return, which does not advance the counter)"""
    excl, period = int(opt["num_exclude_recent"]), int(opt["tree_period"])
    out, counter, cur = [], 0, 0
    for size in sizes_at_call:
        if size < excl + 1:
            out.append(0)
            continue
        if counter % period == 0:
            cur = size - excl
        counter += 1
        out.append(cur)
    return np.asarray(out, np.int32)

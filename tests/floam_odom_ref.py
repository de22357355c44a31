"""TEST INFRASTRUCTURE: the lattice voxel filter with a crop box (iba_lattice_build, include/iba_mi355x.h) and the host-side rules of F-LOAM's
local map around it, restated in numpy. Imports nothing from the product; the shared expressions (the point transform, the sequential sums) are
those of tests/submap_ref.py. The rules:
  L1  rule 1 of submap_ref: float32 widened to f64, q_r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], members in list order, a member's points in
      scan order; a non-finite point is dropped and counted
  L2  with a crop box, a point is kept iff lo[a] <= q[a] <= hi[a] on all three axes (both ends inclusive); the others are counted in n_cropped
  L3  cell i[a] = floor(q[a] / leaf): IEEE f64 division, then floor; the origin is the anchor
  L4  a cell's point = (sum of its q, SEQUENTIALLY in concatenation order) / float(count), out applied after, cells ascending (ix, iy, iz)
and of the map (the reference's odomEstimationClass / System::Track):
  O2  downSamplingToMap: the filter without crop in the scan's own frame, leaf = map_resolution (edge) / 2 map_resolution (surf), narrowed to float32
  O3  initMapWithPoints: the raw features moved by T0 with L1's expression, narrowed to float32
  O4  T_pred = T[k-1] (inv(T[k-2]) T[k-1]), inv = [R^T, -R^T t]
  O5  max(outer_passes, init_passes - k) passes at step k
  O6  addPointsToMap: members [old map, identity; down-sampled cloud, T], crop t +- crop_half, the filter, narrowed to float32"""
import numpy as np

import submap_ref as V

MAX_AXIS_CELLS = 1 << 17


def cells(q, leaf):
    """rule L3 on q [k, 3] f64 -> int64 [k, 3]"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    return np.floor(q / np.float64(leaf)).astype(np.int64)


def inside(q, lo, hi):
    """rule L2 on q [k, 3] -> bool [k]"""
    q = np.asarray(q, np.float64).reshape(-1, 3)
    lo = np.asarray(lo, np.float64); hi = np.asarray(hi, np.float64)
    return ((lo <= q) & (q <= hi)).all(1)


def lattice(members, leaf, out=None, crop=None):
    """members: [(points [n, 3] float32, pose)], crop: None or (lo [3], hi [3])
    -> dict(xyz [V, 3] f64, count [V] int32, n_dropped, n_cropped, idx [V, 3] int64)"""
    q, dropped = V.concatenate(members)
    cropped = 0
    if crop is not None and len(q):
        keep = inside(q, crop[0], crop[1])
        cropped = int((~keep).sum())
        q = q[keep]
    if len(q) == 0:
        return dict(xyz=np.zeros((0, 3)), count=np.zeros(0, np.int32), n_dropped=dropped, n_cropped=cropped, idx=np.zeros((0, 3), np.int64))
    idx = cells(q, leaf)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))          # stable: equal cells keep their concatenation order
    si, sq = idx[order], q[order]
    head = np.r_[True, np.any(si[1:] != si[:-1], axis=1)]
    start = np.flatnonzero(head)
    count = np.diff(np.r_[start, len(sq)])
    acc = np.zeros((len(start), 3))
    live = np.arange(len(start))
    r = 0
    while len(live):                                                # rank r of every cell that has one: acc = (..((0 + q_0) + q_1) + ..)
        acc[live] = acc[live] + sq[start[live] + r]
        r += 1
        live = live[count[live] > r]
    xyz = acc / count.astype(np.float64)[:, None]
    if out is not None:
        xyz = V.apply(out, xyz)
    return dict(xyz=xyz, count=count.astype(np.int32), n_dropped=dropped, n_cropped=cropped, idx=si[start])


def span(idx):
    """cells along each axis that a result spans (max - min + 1); the device refuses more than MAX_AXIS_CELLS"""
    return (idx.max(0) - idx.min(0) + 1) if len(idx) else np.zeros(3, np.int64)


def narrow(xyz):
    """f64 -> float32, round to nearest even (what a cloud becomes when it is made a frame)"""
    return np.ascontiguousarray(np.asarray(xyz, np.float64).reshape(-1, 3).astype(np.float32))


def downsample(edge, surf, map_resolution):
    """rule O2 -> (edge cloud, surf cloud) float32"""
    I = np.eye(4)
    return (narrow(lattice([(edge, I)], map_resolution)["xyz"]), narrow(lattice([(surf, I)], 2.0 * map_resolution)["xyz"]))


def init_map(edge, surf, T0):
    """rule O3 -> (map edge, map surf) float32: the raw features moved by T0 (non-finite points dropped)"""
    return narrow(V.concatenate([(edge, T0)])[0]), narrow(V.concatenate([(surf, T0)])[0])


def rigid_inverse(T):
    """[R^T, -R^T t] of a 4x4"""
    T = np.asarray(T, np.float64).reshape(4, 4)
    M = np.eye(4)
    M[:3, :3] = T[:3, :3].T
    M[:3, 3] = -(T[:3, :3].T @ T[:3, 3])
    return M


def predict(T_prev2, T_prev):
    """rule O4: the constant-velocity prediction from the poses of steps k - 2 and k - 1"""
    T_prev = np.asarray(T_prev, np.float64).reshape(4, 4)
    return T_prev @ (rigid_inverse(T_prev2) @ T_prev)


def pass_schedule(n_scans, init_passes=12, outer_passes=2):
    """rule O5: passes per step; step 0 (the map's initialisation) solves nothing"""
    return [0] + [max(outer_passes, init_passes - k) for k in range(1, n_scans)]


def crop_box(T, crop_half):
    """rule O6's box: t +- crop_half per axis, in f64"""
    t = np.asarray(T, np.float64).reshape(4, 4)[:3, 3]
    return t - np.float64(crop_half), t + np.float64(crop_half)


def update_map(map_edge, map_surf, src_edge, src_surf, T, map_resolution, crop_half):
    """rule O6 -> (map edge, map surf) float32 and the two filter results"""
    I = np.eye(4)
    box = crop_box(T, crop_half)
    e = lattice([(map_edge, I), (src_edge, T)], map_resolution, crop=box)
    s = lattice([(map_surf, I), (src_surf, T)], 2.0 * map_resolution, crop=box)
    return narrow(e["xyz"]), narrow(s["xyz"]), e, s


def track(scans, T0, extract_opt, map_opt=None, map_resolution=0.4, crop_half=100.0, init_passes=12):
    """rules O1-O6 on one track, free running: scans = [points [P, 3] float32] in time order -> list of dict(T_pred, T, passes, status, solve (the
    registration's result, None at step 0), src_edge, src_surf, map_edge, map_surf (the map AFTER the step)). Uses the restatements of the two
    stages it joins (tests/floam_ref.py, tests/floam_map_ref.py)."""
    import floam_map_ref as M
    import floam_ref as F
    o = dict(map_opt or {})
    floor = M.options(**o)["outer_passes"]
    T0 = np.asarray(T0, np.float64).reshape(4, 4)
    steps = []
    for k, scan in enumerate(scans):
        f = F.extract(scan, extract_opt)
        se, ss = downsample(f["edge_xyz"], f["surf_xyz"], map_resolution)
        if k == 0:
            me, ms = init_map(f["edge_xyz"], f["surf_xyz"], T0)
            steps.append(dict(T_pred=T0.copy(), T=T0.copy(), passes=0, status=0, solve=None, src_edge=se, src_surf=ss, map_edge=me, map_surf=ms))
            continue
        T_pred = predict(steps[k - 2]["T"] if k >= 2 else T0, steps[k - 1]["T"])
        passes = max(floor, init_passes - k)
        r = M.register(T_pred, se, ss, steps[k - 1]["map_edge"], steps[k - 1]["map_surf"], dict(o, outer_passes=passes))
        me, ms, _, _ = update_map(steps[k - 1]["map_edge"], steps[k - 1]["map_surf"], se, ss, r["T"], map_resolution, crop_half)
        steps.append(dict(T_pred=T_pred, T=r["T"], passes=r["passes"], status=r["status"], solve=r, src_edge=se, src_surf=ss, map_edge=me, map_surf=ms))
    return steps


# ---- the track the tests share: the room of floam_ref.room_scan seen from origins 0.2 m apart; the ground truth is the origin ----
TRACK = dict(lines=16, per_ring=300, seed=40, n_scans=8, step=0.2, map_resolution=0.4, crop_half=100.0, init_passes=12)


def track_scans(n_scans=None, cfg=TRACK):
    import floam_ref as F
    n = cfg["n_scans"] if n_scans is None else n_scans
    return [F.room_scan(cfg["lines"], per_ring=cfg["per_ring"], seed=cfg["seed"] + k, origin=(cfg["step"] * k, 0.0)) for k in range(n)]


def track_truth(k, cfg=TRACK):
    T = np.eye(4)
    T[0, 3] = cfg["step"] * k
    return T


def track_extract_options(cfg=TRACK):
    import floam_ref as F
    return F.options(num_lines=cfg["lines"])


def track_error(T, k, cfg=TRACK):
    """position error of a pose of scan k against the ground truth (metres)"""
    return float(np.linalg.norm(np.asarray(T, np.float64).reshape(4, 4)[:3, 3] - track_truth(k, cfg)[:3, 3]))


# The reference chain's own final position error on TRACK, measured by tests/test_floam_odom_cpu.py (which asserts that a run reproduces it) and
# quoted in profiles/floam_odom_parity.md. The GPU tier's whole-track gate reads it from here: it is the restatement's figure, never the device's.
E_REF = 0.1241950267624765

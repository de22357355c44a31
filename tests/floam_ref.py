"""numpy restatement of iba_floam_extract's rules (include/iba_mi355x.h, "F-LOAM feature extraction"): the reference's
LaserProcessingClass::featureExtraction with the order of every floating-point operation fixed. The device result is compared with this byte for
byte. Float32 work stays in np.float32 arrays (numpy rounds every operation on its own and has no fused multiply-add), f64 work in np.float64."""
import math

import numpy as np

MAX_RING_POINTS = 8192
DEFAULTS = dict(num_lines=64, min_distance=3.0, max_distance=90.0, min_ring_points=131, num_sectors=6, max_edges_per_sector=20, neighbour_span=5,
                edge_curvature=0.1, neighbour_gap2=0.05)


class Unsupported(Exception):
    """rule 3: a ring with more than MAX_RING_POINTS points (args: scan-local ring, its size)"""


def options(**kw):
    o = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in o:
            raise KeyError(k)
        o[k] = v
    return o


# ---- rules 1 and 2 ----
def angles(scan, opt):
    """-> (finite [P] bool, d [P] f64, angle [P] f64 in degrees); d and angle are meaningless where finite is False"""
    p = np.asarray(scan, np.float32).reshape(-1, 3)
    finite = np.isfinite(p).all(axis=1)
    q = np.where(finite[:, None], p, np.float32(1.0)).astype(np.float64)
    with np.errstate(all="ignore"):
        d = np.sqrt(q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1])
        ang = np.arctan(q[:, 2] / d) * 180 / math.pi
    return finite, d, ang


def ring_expr(ang, lines):
    """the reference's expression BEFORE the truncation, and the mask of the angles its extra 64-line test keeps"""
    with np.errstate(all="ignore"):
        if lines == 16:
            return (ang + 15) / 2 + 0.5, np.ones(ang.shape, bool), np.zeros(ang.shape, np.int64)
        if lines == 32:
            return (ang + 92.0 / 3.0) * 3.0 / 4.0, np.ones(ang.shape, bool), np.zeros(ang.shape, np.int64)
        if lines == 64:
            hi = ang >= -8.83
            e = np.where(hi, (2 - ang) * 3.0 + 0.5, (-8.83 - ang) * 2.0 + 0.5)
            return e, ~((ang > 2) | (ang < -24.33)), np.where(hi, 0, 32)
    raise ValueError("num_lines must be 16, 32 or 64")


def classify(scan, opt):
    """-> (ring [P] int64, -1 where the point is skipped; dict of the three counters)"""
    finite, d, ang = angles(scan, opt)
    inside = finite & ~((d < opt["min_distance"]) | (d > opt["max_distance"]))
    e, keep, add = ring_expr(ang, opt["num_lines"])
    ok = inside & keep & ~np.isnan(ang)
    ring = np.full(len(d), -1, np.int64)
    ring[ok] = add[ok] + np.trunc(e[ok]).astype(np.int64)          # C truncation towards zero
    ok &= (ring >= 0) & (ring < opt["num_lines"])
    ring[~ok] = -1
    return ring, dict(n_nonfinite=int((~finite).sum()), n_out_of_range=int((finite & ~inside).sum()), n_no_ring=int((inside & ~ok).sum()))


def ring_centre(lines, r):
    """the elevation (degrees) in the middle of the angles that rule 2 sends to ring r"""
    if lines == 16:
        return 2.0 * r - 15.0
    if lines == 32:
        return (r + 0.5) * 4.0 / 3.0 - 92.0 / 3.0
    if r == 0:
        return 2.0 - 1.0 / 12.0                      # (2 - 1/6, 2]: the upper half is cut by angle > 2
    if r < 32:
        return 2.0 - r / 3.0
    if r == 32:
        return 0.5 * (-9.08 + -8.5)                  # 32 from the first expression above -8.83, 32 + 0 from the second below it
    if r == 63:
        return 0.5 * (-24.33 + -24.08)
    return -8.83 - (r - 32) / 2.0


def ring_margin(scan, opt):
    """-> (angle margin in degrees, distance margin in metres): the smallest distance of a kept point's angle from a boundary of rule 2 and of a finite
    point's d from min_distance / max_distance. inf when there is no such point."""
    finite, d, ang = angles(scan, opt)
    dm = np.inf
    if finite.any():
        dm = float(min(np.abs(d[finite] - opt["min_distance"]).min(), np.abs(d[finite] - opt["max_distance"]).min()))
    inside = finite & ~((d < opt["min_distance"]) | (d > opt["max_distance"]))
    a = ang[inside]
    if not len(a):
        return np.inf, dm
    lines = opt["num_lines"]
    e, _, _ = ring_expr(a, lines)
    slope = {16: 0.5, 32: 0.75}.get(lines)
    if slope is None:
        slope = np.where(a >= -8.83, 3.0, 2.0)
    lo, hi = np.floor(e), np.floor(e) + 1                         # the integers around e; 0 is no boundary (truncation sends (-1, 1) to 0)
    lo = np.where(lo == 0, -1.0, lo)
    hi = np.where(hi == 0, 1.0, hi)
    m = np.minimum(e - lo, hi - e) / slope
    if lines == 64:
        for b in (2.0, -8.83, -24.33):
            m = np.minimum(m, np.abs(a - b))
    return float(m.min()), dm


# ---- rules 4 to 8, one ring ----
def curvature(p):
    """p [n, 3] float32, n >= 11 -> value [n - 10] f64 of the positions 5 .. n - 6 (rule 4)"""
    p = np.asarray(p, np.float32)
    n = len(p)
    w = lambda k: p[5 + k:n - 5 + k]
    with np.errstate(all="ignore"):
        s = (((w(-5) + w(-4)) + w(-3)) + w(-2)) + w(-1)
        s = s - np.float32(10) * w(0)
        for k in range(1, 6):
            s = s + w(k)
        assert s.dtype == np.float32
        dd = s.astype(np.float64)
        v = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    return np.where(np.isnan(v), np.inf, v)


def gap2(p, a, b):
    with np.errstate(all="ignore"):
        df = (p[a] - p[b]).astype(np.float64)
        return (df[0] * df[0] + df[1] * df[1]) + df[2] * df[2]


def sector_bounds(n, num_sectors):
    """rule 5: [(first entry, end)] of the curvature entries [0, n - 10)"""
    total = n - 10
    ln = total // num_sectors
    return [(ln * s, (ln * (s + 1) - 1) if s < num_sectors - 1 else total - 1) for s in range(num_sectors)]


def sector_features(p, val, lo, hi, opt):
    """entries [lo, hi) of one ring -> (edge positions in pick order, surf positions in ascending (value, position) order); positions index p"""
    if hi <= lo:
        return [], []
    pos = np.arange(lo, hi) + 5
    order = np.lexsort((pos, val[lo:hi]))
    pos, v = pos[order], val[lo:hi][order]
    marked = np.zeros(len(p), bool)
    edges, count = [], 0
    for i in range(len(pos) - 1, -1, -1):
        ind = int(pos[i])
        if marked[ind]:
            continue
        if v[i] <= opt["edge_curvature"]:
            break
        count += 1
        marked[ind] = True
        if count > opt["max_edges_per_sector"]:
            break
        edges.append(ind)
        for k in range(1, 6):
            if gap2(p, ind + k, ind + k - 1) > opt["neighbour_gap2"]:
                break
            marked[ind + k] = True
        for k in range(-1, -6, -1):
            if gap2(p, ind + k, ind + k + 1) > opt["neighbour_gap2"]:
                break
            marked[ind + k] = True
    return edges, [int(q) for q in pos if not marked[q]]


def ring_features(p, opt):
    """one ring list p [n, 3] float32 -> (edge positions, surf positions) in rule-9 order"""
    p = np.asarray(p, np.float32)
    if len(p) < opt["min_ring_points"]:
        return [], []
    val = curvature(p)
    E, S = [], []
    for lo, hi in sector_bounds(len(p), opt["num_sectors"]):
        e, s = sector_features(p, val, lo, hi, opt)
        E += e
        S += s
    return E, S


def extract(scan, opt):
    """one scan [P, 3] float32 -> dict(edge_index, edge_xyz, surf_index, surf_xyz, n_nonfinite, n_out_of_range, n_no_ring, ring_points [num_lines] int32)"""
    scan = np.ascontiguousarray(scan, np.float32).reshape(-1, 3)
    ring, out = classify(scan, opt)
    E, S = [], []
    sizes = np.zeros(opt["num_lines"], np.int32)
    for r in range(opt["num_lines"]):
        idx = np.flatnonzero(ring == r)                            # original order: a stable partition
        sizes[r] = len(idx)
        if len(idx) > MAX_RING_POINTS:
            raise Unsupported(r, len(idx))
        e, s = ring_features(scan[idx], opt)
        E += [int(idx[q]) for q in e]
        S += [int(idx[q]) for q in s]
    E, S = np.asarray(E, np.int32), np.asarray(S, np.int32)
    out.update(edge_index=E, edge_xyz=scan[E].reshape(-1, 3), surf_index=S, surf_xyz=scan[S].reshape(-1, 3), ring_points=sizes)
    return out


# ---- fixtures shared by the CPU and the GPU tier (the CPU tier asserts their margins) ----
def elevation(lines, r, shift=0.05):
    """ring r's centre moved by `shift` degrees towards the middle of the fan"""
    c = ring_centre(lines, r)
    mid = ring_centre(lines, lines // 2)
    if lines == 64 and r == 32:
        return c + shift                                           # away from the -8.83 seam, which lies below this ring's centre
    return c + (shift if c < mid else -shift)


def points_at(az_deg, rng_xy, elev_deg):
    """points at azimuth, xy range and elevation, narrowed to float32"""
    az, el = np.deg2rad(np.asarray(az_deg, np.float64)), np.deg2rad(np.asarray(elev_deg, np.float64))
    r = np.asarray(rng_xy, np.float64)
    return np.stack([r * np.cos(az), r * np.sin(az), r * np.tan(el)], axis=-1).astype(np.float32)


def room_range(az_deg, half=(9.0, 6.5), posts=((4.0, 2.5, 0.35), (-5.0, 3.0, 0.4), (2.0, -4.0, 0.3), (-3.0, -3.5, 0.45)), origin=(0.0, 0.0)):
    """xy range from `origin` to a box of half-extents `half` with round posts (x, y, radius) inside, per azimuth"""
    az = np.deg2rad(np.asarray(az_deg, np.float64))
    c, s = np.cos(az), np.sin(az)
    ox, oy = origin
    with np.errstate(all="ignore"):
        tx = np.where(c > 0, (half[0] - ox) / c, np.where(c < 0, (-half[0] - ox) / c, np.inf))
        ty = np.where(s > 0, (half[1] - oy) / s, np.where(s < 0, (-half[1] - oy) / s, np.inf))
    t = np.minimum(tx, ty)
    for px, py, pr in posts:
        mx, my = px - ox, py - oy
        b = mx * c + my * s
        disc = b * b - (mx * mx + my * my - pr * pr)
        with np.errstate(all="ignore"):
            hit = b - np.sqrt(disc)
        t = np.where((disc > 0) & (hit > 0) & (hit < t), hit, t)
    return t


def room_scan(lines, per_ring=300, seed=0, origin=(0.0, 0.0)):
    """a `lines`-ring scan of the room in firing order (azimuth major, ring minor, like a spinning sensor), elevations at elevation(lines, r) with a
    jitter of 0.02 degrees, ranges with 5 mm noise"""
    rng = np.random.default_rng(seed)
    az = np.repeat(np.linspace(-180.0, 180.0, per_ring, endpoint=False), lines) + rng.uniform(-0.1, 0.1, per_ring * lines)
    rid = np.tile(np.arange(lines), per_ring)
    el = np.asarray([elevation(lines, r) for r in range(lines)])[rid] + rng.uniform(-0.02, 0.02, per_ring * lines)
    t = room_range(az, origin=origin) + rng.normal(0.0, 0.005, per_ring * lines)
    keep = rng.uniform(size=len(az)) > 0.03                         # dropouts: the rings differ in size
    return points_at(az[keep], t[keep], el[keep])


def ring_scan(lines, sizes, seed=0, rng_xy=12.0, wobble=0.3):
    """rings of EXACT sizes: sizes = {ring: points}; each ring a closed curve of xy range rng_xy + wobble * sin(5 az), points in ring order"""
    out = []
    rng = np.random.default_rng(seed)
    for r, n in sizes.items():
        az = np.linspace(-180.0, 180.0, n, endpoint=False)
        t = rng_xy + wobble * np.sin(np.deg2rad(5 * az)) + rng.normal(0.0, 0.003, n)
        t = t + 0.5 * (np.arange(n) % 97 == 0)                      # a few true jumps
        out.append(points_at(az, t, np.full(n, elevation(lines, r))))
    return np.concatenate(out) if out else np.zeros((0, 3), np.float32)


def spike_ring(n, spikes, lines=64, r=10, height=0.5, rng_xy=10.0):
    """a smooth ring of n points (xy range rng_xy, points 2 pi rng_xy / n apart) with isolated range spikes of `height` at the given positions"""
    az = np.linspace(-180.0, 180.0, n, endpoint=False)
    t = np.full(n, rng_xy)
    t[np.asarray(spikes, int)] += height
    return points_at(az, t, np.full(n, elevation(lines, r)))


# float32 displacements found by a search over the restatement itself (curvature() / gap2() of lattice_ring with trial values: x sets the
# coarse part of the sum of squares, z the middle part, y, which is exactly 0 around these points, the last bits)
LATTICE_CURV_FIX = tuple(float.fromhex(v) for v in ("0x1.43cc36p-2", "0x1.d082b6p-9", "0x1.f1f51ap-14"))   # the entry before it has curvature 0.1 exactly
LATTICE_GAP_FIX = tuple(float.fromhex(v) for v in ("0x1.c9f1dcp-3", "0x1.22d87ep-11", "0x1.0e165ep-19"))    # its gap to the pick before it is 0.05 exactly
LATTICE_Z0 = -215.0 / 256.0


def lattice_ring(n=400, curv_fix=LATTICE_CURV_FIX, gap_fix=LATTICE_GAP_FIX, at=200, stretch=32):
    """-> (p [n, 3] float32 inside ring 20 of a 64-line sensor, position whose curvature is exactly 0.1, position of the pick whose upper neighbour
    sits at a squared gap of exactly 0.05). A line of points 1/128 apart (along y, along x where y is exactly 0: positions at .. at + stretch), every
    coordinate a small dyadic number, so the float32 chains are exact: curvature exactly 0 on the straight parts, exactly 0.0625 on the five entries
    either side of a 0.25 step-out (every 16th point), exactly 6.25 on the step-outs themselves: ties below, at and above the thresholds."""
    f32 = np.float32
    i = np.arange(n)
    x = np.where(i < at, 10.0, np.where(i <= at + stretch, 10.0 + (i - at) / 128.0, 10.0 + stretch / 128.0))
    y = np.where(i < at, (i - at) / 128.0, np.where(i <= at + stretch, 0.0, (i - at - stretch) / 128.0))
    out = (i % 16 == 8) & ~((i >= at - 6) & (i <= at + stretch + 6))
    x = x + np.where(out, np.where(i < at, 0.25, -0.25), 0.0)
    p = np.stack([x, y, np.full(n, LATTICE_Z0)], axis=1).astype(f32)
    c1, g = at + 8, at + 22
    p[c1 + 1] = (p[c1 + 1, 0] + f32(curv_fix[0]), f32(curv_fix[2]), p[c1 + 1, 2] + f32(curv_fix[1]))
    p[g, 0] = p[g, 0] + f32(0.25)
    p[g + 1] = (p[g, 0] - f32(gap_fix[0]), f32(gap_fix[2]), p[g, 2] + f32(gap_fix[1]))
    return p, c1, g


def quirk_ring(lines=64, r=10, n=1810, rng_xy=10.0):
    """-> (p, dict): a smooth ring of n = 10 + 6 * 300 points with (a) a range kink (slope 0.02 per point either side) on the LAST entry of sector 0, whose
    marks reach the unassigned entry and the first entries of sector 1, and (b) 25 isolated range spikes of 0.5, 11 positions apart, in sector 2"""
    ln = (n - 10) // 6
    kink = 5 + ln - 2
    spikes = [5 + 2 * ln + 5 + 11 * i for i in range(25)]
    az = np.linspace(-180.0, 180.0, n, endpoint=False)
    t = rng_xy + 0.02 * np.clip(6 - np.abs(np.arange(n) - kink), 0, None)
    t[spikes] += 0.5
    return points_at(az, t, np.full(n, elevation(lines, r))), dict(kink=kink, spikes=spikes, sector_len=ln)


def poison_scan(seed=3):
    """a 64-line room scan with NaN / +-inf coordinates, points inside min_distance and beyond max_distance and elevations outside the fan spread through
    it -> (scan, expected counters); the removals shorten the ring lists, so the curvature windows close up over them"""
    rng = np.random.default_rng(seed)
    s = room_scan(64, per_ring=200, seed=seed).copy()
    hit = rng.choice(len(s), 400, replace=False)
    s[hit[:40], rng.integers(0, 3, 40)] = np.nan
    s[hit[40:70], rng.integers(0, 3, 30)] = np.inf
    s[hit[70:100], rng.integers(0, 3, 30)] = -np.inf
    s[hit[100:200]] = points_at(rng.uniform(-180, 180, 100), rng.uniform(0.2, 2.5, 100), rng.uniform(-20, 0, 100))       # inside 3 m
    s[hit[200:300]] = points_at(rng.uniform(-180, 180, 100), rng.uniform(95.0, 200.0, 100), rng.uniform(-20, 0, 100))   # beyond 90 m
    s[hit[300:350]] = points_at(rng.uniform(-180, 180, 50), rng.uniform(5.0, 9.0, 50), rng.choice([10.0, 20.0, 45.0], 50))    # above the fan
    s[hit[350:400]] = points_at(rng.uniform(-180, 180, 50), rng.uniform(5.0, 9.0, 50), rng.choice([-30.0, -40.0, -60.0], 50))  # below it
    return s, dict(n_nonfinite=100, n_out_of_range=200, n_no_ring=100)


_fixtures = {}


def fixtures():
    """every scan the GPU tier extracts features from: name -> (scan [P, 3] float32, options). Built once."""
    if not _fixtures:
        f = _fixtures
        for k in range(3):
            f["room64_%d" % k] = (room_scan(64, 300, seed=10 + k, origin=(0.4 * k, -0.3 * k)), options())
        f["room16"] = (room_scan(16, 300, seed=20), options(num_lines=16))
        f["room32"] = (room_scan(32, 300, seed=21), options(num_lines=32))
        f["sizes"] = (ring_scan(64, {5: 130, 6: 131, 7: 200, 40: MAX_RING_POINTS}, seed=1), options())
        f["sizes_one_sector"] = (f["sizes"][0], options(num_sectors=1))
        f["too_long"] = (ring_scan(64, {3: 150, 41: MAX_RING_POINTS + 1}, seed=2), options())
        f["quirks"] = (quirk_ring()[0], options())
        f["lattice"] = (lattice_ring()[0], options())
        f["poison"] = (poison_scan()[0], options())
        f["tiny"] = (room_scan(64, 100, seed=30), options())
        f["empty"] = (np.zeros((0, 3), np.float32), options())
        f["room64_one_sector"] = (f["room64_0"][0], options(num_sectors=1))
        f["room64_no_edges"] = (f["room64_0"][0], options(max_edges_per_sector=0))
        f["room64_many"] = (f["room64_0"][0], options(num_sectors=64, max_edges_per_sector=64, min_ring_points=11))
    return _fixtures

"""The scan-side index of a handle — the implicit balanced kd-tree of csrc/iba_build.hpp, the leaf-ordered points and the boxes — restated in numpy
LEVEL BY LEVEL, the way csrc/iba_index_kernels.hpp builds it on the device (the host build recurses and partitions with std::nth_element), and the
voxel clouds both tiers of the index tests run on. Test infrastructure only.

Rules (the kernel file's header states the same):
  depth    D = smallest D with (P >> D) <= 24, at most 11.
  level d  segment (d, k) = tree positions [k P >> d, (k + 1) P >> d), mid = (2k + 1) P >> (d + 1): float32 min / max per axis, extents as float32
           subtractions, split dimension = the first axis with strictly the largest extent, the segment ordered by (value along that axis with
           -0.0 == +0.0, original index) — np.lexsort on (index, key with the zeros merged) —, split = the value (its own bits) at rank mid.
  final    inside a leaf ascending original index.
  boxes    per 64 tree positions min xyz, NaN, max xyz, largest |coordinate|; of equal values (-0.0 / +0.0) the first in tree order stays."""
import numpy as np

import submap_ref as V

LEAF_TARGET, MAX_DEPTH, CHUNK = 24, 11, 64
I4 = np.eye(4)


def depth_for(P):
    D = 0
    while (P >> D) > LEAF_TARGET and D < MAX_DEPTH:
        D += 1
    return D


def ordered(v):
    """order-preserving uint32 key of float32 values; both zeros share one key"""
    b = np.ascontiguousarray(v, np.float32).view(np.uint32).astype(np.uint64)
    b = np.where((b & 0x7FFFFFFF) == 0, 0, b)
    return np.where(b & 0x80000000, (~b) & 0xFFFFFFFF, b | 0x80000000).astype(np.uint64)


def _first_min(v):
    """`if (x < mn) mn = x` in ascending position: the FIRST of the values that compare equal to the minimum"""
    return v[np.flatnonzero(v == v.min())[0]]


def _first_max(v):
    return v[np.flatnonzero(v == v.max())[0]]


def build(pts):
    """pts [P, 3] float32 -> dict(depth, perm [P] u32, node_dim / node_split [(1 << D) - 1], xyz_tree [3, P], chunk_box [chunks, 8], frame_box [8])"""
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    P = len(pts)
    D = depth_for(P)
    order = np.arange(P, dtype=np.int64)
    nn = (1 << D) - 1
    dim_out, split_out = np.zeros(nn, np.uint32), np.zeros(nn, np.float32)
    for d in range(D):
        for k in range(1 << d):
            lo, hi, mid = (k * P) >> d, ((k + 1) * P) >> d, ((2 * k + 1) * P) >> (d + 1)
            seg = order[lo:hi]
            v = pts[seg]
            mn, mx = v.min(0), v.max(0)
            ext = (mx - mn).astype(np.float32)
            dim = 0
            for a in (1, 2):
                if ext[a] > ext[dim]:
                    dim = a
            assert lo < mid < hi, "a segment above the leaves holds more than 24 points: the host's other branches are unreachable"
            o = np.lexsort((seg, ordered(v[:, dim])))
            order[lo:hi] = seg[o]
            dim_out[(1 << d) - 1 + k] = dim
            split_out[(1 << d) - 1 + k] = pts[order[mid], dim]
    for j in range(1 << D):
        lo, hi = (j * P) >> D, ((j + 1) * P) >> D
        order[lo:hi] = np.sort(order[lo:hi])
    t = pts[order]
    nan = np.float32(np.nan)
    nc = (P + CHUNK - 1) // CHUNK
    box = np.full((nc, 8), nan, np.float32)
    for c in range(nc):
        w = t[c * CHUNK:(c + 1) * CHUNK]
        for a in range(3):
            box[c, a], box[c, 4 + a] = _first_min(w[:, a]), _first_max(w[:, a])
        box[c, 7] = max(np.abs(box[c, :3]).max(), np.abs(box[c, 4:7]).max())
    fbox = np.full(8, nan, np.float32)
    if P:
        for a in range(3):
            fbox[a], fbox[4 + a] = _first_min(box[:, a]), _first_max(box[:, 4 + a])
    return dict(depth=D, perm=order.astype(np.uint32), node_dim=dim_out, node_split=split_out, xyz_tree=np.ascontiguousarray(t.T), chunk_box=box, frame_box=fbox)


KEYS = ("perm", "xyz_tree", "node_dim", "node_split", "chunk_box", "frame_box")


def first_difference(a, b):
    """None when two indices are equal as raw bytes, else words that name the first difference: the node (level, k, dim, split) or the tree position"""
    if a["depth"] != b["depth"]:
        return "depth %d != %d" % (a["depth"], b["depth"])
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.shape != y.shape or x.dtype != y.dtype:
            return "%s: shape / type %s %s != %s %s" % (key, x.shape, x.dtype, y.shape, y.dtype)
    nd = np.flatnonzero((a["node_dim"] != b["node_dim"]) | (a["node_split"].view(np.uint32) != b["node_split"].view(np.uint32)))
    if len(nd):
        i = int(nd[0]); lvl = (i + 1).bit_length() - 1
        return "node level %d k %d: dim %d split %r (0x%08x) != dim %d split %r (0x%08x); %d nodes differ" % (
            lvl, i + 1 - (1 << lvl), a["node_dim"][i], float(a["node_split"][i]), a["node_split"].view(np.uint32)[i], b["node_dim"][i], float(b["node_split"][i]), b["node_split"].view(np.uint32)[i], len(nd))
    for key in KEYS:
        x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key])
        if x.tobytes() != y.tobytes():
            xv, yv = x.view(np.uint32).reshape(x.shape), y.view(np.uint32).reshape(y.shape)
            bad = np.argwhere(xv != yv)
            return "%s at %s: 0x%08x != 0x%08x; %d words differ" % (key, bad[0].tolist(), xv[tuple(bad[0])], yv[tuple(bad[0])], len(bad))
    return None


# ---- the shared scene and its clouds ----
P_EDGES = (1, 24, 25, 49, 63, 64, 65)
_cache = {}


def scene(synth):
    """8 scans of 3000 points + a scan snapped to a 0.25 m lattice + a scan whose y column is, for every other point, the smallest float32 of either sign
    (the `zeros` pose scales y by 0.25: those averages narrow to -0.0f / +0.0f) + an empty scan -> (scans, poses, ids)"""
    if "scene" not in _cache:
        prob, meta = synth.make_scene(n_frames=8, pts_per_frame=3000, n_keypoints=50, seed=11)
        scans = [prob.frame_points(f).copy() for f in range(8)]
        poses = [meta["Twl"][f].copy() for f in range(8)]
        snapped = (np.round(scans[4].astype(np.float64) * 4.0) / 4.0).astype(np.float32)
        tiny = np.float32(1.4e-45)
        zeros = scans[2].copy()
        odd = np.arange(1, len(zeros), 2)
        zeros[odd, 1] = np.where((odd // 2) % 2 == 0, tiny, -tiny)
        scans += [snapped, zeros, np.zeros((0, 3), np.float32)]
        _cache["scene"] = (scans, poses, dict(snapped=8, zeros=9, empty=10))
    return _cache["scene"]


ZERO_POSE = np.diag([1.0, 0.25, 1.0, 1.0])


def _count(q, voxel):
    idx, _ = V.indices(q, voxel)
    return len(np.unique((idx[:, 0] << 40) | (idx[:, 1] << 20) | idx[:, 2]))


def voxel_for(scan, target):
    """a voxel size at which LoadPCD of `scan` has exactly `target` voxels, searched downwards on a fixed geometric ladder with the restatement's index expression"""
    q = np.asarray(scan, np.float32).astype(np.float64)
    for voxel in np.geomspace(400.0, 1.0, 6000):
        if _count(q, float(voxel)) == target:
            return float(voxel)
    raise AssertionError("no voxel size on the ladder gives %d voxels" % target)


def cases(synth):
    """[(name, (frames, poses, out, voxel))]: P = 0, 1, 24, 25, 49, 63, 64, 65, a P with P % 4 != 0, the lattice, the signed zeros, a merged cloud, one
    above 49 152 voxels (depth 11, leaves above 24 points)"""
    if "cases" not in _cache:
        scans, poses, ids = scene(synth)
        out = [("P=0", ([ids["empty"]], [I4], None, 0.4))]
        for t in P_EDGES:
            out.append(("P=%d" % t, ([0], [I4], None, voxel_for(scans[0], t))))
        q1 = scans[1].astype(np.float64)
        odd = next(v for v in (0.4, 0.41, 0.42, 0.43, 0.44, 0.45, 0.46, 0.47) if _count(q1, v) % 4 != 0)
        out.append(("P%4", ([1], [I4], None, odd)))
        out.append(("lattice", ([ids["snapped"]], [I4], None, 0.25)))      # the lattice step: every voxel holds equal points, the averages stay on the lattice
        out.append(("zeros", ([ids["zeros"]], [ZERO_POSE], None, 0.4)))
        out.append(("merged", ([3, 4, 5], [poses[3], poses[4], poses[5]], V.inverse34(poses[4]), 0.4)))
        big_fr, big_ps = [], []
        for shift in (0.0, 150.0, 300.0):
            for f in range(8):
                T = np.array(poses[f], np.float64).reshape(-1, 4)[:3].copy()
                T4 = np.eye(4); T4[:3] = T; T4[1, 3] += shift
                big_fr.append(f); big_ps.append(T4)
        out.append(("deep", (big_fr, big_ps, None, 0.05)))
        _cache["cases"] = out
    return _cache["cases"]


def clouds(synth):
    """the float32 clouds of cases() from the restatement of the voxel pass (tests/submap_ref.py), CPU only: {name: [P, 3] float32}"""
    if "clouds" not in _cache:
        scans, _, _ = scene(synth)
        res = {}
        for name, (fr, ps, o, voxel) in cases(synth):
            res[name] = V.build([(scans[f], T) for f, T in zip(fr, ps)], voxel, o)["xyz"].astype(np.float32)
        _cache["clouds"] = res
    return _cache["clouds"]

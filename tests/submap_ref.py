"""TEST INFRASTRUCTURE: voxel down-sampling and merged sub-map clouds (iba_submap_build, include/iba_mi355x.h) restated in numpy. Imports nothing
from the product. The rules (Open3D's public PointCloud::Transform, operator+= and VoxelDownSample, with the choices the header fixes):
  1  a member's float32 points widened to f64; q_r = ((T[r,0] x + T[r,1] y) + T[r,2] z) + T[r,3], four separately rounded operations (numpy's
     elementwise arithmetic: no fma); a point with a non-finite coordinate before or after the transform is dropped and counted
  2  minb = min over the kept q - 0.5 voxel; index = floor((q - minb) / voxel)
  3  a voxel's point = (sum of its q, SEQUENTIALLY in concatenation order: members in list order, points in scan order) / float(count).
     np.sum / np.add.reduce are pairwise and are not used: the sums are accumulated by rank inside the voxel
  4  out (None: none) applied to every averaged point with the expression of rule 1
  5  voxels in ascending (ix, iy, iz)"""
import numpy as np


def pose34(T):
    """a 3x4 / 4x4 / 12-vector as a 3x4 f64 array"""
    return np.asarray(T, np.float64).reshape(-1, 4)[:3].copy()


def apply(T, p):
    """rule 1's expression on points p [n, 3] (f64) -> [n, 3]"""
    T = pose34(T)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return np.stack([((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(3)], 1)


def concatenate(members):
    """members: [(points [n, 3] float32, pose)] -> (kept q [k, 3] in concatenation order, dropped count)"""
    qs, dropped = [], 0
    for pts, T in members:
        p = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
        q = apply(T, p)
        keep = np.isfinite(p).all(1) & np.isfinite(q).all(1)
        dropped += int((~keep).sum())
        qs.append(q[keep])
    return (np.concatenate(qs) if qs else np.zeros((0, 3))), dropped


def indices(q, voxel):
    """rule 2 -> (integer indices [k, 3], minb)"""
    voxel = np.float64(voxel)
    minb = q.min(0) - np.float64(0.5) * voxel
    return np.floor((q - minb) / voxel).astype(np.int64), minb


def build(members, voxel, out=None):
    """-> dict(xyz [V, 3] f64, count [V] int32, n_dropped, idx [V, 3] int64 (the voxel indices, for the tests), minb)"""
    q, dropped = concatenate(members)
    if len(q) == 0:
        return dict(xyz=np.zeros((0, 3)), count=np.zeros(0, np.int32), n_dropped=dropped, idx=np.zeros((0, 3), np.int64), minb=None)
    idx, minb = indices(q, voxel)
    order = np.lexsort((idx[:, 2], idx[:, 1], idx[:, 0]))          # stable: equal keys keep their concatenation order
    si, sq = idx[order], q[order]
    head = np.r_[True, np.any(si[1:] != si[:-1], axis=1)]
    start = np.flatnonzero(head)
    count = np.diff(np.r_[start, len(sq)])
    acc = np.zeros((len(start), 3))
    live = np.arange(len(start))
    r = 0
    while len(live):                                                # rank r of every voxel that has one: acc = (..((0 + q_0) + q_1) + ..)
        acc[live] = acc[live] + sq[start[live] + r]
        r += 1
        live = live[count[live] > r]
    xyz = acc / count.astype(np.float64)[:, None]
    if out is not None:
        xyz = apply(out, xyz)
    return dict(xyz=xyz, count=count.astype(np.int32), n_dropped=dropped, idx=si[start], minb=minb)


def load_pcd(points, voxel):
    """BackEndOptimizer::LoadPCD: one member, the identity pose, no output transform"""
    return build([(points, np.eye(4))], voxel)


def inverse34(T):
    """pose^-1 of a rigid 3x4 / 4x4 (what MergeLoadPCD passes as the output transform), as a 4x4"""
    M = np.eye(4); M[:3] = pose34(T)
    return np.linalg.inv(M)

"""numpy restatement of the scan-to-image projection's rules P2-P9 (include/iba_mi355x.h, iba_project_*), what tests/test_gpu_project.py holds the
device against byte for byte. All arithmetic is IEEE f64 in the header's expression order (numpy's ufuncs do not contract); the z-buffer is an
integer minimum (np.minimum.at), so no result depends on an order. The pose (P1) is an INPUT: the 12 doubles iba_projection_pose returns."""
import numpy as np

IN_FRONT, INSIDE, VISIBLE = 1, 2, 4
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
STOPS = np.array([[0, 0, 255], [0, 255, 255], [0, 255, 0], [255, 255, 0], [255, 0, 0]], np.float64)   # zn = 0, 0.25, 0.5, 0.75, 1


def project(points, Rt, camera, splat=1, occlusion_tol=0.02, z_min=0.1, z_max=120.0, v_focal_is_fx=0):
    """points [n, 3] float32 in the caller's order, Rt [3, 4], camera (fx, fy, cx, cy, W, H) -> dict(uv [n, 2] f64, z [n] f32, flags [n] u8,
    depth [H, W] f32, index [H, W] u32, counts)"""
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = len(pts)
    Rt = np.asarray(Rt, np.float64).reshape(3, 4)
    fx, fy, cx, cy, W, H = (float(c) for c in camera)
    Wi, Hi, r = int(W), int(H), int(splat)
    f = fx if v_focal_is_fx else fy
    x, y, z = (pts[:, k].astype(np.float64) for k in range(3))                                       # P2
    finite = np.isfinite(pts).all(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        q = [((Rt[k, 0] * x + Rt[k, 1] * y) + Rt[k, 2] * z) + Rt[k, 3] for k in range(3)]
        front = finite & (z_min < q[2]) & (q[2] < z_max)                                             # P3
    u, v, z32 = np.zeros(n), np.zeros(n), np.zeros(n, np.float32)
    qx, qy, qz = (a[front] for a in q)
    u[front] = (fx * qx + cx * qz) / qz
    v[front] = (f * qy + cy * qz) / qz
    z32[front] = qz.astype(np.float32)
    inside = front & (0.0 <= u) & (u < W) & (0.0 <= v) & (v < H)
    ins = np.flatnonzero(inside)
    iu, iv = np.floor(u[ins]).astype(np.int64), np.floor(v[ins]).astype(np.int64)
    key = (z32[ins].view(np.uint32).astype(np.uint64) << np.uint64(32)) | ins.astype(np.uint64)      # P4
    zbuf = np.full(Wi * Hi, EMPTY_KEY, np.uint64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            xx, yy = iu + dx, iv + dy
            ok = (xx >= 0) & (xx < Wi) & (yy >= 0) & (yy < Hi)
            np.minimum.at(zbuf, yy[ok] * Wi + xx[ok], key[ok])
    holds = zbuf != EMPTY_KEY                                                                        # P5
    depth = np.where(holds, (zbuf >> np.uint64(32)).astype(np.uint32), np.uint32(0)).astype(np.uint32).view(np.float32).reshape(Hi, Wi)
    index = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.uint32).reshape(Hi, Wi)
    visible = np.zeros(n, bool)                                                                      # P6
    zwin = depth[iv, iu]
    visible[ins] = z32[ins].astype(np.float64) <= zwin.astype(np.float64) * (1.0 + occlusion_tol)
    flags = (front * IN_FRONT + inside * INSIDE + visible * VISIBLE).astype(np.uint8)
    counts = dict(n_points=n, n_skipped=int((~finite).sum()), n_in_front=int(front.sum()), n_inside=int(inside.sum()), n_visible=int(visible.sum()),
                  n_pixels=int(holds.sum()))                                                         # P9
    return dict(uv=np.stack([u, v], axis=1), z=z32, flags=flags, depth=depth, index=index, counts=counts)


def colorize(res, rgb):
    """P7: res of project(), rgb [H, W, 3] uint8 -> [n, 3] uint8"""
    img = np.asarray(rgb, np.uint8).astype(np.float64)
    Hi, Wi = img.shape[:2]
    out = np.zeros((len(res["flags"]), 3), np.uint8)
    vis = np.flatnonzero(res["flags"] & VISIBLE)
    u, v = res["uv"][vis, 0], res["uv"][vis, 1]
    x0, y0 = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    x1, y1 = np.minimum(x0 + 1, Wi - 1), np.minimum(y0 + 1, Hi - 1)
    a, b = (u - x0)[:, None], (v - y0)[:, None]
    c00, c01, c10, c11 = img[y0, x0], img[y1, x0], img[y0, x1], img[y1, x1]                          # the first index of c is x
    c = ((1.0 - a) * ((1.0 - b) * c00 + b * c01)) + (a * ((1.0 - b) * c10 + b * c11))
    out[vis] = np.floor(c + 0.5).astype(np.uint8)
    return out


def gradient(zn):
    """P8's palette: zn scalar or array -> uint8 [..., 3]; zn is clamped to [0, 1], NaN counts as 0"""
    zn = np.asarray(zn, np.float64)
    zn = np.where(zn > 0.0, zn, 0.0)
    zn = np.where(zn > 1.0, 1.0, zn)
    s = 4.0 * zn
    k = np.minimum(np.floor(s).astype(np.int64), 3)
    f = (s - k)[..., None]
    return np.floor(((1.0 - f) * STOPS[k] + f * STOPS[k + 1]) + 0.5).astype(np.uint8)


def overlay(res, rgb=None, z_near=2.0, z_far=60.0):
    """P8: res of project(), rgb [H, W, 3] uint8 or None (black) -> [H, W, 3] uint8"""
    Hi, Wi = res["depth"].shape
    out = np.zeros((Hi, Wi, 3), np.uint8) if rgb is None else np.asarray(rgb, np.uint8).copy()
    holds = res["index"] != np.uint32(0xFFFFFFFF)
    z = res["depth"][holds].astype(np.float64)
    zn = np.minimum(np.maximum((z - z_near) / (z_far - z_near), 0.0), 1.0)
    out[holds] = gradient(zn)
    return out

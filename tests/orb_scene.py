"""Seeded grey test images and a seeded BRIEF test-pair table for the ORB tests. An image is a mosaic of 20-pixel blocks on a grey ground: filled
rectangles and checkerboards at contrasts 40 (above ini_th_fast = 20), 12 (between the thresholds 7 and 20) and 4 (below both), blocks of two-valued
noise (equal adjacent FAST scores), and — where the image is large enough — a flat region of whole cells."""
import numpy as np

BLOCK = 20
KINDS = ("rect40", "rect12", "rect4", "check40", "check12", "check4", "noise", "flat")


def pattern(seed=7):
    """256 x 4 int8 (x0 y0 x1 y1), every point inside the disc x^2 + y^2 <= 324"""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < 512:
        x, y = (int(v) for v in rng.integers(-18, 19, 2))
        if x * x + y * y <= 324:
            pts.append((x, y))
    return np.array(pts, np.int8).reshape(256, 4)


def image(W, H, seed):
    """uint8 [H, W]"""
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 100, np.uint8)
    flat_x, flat_y = (int(0.45 * W), int(0.5 * H)) if W >= 150 else (0, H)   # the flat region: x < flat_x and y >= flat_y
    for by in range(0, H, BLOCK):
        for bx in range(0, W, BLOCK):
            kind = KINDS[int(rng.integers(0, len(KINDS)))]
            if bx < flat_x and by >= flat_y or kind == "flat":
                continue
            h, w = min(BLOCK, H - by), min(BLOCK, W - bx)
            blk = img[by:by + h, bx:bx + w]
            if kind == "noise":
                blk[:] = np.where(rng.integers(0, 2, (h, w)) == 1, 140, 100).astype(np.uint8)
                continue
            c = int(kind[5:] if kind.startswith("check") else kind[4:])
            sign = 1 if rng.integers(0, 2) else -1
            if kind.startswith("rect"):
                x0, y0 = (int(v) for v in rng.integers(2, 8, 2))
                x1, y1 = (int(v) for v in rng.integers(11, 18, 2))
                blk[y0:min(y1, h), x0:min(x1, w)] = 100 + sign * c
            else:
                yy, xx = np.mgrid[0:h, 0:w]
                blk[:] = np.where(((yy // 5) + (xx // 5)) % 2 == 0, 100 + sign * c, 100).astype(np.uint8)
    return img


def strided(img, pad=13):
    """the same pixels in a buffer whose rows are pad bytes longer (stride > W); the padding holds 255"""
    H, W = img.shape
    buf = np.full((H, W + pad), 255, np.uint8)
    buf[:, :W] = img
    return buf[:, :W]

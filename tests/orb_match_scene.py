"""Seeded frames for the windowed-matching tests and bench: a sequence in which frame k + 1 is frame k with jittered positions and angles and a few
flipped bits per descriptor. Half of the keypoints lie in a dense cluster (long candidate lists), some are near-copies of a neighbour (equal or close
distances: ratio rejections and displacements) and some turn by a random angle (rotation removals)."""
import numpy as np

import orb_match_ref as R

F = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SCALE_FACTORS = (F(1.2) ** np.arange(8)).astype(F)


def flip(d, bits):
    """the descriptor d with the given bits flipped"""
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[int(b) // 8] ^= np.uint8(1 << (int(b) % 8))
    return d


def first_frame(n, rng, bounds=BOUNDS, sigma=45.0):
    half = n // 2
    x0, x1, y0, y1 = bounds
    xy = np.concatenate([np.stack([rng.uniform(x0 + 5, x1 - 5, n - half), rng.uniform(y0 + 5, y1 - 5, n - half)], 1),
                         np.stack([rng.normal(0.5 * (x0 + x1), sigma, half), rng.normal(0.5 * (y0 + y1), sigma, half)], 1)])
    desc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    for i in range(0, n, 9):                      # near-copies of the next keypoint: the same place within a few pixels, the descriptor within 3 bits
        if i + 1 < n:
            xy[i] = xy[i + 1] + rng.uniform(-4, 4, 2)
            desc[i] = flip(desc[i + 1], rng.choice(256, int(rng.integers(0, 4)), replace=False))
    octave = np.where(rng.uniform(size=n) < 0.45, 0, rng.integers(1, 8, n))
    octave[0:n - 1:9] = octave[1:n:9][:len(octave[0:n - 1:9])]      # a near-copy shares its neighbour's octave
    return R.make_frame(xy.astype(F), octave, rng.uniform(0, 360, n).astype(F), desc, bounds)


def next_frame(f, rng):
    n = len(f["octave"])
    xy = f["xy"] + rng.normal(0, 2.0, (n, 2)).astype(F)
    turn = np.where(rng.uniform(size=n) < 0.12, rng.uniform(-180, 180, n), rng.normal(0, 4, n))
    angle = np.mod(f["angle"].astype(np.float64) + turn, 360.0).astype(F)
    angle[angle >= F(360)] = F(0)
    desc = np.array([flip(d, rng.choice(256, int(rng.integers(0, 9)), replace=False)) for d in f["desc"]], np.uint8).reshape(n, 32)
    return R.make_frame(xy, f["octave"], angle, desc, f["bounds"])


def sequence(n_frames, n, seed, bounds=BOUNDS, sigma=45.0):
    rng = np.random.default_rng(seed)
    frames = [first_frame(n, rng, bounds, sigma)]
    for _ in range(n_frames - 1):
        frames.append(next_frame(frames[-1], rng))
    return frames


def init_job(frames, a, b, window=100, n_queries=None):
    """SearchForInitialization from frame a to frame b: prev_matched = frame a's own positions"""
    q = R.init_queries(frames[a], frames[a]["xy"], window)
    k = len(q["radius"]) if n_queries is None else n_queries
    return dict({key: v[:k] for key, v in q.items()}, query_frame=a, train_frame=b, rule=R.INIT)


def claim_job(frames, a, b, th=15.0, n_queries=None, seed=0):
    """SearchByProjection from the last frame a into the current frame b: world points that project onto frame a's keypoints under the identity pose"""
    rng = np.random.default_rng(seed)
    f = frames[a]
    n = len(f["octave"])
    x0, x1, y0, y1 = (float(v) for v in frames[b]["bounds"])
    fx, fy, cx, cy = 500.0, 500.0, 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    z = rng.uniform(2, 30, n)
    X = np.stack([(f["xy"][:, 0] - cx) / fx * z, (f["xy"][:, 1] - cy) / fy * z, z], 1).astype(F)
    has, outl = (rng.uniform(size=n) < 0.9).astype(np.uint8), (rng.uniform(size=n) < 0.05).astype(np.uint8)
    q = R.motion_queries(f, has, outl, X, np.eye(3, 4, dtype=F), fx, fy, cx, cy, frames[b]["bounds"], SCALE_FACTORS, th)
    k = n if n_queries is None else n_queries
    return dict({key: v[:k] for key, v in q.items()}, query_frame=a, train_frame=b, rule=R.CLAIM)

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


N_LIMIT = 32768                              # IBA_ORB_MATCH_MAX_KEYPOINTS
FILL_FIRST, FILL_N, FILL_CELL = 16384, 150, (20, 10)
LIMIT_TARGETS = (0, 8191, 8192) + tuple(range(N_LIMIT - 32, N_LIMIT)) + tuple(range(FILL_FIRST + 60, FILL_FIRST + 70))


def limit_scene(seed=17, n_queries=300):
    """frame 0: exactly N_LIMIT keypoints at random places, about ten per cell. The FILL_N keypoints from index FILL_FIRST (a multiple of 64) on lie
    in the one cell FILL_CELL and nothing else does: two whole trips of the ordered fill have all 64 lanes in that cell and a third has 22. Frame 1:
    n_queries keypoints, each half a pixel from a keypoint of frame 0 with its angle and its descriptor within 6 bits: LIMIT_TARGETS first (index 0,
    the two sides of 8192, the last 32, ten of the filled cell), then random ones; every eighth repeats its predecessor's target. One CLAIM job from
    frame 1 into frame 0, whose state is in global memory at this size"""
    rng = np.random.default_rng(seed)
    n = N_LIMIT
    xy = np.stack([rng.uniform(5, 635, n), rng.uniform(5, 475, n)], 1).astype(F)
    fill = np.arange(FILL_FIRST, FILL_FIRST + FILL_N)
    cx, cy = 10.0 * FILL_CELL[0], 10.0 * FILL_CELL[1]                        # ten pixels per cell: the cell's centre
    inside = (np.abs(xy[:, 0] - F(cx)) <= 5) & (np.abs(xy[:, 1] - F(cy)) <= 5)
    xy[inside, 0] += F(20.0)
    xy[fill] = np.stack([rng.uniform(cx - 4, cx + 4, FILL_N), rng.uniform(cy - 4, cy + 4, FILL_N)], 1)
    train = R.make_frame(xy, rng.integers(0, 3, n), rng.uniform(0, 360, n).astype(F), rng.integers(0, 256, (n, 32)), BOUNDS)
    target = np.concatenate([LIMIT_TARGETS, rng.choice(n, n_queries - len(LIMIT_TARGETS), replace=False)]).astype(np.int64)
    target[7::8] = target[6::8][:len(target[7::8])]
    qdesc = np.array([flip(train["desc"][t], rng.choice(256, k % 7, replace=False)) for k, t in enumerate(target)], np.uint8)
    query = R.make_frame(train["xy"][target] + F(0.5), train["octave"][target], train["angle"][target], qdesc, BOUNDS)
    k = n_queries
    job = {"query_frame": 1, "train_frame": 0, "rule": R.CLAIM, "centre_xy": query["xy"].copy(), "radius": np.full(k, 12.0, F), "level_range": np.tile(np.array([-1, -1], np.int32), (k, 1)),
           "query_index": np.arange(k, dtype=np.int32), "valid": None}
    return {"frames": [train, query], "jobs": [job], "target": target}


def check_limit(sc, grids, refs):
    """the conditions of limit_scene(), on the REFERENCE's grid and results"""
    n, r, target = N_LIMIT, refs[0], sc["target"]
    off, lst = grids[0]
    assert len(sc["frames"][0]["octave"]) == n and off[-1] == n and FILL_FIRST % 64 == 0 and FILL_N >= 130 and FILL_N % 64
    cell = FILL_CELL[0] * R.ROWS + FILL_CELL[1]
    assert lst[off[cell]:off[cell + 1]].tolist() == list(range(FILL_FIRST, FILL_FIRST + FILL_N))
    assert int(np.max(np.diff(off))) == FILL_N and int(np.sum(np.diff(off) > 0)) > 2500
    # the window job reads the filled cell, and claims up to the last keypoint
    assert r["max_segment"] >= FILL_N and all(r["match"][k] == target[k] for k in range(len(LIMIT_TARGETS)) if k % 8 != 7)
    assert n - 1 in r["match"] and int(np.sum(r["match"] >= n - 32)) >= 28 and r["n_matches"] > 250
    again = [k for k in range(7, len(target), 8)]                            # a repeated target is taken: the query gets another keypoint or none
    assert all(r["match"][k] != target[k] for k in again) and all(r["match"][k - 1] == target[k] for k in again)

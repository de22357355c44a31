"""Seeded synthetic frame pairs for the two-view initialisation tests (tests/test_twoview_cpu.py, tests/test_gpu_twoview.py), and the reference
results of the scene list, computed once per process by tests/twoview_ref.py and shared by every test that compares with them.

A pair is a pinhole camera (700 / 700 / 620 / 188, a 1240 x 376 image) that sees n points at depths 6-20 m, moves by `baseline` metres along x with a
small yaw, and matches them with pixel noise and a share of random outliers; frame 2 holds extra keypoints and is shuffled, and a share of frame 1's
keypoints is unmatched (-1). The seeds of SCENES were picked by running the reference: with the 8-point F and no refinement a general pair at a 1 m
baseline is accepted at 4-5 degrees of parallax for some seeds and refused (n_good below 0.9 N) for others, which is the reference's behaviour."""
import functools

import numpy as np

import twoview_ref as ref

K4 = (700.0, 700.0, 620.0, 188.0)
W, H = 1240.0, 376.0
ITERATIONS = 70          # of the scene list's one call


def make_pair(seed, n=300, baseline=1.0, noise=0.3, outliers=0.2, planar=False, unmatched=0.1, extra2=23, yaw=0.01, same_place=False, identical=False):
    """-> dict(xy1 [n, 2] f32, xy2 [n + extra2, 2] f32, matches12 [n] i32, K)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = K4
    u, v = rng.uniform(0, W, n), rng.uniform(0, H, n)
    Z = rng.uniform(6, 20, n)
    if planar:
        Z = 12.0 + 0.004 * (u - cx) + 0.002 * (v - cy)          # a slanted plane
    X = np.stack([(u - cx) / fx * Z, (v - cy) / fy * Z, Z], 1)
    c, s = np.cos(yaw), np.sin(yaw)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    X2 = X @ R.T + np.array([-baseline, 0, 0])
    xy1 = np.stack([u, v], 1) + rng.normal(0, noise, (n, 2)) if noise else np.stack([u, v], 1)
    xy2 = np.stack([fx * X2[:, 0] / X2[:, 2] + cx, fy * X2[:, 1] / X2[:, 2] + cy], 1)
    if noise:
        xy2 = xy2 + rng.normal(0, noise, (n, 2))
    if identical:
        xy2 = xy1.copy()
    out = rng.random(n) < outliers
    xy2[out] = np.stack([rng.uniform(0, W, out.sum()), rng.uniform(0, H, out.sum())], 1)
    n2 = n + extra2
    xy2 = np.concatenate([xy2, np.stack([rng.uniform(0, W, extra2), rng.uniform(0, H, extra2)], 1)])
    perm = rng.permutation(n2)                                   # new index -> old index
    inv = np.argsort(perm)
    matches12 = inv[:n].astype(np.int32)
    matches12[rng.random(n) < unmatched] = -1
    xy1 = xy1.astype(np.float32)
    if same_place:
        xy1[:] = (100.0, 50.0)
    return {"xy1": xy1, "xy2": np.ascontiguousarray(xy2[perm], np.float32), "matches12": matches12, "K": K4}


def n_matches(p):
    return int((p["matches12"] >= 0).sum())


def with_sets(p, iterations, seed):
    p = dict(p)
    N = n_matches(p)
    p["sets"] = ref.make_sets(N, iterations, seed) if N >= 8 else None
    return p


# name -> (the status the reference must give, the model it must take or None, make_pair's arguments). Ragged on purpose: n, n2 and N all differ.
SCENES = (
    ("general_ok", ref.OK, 0, dict(seed=0, n=300)),
    ("plane_ok", ref.OK, 1, dict(seed=1, n=280, planar=True, outliers=0.1)),
    ("refused_few_points", ref.TOO_FEW_POINTS, 0, dict(seed=1, n=300)),
    ("low_parallax", ref.LOW_PARALLAX, None, dict(seed=0, n=260, baseline=0.12, outliers=0.0, noise=0.05)),
    ("no_clear_winner", ref.NO_CLEAR_WINNER, None, dict(seed=0, n=240, baseline=0.004, outliers=0.0, noise=0.05)),
    ("h_degenerate", ref.H_DEGENERATE, 1, dict(seed=5, n=200, identical=True, outliers=0.0, noise=0.0, extra2=5)),
    ("too_few_matches", ref.TOO_FEW_MATCHES, None, dict(seed=6, n=9, unmatched=0.5, outliers=0.0)),
    ("no_model", ref.NO_MODEL, None, dict(seed=7, n=40, same_place=True, outliers=0.0)),       # T1 is not finite: every hypothesis is NaN
)
SETS_SEED = 1000


@functools.lru_cache(maxsize=None)
def scene_pairs(iterations=ITERATIONS):
    """the scene list with its sets, in SCENES' order"""
    return tuple(with_sets(make_pair(**kw), iterations, SETS_SEED) for _, _, _, kw in SCENES)


def reference(p, iterations, **opts):
    return ref.twoview(p["xy1"], p["xy2"], p["matches12"], p["K"], p["sets"], iterations=iterations, **opts)


@functools.lru_cache(maxsize=None)
def scene_reference(iterations=ITERATIONS):
    """the reference's results of the scene list under the default options: computed once, shared, never written to"""
    return tuple(reference(p, iterations) for p in scene_pairs(iterations))


# ---- eight small pairs for the calls of more pairs than one block of lanes: cheap references, every way through the acceptance ----
SMALL_ITERATIONS = 9
# (the status the reference must give, make_pair's arguments; the sets' seed is the pair's). The seeds were picked by running the reference alone.
SMALL = (
    (ref.OK, dict(seed=5, n=64, noise=0.1)),                                   # F, accepted
    (ref.TOO_FEW_POINTS, dict(seed=1, n=8, noise=0.1)),                        # F, refused by the acceptance: no candidate
    (ref.LOW_PARALLAX, dict(seed=1, n=60, baseline=0.12, noise=0.05)),         # F, a candidate, refused on its parallax
    (ref.OK, dict(seed=1, n=64, planar=True)),                                 # H, eight hypotheses, accepted
    (ref.TOO_FEW_POINTS, dict(seed=4, n=40, noise=0.1)),
    (ref.OK, dict(seed=2, n=56, noise=0.1)),
    (ref.NO_CLEAR_WINNER, dict(seed=1, n=60, baseline=0.05, noise=0.02)),      # H, no candidate
    (ref.TOO_FEW_MATCHES, dict(seed=6, n=9, unmatched=0.5)),                   # N < 8
)


@functools.lru_cache(maxsize=None)
def small_pairs():
    return tuple(with_sets(make_pair(**dict(dict(unmatched=0.0, outliers=0.0), **kw)), SMALL_ITERATIONS, kw["seed"]) for _, kw in SMALL)


@functools.lru_cache(maxsize=None)
def small_reference():
    """the reference's results of small_pairs(): computed once, shared, never written to"""
    return tuple(reference(p, SMALL_ITERATIONS) for p in small_pairs())


def check_small_reference():
    """what the reference itself must say of the eight: the statuses of SMALL; seven pairs of 8..64 matches and one below 8; an accepted pair, a pair
    refused by the acceptance and the pair below 8 matches; no parallax so near the threshold that acos' one-ulp freedom could flip a status"""
    refs = small_reference()
    assert [e["status"] for e in refs] == [st for st, _ in SMALL], [e["status"] for e in refs]
    N = [n_matches(p) for p in small_pairs()]
    assert all(8 <= n <= 64 for n in N[:7]) and min(N[:7]) == 8 and max(N[:7]) == 64 and N[7] < 8, N
    assert {e["model"] for e in refs if e["status"] == ref.OK} == {0, 1}
    for e in refs:
        if e["status"] in (ref.OK, ref.LOW_PARALLAX):
            assert e["chosen"] >= 0 and abs(float(e["parallax_deg"][e["chosen"]]) - 1.0) > 1e-3
        else:
            assert e["chosen"] == -1


def cycle_of_small(n):
    """the indices into small_pairs() of a call of n pairs: pair k % 8, and pair 0 again as the last"""
    return [k % 8 for k in range(n - 1)] + [0]


def output_bytes(res, pair):
    """the bytes of every output of one pair that does not need keep_stages: read() (parallax_deg too), matches() and points()"""
    d = res.read(pair)
    arrays = zip(("list", "inlier", "points", "triangulated"), res.matches(pair) + res.points(pair))
    return [(k, np.asarray(d[k]).tobytes()) for k in sorted(d)] + [(k, x.tobytes()) for k, x in arrays]


# ---- comparing a library result (twoview.Twoview) with a reference dict: every output and kept stage, named ----
SCALARS = ("status", "n_matches", "model", "n_hyp", "chosen", "best_it_H", "best_it_F", "n_inliers_H", "n_inliers_F", "SH", "SF", "RH")
ARRAYS = ("H21", "F21", "n_good", "cos_parallax", "R21", "t21")


def ulp_apart(a, b):
    """the distance of two float32 arrays in units in the last place (both finite and of one sign, or equal)"""
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)


def differences(res, pair, e, stages=True):
    """-> a list of (name, number of differing bytes) over every output and kept stage of one pair; parallax_deg counts where it is more than one
    float32 ulp away (libm's acos is not correctly rounded)"""
    out = []

    def same(name, a, b):
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(np.asarray(b).astype(np.asarray(a).dtype))
        n = int((np.frombuffer(a.tobytes(), np.uint8) != np.frombuffer(b.tobytes(), np.uint8)).sum()) if a.shape == b.shape else -1
        if n:
            out.append((name, n))

    d = res.read(pair)
    for k in SCALARS + ARRAYS:
        same(k, np.asarray(d[k]), np.asarray(e[k]))
    both_nan = np.isnan(d["parallax_deg"]) & np.isnan(e["parallax_deg"])          # acos of a cosine above 1: a NaN's sign and payload are the machine's
    far = int(((ulp_apart(d["parallax_deg"], e["parallax_deg"]) > 1) & ~both_nan).sum())
    if far:
        out.append(("parallax_deg", far))
    lst, inl = res.matches(pair)
    pts, tri = res.points(pair)
    same("list", lst, e["list"]); same("inlier", inl, e["inlier"]); same("points", pts, e["points"]); same("triangulated", tri, e["triangulated"])
    if stages:
        its = res.iterations_of(pair)
        for k in its:
            same(k, its[k], e[k])
        for h in range(8):
            hy = res.hypothesis(pair, h)
            same("hyp %d R" % h, hy["R"], e["hyp_R"][h]); same("hyp %d t" % h, hy["t"], e["hyp_t"][h])
            same("hyp %d points" % h, hy["points"], e["hyp_points"][h]); same("hyp %d verdict" % h, hy["verdict"], e["hyp_verdict"][h])
            if hy["n_good"] != int(e["n_good"][h]):
                out.append(("hyp %d n_good" % h, 4))
    return out

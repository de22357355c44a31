"""Scenes for the local-map point matching tests (tests/test_map_match_cpu.py, tests/test_gpu_map_match.py), in the dict forms of map_match_ref.py.

hand_scene(): the identity pose, one 640 x 480 frame, fx = fy = 500, cx = 320, cy = 240. With the identity pose Pc = P and PO = P exactly, so a point
(0, 0, z) has dist = z, projects to (320, 240) and its view_cos is n_z: every edge of L1 and L2 is reached with exact float32 values. The L4 cases are
`sites` 40 pixels apart (further than any window of the scene reaches): a point projecting onto the site and keypoints around it whose descriptors
lie at chosen distances from the point's. `where` names the table index of every case; the tests assert on the REFERENCE's output that each case
occurs before they compare anything with it.

random_scene(): two posed frames over one table with families of near-identical points (ratio refusals, claim chains), the job shapes of the issue
and an empty frame.  e2e_scene(): noise-free, distinct descriptors.

large_scene(), limit_scene(), many_jobs_scene(): real frame sizes, a frame at the declared limit of keypoints, 139 jobs in a call; SIZES names each
with the conditions that are asserted on the reference's results (profiles/local_mapping_shapes.md)."""
import numpy as np

import map_match_ref as R
import orb_match_ref as M

F = np.float32
BOUNDS = (0.0, 640.0, 0.0, 480.0)
K = (500.0, 500.0, 320.0, 240.0)


def scale_factors(n=8, s=1.2):
    sf = [F(1.0)]
    for _ in range(n - 1):
        sf.append(F(sf[-1] * F(s)))
    return np.array(sf, F)


SF = scale_factors()
IDENTITY = np.eye(3, 4, dtype=F)


def flip(d, bits):
    d = np.array(d, np.uint8).copy()
    for b in bits:
        d[b // 8] ^= np.uint8(1 << (b % 8))
    return d


def at_distance(base, d, rng):
    """a descriptor at Hamming distance d from base"""
    return flip(base, rng.choice(256, d, replace=False))


def up(x):
    return np.nextafter(F(x), F(np.inf))


def down(x):
    return np.nextafter(F(x), F(-np.inf))


class _Builder:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.xyz, self.normal, self.min_d, self.max_d, self.desc = [], [], [], [], []
        self.kxy, self.koct, self.kdesc = [], [], []
        self.where = {}

    def point(self, name, P, n, min_d, max_d, desc=None):
        self.where[name] = len(self.xyz)
        self.xyz.append(P); self.normal.append(n); self.min_d.append(min_d); self.max_d.append(max_d)
        self.desc.append(self.rng.integers(0, 256, 32).astype(np.uint8) if desc is None else desc)
        return len(self.xyz) - 1

    def keypoint(self, x, y, octave, desc):
        self.kxy.append((x, y)); self.koct.append(octave); self.kdesc.append(desc)
        return len(self.koct) - 1

    def site_point(self, name, site, level, desc=None, z=4.0, cos=0.9):
        """a point that projects onto the site (within rounding) at the given predicted level, view_cos about `cos` (below 0.998: r = 4)"""
        px, py = 40.0 + 40.0 * (site % 15), 40.0 + 40.0 * (site // 15)
        P = np.array([(px - K[2]) / K[0] * z, (py - K[3]) / K[1] * z, z])
        d = np.linalg.norm(P)
        return self.point(name, P, P / d * cos, 0.1, d * float(SF[level]) * 0.95, desc), (px, py)

    def cluster(self, name, site, level, kps, desc=None):
        """kps: (dx, dy, octave, distance from the point's descriptor) -> the keypoint indices"""
        p, (px, py) = self.site_point(name, site, level, desc)
        return p, [self.keypoint(px + dx, py + dy, o, at_distance(self.desc[p], d, self.rng)) for dx, dy, o, d in kps]


def hand_scene():
    b = _Builder(7)
    rng = b.rng
    kp = {}
    # ---- L4, one site each ----
    _, kp["lone"] = b.cluster("lone", 0, 0, [(1, 1, 0, 30)])
    _, kp["tie_same_level"] = b.cluster("tie_same_level", 1, 0, [(1, 0, 0, 20), (-1, 1, 0, 20)])
    _, kp["tie_zero"] = b.cluster("tie_zero", 2, 0, [(1, 0, 0, 0), (-1, 0, 0, 0)])
    _, kp["tie_other_level"] = b.cluster("tie_other_level", 3, 2, [(1, 0, 1, 20), (-1, 1, 2, 20)])
    _, kp["only_256"] = b.cluster("only_256", 4, 0, [(0, 1, 0, 256)])
    _, kp["at_th_high"] = b.cluster("at_th_high", 5, 0, [(1, 1, 0, 100)])
    _, kp["above_th_high"] = b.cluster("above_th_high", 6, 0, [(1, 1, 0, 101)])
    _, kp["ratio_pass"] = b.cluster("ratio_pass", 7, 0, [(1, 0, 0, 40), (0, 1, 0, 60)])
    _, kp["ratio_refuse"] = b.cluster("ratio_refuse", 8, 0, [(1, 0, 0, 50), (0, 1, 0, 60)])
    _, kp["level0"] = b.cluster("level0", 9, 0, [(1, 0, 1, 5), (0, 1, 0, 50)])                   # the range (-1, 0) leaves the octave-1 keypoint out
    _, kp["occupied"] = b.cluster("occupied", 10, 0, [(1, 0, 0, 10), (0, 1, 0, 40)])             # the first is occupied
    b.site_point("segment0", 11, 0)                                                              # nothing around it
    # the claim chain: three points on one site, two keypoints
    base = rng.integers(0, 256, 32).astype(np.uint8)
    pa, (px, py) = b.site_point("chain_a", 12, 0, base)
    b.site_point("chain_b", 12, 0, flip(base, range(200, 205)))
    b.site_point("chain_c", 12, 0, flip(base, range(210, 213)))
    kp["chain"] = [b.keypoint(px + 1, py, 0, flip(base, range(10))), b.keypoint(px, py + 1, 0, flip(base, range(30)))]
    # ---- segment lengths 63, 64, 65, 200 (1 and 0 are above): random descriptors, and two planted at 30 and 60 so that the winner is deep in the list ----
    for i, n in enumerate((63, 64, 65, 200)):
        p, (px, py) = b.site_point("segment%d" % n, 15 + i, 0)
        plant = {int(n * 0.9): 30, int(n * 0.45): 60}
        for k in range(n):
            d = at_distance(b.desc[p], plant[k], rng) if k in plant else rng.integers(0, 256, 32).astype(np.uint8)
            b.keypoint(px + rng.uniform(-3, 3), py + rng.uniform(-3, 3), 0, d)
    # ---- keypoints of every octave where the points (0, 0, z) project ----
    for o in range(8):
        b.keypoint(321.0 + 0.25 * o, 241.0, o, rng.integers(0, 256, 32).astype(np.uint8))
    # ---- L1 / L2 edges ----
    Z = (0.0, 0.0, 1.0)
    b.point("skipped", (0, 0, 4), Z, 0.1, 10)
    b.point("depth", (0, 0, -4), Z, 0.1, 10)
    b.point("z_plus_zero", (1, 1, 0.0), Z, 0.1, 10)
    b.point("z_minus_zero", (1, 1, -0.0), Z, 0.1, 10)                 # -0.0 only under the pose of the `negzero` job
    b.point("bounds", (10, 0, 5), Z, 0.1, 10)
    b.point("u_min_x", (-3.2, 0, 5), Z, 0.1, 10)
    b.point("u_max_x", (3.2, 0, 5), Z, 0.1, 10)
    near = F(F(0.8) * F(5.0))
    b.point("dist_at_min", (0, 0, near), Z, 5.0, 10)
    b.point("dist_below_min", (0, 0, down(near)), Z, 5.0, 10)
    far = F(F(1.2) * F(5.0))
    b.point("dist_at_max", (0, 0, far), Z, 0.1, 5.0)
    b.point("dist_above_max", (0, 0, up(far)), Z, 0.1, 5.0)
    b.point("cos_at_limit", (0, 0, 4), (0, 0, 0.5), 0.1, 10)
    b.point("cos_below_limit", (0, 0, 4), (0, 0, down(0.5)), 0.1, 10)
    b.point("cos_f0998", (0, 0, 4), (0, 0, F(0.998)), 0.1, 10)
    b.point("cos_below_f0998", (0, 0, 4), (0, 0, down(F(0.998))), 0.1, 10)
    b.point("ratio_at_sf3", (0, 0, 2), Z, 0.1, F(2.0) * SF[3])
    b.point("ratio_above_sf3", (0, 0, 2), Z, 0.1, F(2.0) * up(SF[3]))
    b.point("ratio_one", (0, 0, 2), Z, 0.1, 2.0)
    b.point("ratio_above_last", (0, 0, 2), Z, 0.1, F(2.0) * SF[7] * F(1.5))
    frame = M.make_frame(b.kxy, b.koct, np.zeros(len(b.koct)), b.kdesc, BOUNDS)
    table = R.make_table(b.xyz, b.normal, b.min_d, b.max_d, b.desc)
    P = len(b.xyz)
    skip = np.zeros(P, np.uint8); skip[b.where["skipped"]] = 1
    occ = np.zeros(len(b.koct), np.uint8); occ[kp["occupied"][0]] = 1
    negzero = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [-0.0, -0.0, 1, -0.0]], F)
    order = np.arange(P, dtype=np.int32)
    jobs = [R.make_job(0, IDENTITY, K, SF, 1.0, None, skip, occ),                               # 0: all P in order, th == 1
            R.make_job(0, IDENTITY, K, SF, 2.0, None, skip, occ),                               # 1: th != 1
            R.make_job(0, IDENTITY, K, SF, 1.0, order[::-1].copy(), skip[::-1].copy(), occ),    # 2: the list reversed
            R.make_job(0, negzero, K, SF, 1.0, [b.where["z_minus_zero"], b.where["lone"], b.where["z_plus_zero"]])]     # 3: PcZ == -0.0
    return {"frames": [frame], "table": table, "jobs": jobs, "where": b.where, "kp": kp}


def pose(rx, ry, rz, t):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    Rm = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    return np.concatenate([Rm, np.asarray(t, float).reshape(3, 1)], 1)


def _project(T, X):
    pc = X @ T[:, :3].T + T[:, 3]
    with np.errstate(all="ignore"):
        return np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1), pc[:, 2]


def random_scene(seed=5, n_families=100, n_kp=450):
    rng = np.random.default_rng(seed)
    poses = [pose(0.01, -0.02, 0.015, (0.05, -0.03, 0.1)), pose(-0.02, 0.03, -0.01, (-0.2, 0.05, 0.3))]
    # families of three near-identical points
    centre = np.stack([rng.uniform(-5, 5, n_families), rng.uniform(-3.5, 3.5, n_families), rng.uniform(-2, 14, n_families)], 1)
    base = rng.integers(0, 256, (n_families, 32)).astype(np.uint8)
    xyz, desc = [], []
    for c, d in zip(centre, base):
        for _ in range(3):
            xyz.append(c + rng.normal(0, 0.01, 3)); desc.append(at_distance(d, int(rng.integers(0, 16)), rng))
    xyz, desc = np.array(xyz), np.array(desc)
    P = len(xyz)
    d0 = np.linalg.norm(xyz, axis=1)
    normal = xyz / d0[:, None]
    odd = rng.uniform(size=P) < 0.15
    normal[odd] = rng.normal(size=(int(odd.sum()), 3))
    max_d = d0 * rng.uniform(0.7, 4.5, P)
    min_d = max_d / 1.2 ** 7
    table = R.make_table(xyz, normal, min_d, max_d, desc)
    frames, picks = [], []
    for T in poses:
        uv, z = _project(T, xyz)
        ok = np.flatnonzero((z > 0.1) & (uv[:, 0] > 5) & (uv[:, 0] < 635) & (uv[:, 1] > 5) & (uv[:, 1] < 475))
        pick = rng.choice(ok, min(len(ok), int(0.7 * n_kp)), replace=False)
        picks.append(pick)
        kxy = uv[pick] + rng.normal(0, 1.5, (len(pick), 2))
        lvl = np.clip(np.ceil(np.log(np.maximum(max_d[pick] / d0[pick], 1e-9)) / np.log(1.2)), 0, 7).astype(int)
        koct = np.clip(lvl - rng.integers(0, 2, len(pick)), 0, 7)
        kdesc = np.array([at_distance(desc[p], int(rng.integers(0, 110)), rng) for p in pick])
        n_extra = n_kp - len(pick)
        kxy = np.concatenate([kxy, np.stack([rng.uniform(0, 640, n_extra), rng.uniform(0, 480, n_extra)], 1)])
        koct = np.concatenate([koct, rng.integers(0, 8, n_extra)])
        kdesc = np.concatenate([kdesc, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        shuffle = rng.permutation(n_kp)
        frames.append(M.make_frame(kxy[shuffle], koct[shuffle], np.zeros(n_kp), kdesc[shuffle], BOUNDS))
    frames.append(M.make_frame(np.zeros((0, 2)), [], [], np.zeros((0, 32)), BOUNDS))                 # a frame with n == 0
    rest = rng.permutation(np.setdiff1d(np.arange(P), picks[1][:1]))[:256]
    sub = np.concatenate([picks[1][:1], rest]).astype(np.int32)              # 257 distinct points; the first has a keypoint in frame 1
    near1 = pose(-0.02, 0.03, -0.01, (-0.21, 0.05, 0.3))                    # frame 1 under a pose a little off its own
    jobs = [R.make_job(0, poses[0], K, SF, 1.0),                                                                        # 0: all P in order
            R.make_job(1, poses[1], K, SF, 3.0, sub, rng.uniform(size=257) < 0.1, rng.uniform(size=n_kp) < 0.1),        # 1: a subset, th != 1, skip, occupied
            R.make_job(1, poses[1], K, SF, 3.0, sub),                                                                   # 2: the same subset, nothing skipped or occupied
            R.make_job(1, poses[1], K, SF, 3.0, sub[rng.permutation(257)]),                                             # 3: job 2 permuted
            R.make_job(1, poses[0], K, SF[:5], 5.0, np.zeros(0, np.int32)),                                             # 4: n_points == 0
            R.make_job(1, poses[1], K, SF, 1.0, sub[:1]),                                                               # 5: 1
            R.make_job(0, poses[0], K, SF, 5.0, sub[:255]),                                                             # 6: 255, frame 0 again
            R.make_job(1, near1, K, SF[:3], 1.0, sub[1:257]),                                                           # 7: 256, another pose and a short scale table
            R.make_job(2, poses[0], K, SF, 1.0)]                                                                        # 8: the empty frame
    return {"frames": frames, "table": table, "jobs": jobs}


def large_scene(seed=5):
    """random_scene() at the caller's frame size: P = 2100 points (9 frustum blocks in job 0) over frames of 2100 = 65 * 32 + 20 keypoints, so that the
    last word of the claimed bitmap is partly in range. The last job is job 0 again with three keypoints in ten occupied (the subset jobs' occupied
    bytes happen to miss the last word)"""
    sc = random_scene(seed, 700, 2100)
    j0 = sc["jobs"][0]
    occ = np.random.default_rng(seed + 1).uniform(size=2100) < 0.3
    sc["jobs"].append(R.make_job(j0["frame"], j0["Tcw"], j0["K"], j0["scale_factors"], j0["th"], None, None, occ))
    return sc


N_LIMIT = 32768                              # IBA_ORB_MATCH_MAX_KEYPOINTS
LIMIT_PLANTED = (0, 8191, 8192) + tuple(range(N_LIMIT - 32, N_LIMIT))


def limit_scene(seed=3):
    """one frame of exactly N_LIMIT keypoints under the identity pose. Random positions and descriptors alone give no match (distances near 128), so
    the cases are planted: every keypoint of LIMIT_PLANTED (index 0, the two sides of 8192 and the whole last bitmap word) sits half a pixel from
    its own site (40 pixels apart) with its point's predicted level as octave and a descriptor 5 to 24 bits from its point's. `point_of_kp` names
    the table index of every planted keypoint's point. Two more points: `second` projects onto the site of keypoint N_LIMIT - 1 after that
    keypoint's own point (the claim is read back from the last word: nothing is left for it); keypoint `occupied_kp`, in the last word, is occupied
    in job 0 and free in job 1, and so is keypoint 8191."""
    b = _Builder(seed)
    rng = b.rng
    n = N_LIMIT
    kxy = np.stack([rng.uniform(5, 635, n), rng.uniform(5, 475, n)], 1)
    koct = rng.integers(0, 8, n)
    kdesc = rng.integers(0, 256, (n, 32)).astype(np.uint8)
    point_of_kp = {}
    for s, c in enumerate(LIMIT_PLANTED):
        level = s % 8
        p, (px, py) = b.site_point("kp%d" % c, s, level)
        kxy[c], koct[c], kdesc[c] = (px + 0.5, py + 0.25), level, at_distance(b.desc[p], 5 + s % 20, rng)
        point_of_kp[c] = p
    last = LIMIT_PLANTED.index(n - 1)
    b.site_point("second", last, last % 8, flip(b.desc[point_of_kp[n - 1]], range(3)))
    frame = M.make_frame(kxy, koct, np.zeros(n), kdesc, BOUNDS)
    table = R.make_table(b.xyz, b.normal, b.min_d, b.max_d, b.desc)
    occupied_kp = n - 18
    occ = np.zeros(n, np.uint8); occ[[8191, occupied_kp]] = 1
    occ[rng.choice(np.setdiff1d(np.arange(n), LIMIT_PLANTED), 500, replace=False)] = 1
    jobs = [R.make_job(0, IDENTITY, K, SF, 1.0, None, None, occ), R.make_job(0, IDENTITY, K, SF, 1.0)]
    return {"frames": [frame], "table": table, "jobs": jobs, "where": b.where, "point_of_kp": point_of_kp, "occupied_kp": occupied_kp}


MANY_LENGTHS = (0, 1, 255, 256, 257, None)     # None: points == NULL, the whole table


def many_jobs_scene(seed=21, n_jobs=139):
    """n_jobs jobs over the table and the three frames of random_scene() (frame 2 is empty): the frame cycles with j, the list length through
    MANY_LENGTHS every three jobs, three poses, th from three values, skip bytes on every fourth job and occupied bytes on every fifth. The first, the middle and the
    last job have 257, 256 and 255 points in frame 0"""
    base = random_scene()
    rng = np.random.default_rng(seed)
    P = len(base["table"]["min_dist"])
    poses = [pose(0.01, -0.02, 0.015, (0.05, -0.03, 0.1)), pose(-0.02, 0.03, -0.01, (-0.2, 0.05, 0.3)), pose(-0.02, 0.03, -0.01, (-0.21, 0.05, 0.3))]
    jobs = []
    for j in range(n_jobs):
        frame, L = j % 3, MANY_LENGTHS[(j // 3 + 4) % 6]
        T = poses[frame if (j // 18) % 3 != 2 else (j + 1) % 3]          # its frame's own pose, or the next frame's
        pts = None if L is None else rng.permutation(P)[:L].astype(np.int32)
        n, nk = P if L is None else L, len(base["frames"][frame]["octave"])
        skip = rng.uniform(size=n) < 0.1 if j % 4 == 1 else None
        occ = rng.uniform(size=nk) < 0.1 if j % 5 == 2 else None
        jobs.append(R.make_job(frame, T, K, SF, (1.0, 3.0, 5.0)[(j // 2) % 3], pts, skip, occ))
    return {"frames": base["frames"], "table": base["table"], "jobs": jobs}


# ---- the conditions of the three scenes above, asserted on the REFERENCE's results before anything is compared with them ----

def check_large(sc, refs):
    """2100 points and keypoints: 9 blocks of 256 slots in job 0, a partial last bitmap word that is claimed and that is seeded from `occupied`"""
    free, taken = refs[0], refs[9]
    assert free["n_points"] == 2100 == len(sc["frames"][0]["octave"]) and 2100 % 32 == 20 and -(-free["n_points"] // 256) == 9
    assert max(int(r["match"].max()) for r in refs if r["n_points"]) >= 2080 and free["match"].max() == 2099
    occ = sc["jobs"][9]["occupied"]
    assert sc["jobs"][0]["occupied"] is None and all(same_bytes(sc["jobs"][0][k], sc["jobs"][9][k]) for k in ("Tcw", "scale_factors")) and same_bytes(free["off"], taken["off"])
    # an occupied keypoint of the last word is the nearest candidate of a point: free, the point takes it; occupied, it does not
    high = [k for k in range(2100) if free["match"][k] >= 2080 and occ[free["match"][k]]]
    assert high and all(taken["match"][k] != free["match"][k] for k in high) and np.all(taken["point_of"][occ != 0] == -1)
    assert int(np.sum(taken["match"] >= 2080)) > 0 and taken["n_second_choice"] > 0


def check_limit(sc, refs):
    n = N_LIMIT
    w, pk, taken, free = sc["where"], sc["point_of_kp"], refs[0], refs[1]
    assert len(sc["frames"][0]["octave"]) == n and taken["n_candidates"] > 0
    assert taken["match"][pk[n - 1]] == n - 1 and taken["match"][pk[0]] == 0 and taken["match"][pk[8192]] == 8192 and taken["point_of"][n - 1] == pk[n - 1]
    # the claim of keypoint n - 1 is read back: the second point on its site finds it among its candidates and is refused
    a, b = taken["off"][w["second"]], taken["off"][w["second"] + 1]
    assert n - 1 in taken["index"][a:b] and taken["match"][w["second"]] == -1 and pk[n - 1] < w["second"]
    # occupied keypoints in the last word and below 8192 are refused to their points
    for c in (sc["occupied_kp"], 8191):
        assert sc["jobs"][0]["occupied"][c] and taken["match"][pk[c]] == -1 and free["match"][pk[c]] == c, c
    assert sc["occupied_kp"] >= n - 32 and all(free["match"][p] == c for c, p in pk.items()) and free["n_matches"] == len(pk) == taken["n_matches"] + 2


def check_many(sc, refs):
    assert len(refs) >= 130 and {r["n_points"] for r in refs} == {0, 1, 255, 256, 257, 300} and {j["frame"] for j in sc["jobs"]} == {0, 1, 2}
    assert len(sc["frames"][2]["octave"]) == 0 and len({j["Tcw"].tobytes() for j in sc["jobs"]}) >= 3
    assert sum(j["skip"] is not None for j in sc["jobs"]) > 10 and sum(j["occupied"] is not None for j in sc["jobs"]) > 10
    assert sum(r["n_matches"] > 0 for r in refs) > 40 and sum(r["n_second_choice"] for r in refs) > 0
    n = len(refs)
    assert [(sc["jobs"][j]["frame"], refs[j]["n_points"]) for j in (0, n // 2, n - 1)] == [(0, 257), (0, 256), (0, 255)] and all(refs[j]["n_matches"] > 0 for j in (0, n // 2, n - 1))


SIZES = {"large": (large_scene, check_large), "limit": (limit_scene, check_limit), "many": (many_jobs_scene, check_many)}      # scene -> (builder, conditions on the reference)


def e2e_scene(seed=11, P=200):
    """noise-free: keypoints are the float32 projections (by the rules' own arithmetic) of a part of the points, each with its point's descriptor and
    the octave the rules predict; random descriptors are distinct and far apart"""
    rng = np.random.default_rng(seed)
    T = pose(0.02, -0.01, 0.03, (0.1, -0.05, 0.2)).astype(F)
    xyz = np.stack([rng.uniform(-5, 5, P), rng.uniform(-3.5, 3.5, P), rng.uniform(4, 12, P)], 1).astype(F)
    d0 = np.linalg.norm(xyz, axis=1)
    table = R.make_table(xyz, xyz / d0[:, None], d0 / 4, d0 * rng.uniform(1.0, 3.0, P), rng.integers(0, 256, (P, 32)).astype(np.uint8))
    Tf = np.ascontiguousarray(T).reshape(-1)
    Ow = R.camera_centre(Tf)
    views = [R.frustum(Tf, Ow, tuple(F(v) for v in K), tuple(F(v) for v in BOUNDS), SF, 0.5, table["xyz"][p], table["normal"][p], table["min_dist"][p], table["max_dist"][p]) for p in range(P)]
    seen = [p for p in range(P) if views[p][0] == R.IN_VIEW and rng.uniform() < 0.8]
    order = rng.permutation(len(seen))
    point_of_kp = np.array(seen, np.int32)[order]
    frame = M.make_frame([(views[p][1], views[p][2]) for p in point_of_kp], [views[p][4] for p in point_of_kp], np.zeros(len(seen)), table["desc"][point_of_kp], BOUNDS)
    return {"frames": [frame], "table": table, "jobs": [R.make_job(0, T, K, SF, 1.0)], "point_of_kp": point_of_kp, "Tcw": T, "in_view": np.array([v[0] == R.IN_VIEW for v in views])}


# ---- a scene through the library, and the byte-for-byte comparison with the reference's results ----

def lib_args(mm, om, scene):
    """(frames, table, jobs) of the ctypes mirror (mm = the package's map_match, om = its orb_match)"""
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in scene["frames"]]
    t = scene["table"]
    table = mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"])
    jobs = [mm.job(j["frame"], j["Tcw"], j["K"], j["scale_factors"], j["th"], len(t["min_dist"]) if j["points"] is None else len(j["points"]), j["points"], j["skip"], j["occupied"])
            for j in scene["jobs"]]
    return frames, table, jobs


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def assert_equal(res, refs, keep_stages=True):
    """every output and kept stage of a MapMatches against the reference's list of results"""
    assert len(res) == len(refs)
    for j, ref in enumerate(refs):
        c = res.counts(j)
        assert c["n_points"] == ref["n_points"] and c["n_candidates"] == ref["n_candidates"] and c["n_matches"] == ref["n_matches"], (j, c, ref["n_candidates"], ref["n_matches"])
        assert same_bytes(c["status"], ref["counts"]), (j, c["status"], ref["counts"])
        got = res.read(j)
        for k in ("status", "u", "v", "view_cos", "level", "radius", "match", "dist"):
            assert same_bytes(got[k], ref[k]), (j, k, np.flatnonzero(got[k] != ref[k])[:8])
        assert same_bytes(res.keypoints(j), ref["point_of"]), (j, "point_of")
        if keep_stages:
            off, idx, d = res.lists(j)
            assert same_bytes(off, ref["off"]) and same_bytes(idx, ref["index"]) and same_bytes(d, ref["cdist"]), (j, "lists")


def check_end_to_end(mm, om, ps, host):
    """the new entry point (host: its host restatement) -> iba_map_match_pose_edges -> the pose optimisation, on e2e_scene(); ps = the package's pose"""
    sc = e2e_scene()
    ref = R.run(sc["frames"], sc["table"], sc["jobs"])[0]
    owner = sc["point_of_kp"]                                            # keypoint -> its point
    nk = len(owner)
    assert nk >= 100 and sc["in_view"][owner].all() and sc["in_view"].sum() > nk
    # every in-view point that has a keypoint claims exactly that keypoint, on the reference's output
    assert np.array_equal(ref["match"][owner], np.arange(nk)) and np.all(ref["dist"][owner] == 0) and ref["n_matches"] == nk
    fr, tb, jb = lib_args(mm, om, sc)
    m = mm.match_host(fr, tb, jb, keep_stages=1) if host else mm.match(fr, tb, jb, keep_stages=1)
    assert_equal(m, [ref])
    point_of = m.keypoints(0)
    m.close()
    f = sc["frames"][0]
    lv = (F(1.0) / (SF * SF)).astype(F)
    xyz, obs, w, idx = mm.pose_edges(None, point_of, None, len(sc["table"]["min_dist"]), sc["table"]["xyz"], f["xy"], f["octave"], lv)
    assert np.array_equal(idx, np.arange(nk)) and same_bytes(xyz, sc["table"]["xyz"][owner]) and same_bytes(obs, f["xy"])
    # from a pose a little off the true one the optimisation comes back to it: the observations are float32 roundings of exact projections
    # (below 1e-4 pixel at 640), so every edge is an inlier and the pose agrees to 1e-4
    start = np.array(sc["Tcw"], np.float64)
    start[:, 3] += (0.02, -0.015, 0.03)
    job = ps.job(start, xyz, obs, w, K)
    out = ps.optimize_host([job]) if host else ps.optimize([job])
    got = out.read(0)
    out.close()
    assert got["n"] == nk and got["n_inliers"] == nk, got
    assert np.max(np.abs(got["Tcw12"] - np.array(sc["Tcw"], np.float64))) < 1e-4, got["Tcw12"]

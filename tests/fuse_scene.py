"""Scenes for the map-point fusion tests (tests/test_fuse_cpu.py, tests/test_gpu_fuse.py), in the dict forms of fuse_ref.py.

hand_scene(): the identity pose, one 640 x 480 frame, fx = fy = 500, cx = 320, cy = 240, th = 3. With the identity pose Pc = P and PO = P exactly, so
a point (0, 0, z) has dist = z and dot = z n_z, and a point (x, 0, 1) projects to 500 x + 320: every edge of F2-F4 is reached with exact float32
values. The F5 cases are `sites` 40 pixels apart (further than any window of the scene reaches): a point projecting onto the site and keypoints around
it whose descriptors lie at chosen distances from the point's. `where` names the table index of every case; the tests assert on the REFERENCE's
output that each case occurs before they compare anything with it.

random_scene(): two posed frames over one table with families of near-identical points, slot counts that are no multiple of 64, a job with
n_points == 0, NULL entries, points == NULL and an empty frame.

map_scene(): 5 noise-free keyframes (4 = the current one) over landmarks whose table copies are deliberate duplicates held by different keyframes
with different observation counts; every keyframe sees every landmark, its keypoint being the float32 projection by the rules' own arithmetic with
the landmark's descriptor and the predicted octave. The landmark kinds: `single` (one copy, held by the current keyframe: ADD in every target),
`into_held` (the current copy dies into a copy with more observations: REPLACED_BY_HELD, then STALE_BAD), `equal` (equal counts: REPLACES_HELD, then
STALE_IN_KEYFRAME in the keyframe that just received the survivor), `chain` (c into a, then b against a in the second call) and, unless clean,
`twin` (the survivor already sits in one of the dying point's keyframes: that holder becomes -1) and `held_bad` (the picked keypoint holds a bad
point). clean = True leaves the last two out: after the recipe every keypoint that sees a landmark then holds its survivor, which neither an erased
twin nor a bad holder can. bit_noise flips up to that many descriptor bits per keypoint (profiles/fuse_parity.md: the descriptor deviation).

large_scene(), limit_scene(), many_jobs_scene(): real frame sizes, a frame at the declared limit of keypoints, 139 jobs in a call; SIZES names each
with the conditions that are asserted on the reference's results (profiles/local_mapping_shapes.md).

e2e_scene(): the chain from iba_triangulate; see there."""
import numpy as np

import fuse_ref as R
import map_match_scene as MS
import orb_match_ref as M

F = np.float32
BOUNDS, K, SF, IDENTITY = MS.BOUNDS, MS.K, MS.SF, MS.IDENTITY
LV = (F(1.0) / (SF * SF)).astype(F)          # mvInvLevelSigma2
TH = 3.0
flip, at_distance, up, down, pose, same_bytes = MS.flip, MS.at_distance, MS.up, MS.down, MS.pose, MS.same_bytes
SEGMENTS = (7, 8, 9, 15, 16, 17, 63, 64, 65, 200)


def hand_scene():
    b = MS._Builder(17)
    rng = b.rng
    kp = {}
    # ---- F5, one site each (radius 3 at level 0; the gate at octave 0 refuses e2 > 5.99) ----
    _, kp["lone"] = b.cluster("lone", 0, 0, [(1, 1, 0, 30)])
    _, kp["pick_50"] = b.cluster("pick_50", 1, 0, [(1, 1, 0, 50)])
    _, kp["pick_51"] = b.cluster("pick_51", 2, 0, [(1, 1, 0, 51)])
    _, kp["tie"] = b.cluster("tie", 3, 0, [(1, 0, 0, 20), (-1, 1, 0, 20)])
    _, kp["gated_winner"] = b.cluster("gated_winner", 4, 0, [(2.75, 0, 0, 5), (1, 0, 0, 40)])          # e2 = 7.5625 > 5.99: the candidate at 5 is refused
    _, kp["level0"] = b.cluster("level0", 5, 0, [(1, 0, 1, 5), (0, 1, 0, 45)])                         # levels (-1, 0) leave the octave-1 keypoint out
    _, kp["level_top"] = b.cluster("level_top", 6, 7, [(1, 0, 7, 30), (0, 1, 5, 3)])                   # levels (6, 7) leave the octave-5 keypoint out
    _, kp["only_256"] = b.cluster("only_256", 7, 0, [(0, 1, 0, 256)])
    b.site_point("no_candidate", 8, 0)                                                                 # nothing around it
    for i, n in enumerate(SEGMENTS):          # random descriptors, and two planted at 30 and 60 near the centre so that the winner is deep in the list and passes the gate
        p, (px, py) = b.site_point("segment%d" % n, 15 + i, 0)
        plant = {int(n * 0.9): 30, int(n * 0.45): 60}
        for k in range(n):
            d = at_distance(b.desc[p], plant[k], rng) if k in plant else rng.integers(0, 256, 32).astype(np.uint8)
            w = 1.0 if k in plant else 2.8
            b.keypoint(px + rng.uniform(-w, w), py + rng.uniform(-w, w), 0, d)
    for o in range(8):                        # keypoints of every octave where the points (0, 0, z) project
        b.keypoint(321.0 + 0.25 * o, 241.0, o, rng.integers(0, 256, 32).astype(np.uint8))
    # ---- F1-F4 edges ----
    Z = (0.0, 0.0, 1.0)
    b.point("skipped", (0, 0, 4), Z, 0.1, 10)
    b.point("depth", (0, 0, -4), Z, 0.1, 10)
    b.point("z_plus_zero", (1, 1, 0.0), Z, 0.1, 10)
    b.point("bounds", (10, 0, 5), Z, 0.1, 10)
    b.point("u_min_x", (-0.64, 0, 1), (-0.64, 0, 1), 0.1, 10)             # 500 * (float)0.64 rounds to 320: u == 0 and u == 640 exactly
    b.point("u_max_x", (0.64, 0, 1), (0.64, 0, 1), 0.1, 10)
    near = F(F(0.8) * F(5.0))
    b.point("dist_at_min", (0, 0, near), Z, 5.0, 10)
    b.point("dist_below_min", (0, 0, down(near)), Z, 5.0, 10)
    far = F(F(1.2) * F(5.0))
    b.point("dist_at_max", (0, 0, far), Z, 0.1, 5.0)
    b.point("dist_above_max", (0, 0, up(far)), Z, 0.1, 5.0)
    b.point("dot_at_limit", (0, 0, 4), (0, 0, 0.5), 0.1, 10)
    b.point("dot_below_limit", (0, 0, 4), (0, 0, down(0.5)), 0.1, 10)
    frame = M.make_frame(b.kxy, b.koct, np.zeros(len(b.koct)), b.kdesc, BOUNDS)
    table = R.make_table(b.xyz, b.normal, b.min_d, b.max_d, b.desc)
    P = len(b.xyz)
    skip = np.zeros(P, np.uint8); skip[b.where["skipped"]] = 1
    rev = np.concatenate([[-1], np.arange(P, dtype=np.int32)[::-1], [-7]]).astype(np.int32)            # the list reversed between two NULL entries
    jobs = [R.make_job(0, IDENTITY, K, SF, LV, TH, None, skip),                                        # 0: all P in order
            R.make_job(0, IDENTITY, K, SF, LV, TH, rev, np.concatenate([[0], skip[::-1], [0]])),       # 1
            R.make_job(0, IDENTITY, K, SF, LV, 5.0, None, skip)]                                       # 2: a wider window
    return {"frames": [frame], "table": table, "jobs": jobs, "where": b.where, "kp": kp}


def random_scene(seed=9, n_families=100, n_kp=300):
    rng = np.random.default_rng(seed)
    base = MS.random_scene(seed, n_families, n_kp)
    frames, table = base["frames"], base["table"]
    poses = [pose(0.01, -0.02, 0.015, (0.05, -0.03, 0.1)), pose(-0.02, 0.03, -0.01, (-0.2, 0.05, 0.3))]
    P = len(table["min_dist"])
    sub = rng.permutation(P)[:257].astype(np.int32)
    holes = sub.copy(); holes[rng.uniform(size=257) < 0.1] = -1
    near1 = pose(-0.02, 0.03, -0.01, (-0.21, 0.05, 0.3))
    jobs = [R.make_job(0, poses[0], K, SF, LV, TH),                                                    # 0: points == NULL: all P = 300 in order
            R.make_job(1, poses[1], K, SF, LV, TH, holes, rng.uniform(size=257) < 0.1),               # 1: 257 with NULL entries and skip bytes
            R.make_job(1, poses[1], K, SF, LV, 5.0, sub),                                              # 2: the same list, a wider window
            R.make_job(1, poses[0], K, SF, LV, TH, np.zeros(0, np.int32)),                             # 3: n_points == 0
            R.make_job(1, poses[1], K, SF, LV, TH, sub[:1]),                                           # 4: 1
            R.make_job(0, poses[0], K, SF, LV, 4.0, sub[:255]),                                        # 5: 255, frame 0 again
            R.make_job(1, near1, K, SF, LV, TH, np.concatenate([sub[1:130], sub[1:130]])),             # 6: 258 with every entry twice
            R.make_job(2, poses[0], K, SF, LV, TH)]                                                    # 7: the empty frame
    return {"frames": frames, "table": table, "jobs": jobs}


def large_scene(seed=9):
    """random_scene() at the caller's frame size: P = 2100 points (9 frustum and pick blocks in job 0) over frames of 2100 keypoints. Random depths
    give no NOT_FINITE, so the last job looks along z from exactly point 0's depth: PcZ == 0 for it"""
    sc = random_scene(seed, 700, 2100)
    T = IDENTITY.copy()
    T[2, 3] = -sc["table"]["xyz"][0, 2]
    sc["jobs"].append(R.make_job(0, T, K, SF, LV, TH, np.arange(300, dtype=np.int32)))
    return sc


def limit_scene():
    """the frame of exactly IBA_ORB_MATCH_MAX_KEYPOINTS keypoints and the table of map_match_scene.limit_scene(): every planted keypoint lies within
    a pixel of its point's projection and within 24 bits of its descriptor, so its point picks it; job 1 is the list reversed with a wider window"""
    base = MS.limit_scene()
    P = len(base["table"]["min_dist"])
    jobs = [R.make_job(0, IDENTITY, K, SF, LV, TH), R.make_job(0, IDENTITY, K, SF, LV, 5.0, np.arange(P, dtype=np.int32)[::-1].copy())]
    return {"frames": base["frames"], "table": base["table"], "jobs": jobs, "where": base["where"], "point_of_kp": base["point_of_kp"]}


def many_jobs_scene(seed=27, n_jobs=139):
    """n_jobs jobs over the table and the three frames of random_scene() (frame 2 is empty): the frame cycles with j, the list length through
    map_match_scene.MANY_LENGTHS every three jobs, three poses, th from three values, NULL entries and skip bytes on every fourth job. The
    first, the middle and the last job have 257, 256 and 255 points in frame 0"""
    base = random_scene()
    rng = np.random.default_rng(seed)
    P = len(base["table"]["min_dist"])
    poses = [pose(0.01, -0.02, 0.015, (0.05, -0.03, 0.1)), pose(-0.02, 0.03, -0.01, (-0.2, 0.05, 0.3)), pose(-0.02, 0.03, -0.01, (-0.21, 0.05, 0.3))]
    jobs = []
    for j in range(n_jobs):
        frame, L = j % 3, MS.MANY_LENGTHS[(j // 3 + 4) % 6]
        T = poses[frame if (j // 18) % 3 != 2 else (j + 1) % 3]          # its frame's own pose, or the next frame's
        pts = None if L is None else rng.permutation(P)[:L].astype(np.int32)
        skip = None
        if j % 4 == 1:
            skip = rng.uniform(size=P if L is None else L) < 0.1
            if pts is not None:
                pts[rng.uniform(size=L) < 0.1] = -1
        jobs.append(R.make_job(frame, T, K, SF, LV, (3.0, 4.0, 5.0)[(j // 2) % 3], pts, skip))
    return {"frames": base["frames"], "table": base["table"], "jobs": jobs}


# ---- the conditions of the three scenes above, asserted on the REFERENCE's results before anything is compared with them ----

def check_large(sc, refs):
    total = np.sum([r["counts"] for r in refs], 0)
    assert refs[0]["n_points"] == 2100 == len(sc["frames"][0]["octave"]) and -(-refs[0]["n_points"] // 256) == 9
    assert np.all(total > 0) and sum(r["n_gated_winner"] for r in refs) > 0, total
    assert max(int(r["match"].max()) for r in refs if r["n_points"]) >= 2080 and refs[-1]["status"][0] == R.NOT_FINITE


def check_limit(sc, refs):
    n = MS.N_LIMIT
    pk = sc["point_of_kp"]
    assert len(sc["frames"][0]["octave"]) == n and refs[0]["n_candidates"] > 0
    for c, p in pk.items():
        assert refs[0]["status"][p] == R.PICKED and refs[0]["match"][p] == c, (c, p)
    assert int(np.sum((refs[0]["status"] == R.PICKED) & (refs[0]["match"] >= n - 32))) >= 32 and refs[0]["match"][pk[n - 1]] == n - 1
    P = refs[0]["n_points"]
    assert refs[1]["match"][P - 1 - pk[n - 1]] == n - 1 and refs[1]["match"][P - 1 - pk[8192]] == 8192


def check_many(sc, refs):
    n = len(refs)
    assert n >= 130 and {r["n_points"] for r in refs} == {0, 1, 255, 256, 257, 300} and {j["frame"] for j in sc["jobs"]} == {0, 1, 2}
    assert len(sc["frames"][2]["octave"]) == 0 and len({j["Tcw"].tobytes() for j in sc["jobs"]}) >= 3 and sum(j["skip"] is not None for j in sc["jobs"]) > 10
    assert sum(r["n_picked"] > 0 for r in refs) > 40 and sum(r["n_gated_winner"] for r in refs) > 0
    assert [(sc["jobs"][j]["frame"], refs[j]["n_points"]) for j in (0, n // 2, n - 1)] == [(0, 257), (0, 256), (0, 255)] and all(refs[j]["n_picked"] > 0 for j in (0, n // 2, n - 1))


SIZES = {"large": (large_scene, check_large), "limit": (limit_scene, check_limit), "many": (many_jobs_scene, check_many)}      # scene -> (builder, conditions on the reference)


# ---- the map scene ----

KINDS = ("single", "into_held", "equal", "chain", "twin", "held_bad")
CURRENT, TARGETS = 4, (0, 1, 2, 3)


def map_scene(seed=23, per_kind=6, clean=False, n_extra=12, bit_noise=0):
    rng = np.random.default_rng(seed)
    poses = [pose(0.01 * k, -0.008 * k, 0.005 * k, (0.08 * k - 0.16, 0.03 * k, 0.02 * k)).astype(F) for k in range(5)]
    kinds = [kd for kd in KINDS if not (clean and kd in ("twin", "held_bad")) for _ in range(per_kind)]
    W = len(kinds)
    lm_xyz = np.stack([rng.uniform(-2, 2, W), rng.uniform(-1.5, 1.5, W), rng.uniform(5, 8, W)], 1).astype(F)
    d0 = np.linalg.norm(lm_xyz, axis=1)
    lm_normal, lm_min, lm_max = (lm_xyz / d0[:, None]).astype(F), (d0 / 4).astype(F), (d0 * rng.uniform(1.0, 3.0, W)).astype(F)
    lm_desc = rng.integers(0, 256, (W, 32)).astype(np.uint8)
    # the table: the copies of every landmark, and which keyframes hold which copy
    xyz, normal, mn, mx, desc, lm_of, held_in = [], [], [], [], [], [], []

    def copy(w, kfs):
        xyz.append(lm_xyz[w]); normal.append(lm_normal[w]); mn.append(lm_min[w]); mx.append(lm_max[w]); desc.append(lm_desc[w]); lm_of.append(w); held_in.append(tuple(kfs))
        return len(lm_of) - 1

    twin_of, bad = {}, []
    for w, kd in enumerate(kinds):
        if kd == "single":
            copy(w, [4])
        elif kd == "into_held":
            copy(w, [4]); copy(w, [0, 1, 2, 3])
        elif kd == "equal":
            copy(w, [4, 1]); copy(w, [0, 2])
        elif kd == "chain":
            copy(w, [4]); copy(w, [0, 1]); copy(w, [2, 3])
        elif kd == "twin":
            twin_of[w] = copy(w, [4]); copy(w, [0, 1, 2])                # the first copy also sits on the twin keypoint of keyframe 1
        elif kd == "held_bad":
            copy(w, [4]); bad.append(copy(w, [0]))
    order = rng.permutation(len(lm_of))                                   # the table in no particular order
    inv = np.argsort(order)
    table = R.make_table(np.array(xyz)[order], np.array(normal)[order], np.array(mn)[order], np.array(mx)[order], np.array(desc)[order])
    lm_of, held_in = np.array(lm_of, np.int32)[order], [held_in[i] for i in order]
    twin_of, bad = {w: int(inv[p]) for w, p in twin_of.items()}, [int(inv[p]) for p in bad]
    P = len(lm_of)
    # the keyframes: every landmark's float32 projection by the rules' own arithmetic, in a shuffled keypoint order, and unheld extras
    frames, kp_of, holders, kp_lm = [], [], [], []
    for k in range(5):
        T = np.ascontiguousarray(poses[k]).reshape(-1)
        Ow = R.camera_centre(T)
        views = [R.frustum(T, Ow, tuple(F(v) for v in K), BOUNDS, SF, 0.5, TH, lm_xyz[w], lm_normal[w], lm_min[w], lm_max[w]) for w in range(W)]
        assert all(v[0] == R.PICKED for v in views)
        kxy = [(v[1], v[2]) for v in views]; koct = [v[3] for v in views]; klm = list(range(W)); khold = [-1] * W
        kdesc = [at_distance(lm_desc[w], int(rng.integers(0, bit_noise + 1)), rng) if bit_noise else lm_desc[w] for w in range(W)]
        for p in range(P):
            if k in held_in[p]:
                khold[lm_of[p]] = p
        if k == 1:                                                        # the twin keypoints: a pixel away, 10 bits away, holding the current keyframe's copy
            for w, p in twin_of.items():
                kxy.append((views[w][1] + F(1.0), views[w][2])); koct.append(views[w][3]); kdesc.append(flip(lm_desc[w], range(10))); klm.append(-1); khold.append(p)
        for _ in range(n_extra):
            kxy.append((rng.uniform(5, 635), rng.uniform(5, 475))); koct.append(int(rng.integers(0, 8))); kdesc.append(rng.integers(0, 256, 32).astype(np.uint8)); klm.append(-1); khold.append(-1)
        sh = rng.permutation(len(klm))
        frames.append(M.make_frame(np.array(kxy, F)[sh], np.array(koct)[sh], np.zeros(len(sh)), np.array(kdesc)[sh], BOUNDS))
        kp_lm.append(np.array(klm, np.int32)[sh]); holders.append(np.array(khold, np.int32)[sh])
        kp_of.append({int(w): int(i) for i, w in enumerate(kp_lm[-1]) if w >= 0})
    m = R.make_map([len(h) for h in holders], P, np.concatenate(holders))
    m["bad"][bad] = 1
    m["found"][:] = rng.integers(0, 9, P); m["visible"][:] = m["found"] + rng.integers(0, 5, P)
    return {"frames": frames, "table": table, "poses": poses, "map": m, "kinds": kinds, "lm_of": lm_of, "kp_lm": kp_lm, "kp_of": kp_of, "n_landmarks": W, "twin_of": twin_of, "bad": bad}


def random_map(rng, K=4, n_kp=6, P=10):
    """a small random map for the randomised fold run, with a few bad points, and a made-up job (points, status, match) against keyframe 0"""
    holder = np.full(K * n_kp, -1, np.int32)
    for k in range(K):
        pts = rng.permutation(P)[:n_kp]
        sel = rng.uniform(size=n_kp) < 0.6
        holder[k * n_kp:(k + 1) * n_kp] = np.where(sel, pts, -1)
    m = R.make_map([n_kp] * K, P, holder)
    m["bad"][:] = rng.uniform(size=P) < 0.15
    m["found"][:] = rng.integers(0, 5, P); m["visible"][:] = rng.integers(0, 5, P)
    return m


# ---- a scene through the library, and the byte-for-byte comparison with the reference's results ----

def lib_args(fz, mm, om, scene):
    """(frames, table, jobs) of the ctypes mirrors (fz = the package's fuse, mm = its map_match, om = its orb_match)"""
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in scene["frames"]]
    t = scene["table"]
    table = mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"])
    jobs = [lib_job(fz, j, len(t["min_dist"])) for j in scene["jobs"]]
    return frames, table, jobs


def lib_job(fz, j, P):
    return fz.job(j["frame"], j["Tcw"], j["K"], j["scale_factors"], j["inv_level_sigma2"], j["th"], P if j["points"] is None else len(j["points"]), j["points"], j["skip"])


def assert_equal(res, refs, keep_stages=True):
    """every output and kept stage of a Fusion against the reference's list of results"""
    assert len(res) == len(refs)
    for j, ref in enumerate(refs):
        c = res.counts(j)
        assert c["n_points"] == ref["n_points"] and c["n_candidates"] == ref["n_candidates"] and c["n_picked"] == ref["n_picked"], (j, c, ref["n_candidates"], ref["n_picked"])
        assert same_bytes(c["status"], ref["counts"]), (j, c["status"], ref["counts"])
        got = res.read(j)
        for k in ("status", "u", "v", "level", "radius", "match", "dist"):
            assert same_bytes(got[k], ref[k]), (j, k, np.flatnonzero(got[k] != ref[k])[:8])
        if keep_stages:
            off, idx, d = res.lists(j)
            assert same_bytes(off, ref["off"]) and same_bytes(idx, ref["index"]) and same_bytes(d, ref["cdist"]), (j, "lists")


def same_results(a, b, n_jobs, keep_stages=True):
    """two Fusions byte for byte"""
    for j in range(n_jobs):
        ca, cb = a.counts(j), b.counts(j)
        assert all(np.array_equal(ca[k], cb[k]) for k in ca), (j, ca, cb)
        ra, rb = a.read(j), b.read(j)
        assert all(same_bytes(ra[k], rb[k]) for k in ra), j
        assert not keep_stages or all(same_bytes(x, y) for x, y in zip(a.lists(j), b.lists(j))), j


def assert_map_equal(fmap, world):
    w = world.arrays()
    for k in ("holder", "bad", "replaced_by", "found", "visible", "descriptor_stale"):
        assert same_bytes(getattr(fmap, k), w[k]), (k, np.flatnonzero(getattr(fmap, k) != w[k])[:8])


def recipe(fz, call, frames, table, sc, fmap, world=None, mode=R.LOCAL, **opts):
    """one SearchInNeighbors step through the library: `call` is fz.fuse or fz.fuse_host over (frames, table, jobs). One call with a job per target
    over holder[current], the folds in target order, iba_fuse_candidates, one call into the current keyframe, its fold. With a World the object
    restatement runs beside it on the library's picks and every op, other, n_fused and array is compared after every job.
    -> the list of (keyframe, op) per fold"""
    ops = []

    def step(keyframes, lists):
        skips = [fz.skip(fmap, k, pl) for k, pl in zip(keyframes, lists)]
        if world is not None:
            for k, pl, sk in zip(keyframes, lists, skips):
                assert same_bytes(sk, world.skip(k, pl))
        jobs = [fz.job(k, sc["poses"][k], K, SF, LV, TH, len(pl), pl, sk) for k, pl, sk in zip(keyframes, lists, skips)]
        res = call(frames, table, jobs, **opts)
        for j, k in enumerate(keyframes):
            got = res.read(j)
            op, other, nf = res.apply(j, k, fmap, mode)
            if world is not None:
                wop, wother, wnf = world.fold(k, lists[j], got["status"], got["match"], mode)
                assert same_bytes(op, wop) and same_bytes(other, wother) and nf == wnf, (k, op, wop)
                assert_map_equal(fmap, world)
            ops.append((k, op))
        res.close()

    mine = fmap.held(CURRENT).copy()                                   # vpMapPointMatches: a copy, NULL entries included
    step(list(TARGETS), [mine] * len(TARGETS))
    cands = fz.candidates(fmap, TARGETS)
    if world is not None:
        assert same_bytes(cands, world.candidates(TARGETS))
    step([CURRENT], [cands])
    return ops


def check_known_answer(sc, fmap):
    """on the clean map scene after the recipe: as many points that are not bad as landmarks, every keypoint that sees a landmark holds that
    landmark's survivor, and every replaced_by chain ends at a survivor"""
    alive = np.flatnonzero(fmap.bad == 0)
    assert len(alive) == sc["n_landmarks"] and sorted(sc["lm_of"][alive].tolist()) == list(range(sc["n_landmarks"]))
    survivor = {int(sc["lm_of"][p]): int(p) for p in alive}
    for k in range(5):
        held = fmap.held(k)
        for i, w in enumerate(sc["kp_lm"][k]):
            assert held[i] == (survivor[int(w)] if w >= 0 else -1), (k, i, int(w), int(held[i]))
    for p in range(fmap.P):
        q, hops = p, 0
        while fmap.bad[q]:
            q, hops = int(fmap.replaced_by[q]), hops + 1
            assert q >= 0 and hops <= fmap.P
        assert q == survivor[int(sc["lm_of"][p])]


def fuse_map(fz, m):
    return fz.FuseMap(m["kp_off"], m["holder"], m["P"], m["bad"], m["replaced_by"], m["found"], m["visible"])


# ---- the chain from iba_triangulate ----

def e2e_scene(seed=31, W=40, n_extra=10):
    """5 noise-free keyframes that move sideways (0.3 per step: enough parallax for the triangulation) over W landmarks which every keyframe sees.
    Every landmark has ONE table point. Half of them are `old`: held in keyframes 0-3, free in the current keyframe 4. The others are `fresh`: held
    in keyframes {0, 1, 2}, {1, 2} or {2} and free in 3 and 4, where iba_triangulate (current 4, neighbour 3) creates a second point for them. A
    landmark's max_dist puts max_dist / dist half a level away from the table entries in every keyframe, so its predicted level is one number n in
    all five and its keypoints have octave n. -> the scene, with the arguments of the triangulation"""
    rng = np.random.default_rng(seed)
    poses = [pose(0.004 * k, -0.006 * k, 0.003 * k, (0.3 * k - 0.6, 0.02 * k, 0.0)).astype(F) for k in range(5)]
    X = np.stack([rng.uniform(-2, 2, W), rng.uniform(-1.5, 1.5, W), rng.uniform(5, 8, W)], 1).astype(F)
    d0 = np.linalg.norm(X, axis=1)
    n_of = rng.integers(0, 7, W)
    mx = (d0 * 1.2 ** (n_of - 0.5)).astype(F)
    desc = rng.integers(0, 256, (W, 32)).astype(np.uint8)
    table = R.make_table(X, X / d0[:, None], mx / F(1.2 ** 7), mx, desc)
    held_sets = [(0, 1, 2, 3) if w % 2 == 0 else ((0, 1, 2), (1, 2), (2,))[(w // 2) % 3] for w in range(W)]
    frames, kp_lm, holders = [], [], []
    for k in range(5):
        T = np.ascontiguousarray(poses[k]).reshape(-1)
        Ow = R.camera_centre(T)
        views = [R.frustum(T, Ow, tuple(F(v) for v in K), BOUNDS, SF, 0.5, TH, X[w], table["normal"][w], table["min_dist"][w], table["max_dist"][w]) for w in range(W)]
        assert all(v[0] == R.PICKED and v[3] == n_of[w] for w, v in enumerate(views))
        kxy = [(v[1], v[2]) for v in views] + [(rng.uniform(5, 635), rng.uniform(5, 475)) for _ in range(n_extra)]
        koct = [v[3] for v in views] + [int(o) for o in rng.integers(0, 8, n_extra)]
        kdesc = np.concatenate([desc, rng.integers(0, 256, (n_extra, 32)).astype(np.uint8)])
        klm = np.concatenate([np.arange(W), np.full(n_extra, -1)]).astype(np.int32)
        sh = rng.permutation(W + n_extra)
        frames.append(M.make_frame(np.array(kxy, F)[sh], np.array(koct)[sh], np.zeros(len(sh)), kdesc[sh], BOUNDS))
        kp_lm.append(klm[sh])
        holders.append(np.array([w if (w >= 0 and k in held_sets[w]) else -1 for w in klm[sh]], np.int32))
    m = R.make_map([W + n_extra] * 5, W, np.concatenate(holders))
    return {"frames": frames, "table": table, "poses": poses, "map": m, "lm_of": np.arange(W, dtype=np.int32), "kp_lm": kp_lm, "n_landmarks": W,
            "fresh": [w for w in range(W) if w % 2], "node": [np.where(lm >= 0, lm % 8, -1).astype(np.int32) for lm in kp_lm]}


def check_end_to_end(fz, mm, om, tr, host):
    """iba_triangulate (host: its host restatement) on e2e_scene() -> the created points appended to the table that already holds those landmarks
    and entered into the holders of the two keyframes -> the recipe through iba_fuse (host: iba_debug_fuse_host) -> the known answer"""
    sc = e2e_scene()
    m, t, W = sc["map"], sc["table"], sc["n_landmarks"]
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in sc["frames"]]
    held = lambda k: m["holder"][m["kp_off"][k]:m["kp_off"][k + 1]]
    kfs = [tr.keyframe(k, sc["poses"][k], K, sc["node"][k], (held(k) >= 0).astype(np.uint8), 6.5) for k in range(5)]
    tjob = tr.job(CURRENT, [3], SF, (SF * SF).astype(F), 1.2)
    res = tr.triangulate_host(frames, kfs, [tjob]) if host else tr.triangulate(frames, kfs, [tjob])
    new = res.points(0)
    res.close()
    # every fresh landmark, and nothing else, got a second point between its two free keypoints
    lm_new = sc["kp_lm"][CURRENT][new["idx1"]]
    assert sorted(lm_new.tolist()) == sc["fresh"] and np.array_equal(sc["kp_lm"][3][new["idx2"]], lm_new) and np.all(new["neighbour"] == 0)
    assert np.max(np.abs(new["xyz"] - t["xyz"][lm_new])) < 1e-3 and same_bytes(new["desc"], t["desc"][lm_new])
    n_new = len(lm_new)
    cat = lambda key: np.concatenate([t[key], new[key]])
    table = mm.points(cat("xyz"), cat("normal"), cat("min_dist"), cat("max_dist"), cat("desc"))
    big = R.make_map(np.diff(m["kp_off"]), W + n_new, m["holder"])
    for i in range(n_new):
        big["holder"][big["kp_off"][CURRENT] + new["idx1"][i]] = W + i
        big["holder"][big["kp_off"][3] + new["idx2"][i]] = W + i
    full = dict(sc, map=big, lm_of=np.concatenate([sc["lm_of"], lm_new]).astype(np.int32))
    fmap, world = fuse_map(fz, big), R.World(big)
    ops = recipe(fz, fz.fuse_host if host else fz.fuse, frames, table, full, fmap, world)
    seen = set(np.concatenate([op for _, op in ops]).tolist())
    assert {R.OP_ADD, R.OP_REPLACED_BY_HELD, R.OP_REPLACES_HELD, R.OP_STALE_BAD, R.OP_STALE_IN_KEYFRAME} <= seen, seen
    assert int(np.sum(fmap.bad)) == n_new and int(np.sum(ops[4][1] == R.OP_ADD)) == W - n_new          # one copy of every fresh landmark died; the old ones were added to keyframe 4
    check_known_answer(full, fmap)

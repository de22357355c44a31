"""The scenes of the map-point refresh tests (tests/test_refresh_cpu.py, tests/test_gpu_refresh.py), as dicts of tests/refresh_ref.py, and the
comparison of a library result with the reference restatement's. hand_scene(): about 1100 tiny keyframes and points whose observation counts sit on
every boundary of the device's shapes, with the named cases in `where`. random_scene(): 300 points with geometric observation counts."""
import numpy as np

import map_match_scene as MS
import orb_match_ref as M
import refresh_ref as R

F = np.float32
SF, BOUNDS, pose, flip, at_distance, same_bytes = MS.SF, MS.BOUNDS, MS.pose, MS.flip, MS.at_distance, MS.same_bytes
COUNTS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 63, 64, 65, 255, 256, 257, 1024)
N_KEYFRAMES, N_BAD_KEYFRAMES = 1100, 10


class _Builder:
    """keyframes with free keypoints that points claim one by one, so that a point's observed descriptors are its own"""

    def __init__(self, seed, n_kf, n_bad):
        self.rng = rng = np.random.default_rng(seed)
        self.n_good = n_kf - n_bad
        self.n_kp = rng.integers(4, 13, n_kf)
        self.desc = [rng.integers(0, 256, (n, 32)).astype(np.uint8) for n in self.n_kp]
        self.octave = [rng.integers(0, 8, n).astype(np.int32) for n in self.n_kp]
        self.used = np.zeros(n_kf, np.int64)
        self.poses = [pose(*rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3)).astype(F) for _ in range(n_kf)]
        self.bad = np.arange(n_kf) >= self.n_good
        self.xyz, self.ref, self.point_bad, self.obs = [], [], [], []

    def claim(self, k, desc, octave=None):
        i = int(self.used[k])
        assert i < self.n_kp[k]
        self.used[k] += 1
        self.desc[k][i] = desc
        if octave is not None:
            self.octave[k][i] = octave
        return i

    def keyframes_for(self, n, bad=0):
        """n distinct keyframes with a free keypoint, `bad` of them bad ones, in a shuffled order"""
        good = np.flatnonzero((self.used < self.n_kp) & ~self.bad)
        ks = list(self.rng.choice(good, n - bad, replace=False)) + list(self.rng.choice(np.flatnonzero(self.bad & (self.used < self.n_kp)), bad, replace=False))
        return [int(k) for k in self.rng.permutation(ks)]

    def point(self, descs, kfs, ref=None, xyz=None, bad=False, ref_octave=None):
        """a point observed in kfs with the given descriptors; ref = the position of its reference keyframe in the list, or a keyframe index as (k,)"""
        rng = self.rng
        self.xyz.append(np.array([rng.uniform(-3, 3), rng.uniform(-2, 2), rng.uniform(4, 9)], F) if xyz is None else np.asarray(xyz, F))
        pos = int(rng.integers(0, len(kfs))) if (ref is None and len(kfs)) else ref
        obs = [(k, self.claim(k, d, ref_octave if j == pos else None)) for j, (k, d) in enumerate(zip(kfs, descs))]
        self.ref.append(pos[0] if isinstance(pos, tuple) else kfs[pos] if len(kfs) else 0)
        self.point_bad.append(bad)
        self.obs.append(obs)
        return len(self.obs) - 1

    def noisy(self, n):
        base = self.rng.integers(0, 256, 32).astype(np.uint8)
        return [at_distance(base, int(self.rng.integers(0, 60)), self.rng) for _ in range(n)]

    def scene(self, points=None):
        rng, P = self.rng, len(self.obs)
        frames = [M.make_frame(rng.uniform(5, 475, (n, 2)), self.octave[k], np.zeros(n), self.desc[k], BOUNDS) for k, n in enumerate(self.n_kp)]
        keyframes = [R.make_keyframe(k, self.poses[k], SF, self.bad[k]) for k in range(len(self.n_kp))]
        xyz = np.array(self.xyz, F).reshape(P, 3)
        stale = xyz / np.linalg.norm(xyz, axis=1, keepdims=True)
        table = R.make_table(xyz, stale, rng.uniform(0.5, 1.5, P), rng.uniform(10, 20, P), rng.integers(0, 256, (P, 32)))
        off = np.concatenate([[0], np.cumsum([len(o) for o in self.obs])]).astype(np.int32)
        flat = [e for o in self.obs for e in o]
        return {"frames": frames, "keyframes": keyframes, "table": table, "point_bad": np.array(self.point_bad, np.uint8), "ref_keyframe": np.array(self.ref, np.int32), "obs_off": off,
                "obs_keyframe": np.array([e[0] for e in flat], np.int32), "obs_keypoint": np.array([e[1] for e in flat], np.int32),
                "list": None if points is None else np.asarray(points, np.int32)}


def hand_scene():
    b = _Builder(41, N_KEYFRAMES, N_BAD_KEYFRAMES)
    rng, w = b.rng, {}
    for n in COUNTS:                                                      # (the 1090 good keyframes hold the 1024 of the last one)
        w["count%d" % n] = b.point(b.noisy(n), b.keyframes_for(n))
    A, C, D_, E = (rng.integers(0, 256, 32).astype(np.uint8) for _ in range(4))
    w["tie_first_last"] = b.point([A, C, D_, A], b.keyframes_for(4))      # rows 0 and 3 have the median 0
    w["tie_middle"] = b.point([C, A, A, D_, A, E], b.keyframes_for(6))    # rows 1, 2 and 4
    w["tie_all"] = b.point([A] * 9, b.keyframes_for(9))
    w["bad_across_bin"] = b.point(b.noisy(65), b.keyframes_for(65, bad=2))
    w["all_bad"] = b.point(b.noisy(3), b.keyframes_for(3, bad=3))
    w["bad_point"] = b.point(b.noisy(4), b.keyframes_for(4), bad=True)
    kfs = b.keyframes_for(5)
    w["no_ref"] = b.point(b.noisy(5), kfs, ref=(next(k for k in range(b.n_good) if k not in kfs),))
    kfs = b.keyframes_for(6)
    w["degenerate"] = b.point(b.noisy(6), kfs, xyz=R.camera_centre(np.ascontiguousarray(b.poses[kfs[4]]).reshape(-1)))
    w["ref_octave3"] = b.point(b.noisy(7), b.keyframes_for(7), ref=2, ref_octave=3)
    w["ref_last_level"] = b.point(b.noisy(7), b.keyframes_for(7), ref=6, ref_octave=7)
    w["ref_octave0"] = b.point(b.noisy(2), b.keyframes_for(2), ref=1, ref_octave=0)
    P = len(b.obs)
    sc = b.scene(list(range(P)) + [w["count17"], w["tie_middle"]])        # two duplicated entries at the end
    sc["where"] = w
    return sc


def random_scene(seed=77, P=300, n_kf=160, n_kp=12):
    rng = np.random.default_rng(seed)
    frames = [M.make_frame(rng.uniform(5, 475, (n_kp, 2)), rng.integers(0, 8, n_kp), np.zeros(n_kp), rng.integers(0, 256, (n_kp, 32)), BOUNDS) for _ in range(n_kf)]
    keyframes = [R.make_keyframe(k, pose(*rng.uniform(-0.3, 0.3, 3), rng.uniform(-2, 2, 3)), SF, rng.uniform() < 0.1) for k in range(n_kf)]
    counts = np.minimum(rng.geometric(0.12, P), 64)
    counts[rng.choice(P, 8, replace=False)] = rng.integers(65, 150, 8)    # the tail past one wave
    counts[rng.choice(P, 5, replace=False)] = 0
    obs_kf = [rng.choice(n_kf, n, replace=False) for n in counts]
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    xyz = np.stack([rng.uniform(-3, 3, P), rng.uniform(-2, 2, P), rng.uniform(4, 9, P)], 1).astype(F)
    table = R.make_table(xyz, xyz / np.linalg.norm(xyz, axis=1, keepdims=True), rng.uniform(0.5, 1.5, P), rng.uniform(10, 20, P), rng.integers(0, 256, (P, 32)))
    ref = np.array([int(rng.choice(k)) if len(k) and rng.uniform() < 0.95 else int(rng.integers(0, n_kf)) for k in obs_kf], np.int32)
    pts = rng.permutation(P)[:200]
    return {"frames": frames, "keyframes": keyframes, "table": table, "point_bad": (rng.uniform(size=P) < 0.05).astype(np.uint8), "ref_keyframe": ref, "obs_off": off,
            "obs_keyframe": np.concatenate(obs_kf).astype(np.int32), "obs_keypoint": rng.integers(0, n_kp, int(off[-1])).astype(np.int32),
            "list": np.concatenate([pts, pts[:7]]).astype(np.int32)}


def lib_args(rf, mm, om, sc):
    """the positional arguments of rf.refresh / rf.refresh_host (rf = the package's refresh, mm = its map_match, om = its orb_match) up to the list"""
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in sc["frames"]]
    kfs = [rf.keyframe(k["frame"], k["Tcw"], k["scale_factors"], k["bad"]) for k in sc["keyframes"]]
    t = sc["table"]
    return [frames, kfs, mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"]), sc["point_bad"], sc["ref_keyframe"], sc["obs_off"], sc["obs_keyframe"],
            sc["obs_keypoint"], sc["list"]]


OUTPUTS = ("status", "desc_state", "geo_state", "best_obs", "best_median", "n_desc", "normal", "min_dist", "max_dist", "desc")


def assert_equal(res, ref, keep_stages=True):
    """every output, count and kept stage of a Refreshed against the reference restatement's result"""
    got, c = res.read(), res.counts()
    assert len(res) == len(ref["point"])
    for key in OUTPUTS:
        assert same_bytes(got[key], ref[key]), (key, np.flatnonzero(np.any((got[key] != ref[key]).reshape(len(ref["point"]), -1), axis=1))[:8])
    for key in ("status", "desc_state", "geo_state"):
        assert same_bytes(c[key], ref["counts"][key]), (key, c[key], ref["counts"][key])
    assert c["n_points"] == ref["counts"]["n_points"] and c["n_desc_changed"] == ref["counts"]["n_desc_changed"]
    if keep_stages:
        off, med = res.medians()
        assert same_bytes(off, ref["med_off"]) and same_bytes(med, ref["median"]) and c["n_rows"] == len(ref["median"])


def check_triangulate_chain(rf, mm, om, tr, host):
    """iba_triangulate on the random scene of tests/triangulate_scene.py, then the refresh of every created point from its two observations listed
    current keyframe first: normal, min_dist, max_dist and desc must be R8's, that is iba_triangulation_points', byte for byte"""
    import triangulate_scene as TS
    sc = TS.random_scene()
    frames, tkfs, tjobs = TS.lib_args(tr, om, sc)
    res = tr.triangulate_host(frames, tkfs, tjobs) if host else tr.triangulate(frames, tkfs, tjobs)
    kfs = [rf.keyframe(k["frame"], k["Tcw"], TS.SF) for k in sc["keyframes"]]
    n_total = 0
    for j, job in enumerate(sc["jobs"]):
        new = res.points(j)
        n = len(new["idx1"])
        if not n:
            continue
        n_total += n
        other = np.asarray(job["neighbours"], np.int32)[new["neighbour"]]
        table = mm.points(new["xyz"], np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros((n, 32)))
        args = [frames, kfs, table, None, np.full(n, job["current"], np.int32), 2 * np.arange(n + 1), np.stack([np.full(n, job["current"]), other], 1).reshape(-1),
                np.stack([new["idx1"], new["idx2"]], 1).reshape(-1)]
        out = rf.refresh_host(*args) if host else rf.refresh(*args)
        got = out.read()
        out.close()
        assert np.all(got["status"] == R.REFRESHED) and np.all(got["geo_state"] == R.GEO_UPDATED) and np.all(got["best_obs"] == 0) and np.all(got["best_median"] == 0)
        for key in ("normal", "min_dist", "max_dist", "desc"):
            assert same_bytes(got[key], new[key]), (j, key)
    res.close()
    assert n_total > 100


def check_fuse_chain(rf, fz, mm, om, host):
    """iba_fuse and iba_fuse_apply (the recipe of tests/fuse_scene.py on its map scene), iba_refresh_observations, iba_refresh of the
    descriptor_stale survivors, iba_refresh_store: the table must equal the restatement's over the observations of the OBJECT restatement of the
    fold, and every descriptor_stale of a survivor must be cleared"""
    import fuse_ref as FR
    import fuse_scene as FS
    sc = FS.map_scene(bit_noise=30)
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in sc["frames"]]
    t = sc["table"]
    fmap, world = FS.fuse_map(fz, sc["map"]), FR.World(sc["map"])
    FS.recipe(fz, fz.fuse_host if host else fz.fuse, frames, mm.points(t["xyz"], t["normal"], t["min_dist"], t["max_dist"], t["desc"]), sc, fmap, world)
    off, okf, okp = rf.observations(fmap)
    # the same lists from the objects: a MapPoint's observation dict in keyframe order
    walked = [sorted((kf.id, idx) for kf, idx in mp.mObservations.items()) for mp in world.pts]
    assert [list(zip(okf[off[p]:off[p + 1]].tolist(), okp[off[p]:off[p + 1]].tolist())) for p in range(fmap.P)] == walked
    stale = np.flatnonzero((fmap.descriptor_stale != 0) & (fmap.bad == 0)).astype(np.int32)
    assert len(stale) >= 6
    ref_kf = np.array([o[-1][0] if o else 0 for o in walked], np.int32)
    rsc = {"frames": sc["frames"], "keyframes": [R.make_keyframe(k, sc["poses"][k], SF) for k in range(5)], "table": t, "point_bad": fmap.bad.copy(), "ref_keyframe": ref_kf, "obs_off": off,
           "obs_keyframe": okf, "obs_keypoint": okp, "list": stale}
    ref = R.run(rsc)
    assert np.all(ref["status"] == R.REFRESHED) and ref["counts"]["n_desc_changed"] > 0 and np.all(ref["n_desc"] >= 2)
    args = lib_args(rf, mm, om, rsc)
    out = rf.refresh_host(*args, keep_stages=1) if host else rf.refresh(*args, keep_stages=1)
    assert_equal(out, ref)
    normal, mn, mx, desc = t["normal"].copy(), t["min_dist"].copy(), t["max_dist"].copy(), t["desc"].copy()
    out.store(normal, mn, mx, desc, fmap.descriptor_stale)
    out.close()
    assert not fmap.descriptor_stale[fmap.bad == 0].any()
    rest = np.setdiff1d(np.arange(fmap.P), stale)
    assert same_bytes(normal[stale], ref["normal"]) and same_bytes(mn[stale], ref["min_dist"]) and same_bytes(mx[stale], ref["max_dist"]) and same_bytes(desc[stale], ref["desc"])
    assert same_bytes(normal[rest], t["normal"][rest]) and same_bytes(desc[rest], t["desc"][rest])


def same_results(a, b, keep_stages=True):
    """two Refreshed byte for byte (the device's and the host restatement's: all but counts.path)"""
    ra, rb, ca, cb = a.read(), b.read(), a.counts(), b.counts()
    for key in OUTPUTS:
        assert same_bytes(ra[key], rb[key]), key
    for key in ("n_points", "n_desc_changed", "n_rows"):
        assert ca[key] == cb[key], key
    for key in ("status", "desc_state", "geo_state"):
        assert same_bytes(ca[key], cb[key]), key
    if keep_stages:
        assert all(same_bytes(x, y) for x, y in zip(a.medians(), b.medians()))

"""Scenes for the new-map-point creation tests (tests/test_triangulate_cpu.py, tests/test_gpu_triangulate.py), in the dict forms of triangulate_ref.py.

hand_scene(): six keyframes of at most 200 keypoints, fx = fy = 512, cx = 320, cy = 240 (powers of two and short binary fractions, so that the
fundamental matrix of the pure translations is exact). Keyframe 0 is the current one at the identity pose. Keyframe 1 is translated along x: the
epipole in its image is not finite and gates nothing. Keyframe 2 is translated along z: the epipole is the principal point in both images, which
gives the epipole gate and a query with den == 0 (the keypoint AT the epipole of image 1). Keyframe 3 is a general pose. Keyframe 4 is too near
(PAIR_SKIPPED), keyframe 5 sits exactly at baseline / median_depth == 0.01f. Every case is a world point X with its own node id: the query is X's
projection into keyframe 0 and the candidates are keypoints of a neighbour at chosen places relative to X's epipolar line with descriptors at chosen
distances from the query's. `where` names the keypoint of keyframe 0 of every case and `cand` the neighbour keypoints; the tests assert on the
REFERENCE's output that each case occurs before they compare anything with it.

Three statuses cannot occur under the default options, whatever the scene; OPEN = (max_cos_parallax 2, chi2_line 100) reaches two of them.
DEGENERATE needs a fourth homogeneous coordinate of exactly zero, that is parallel rays, and those are PARALLAX first; `degenerate_open` is such a
pair, and it is DEGENERATE once max_cos_parallax is opened above 1. REPROJ2 needs a candidate further than sqrt(5.991) sigma from the reprojected
point while it is nearer than sqrt(3.84) sigma, of the same octave, to the query's epipolar line, and the triangulated point reprojects between
the two; `reproj2_open` lies 6 pixels off its line at octave 0 and is NO_MATCH, and REPROJ2 once chi2_line is opened. ZERO_DIST needs x3D == Ow_i
bit for bit, and then z_i = r_2 . (x3D - Ow_i) is zero and DEPTH1 / DEPTH2 come first (in the reference too: its dist == 0 test is a guard); the
stand-alone self-test reaches that line of the shared text with a hand-made centre.

random_scene(): seeded; points in front of a camera that moves, keypoints with pixel noise, descriptors with bit noise, nodes shared by families of
points, the job shapes of the issue. noise_free_scene(): the same with exact projections and exact descriptors, and the true point of every keypoint.

large_scene(), neighbours_scene(), tiny_scene(): frames of 1500 to 2100 keypoints, a job with eleven neighbours, 700 jobs of 1120 blocks; SIZES names
each with the conditions that are asserted on the reference's results (profiles/local_mapping_shapes.md)."""
import numpy as np

import orb_match_ref as M
import triangulate_ref as R
from map_match_scene import at_distance, pose, scale_factors

F = np.float32
K = (512.0, 512.0, 320.0, 240.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
SF = scale_factors()
SIGMA2 = (SF * SF).astype(F)
OPEN = dict(max_cos_parallax=2.0, chi2_line=100.0)
SEGMENTS = {2: (64, 65, 17, 16, 15, 1), 3: (130, 63)}          # neighbour keyframe -> the segment lengths it holds (0 is the node that occurs nowhere)


def project(T, X):
    T = np.asarray(T, F).astype(np.float64).reshape(3, 4)
    pc = T[:, :3] @ np.asarray(X, float) + T[:, 3]
    return np.array([K[0] * pc[0] / pc[2] + K[2], K[1] * pc[1] / pc[2] + K[3]])


class _Hand:
    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        ident = np.eye(3, 4)
        tr = lambda t: np.concatenate([np.eye(3), np.asarray(t, float).reshape(3, 1)], 1)
        self.T = [ident, tr((-0.5, 0, 0)), tr((0, 0, -0.5)), pose(0.01, -0.02, 0.005, (0.6, 0.05, 0.02)), tr((-0.01, 0, 0)), tr((-0.25, 0, 0))]
        self.T = [np.asarray(T, F) for T in self.T]
        self.median = [5.0, 5.0, 5.0, 5.0, 5.0, 25.0]
        self.kps = [[] for _ in self.T]                    # per keyframe: (x, y, octave, desc, node, has_point)
        self.where, self.cand = {}, {}
        self.next_node = 10

    def node(self):
        self.next_node += 10
        return self.next_node

    def kp(self, k, xy, desc, node, octave=0, has=0):
        self.kps[k].append((float(xy[0]), float(xy[1]), int(octave), np.asarray(desc, np.uint8), int(node), int(has)))
        return len(self.kps[k]) - 1

    def rand_desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def point(self, depth=(4.0, 8.0)):
        """a world point well inside every image and away from the principal point (the epipole of keyframe 2)"""
        z = self.rng.uniform(*depth)
        s = self.rng.choice([-1.0, 1.0], 2)
        return np.array([s[0] * self.rng.uniform(0.12, 0.3) * z, s[1] * self.rng.uniform(0.08, 0.2) * z, z])

    def on_line(self, k, X, s=1.0):
        """the projection into keyframe k of the point of ray 1 at s times X's depth: on X's epipolar line"""
        return project(self.T[k], np.asarray(X) * s)

    def off_line(self, k, X, px):
        p, q = self.on_line(k, X), self.on_line(k, X, 1.3)
        d = (q - p) / np.linalg.norm(q - p)
        return p + px * np.array([-d[1], d[0]])

    def query(self, name, X, node=None, octave=0, has=0, desc=None, xy=None):
        node = self.node() if node is None else node
        desc = self.rand_desc() if desc is None else desc
        self.where[name] = self.kp(0, project(self.T[0], X) if xy is None else xy, desc, node, octave, has)
        self.cand[name] = {}
        return desc, node

    def candidate(self, name, label, k, xy, desc, node, octave=0, has=0):
        self.cand[name][label] = (k, self.kp(k, xy, desc, node, octave, has))

    def segment(self, k, L):
        X = self.point()
        name = "segment%d" % L
        d, node = self.query(name, X)
        special = {}
        if L >= 15:
            special = {L // 3: ("off", self.off_line(k, X, 30.0), 20), L // 2: ("true", self.on_line(k, X), 30), L - 1: ("late", self.on_line(k, X, 1.15), 30)}
        else:
            special = {L - 1: ("late", self.on_line(k, X), 30)}
        for p in range(L):
            if p in special:
                label, xy, dist = special[p]
                self.candidate(name, label, k, xy, at_distance(d, dist, self.rng), node)
            else:
                self.candidate(name, "fill%d" % p, k, (self.rng.uniform(20, 620), self.rng.uniform(20, 460)), self.rand_desc(), node)

    def junk(self, k, node):
        """a keypoint of a neighbour in a node that keyframe 0 lacks"""
        self.kp(k, (self.rng.uniform(20, 620), self.rng.uniform(20, 460)), self.rand_desc(), node, int(self.rng.integers(0, 8)))

    def finish(self):
        """shuffle the keypoints of every keyframe, keeping the order inside a node, and rename `where` and `cand`"""
        frames, keyframes, new_index = [], [], []
        for k, kps in enumerate(self.kps):
            n = len(kps)
            assert n <= 200, (k, n)
            nodes = np.array([p[4] for p in kps], np.int64)
            place = self.rng.permutation(n)                # old index -> new index, before the order inside a node is restored
            for v in np.unique(nodes):
                members = np.flatnonzero(nodes == v)
                place[members] = np.sort(place[members])
            new_index.append(place)
            order = np.argsort(place)
            xy = np.array([(kps[i][0], kps[i][1]) for i in order], F).reshape(-1, 2)
            frames.append(M.make_frame(xy, [kps[i][2] for i in order], np.zeros(n), np.array([kps[i][3] for i in order], np.uint8).reshape(-1, 32), BOUNDS))
            keyframes.append(R.make_keyframe(k, self.T[k], K, [kps[i][4] for i in order], np.array([kps[i][5] for i in order], np.uint8), self.median[k]))
        where = {name: int(new_index[0][i]) for name, i in self.where.items()}
        cand = {name: {label: (k, int(new_index[k][i])) for label, (k, i) in c.items()} for name, c in self.cand.items()}
        return frames, keyframes, where, cand


def hand_scene(seed=7):
    h = _Hand(seed)
    rng = h.rng
    near = lambda d, bits: at_distance(d, bits, rng)
    # ---- keyframe 1 (x translation, position 0 of job 0) ----
    X = h.point(); d, n = h.query("lone", X); h.candidate("lone", "true", 1, h.on_line(1, X), near(d, 30), n)
    h.junk(1, n + 5)
    X = h.point(); d, n = h.query("tie", X)
    h.candidate("tie", "first", 1, h.on_line(1, X), near(d, 25), n); h.candidate("tie", "later", 1, h.on_line(1, X, 1.1), near(d, 25), n)
    X = h.point(); d, n = h.query("at_th_low", X); h.candidate("at_th_low", "true", 1, h.on_line(1, X), near(d, 50), n)
    X = h.point(); d, n = h.query("above_th_low", X); h.candidate("above_th_low", "true", 1, h.on_line(1, X), near(d, 51), n)
    h.junk(1, n + 5)
    X = h.point(); d, n = h.query("line_refused", X)
    h.candidate("line_refused", "better", 1, h.off_line(1, X, 30.0), near(d, 10), n); h.candidate("line_refused", "true", 1, h.on_line(1, X), near(d, 30), n)
    X = h.point(); d, n = h.query("same_idx2_a", X)
    h.query("same_idx2_b", X, node=n, desc=near(d, 4), xy=project(h.T[0], X) + (0.4, 0.0))
    h.candidate("same_idx2_a", "true", 1, h.on_line(1, X), near(d, 20), n)
    X = h.point(); d, n = h.query("has_query", X, has=1); h.candidate("has_query", "true", 1, h.on_line(1, X), near(d, 20), n)
    X = h.point(); d, n = h.query("has_candidate", X)
    h.candidate("has_candidate", "has", 1, h.on_line(1, X), near(d, 5), n, has=1); h.candidate("has_candidate", "free", 1, h.on_line(1, X, 1.1), near(d, 30), n)
    X = np.array([3.0, 2.0, 100.0]); d, n = h.query("parallax", X); h.candidate("parallax", "true", 1, h.on_line(1, X), near(d, 20), n)
    X = h.point(); d, n = h.query("depth1", X); h.candidate("depth1", "wrong_side", 1, project(h.T[0], X) + (20.0, 0.0), near(d, 20), n)
    X = h.point(); d, n = h.query("reproj1", X, octave=0); h.candidate("reproj1", "off6", 1, h.off_line(1, X, 6.0), near(d, 20), n, octave=7)
    X = h.point(); d, n = h.query("scale", X, octave=0); h.candidate("scale", "true", 1, h.on_line(1, X), near(d, 20), n, octave=5)
    X = h.point(); d, n = h.query("reproj2_open", X, octave=7); h.candidate("reproj2_open", "off6", 1, h.off_line(1, X, 6.0), near(d, 20), n, octave=0)
    d, n = h.query("degenerate_open", None, xy=(320.0, 240.0)); h.candidate("degenerate_open", "same_place", 1, (320.0, 240.0), near(d, 10), n)
    X = h.point(); d, n = h.query("twice", X)
    h.candidate("twice", "at0", 1, h.on_line(1, X), near(d, 20), n); h.candidate("twice", "at2", 3, h.on_line(3, X), near(d, 15), n)
    X = h.point(); d, n = h.query("refused_then_created", X)
    h.candidate("refused_then_created", "wrong_side", 1, project(h.T[0], X) + (20.0, 0.0), near(d, 20), n); h.candidate("refused_then_created", "true", 2, h.on_line(2, X), near(d, 20), n)
    X = h.point(); d, n = h.query("created_then_no_match", X)
    h.candidate("created_then_no_match", "true", 1, h.on_line(1, X), near(d, 20), n); h.candidate("created_then_no_match", "far", 2, h.on_line(2, X), near(d, 100), n)
    h.query("negative_node", h.point(), node=-1)
    h.kp(1, (100.0, 100.0), h.rand_desc(), -1)
    h.query("segment0", h.point())                                          # its node occurs nowhere
    # ---- keyframe 2 (z translation, position 1): the epipole is (320, 240) in both images ----
    X = h.point(); d, n = h.query("epipole_refused", X)
    p = h.on_line(2, X); u = (p - (320.0, 240.0)) / np.linalg.norm(p - (320.0, 240.0))
    h.candidate("epipole_refused", "better", 2, np.array([320.0, 240.0]) + 6.0 * u, near(d, 10), n); h.candidate("epipole_refused", "true", 2, p, near(d, 30), n)
    h.junk(1, n + 5)                                                        # keyframe 1 holds nodes between those keyframe 0 shares with keyframe 2 only
    d, n = h.query("den_zero", None, xy=(320.0, 240.0)); h.candidate("den_zero", "any", 2, (400.0, 300.0), near(d, 10), n)
    X = np.array([0.05, 0.02, 0.3]); d, n = h.query("depth2", X); h.candidate("depth2", "true", 2, h.on_line(2, X), near(d, 20), n)
    h.junk(2, n + 5); h.junk(1, n + 5)
    for k, lengths in SEGMENTS.items():
        for L in lengths:
            h.segment(k, L)
    h.junk(3, h.next_node + 5); h.junk(3, 15)
    # ---- keyframe 5 (position 4): exactly at the baseline ratio, so it is searched ----
    X = h.point(); d, n = h.query("at_ratio", X); h.candidate("at_ratio", "true", 5, h.on_line(5, X), near(d, 20), n)
    h.kp(4, (50.0, 50.0), h.rand_desc(), 20)                                # the skipped keyframe holds a node of keyframe 0 all the same
    frames, keyframes, where, cand = h.finish()
    jobs = [R.make_job(0, [1, 2, 3, 4, 5], SF, SIGMA2, 1.2), R.make_job(0, [3, 1], SF, SIGMA2, 1.2)]
    return {"frames": frames, "keyframes": keyframes, "jobs": jobs, "where": where, "cand": cand}


JOB_FORMS = ((4, [3, 2, 1, 0]),         # 0
             (2, []),                   # 1: no neighbours
             (3, [1, 5, 0]),            # 2: the empty frame as a neighbour; keyframe 1 is a neighbour here and in job 0
             (5, [0, 1]),               # 3: the empty frame as the current keyframe
             (0, [1]))                  # 4: one neighbour


def _moving_scene(seed, n_points, n_kp, pixel_noise, max_bit_noise, n_nodes, family_bits=None, crowd=None, jobs=None):
    """one keyframe per entry of n_kp along a path, then an empty one. A point's node is its index modulo n_nodes; crowd = (c, m) gives the first m
    points the nodes 0 .. c - 1 instead, so that those nodes hold long segments. jobs: (current, neighbours) pairs, by default the five job forms
    over the first five keyframes and the empty one"""
    rng = np.random.default_rng(seed)
    n_poses = len(n_kp)
    X = np.stack([rng.uniform(-4, 4, n_points), rng.uniform(-3, 3, n_points), rng.uniform(4, 12, n_points)], 1)
    base = rng.integers(0, 256, (n_points, 32)).astype(np.uint8)
    node_of = np.arange(n_points) % n_nodes
    if crowd is not None:
        node_of[:crowd[1]] = np.arange(crowd[1]) % crowd[0]
    if family_bits is not None:                            # the points of a node look alike: wrong candidates come below th_low and meet the gates
        family = rng.integers(0, 256, (n_nodes, 32)).astype(np.uint8)
        base = np.array([at_distance(family[node_of[p]], int(rng.integers(0, family_bits + 1)), rng) for p in range(n_points)], np.uint8)
    poses = [pose(0.004 * i, -0.01 * i, 0.003 * i, (-0.25 * i, 0.02 * i, -0.05 * i)).astype(F) for i in range(n_poses)]
    frames, keyframes, owner = [], [], []
    for i, T in enumerate(poses):
        pc = X @ T[:, :3].astype(float).T + T[:, 3].astype(float)
        uv = np.stack([K[0] * pc[:, 0] / pc[:, 2] + K[2], K[1] * pc[:, 1] / pc[:, 2] + K[3]], 1)
        ok = np.flatnonzero((uv[:, 0] > 5) & (uv[:, 0] < 635) & (uv[:, 1] > 5) & (uv[:, 1] < 475))
        pick = rng.permutation(ok)[:n_kp[i]]
        xy = uv[pick] + (rng.normal(0, pixel_noise, (len(pick), 2)) if pixel_noise else 0.0)
        octave = np.clip(np.round(np.log(pc[pick, 2] / 4.0) / np.log(1.2)), 0, 7).astype(int)
        octave = np.clip(octave + (rng.integers(-1, 2, len(pick)) if pixel_noise else 0), 0, 7)
        desc = np.array([at_distance(base[p], int(rng.integers(0, max_bit_noise + 1)), rng) for p in pick], np.uint8).reshape(-1, 32)
        node = node_of[pick].astype(np.int32)
        node[rng.uniform(size=len(pick)) < 0.03] = -1
        has = (rng.uniform(size=len(pick)) < 0.3).astype(np.uint8)
        frames.append(M.make_frame(xy, octave, np.zeros(len(pick)), desc, BOUNDS))
        depth = R.median_depth(T, X[pick[has != 0]].astype(F)) if has.any() else F(8.0)
        keyframes.append(R.make_keyframe(i, T, K, node, has, depth))
        owner.append(pick)
    frames.append(M.make_frame(np.zeros((0, 2)), [], [], np.zeros((0, 32)), BOUNDS))                 # a frame with n == 0
    keyframes.append(R.make_keyframe(n_poses, poses[2], K, [], None, 8.0))
    if jobs is None:
        jobs = JOB_FORMS
    jobs = [R.make_job(cur, nbs, SF, SIGMA2, 1.2) for cur, nbs in jobs]
    return {"frames": frames, "keyframes": keyframes, "jobs": jobs, "points": X.astype(F), "owner": owner}


def random_scene(seed=5):
    return _moving_scene(seed, 700, (301, 257, 333, 299, 315), 0.6, 30, 40, family_bits=24)


def noise_free_scene(seed=9):
    return _moving_scene(seed, 400, (200, 190, 210, 180, 205), 0.0, 0, 25)


def large_scene(seed=5):
    """random_scene() at the caller's frame sizes: 4000 points over 200 nodes. Spread evenly, a node would hold 20 points and no segment could pass
    20, so 320 of the points crowd into nodes 0 and 1: segments above 64, more than one trip at every pick width"""
    return _moving_scene(seed, 4000, (2001, 1500, 2100, 1999, 2048), 0.6, 30, 200, family_bits=24, crowd=(2, 320))


MANY_NEIGHBOURS = (6, [5, 7, 4, 8, 3, 9, 2, 10, 1, 11, 0])


def neighbours_scene(seed=13):
    """twelve keyframes of 500 keypoints, each a random part of 1200 points; one job: keyframe 6 against the other eleven, nearest first"""
    return _moving_scene(seed, 1200, (500,) * 12, 0.6, 30, 60, family_bits=24, jobs=[MANY_NEIGHBOURS])


def tiny_scene(seed=5, n_jobs=700):
    """n_jobs jobs cycling through the five job forms over keyframes of at most 11 keypoints: 8 blocks per cycle, so 700 jobs are 1120 blocks and
    trg_gather_kernel's scan of the per-block counts goes past its 1024 threads"""
    return _moving_scene(seed, 60, (9, 7, 11, 5, 8), 0.6, 30, 3, family_bits=24, jobs=[JOB_FORMS[j % 5] for j in range(n_jobs)])


def blocks_of(ref):
    """the blocks of a job: one per 256 keypoints of the current keyframe and neighbour"""
    return ref["n_neighbours"] * (-(-ref["n_keypoints"] // 256))


# ---- the conditions of the scenes above, asserted on the REFERENCE's results before anything is compared with them ----

def check_large(sc, refs):
    assert [r["n_keypoints"] for r in refs] == [2048, 2100, 1999, 0, 2001] and refs[0]["n_created"] > 300 and refs[2]["n_created"] > 300
    assert refs[0]["counts"][R.SUPERSEDED] > 0 and refs[2]["counts"][R.SUPERSEDED] > 0
    assert max(int(r["seg_len"].max()) for r in refs if r["seg_len"].size) > 64
    assert all(int(np.sum(sc["keyframes"][k]["node"] >= 0)) > 1024 for k in range(5)) and len(set(np.concatenate([k["node"] for k in sc["keyframes"]]).tolist())) == 201
    assert blocks_of(refs[0]) == 32 and sum(blocks_of(r) for r in refs) == 32 + 24 + 8


def check_neighbours(sc, refs):
    r = refs[0]
    assert len(refs) == 1 and r["n_keypoints"] == 500 and r["n_neighbours"] == 11
    assert (r["status"][5:] == R.SUPERSEDED).any() and (r["status"][5:] == R.CREATED).any() and r["n_created_of"][5:].sum() > 0 and not r["skipped"].any()


def check_tiny(sc, refs):
    first, total = np.cumsum([0] + [blocks_of(r) for r in refs]), sum(r["n_created"] for r in refs)
    assert len(refs) == 700 and first[-1] == 1120 and total == 280
    assert any(r["n_created"] > 0 for j, r in enumerate(refs) if first[j] >= 1024 and blocks_of(r))
    assert len({r["n_created"] for r in refs[:5]}) >= 2 and len({tuple(r["n_created_of"].tolist()) for r in refs[:5]}) == 5 and all(same_bytes(refs[j]["status"], refs[j % 5]["status"]) for j in range(5, 700))


SIZES = {"large": (large_scene, check_large), "neighbours": (neighbours_scene, check_neighbours), "tiny": (tiny_scene, check_tiny)}      # scene -> (builder, conditions on the reference)


# ---- a scene through the library, and the byte-for-byte comparison with the reference's results ----

def lib_args(tr, om, scene):
    """(frames, keyframes, jobs) of the ctypes mirror (tr = the package's triangulate, om = its orb_match)"""
    frames = [om.frame(f["xy"], f["octave"], f["angle"], f["desc"], f["bounds"]) for f in scene["frames"]]
    keyframes = [tr.keyframe(k["frame"], k["Tcw"], k["K"], k["node"], k["has_point"], k["median_depth"]) for k in scene["keyframes"]]
    jobs = [tr.job(j["current"], j["neighbours"], j["scale_factors"], j["level_sigma2"], j["scale_factor"]) for j in scene["jobs"]]
    return frames, keyframes, jobs


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def canon(x):
    """NaNs as the library stores them"""
    x = np.array(x, F, copy=True)
    x.view(np.uint32)[np.isnan(x)] = 0x7FC00000
    return x


def assert_equal(res, refs, keep_stages=True):
    """every output of a Triangulation against the reference's list of results"""
    assert len(res) == len(refs)
    for j, ref in enumerate(refs):
        c = res.counts(j)
        assert (c["n_keypoints"], c["n_neighbours"], c["n_created"]) == (ref["n_keypoints"], ref["n_neighbours"], ref["n_created"]), (j, c)
        assert same_bytes(c["status"], ref["counts"]), (j, c["status"], ref["counts"])
        assert same_bytes(c["n_matches"], ref["n_matches"]) and same_bytes(c["n_created_of"], ref["n_created_of"]), (j, c, ref["n_matches"], ref["n_created_of"])
        got = res.read(j)
        for k in ("status", "match", "dist"):
            assert same_bytes(got[k], ref[k]), (j, k, np.argwhere(got[k] != ref[k])[:8])
        assert same_bytes(canon(got["xyz"]), canon(ref["xyz"])), (j, "xyz", np.argwhere(got["xyz"] != ref["xyz"])[:8])
        pts = res.points(j)
        for k in ("idx1", "neighbour", "idx2", "desc"):
            assert same_bytes(pts[k], ref["points"][k]), (j, "points", k)
        for k in ("xyz", "normal", "min_dist", "max_dist"):
            assert same_bytes(canon(pts[k]), canon(ref["points"][k])), (j, "points", k)
        if keep_stages:
            assert same_bytes(res.segments(j), ref["seg_len"]), (j, "seg_len")


def same_results(a, b, n_jobs, keep_stages=True):
    """two Triangulations byte for byte"""
    for j in range(n_jobs):
        ca, cb = a.counts(j), b.counts(j)
        assert all(np.array_equal(ca[k], cb[k]) for k in ca), (j, ca, cb)
        ra, rb = a.read(j), b.read(j)
        assert all(same_bytes(canon(ra[k]) if ra[k].dtype == F else ra[k], canon(rb[k]) if rb[k].dtype == F else rb[k]) for k in ra), j
        pa, pb = a.points(j), b.points(j)
        assert all(same_bytes(canon(pa[k]) if pa[k].dtype == F else pa[k], canon(pb[k]) if pb[k].dtype == F else pb[k]) for k in pa), j
        if keep_stages:
            assert same_bytes(a.segments(j), b.segments(j)), j

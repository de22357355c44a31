"""GPU tier of the Scan Context entry points, each test through the C ABI (iba_sc_describe / iba_sc_db_read / iba_sc_distance / iba_sc_detect,
include/iba_mi355x.h): descriptors, ring keys (double and float), sector keys and skipped counts byte for byte against tests/sc_ref.py; distances,
shifts, candidates, loop nodes and yaw byte for byte on a trajectory that revisits its start; the same bytes twice and whatever the batch; the
detected loop through iba_submap_build and iba_scan_register; the edges of the domain with their messages. Figures are printed before they are
asserted; with IBA_SC_PARITY_OUT=<file> they are also appended there as JSON lines (profiles/sc_parity.md quotes such a run). Inputs and seeds
were chosen on the CPU from the restatement alone.

The lattice scan sits on ring and sector boundaries on purpose. Its rings are exact by the rules (IEEE sqrt, / and *), and so is the sector of a
point with y == +-0, x > 0 and of the origin column; a point on another sector boundary may fall to either side of it with a correct f64 atan2, so
the two bins it can reach are left out of the lattice comparison (and the lattice's keys, which sum them, with them). Everything else of the lattice
descriptor is compared."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import sc_ref as SC
import submap_ref as V

pytestmark = pytest.mark.gpu
I4 = np.eye(4)


def _note(**kw):
    print("sc-figures", json.dumps(kw))
    p = os.environ.get("IBA_SC_PARITY_OUT")
    if p:
        with open(p, "a") as f:
            f.write(json.dumps(kw) + "\n")


def _handle(pkg, abi, scans, plane_cache=0):
    return pkg.IbaHandle(abi.Problem.from_scans([np.asarray(t, np.float32).reshape(-1, 3) for t in scans]), abi.reference_yaml_params(plane_cache))


def _raises(pkg, call, status, word):
    with pytest.raises(pkg.IbaError) as ex:
        call()
    assert ex.value.status == status and word in str(ex.value), (status, word, ex.value.status, str(ex.value))


def _opt(pkg, o):
    return pkg.sc_options(**{k: v for k, v in o.items()})


_cache = {}


def lattice_scan():
    """points on ring boundaries (range a multiple of max_radius / num_ring = 4, by Pythagorean triples too), on sector boundaries (multiples of 6 degrees), on
    the +x axis with y = +0 and y = -0, on the origin column, at range exactly 80 and one float above, and inside by the xy range but outside by the 3-D norm"""
    pts = []
    for k in range(1, 21):
        pts += [(4.0 * k, 0.0, 0.25 * k), (4.0 * k, -0.0, -0.5 * k), (2.4 * k, 0.0, 3.2 * k), (0.0, 4.0 * k, 0.1 * k), (-4.0 * k, 0.0, 0.2 * k), (0.0, -4.0 * k, 0.3 * k)]
        for a in range(0, 360, 6):
            t = np.deg2rad(a)
            pts.append((3.7 * k * np.cos(t), 3.7 * k * np.sin(t), 0.01 * a - 1.0))
    pts += [(0.0, 0.0, 1.5), (0.0, 0.0, -2.0), (-0.0, 0.0, 2.5), (80.0, 0.0, 0.0), (np.nextafter(np.float32(80.0), np.float32(100.0)), 0.0, 7.0), (79.0, 0.0, 20.0), (0.0, 79.0, -20.0),
            (10.0, 10.0, -1000.0), (10.0, -10.0, -1000.5), (30.0, 0.0, -1000.0), (12.0, 5.0, -999.5)]      # (the last four: inside max_radius only in the 1500 m shape)
    return np.asarray(pts, np.float32)


def lattice_mask(scan, opt):
    """[R, S] True where the lattice descriptor is exact by the rules: every bin that a point on an inexact sector boundary could reach is False"""
    R, S = opt["num_ring"], opt["num_sector"]
    ring, sec, enters, a = SC.bins(scan, opt)
    near = (np.abs(a["sector_arg"] - np.round(a["sector_arg"])) <= 1e-9) & ~a["exact_angle"]
    ok = np.ones((R, S), bool)
    for r, sa in zip(ring[near], np.round(a["sector_arg"][near]).astype(int)):
        for s in (sa - 1, sa):
            ok[r, min(max(s, 0), S - 1)] = False
    return ok


def _scene(synth):
    """50 make_scene scans + a scan with NaN / Inf points, an empty scan, a scan stretched past max_radius, the lattice"""
    if "scene" not in _cache:
        prob, _ = synth.make_scene(n_frames=50, pts_per_frame=4000, n_keypoints=50, seed=5)
        scans = [prob.frame_points(f).copy() for f in range(50)]
        rng = np.random.default_rng(17)
        bad = scans[3].copy()
        hit = rng.choice(len(bad), 90, replace=False)
        bad[hit[:30], rng.integers(0, 3, 30)] = np.nan
        bad[hit[30:60], rng.integers(0, 3, 30)] = np.inf
        bad[hit[60:], rng.integers(0, 3, 30)] = -np.inf
        far = (scans[4].astype(np.float64) * 3.0).astype(np.float32)
        big = np.concatenate([scans[f] for f in range(10, 14)])       # 16000 points: four slices of the bins kernel merge into one node
        scans += [bad, np.zeros((0, 3), np.float32), far, big, lattice_scan()]
        _cache["scene"] = (scans, dict(bad=50, empty=51, far=52, big=53, lattice=54))
    return _cache["scene"]


def _same_db(dev, ref, nodes, what):
    for name in ("desc", "ring", "ring_f", "sector", "skipped"):
        d, r = dev[name][nodes], ref[name][nodes]
        assert d.dtype == r.dtype, (what, name, d.dtype, r.dtype)
        if d.tobytes() != r.tobytes():
            bad = np.flatnonzero(np.any((d != r).reshape(len(nodes), -1) | (np.isnan(d) != np.isnan(r)).reshape(len(nodes), -1), axis=1))
            raise AssertionError((what, name, "nodes that differ", [int(nodes[b]) for b in bad[:8]]))


SHAPES = (dict(), dict(num_ring=64, num_sector=256, max_radius=60.0, lidar_height=2.0, search_ratio=0.05),
          dict(num_ring=5, num_sector=7, max_radius=35.5, lidar_height=1.73, search_ratio=1.0), dict(num_ring=1, num_sector=1), dict(num_ring=33, num_sector=100, search_ratio=0.3, lidar_height=-0.25), dict(num_ring=30, max_radius=1500.0))


def test_descriptors_and_keys_equal_the_restatement_byte_for_byte(pkg, abi, synth):
    scans, ids = _scene(synth)
    h = _handle(pkg, abi, scans)
    frames = list(range(len(scans))) + [3, 3, ids["empty"]]            # a frame may repeat
    plain = [i for i in range(len(frames)) if frames[i] != ids["lattice"]]
    for shape in SHAPES:
        o = SC.options(**shape)
        nd = int(sum(int(SC.non_decisive(scans[f], o).sum()) for f in range(len(scans)) if f != ids["lattice"]))
        ref = SC.describe([scans[f] for f in frames], o)
        db = h.sc_describe(frames, **shape)
        dev = db.read()
        db.close()
        db2 = h.sc_describe(frames, **shape)
        again = db2.read(); part = db2.read(5, 3)
        db2.close()
        mask = lattice_mask(scans[ids["lattice"]], o)
        entered = int(SC.bins(scans[ids["far"]], o)[2].sum())
        _note(test="describe", shape=shape, nodes=len(frames), non_decisive=nd, skipped=int(ref["skipped"].sum()), far_entered=entered, far_points=len(scans[ids["far"]]),
              lattice_bins_compared=int(mask.sum()), lattice_bins=int(mask.size), nonzero_bins=int((ref["desc"] != 0).sum()))
        assert nd == 0, nd                                            # the decisive-point condition on the random scenes, from the CPU alone
        assert len(dev["desc"]) == len(frames)
        _same_db(dev, ref, np.asarray(plain), "shape %r" % (shape,))
        for name in dev:
            assert dev[name].tobytes() == again[name].tobytes(), ("second call", name)
            assert part[name].tobytes() == dev[name][5:8].tobytes(), ("partial read", name)
        L = ids["lattice"]
        assert mask.sum() > 0.5 * mask.size or o["num_sector"] < 8
        assert dev["desc"][L][mask].tobytes() == ref["desc"][L][mask].tobytes(), "lattice bins that are exact by the rules"
        assert dev["skipped"][L] == 0
        assert dev["skipped"][ids["bad"]] == 90 and dev["skipped"][ids["empty"]] == 0 and not dev["desc"][ids["empty"]].any()
        if not shape:
            assert 0 < entered < len(scans[ids["far"]])                # the stretched scan really has points on both sides of max_radius
    h.close()


def test_distances_of_other_shapes_equal_the_restatement(pkg, abi, synth):
    scans, ids = _scene(synth)
    h = _handle(pkg, abi, scans)
    frames = list(range(0, 50, 3)) + [ids["bad"], ids["empty"], ids["far"]]
    rng = np.random.default_rng(29)
    pairs = np.stack([rng.integers(0, len(frames), 40), rng.integers(0, len(frames), 40)], 1).astype(np.int32)
    pairs[:3] = [[0, 0], [len(frames) - 2, 1], [2, len(frames) - 2]]    # a node with itself; the empty scan on either side (NaN: no winner)
    for shape in SHAPES:
        o = SC.options(**shape)
        ref = SC.describe([scans[f] for f in frames], o)
        rd, rs = SC.distances(ref["desc"], pairs, o)
        db = h.sc_describe(frames, **shape)
        dd, ds = db.distance(pairs)
        dd2, ds2 = db.distance(pairs[::-1].copy())
        db.close()
        _note(test="distance-shapes", shape=shape, pairs=len(pairs), radius=SC.search_radius(o), min=float(rd.min()), max_below_no_winner=float(rd[rd < SC.NO_WINNER].max()), no_winner=int((rd == SC.NO_WINNER).sum()))
        assert dd.tobytes() == rd.tobytes() and ds.tobytes() == rs.tobytes(), (shape, np.flatnonzero((dd != rd) | (ds != rs)).tolist())
        assert dd2[::-1].tobytes() == rd.tobytes() and ds2[::-1].tobytes() == rs.tobytes()
        assert rd[1] == SC.NO_WINNER and rs[1] == 0 and rd[2] == SC.NO_WINNER
    h.close()


# ---- a trajectory that revisits its start ----
CITY = dict(seed=11, first=62, again=12, pts=4000, step=2.0, yaw_sectors=5, boxes=400, lidar_height=2.0)


def city(synth):
    """A world of random boxes on a ground plane seen by a 360-degree, 32-ring scanner (synth's ray caster). Pass one: `first` poses 2 m apart along x.
    Pass two revisits the first `again` of them, each up to 0.2 m off and turned by yaw_sectors x 6 degrees (+- 0.01 rad): planted loops with a planted
    column shift. -> (scans, poses 4x4 scan -> world)"""
    if "city" not in _cache:
        c = CITY
        rng = np.random.default_rng(c["seed"])
        nb, gz = c["boxes"], -1.73
        bx = rng.uniform(-40, c["step"] * c["first"] + 40, nb); by = rng.uniform(4, 45, nb) * rng.choice([-1.0, 1.0], nb)
        bh = rng.uniform(0.5, 6.0, nb); bs = rng.uniform(0.5, 3.0, (nb, 2))
        boxes = [(np.array([bx[i] - bs[i, 0], by[i] - bs[i, 1], gz]), np.array([bx[i] + bs[i, 0], by[i] + bs[i, 1], gz + bh[i]])) for i in range(nb)]
        elev = np.deg2rad(np.linspace(-24.8, 8.0, 32))
        where = [(np.array([c["step"] * f, 0.0, 0.0]), rng.uniform(-0.02, 0.02)) for f in range(c["first"])]
        where += [(np.array([c["step"] * f + rng.uniform(-0.2, 0.2), rng.uniform(-0.2, 0.2), 0.0]), np.deg2rad(6.0 * c["yaw_sectors"]) + rng.uniform(-0.01, 0.01)) for f in range(c["again"])]
        scans, poses = [], []
        for o, yaw in where:
            az = np.deg2rad(np.linspace(-180, 180, 360, endpoint=False) + rng.uniform(0, 1))
            E, A = np.meshgrid(elev, az, indexing="ij")
            dl = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
            cs, sn = np.cos(yaw), np.sin(yaw)
            Rm = np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]])
            near = [b for b in boxes if abs(0.5 * (b[0][0] + b[1][0]) - o[0]) < 85]
            t = synth._raycast(o, dl @ Rm.T, gz, (), near, 80.0)
            ok = np.flatnonzero(np.isfinite(t))
            sel = np.sort(rng.choice(ok, min(c["pts"], ok.size), replace=False))
            scans.append((dl[sel] * (t[sel] + rng.normal(0, 0.02, len(sel)))[:, None]).astype(np.float32))
            M = np.eye(4); M[:3, :3] = Rm; M[:3, 3] = o
            poses.append(M)
        _cache["city"] = (scans, np.array(poses))
    return _cache["city"]


def _result_bytes(r, k):
    return (np.array([r.loop_node, r.shift, r.n_candidates], np.int32).tobytes() + np.float64(r.min_dist).tobytes() + np.float32(r.yaw_rad).tobytes() +
            np.array(r.cand_node[:], np.int32).tobytes() + np.array(r.cand_shift[:], np.int32).tobytes() + np.array(r.cand_dist[:], np.float64).tobytes())


def _ref_bytes(r, k):
    cn = np.full(16, -1, np.int32); cs = np.full(16, -1, np.int32); cd = np.full(16, np.nan)
    cn[:k], cs[:k], cd[:k] = r["cand_node"], r["cand_shift"], r["cand_dist"]
    return (np.array([r["loop_node"], r["shift"], int((r["cand_node"] >= 0).sum())], np.int32).tobytes() + np.float64(r["min_dist"]).tobytes() + np.float32(r["yaw_rad"]).tobytes() +
            cn.tobytes() + cs.tobytes() + cd.tobytes())


def test_detection_distance_and_batching_on_a_revisit(pkg, abi, synth):
    scans, poses = city(synth)
    c = CITY
    n = len(scans)
    o = SC.options(lidar_height=c["lidar_height"])
    nd = int(sum(int(SC.non_decisive(s, o).sum()) for s in scans))
    ref = SC.describe(scans, o)
    plan = pkg.sc_replay_plan(list(range(1, n + 1)), lidar_height=c["lidar_height"])
    assert plan.tobytes() == SC.replay_plan(list(range(1, n + 1)), o).tobytes()
    queries = [(i, int(plan[i])) for i in range(n)]
    want = SC.detect(ref, queries, o)
    planted = [w["min_dist"] for i, w in enumerate(want) if i >= c["first"]]
    others = [w["min_dist"] for i, w in enumerate(want) if i < c["first"] and plan[i] > 0]
    _note(test="detect-margins", nodes=n, non_decisive=nd, searched=int((plan > 0).sum()), planted_max=float(max(planted)), others_min=float(min(others)), dist_thres=o["dist_thres"],
          db_end_values=sorted(set(int(p) for p in plan)))
    assert nd == 0
    assert max(planted) < 0.8 * o["dist_thres"] and min(others) > 2.0 * o["dist_thres"]        # the scene's margins, from the restatement alone
    for i, w in enumerate(want):                                                               # the planted loops and nothing else
        assert w["loop_node"] == (i - c["first"] if i >= c["first"] else -1), (i, w["loop_node"])
        if i >= c["first"]:
            assert w["shift"] == (60 - c["yaw_sectors"]) % 60                                  # the query is turned by +5 sectors: the candidate's columns move back by 5
    h = _handle(pkg, abi, scans)
    db = h.sc_describe(list(range(n)), lidar_height=c["lidar_height"])
    _same_db(db.read(), ref, np.arange(n), "the revisit's database")
    got = db.detect(queries)
    again = db.detect(queries)
    for i in range(n):
        assert got[i].struct_size == C.sizeof(abi.IbaScResult)
        assert _result_bytes(got[i], 3) == _ref_bytes(want[i], 3), (i, got[i].loop_node, want[i]["loop_node"], got[i].min_dist, want[i]["min_dist"], got[i].cand_node[:3], want[i]["cand_node"])
        assert _result_bytes(again[i], 3) == _result_bytes(got[i], 3), ("second call", i)
    # a query alone, and inside a batch of 200 at several places
    rng = np.random.default_rng(31)
    mine = (n - 3, int(plan[n - 3]))
    alone = db.detect([mine])[0]
    batch = [queries[int(j)] for j in rng.integers(0, n, 200)]
    for place in (0, 77, 199):
        b = list(batch); b[place] = mine
        r = db.detect(b)
        assert _result_bytes(r[place], 3) == _result_bytes(alone, 3) == _ref_bytes(want[n - 3], 3), place
        assert all(_result_bytes(r[j], 3) == _ref_bytes(want[b[j][0]], 3) for j in range(200))
    # more candidates, a rebuilt set at every call, explicit ranges (db_end below num_candidates, a node inside its own range)
    o2 = SC.options(lidar_height=c["lidar_height"], num_candidates=16, tree_period=1, num_exclude_recent=10, search_ratio=0.25, dist_thres=0.5)
    opt2 = _opt(pkg, o2)
    plan2 = pkg.sc_replay_plan(list(range(1, n + 1)), opt2)
    assert plan2.tobytes() == SC.replay_plan(list(range(1, n + 1)), o2).tobytes()
    q2 = [(i, int(plan2[i])) for i in range(n)] + [(5, 2), (5, 0), (0, n), (n - 1, n), (40, 15)]
    want2 = SC.detect(ref, q2, o2)
    got2 = db.detect(q2, opt2)
    for i in range(len(q2)):
        assert _result_bytes(got2[i], 16) == _ref_bytes(want2[i], 16), (i, q2[i], got2[i].cand_node[:], want2[i]["cand_node"])
    assert got2[n].n_candidates == 2 and got2[n].cand_node[2] == -1 and got2[n + 1].n_candidates == 0 and got2[n + 1].min_dist == SC.NO_WINNER and got2[n + 1].loop_node == -1
    assert got2[n + 2].cand_node[0] == 0 and got2[n + 2].min_dist < 1e-12                       # a node inside its own range finds itself
    # iba_sc_distance on its own
    pairs = np.stack([rng.integers(0, n, 300), rng.integers(0, n, 300)], 1).astype(np.int32)
    pairs[:c["again"]] = [[c["first"] + j, j] for j in range(c["again"])]
    rd, rs = SC.distances(ref["desc"], pairs, o)
    dd, ds = db.distance(pairs)
    one_d, one_s = db.distance(pairs[7:8])
    _note(test="distance", pairs=len(pairs), planted_max=float(rd[:c["again"]].max()), others_min=float(rd[c["again"]:][pairs[c["again"]:, 0] != pairs[c["again"]:, 1]].min()))
    assert dd.tobytes() == rd.tobytes() and ds.tobytes() == rs.tobytes(), np.flatnonzero((dd != rd) | (ds != rs)).tolist()
    assert one_d.tobytes() == rd[7:8].tobytes() and one_s.tobytes() == rs[7:8].tobytes()
    db.close()
    h.close()


def _rz(a):
    T = np.eye(4)
    T[0, 0] = T[1, 1] = np.cos(a); T[0, 1] = -np.sin(a); T[1, 0] = np.sin(a)
    return T


def test_loop_closure_through_the_public_api(pkg, abi, synth):
    """iba_sc_replay_plan -> iba_sc_detect -> iba_submap_build -> iba_scan_register: PerformLoopClosure + LoopClosureRegThread. The start of the
    registration is the detected yaw alone (rotation about z by -yaw_rad, no translation): up to 0.3 m and 3 degrees + 0.01 rad from the planted pose.
    Bounds of the recovered pose, from the inputs alone: 0.1 m — a quarter of the 0.4 m voxel whose centroids are the target, each standing for the
    surface inside its voxel — and 0.005 rad — 0.2 m at 40 m, inside the 0.3 m refine gate. The rotation bound is a third of the start error."""
    scans, poses = city(synth)
    c = CITY
    n = len(scans)
    h = _handle(pkg, abi, scans)
    db = h.sc_describe(list(range(n)), lidar_height=c["lidar_height"])
    plan = pkg.sc_replay_plan(list(range(1, n + 1)), lidar_height=c["lidar_height"])
    q = n - 4
    r = db.detect([(q, int(plan[q]))])[0]
    db.close()
    m = r.loop_node
    assert m == q - c["first"], (m, q)
    k = 3
    fr = list(range(max(m - k, 0), m + k + 1))
    cloud = h.submap_build([(fr, [poses[f] for f in fr], V.inverse34(poses[m]), 0.4)])[0]
    h.close()
    T_gt = np.linalg.inv(poses[m]) @ poses[q]
    T0 = _rz(-float(r.yaw_rad))
    h2 = pkg.IbaHandle(abi.Problem.from_scans([scans[q], cloud["xyz"].astype(np.float32)]), abi.reference_yaml_params(1))
    reg = h2.scan_register([(0, 1, T0)], estimation=0, coarse_dist=1.0, coarse_max_iter=30, refine_dist=0.3, refine_max_iter=30)[0].reg
    h2.close()
    T = reg.T_np()
    dt = float(np.linalg.norm(T[:3, 3] - T_gt[:3, 3])); dr = float(np.arccos(np.clip((np.trace(T[:3, :3].T @ T_gt[:3, :3]) - 1) / 2, -1, 1)))
    dt0 = float(np.linalg.norm(T0[:3, 3] - T_gt[:3, 3])); dr0 = float(np.arccos(np.clip((np.trace(T0[:3, :3].T @ T_gt[:3, :3]) - 1) / 2, -1, 1)))
    _note(test="loop-closure", query=q, loop_node=m, min_dist=r.min_dist, shift=r.shift, yaw_rad=float(r.yaw_rad), members=len(fr), voxels=len(cloud["xyz"]), iterations=reg.iterations, fitness=reg.fitness,
          rmse=reg.inlier_rmse, start_trans_err=dt0, start_rot_err=dr0, trans_err=dt, rot_err=dr)
    assert dt0 >= 0.15                                                  # the start really is off by more than the bound
    assert dt <= 0.1 and dr <= 0.005, (dt, dr)


def test_edges_of_the_domain(pkg, abi, synth):
    scans, ids = _scene(synth)
    h = _handle(pkg, abi, scans[:4])
    for fields, word in ((dict(num_sector=257), "num_sector must be in [1, 256]"), (dict(num_sector=0), "num_sector"), (dict(num_ring=65), "num_ring must be in [1, 64]"), (dict(num_candidates=17), "num_candidates"),
                         (dict(num_candidates=0), "num_candidates"), (dict(max_radius=0.0), "max_radius"), (dict(max_radius=float("nan")), "max_radius"), (dict(lidar_height=float("inf")), "lidar_height"),
                         (dict(search_ratio=-0.1), "search_ratio"), (dict(struct_size=8), "struct_size")):
        _raises(pkg, lambda: h.sc_describe([0, 1], **fields), 1, word)
    _raises(pkg, lambda: h.sc_describe([0, 4]), 1, "node 1 names frame 4 outside")
    _raises(pkg, lambda: h.sc_describe([-1]), 1, "outside")
    _raises(pkg, lambda: h.sc_describe([]), 1, "NULL")
    h.lib.iba_sc_describe.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_void_p)]
    fr = np.zeros(1, np.int32); o = pkg.sc_options(); res = C.c_void_p(None)
    assert h.lib.iba_sc_describe(h.h, fr.ctypes.data, 0, C.byref(o), C.byref(res)) == 1 and b"n must be in [1, 2^20]" in h.lib.iba_last_error(h.h) and not res.value
    assert h.lib.iba_sc_describe(h.h, fr.ctypes.data, 1, None, C.byref(res)) == 1 and b"NULL" in h.lib.iba_last_error(h.h)
    assert h.lib.iba_sc_describe(h.h, fr.ctypes.data, 1, C.byref(o), None) == 1 and b"NULL" in h.lib.iba_last_error(h.h)
    db = h.sc_describe([0, 1])                                          # a database of fewer than num_candidates nodes: the missing slots are -1, no error
    h.close()                                                           # the database outlives the handle
    r = db.detect([(1, 2), (1, 1)])
    assert r[0].n_candidates == 2 and sorted(r[0].cand_node[:2]) == [0, 1] and r[0].cand_node[2] == -1 and r[0].cand_shift[2] == -1 and np.isnan(r[0].cand_dist[2])
    assert r[1].n_candidates == 1 and r[1].cand_node[:3] == [0, -1, -1]
    _raises(pkg, lambda: db.detect([(0, 3)]), 1, "db_end 3 is beyond the database's 2 nodes")
    _raises(pkg, lambda: db.detect([(0, 1), (0, -1)]), 1, "query 1: db_end -1")
    _raises(pkg, lambda: db.detect([(2, 1)]), 1, "node 2 is outside the database's 2 nodes")
    _raises(pkg, lambda: db.detect([(-1, 1)]), 1, "node -1 is outside")
    _raises(pkg, lambda: db.detect([]), 1, "Q must be in [1, 65536]")
    _raises(pkg, lambda: db.detect([(0, 1)] * 65537), 1, "Q must be in [1, 65536]")
    _raises(pkg, lambda: db.detect([(0, 1)], pkg.sc_options(num_sector=61)), 1, "differ from the database's")
    _raises(pkg, lambda: db.detect([(0, 1)], pkg.sc_options(num_sector=300)), 1, "num_sector must be in [1, 256]")
    arr = (abi.IbaScQuery * 1)(); arr[0].struct_size = 12; arr[0].node = 0; arr[0].db_end = 1
    _raises(pkg, lambda: db.detect_raw(arr, 1), 1, "struct_size")
    _raises(pkg, lambda: db.distance([[0, 2]]), 1, "pair 0 names node 2 outside")
    _raises(pkg, lambda: db.distance(np.zeros((0, 2), np.int32)), 1, "NULL")
    _raises(pkg, lambda: db.read(1, 2), 1, "outside the database's 2")
    assert len(db.detect([(0, 1)] * 65536)) == 65536 and len(db) == 2
    db.close()

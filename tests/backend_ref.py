"""Restatement of the back end's plan (include/iba_mi355x.h, iba_backend_plan): SCManage's gates (backend_opt.cpp:338-370) in plain Python floats and
libm calls, expression by expression as the header gives them: test infrastructure."""
import math

import numpy as np

# config/loam/backend.yml
DEFAULTS = dict(keyframe_meter_gap=1.5, keyframe_rad_gap=0.15, lc_keyframe_meter_gap=3.0, lc_keyframe_rad_gap=1.0, cloud_lag=1)


def pose_dif(a, b):
    """PoseDif of two 3x4 (lists of floats, row-major): (|t_b - t_a|, atan2(s, c) of R_b R_a^T)"""
    dx, dy, dz = b[3] - a[3], b[7] - a[7], b[11] - a[11]
    translation = math.sqrt((dx * dx + dy * dy) + dz * dz)
    R = [[(b[r * 4] * a[c * 4] + b[r * 4 + 1] * a[c * 4 + 1]) + b[r * 4 + 2] * a[c * 4 + 2] for c in range(3)] for r in range(3)]
    cs = (((R[0][0] + R[1][1]) + R[2][2]) - 1.0) / 2.0
    vx, vy, vz = R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]
    sn = math.sqrt((vx * vx + vy * vy) + vz * vz) / 2.0
    return translation, math.atan2(sn, cs)


def plan(poses12, **kw):
    """-> dict(keyframes, described, detects, sizes_at_call, accumulators): the last holds every value an accumulator had when it was compared, with
    the gap it was compared against (the margins of a scene are read off it)"""
    o = dict(DEFAULTS)
    for k in kw:
        if k not in o:
            raise KeyError(k)
    o.update(kw)
    P = [[float(v) for v in row] for row in np.asarray(poses12, np.float64).reshape(-1, 12)]
    keyframes, described, detects, sizes, compared = [0], [0], [False], [], []
    t_acc = r_acc = lc_t = lc_r = 0.0
    for j in range(1, len(P)):
        td, rd = pose_dif(P[j - 1], P[j])
        t_acc += td; r_acc += rd; lc_t += td; lc_r += rd
        compared += [(t_acc, o["keyframe_meter_gap"]), (r_acc, o["keyframe_rad_gap"])]
        if t_acc > o["keyframe_meter_gap"] or r_acc > o["keyframe_rad_gap"]:
            t_acc = r_acc = 0.0
            keyframes.append(j); described.append(j - o["cloud_lag"])
            compared += [(lc_t, o["lc_keyframe_meter_gap"]), (lc_r, o["lc_keyframe_rad_gap"])]
            det = lc_t > o["lc_keyframe_meter_gap"] or lc_r > o["lc_keyframe_rad_gap"]
            if det:
                lc_t = lc_r = 0.0
                sizes.append(len(described))
            detects.append(det)
    return dict(keyframes=keyframes, described=described, detects=detects, sizes_at_call=sizes, accumulators=compared)


def rigid_inverse(T):
    """[R^T, -R^T t] of a 4x4, sums in ascending index: the library's rule for every rigid inverse (numpy.linalg.inv rounds differently, and the float32
    narrowing of a sub-map's voxel averages shows it)"""
    import pgo_ref as P
    return P.to44(P.inv12(np.asarray(T, np.float64).reshape(1, 4, 4)))[0]


def run(scans, poses12, voxel=0.2, lc_submap_size=25, loop_overlap_thre=0.5, loop_inlier_rmse_thre=0.2, sc=None, coarse=None, refine=None, smooth=None, measured=None, estimates=None, twins=False, **plan_kw):
    """iba_backend_run's steps 1-10 composed from sc_ref, submap_ref, scan_ref and smooth_ref. Clouds are the float32 narrowing of the voxel averages,
    as the frames of an iba_submap_handle are. measured: {(history, query): T} puts these measurements into the loop factors in place of the
    restatement's own registrations (which are still run, recorded and used for the accept decision): the smoothing stage on the device's inputs.
    estimates: per update the poses [n, 3, 4] that become the current poses after it, in place of the restatement's own result (which is still computed
    from the same start and recorded): every sub-map and every update then starts from exactly what the device started from. twins: every detection
    also carries T_ld, the long-double registration of the same clouds.
    -> dict(poses [N, 3, 4], plan, sc [per call], detections, updates [smooth_ref.optimize results])"""
    import sc_ref as SC
    import scan_ref as R
    import smooth_ref as S
    import submap_ref as V
    sc = SC.options() if sc is None else sc
    coarse = dict(gate=1.0, max_iter=1, rel_fitness=1e-4, rel_rmse=1e-4) if coarse is None else coarse
    refine = dict(gate=0.3, max_iter=0, rel_fitness=1e-6, rel_rmse=1e-6) if refine is None else refine
    raw = np.asarray(poses12, np.float64).reshape(-1, 3, 4)
    N = len(raw)
    raw44 = np.zeros((N, 4, 4)); raw44[:, :3] = raw; raw44[:, 3, 3] = 1.0
    p = plan(raw, **plan_kw)
    clouds = [V.load_pcd(scans[f], voxel)["xyz"].astype(np.float32) for f in p["described"]]
    db = SC.describe(clouds, sc)
    db_end = SC.replay_plan(p["sizes_at_call"], sc)
    hits = SC.detect(db, [(s - 1, int(e)) for s, e in zip(p["sizes_at_call"], db_end)], sc)
    cur = raw44.copy()
    g = S.Graph(raw44[:1])
    g.add(-1, 0, raw44[0], S.PRIOR_VAR)
    detections, updates, call = [], [], 0
    kf_index = {f: k for k, f in enumerate(p["keyframes"])}

    def update(upto):
        g.nodes = np.ascontiguousarray(np.concatenate([g.nodes, raw44[len(g.nodes):upto]]))
        res = S.optimize(g, smooth, nodes=g.nodes)
        res["start"] = g.nodes.copy()
        res["graph"] = S.Graph(g.nodes, [(g.fi[f], g.fj[f], g.Z[f], g.var[f], g.robust[f]) for f in range(g.F)])
        new = res["nodes"].copy()
        if estimates is not None:
            new[:, :3] = np.asarray(estimates[len(updates)], np.float64).reshape(upto, 3, 4)
        g.nodes = new
        cur[:upto] = new
        updates.append(res)

    for j in range(1, N):
        g.add(j - 1, j, S.rel(raw44[j - 1], raw44[j]), S.ODOM_VAR)
        k = kf_index.get(j)
        if k is None or not p["detects"][k]:
            continue
        hit = hits[call]; call += 1
        if hit["loop_node"] < 0:
            continue
        history = p["keyframes"][hit["loop_node"]]
        members = range(max(0, history - lc_submap_size), min(history + lc_submap_size, N))
        tgt = V.build([(scans[f], cur[f]) for f in members], voxel, out=rigid_inverse(cur[history]))["xyz"].astype(np.float32)
        reg = R.register_two_stage(clouds[k], tgt, np.eye(4), coarse, refine)
        ok = bool(reg["fitness"] > loop_overlap_thre and reg["rmse"] < loop_inlier_rmse_thre)
        detections.append(dict(query=j, history=history, sc_dist=hit["min_dist"], fitness=reg["fitness"], rmse=reg["rmse"], T=np.asarray(reg["T"], np.float64), accepted=ok,
                               iterations=reg["iterations"], n_corr=reg["n_corr"], n_target=len(tgt)))
        if twins:
            ld = R.register_two_stage(clouds[k], tgt, np.eye(4), coarse, refine, dtype=np.longdouble)
            assert (ld["iterations"], ld["n_corr"]) == (reg["iterations"], reg["n_corr"])
            detections[-1]["T_ld"] = ld["T"]
        if ok:
            T = np.asarray(reg["T"] if measured is None else measured[(history, j)], np.float64).copy(); T[3] = [0, 0, 0, 1]
            g.add(history, j, T, S.LOOP_VAR, robust=True)
            update(j + 1)
    update(N)
    return dict(poses=cur[:, :3].copy(), plan=p, sc=hits, detections=detections, updates=updates)


# the closed circuit of tests/test_gpu_backend.py and tools/backend_bench.py: 30 frames on a circle of 20, frames 20 .. 29 drive over frames 0 .. 9 again
SCENE = dict(first=20, again=10, radius=6.5, pts=2500, boxes=260, lidar_height=2.0)
_cache = {}


def circuit(synth, seed, scene=None):
    """-> (scans [float32 [n, 3]], truth [N, 4, 4], raw [N, 4, 4]): boxes on a ground plane seen by a 360-degree, 32-ring scanner (synth's ray caster)"""
    import smooth_ref as S
    if seed in _cache:
        return _cache[seed]
    c = SCENE if scene is None else scene
    rng = np.random.default_rng(seed)
    nb, gz = c["boxes"], -1.73
    bx, by = rng.uniform(-45, 45, nb), rng.uniform(-45, 45, nb)
    bh, bs = rng.uniform(0.5, 6.0, nb), rng.uniform(0.5, 3.0, (nb, 2))
    keep = np.abs(np.hypot(bx, by) - c["radius"]) > 4.5          # none on the road
    boxes = [(np.array([bx[i] - bs[i, 0], by[i] - bs[i, 1], gz]), np.array([bx[i] + bs[i, 0], by[i] + bs[i, 1], gz + bh[i]])) for i in range(nb) if keep[i]]
    elev = np.deg2rad(np.linspace(-24.8, 8.0, 32))
    scans, truth = [], []
    for f in range(c["first"] + c["again"]):
        a = 2 * np.pi * (f % c["first"]) / c["first"]
        off = rng.uniform(-0.15, 0.15, 2) if f >= c["first"] else np.zeros(2)
        o = np.array([c["radius"] * np.cos(a) + off[0], c["radius"] * np.sin(a) + off[1], 0.0])
        yaw = a + np.pi / 2 + (rng.uniform(-0.01, 0.01) if f >= c["first"] else 0.0)
        az = np.deg2rad(np.linspace(-180, 180, 360, endpoint=False) + rng.uniform(0, 1))
        E, A = np.meshgrid(elev, az, indexing="ij")
        dl = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], -1).reshape(-1, 3)
        Rm = np.array([[np.cos(yaw), -np.sin(yaw), 0], [np.sin(yaw), np.cos(yaw), 0], [0, 0, 1.0]])
        t = synth._raycast(o, dl @ Rm.T, gz, (), boxes, 80.0)
        ok = np.flatnonzero(np.isfinite(t))
        sel = np.sort(rng.choice(ok, min(c["pts"], ok.size), replace=False))
        scans.append((dl[sel] * (t[sel] + rng.normal(0, 0.02, len(sel)))[:, None]).astype(np.float32))
        M = np.eye(4); M[:3, :3] = Rm; M[:3, 3] = o
        truth.append(M)
    truth = np.array(truth)
    raw = np.zeros_like(truth)
    raw[0] = truth[0]
    for f in range(1, len(truth)):          # the truth's steps with seeded drift
        raw[f] = raw[f - 1] @ S.rel(truth[f - 1], truth[f]) @ S.exp_se3(np.concatenate([rng.normal(0, 1e-3, 3), rng.normal(0, 5e-3, 3)]))[0]
        raw[f, 3] = [0, 0, 0, 1]
    _cache[seed] = (scans, truth, raw)
    return _cache[seed]

"""Seeded scenes for the Sim3 RANSAC tests (tests/test_sim3_cpu.py, tests/test_gpu_sim3.py): two keyframes with known poses, one point table, a true
similarity with scale != 1 between the two cameras, and a choice of noise, outlier share and N. A scene is {"xyz": the table, "jobs": [job, ...]}; a
job is the dict tests/sim3_ref.py reads. Sets are an INPUT of the library, so a scene can plan them: a repeated set is a tie by construction."""
import numpy as np

import sim3_ref as R

F, D = np.float32, np.float64
K = (500.0, 500.0, 320.0, 240.0)
LEVEL_SIGMA2 = np.array([1.2 ** (2 * l) for l in range(8)], F)      # mvLevelSigma2 of scale factor 1.2: [1] = 1.44


def rot(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]], D) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]], D) @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]], D))


def pose(rx, ry, rz, t):
    return np.concatenate([rot(rx, ry, rz), np.asarray(t, D).reshape(3, 1)], axis=1).astype(F)


TRUE = {"s": 1.35, "R": rot(0.05, -0.08, 0.03), "t": np.array([0.2, -0.1, 0.15], D)}    # Xc1 = s R Xc2 + t


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def make_job(rng, N, outliers=0.3, noise_px=0.4, max_iterations=300, sets=None, base=0):
    """-> (job, xyz [2 N, 3]): correspondence i is (table point base + i, table point base + N + i); the last round(outliers * N) are outliers"""
    T1, T2 = pose(0.02, 0.01, -0.03, (0.3, -0.2, 0.1)), pose(-0.04, 0.03, 0.02, (-0.5, 0.1, 0.4))
    c2 = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.0, 1.0, N), rng.uniform(2.5, 8.0, N)], axis=1)
    c1 = TRUE["s"] * c2 @ TRUE["R"].T + TRUE["t"]
    c1 += rng.normal(0, 1, (N, 3)) * (noise_px / K[0]) * c1[:, 2:3]
    n_out = int(round(outliers * N))
    if n_out:
        c1[N - n_out:] = np.stack([rng.uniform(-2, 2, n_out), rng.uniform(-1.5, 1.5, n_out), rng.uniform(3, 10, n_out)], axis=1)
    w1 = (c1 - T1[:, 3].astype(D)) @ T1[:, :3].astype(D)          # R^T (Xc - t)
    w2 = (c2 - T2[:, 3].astype(D)) @ T2[:, :3].astype(D)
    lv1, lv2 = rng.integers(0, 4, N), rng.integers(0, 4, N)
    job = {"Tcw1": T1, "Tcw2": T2, "K1": K, "K2": K, "point1": (base + np.arange(N)).astype(np.int32), "point2": (base + N + np.arange(N)).astype(np.int32),
           "max_err1": np.array([R.truncated_threshold(LEVEL_SIGMA2[l]) for l in lv1], F), "max_err2": np.array([R.truncated_threshold(LEVEL_SIGMA2[l]) for l in lv2], F),
           "sets": random_sets(rng, N, max_iterations) if sets is None else np.asarray(sets, np.int32).reshape(-1, 3), "n_outliers": n_out}
    return job, np.concatenate([w1, w2]).astype(F)


def random_sets(rng, N, iterations):
    if N < 3:
        return np.zeros((iterations, 3), np.int32)
    return np.stack([rng.choice(N, 3, replace=False) for _ in range(iterations)]).astype(np.int32)


def scene(specs, seed=0, **opts):
    """specs: a list of dicts of make_job's keywords -> {"xyz", "jobs", "opts"}; every job's points lie in one table, in job order"""
    rng = np.random.default_rng(seed)
    jobs, xyz, base = [], [], 0
    for sp in specs:
        sp = dict(sp)
        sp.setdefault("max_iterations", opts.get("max_iterations", 300))
        j, w = make_job(rng, base=base, **sp)
        jobs.append(j)
        xyz.append(w)
        base += len(w)
    return {"xyz": np.concatenate(xyz).astype(F), "jobs": jobs, "opts": opts}


def planned_sets(N, n_out, iterations, good_at):
    """iterations sets: the all-inlier triple (0, 1, 2) at the iterations of good_at, an all-outlier triple elsewhere"""
    s = np.tile(np.array([N - 1, N - 2, N - 3], np.int32), (iterations, 1))
    assert n_out >= 3
    s[list(good_at)] = (0, 1, 2)
    return s


def scene_list():
    """the scene the CPU and GPU tests share: statuses OK, NO_MORE and TOO_FEW, ragged N and budgets (asserted on the reference in the tests)"""
    return scene([{"N": 60, "outliers": 0.3}, {"N": 30, "outliers": 0.9}, {"N": 12}, {"N": 97, "outliers": 0.5}, {"N": 20, "outliers": 0.0}, {"N": 25, "outliers": 0.1},
                  {"N": 40, "outliers": 0.25, "sets": planned_sets(40, 10, 300, (4, 9, 17))}], seed=11)


def three_event_scene(N=40, iterations=30, good_at=(4, 9, 17)):
    """one job whose sets repeat one all-inlier triple at good_at and hold an all-outlier triple elsewhere: three events, each a tie with the one before"""
    return scene([{"N": N, "outliers": 0.25, "sets": planned_sets(N, 10, iterations, good_at)}], seed=5, max_iterations=iterations, min_inliers=3)


def lib_job(sm, job):
    return sm.job(job["Tcw1"], job["Tcw2"], job["K1"], job["K2"], job["point1"], job["point2"], job["max_err1"], job["max_err2"], job["sets"])


def lib_solve(sm, sc, host=False, device=0, **more):
    """the scene through the library -> Sim3Batch"""
    opts = dict(sc["opts"], **more)
    tb, jobs = sm.table(sc["xyz"]), [lib_job(sm, j) for j in sc["jobs"]]
    return sm.solve_host(tb, jobs, **opts) if host else sm.solve(tb, jobs, device=device, **opts)


def ref_run(sc, **more):
    opts = dict(sc["opts"], **more)
    return [R.run(sc["xyz"], j, **opts) for j in sc["jobs"]]


def compare(res, refs, opts, stages, label=""):
    """every output of a Sim3Batch against the reference's, byte for byte; the first mismatch names its job and stage"""
    assert len(res) == len(refs)
    E = opts.get("max_events", 1)
    for b, ref in enumerate(refs):
        at = "%s job %d: " % (label, b)
        r = res.read(b)
        if stages and ref["iterations"]:                                     # stage by stage first, so that a mismatch names the earliest
            st = res.iterations(b)
            for key in ("s", "R", "t", "inlier"):
                assert same_bytes(st[key], ref[key]), at + "stage " + key + " at iteration %s" % np.argwhere(st[key].reshape(len(st[key]), -1) != ref[key].reshape(len(ref[key]), -1))[:1]
        assert same_bytes(res.counts(b), ref["counts"]), at + "counts"
        for key in ("status", "n", "iterations", "n_events", "best_it", "best_inliers", "sweep_cap_hits"):
            assert r[key] == ref[key], at + key + " %s != %s" % (r[key], ref[key])
        assert r["n_listed"] == min(ref["n_events"], E), at + "n_listed"
        for k in range(r["n_listed"]):
            got, want = res.event(b, k), ref["events"][k]
            for key in ("iteration", "n_inliers"):
                assert got[key] == want[key], at + "event %d %s" % (k, key)
            for key in ("s", "R", "t", "inlier"):
                assert same_bytes(np.asarray(got[key]), np.asarray(want[key])), at + "event %d %s" % (k, key)
        got = res.best(b)
        if ref["status"] == R.TOO_FEW:
            assert got["iteration"] == -1 and got["n_inliers"] == 0 and not got["inlier"].any() and not got["R"].any()
        else:
            want = ref["best"]
            assert (got["iteration"], got["n_inliers"]) == (want["iteration"], want["n_inliers"]), at + "best"
            for key in ("s", "R", "t", "inlier"):
                assert same_bytes(np.asarray(got[key]), np.asarray(want[key])), at + "best " + key


# ---- the two CPU measurements (tests/test_sim3_cpu.py asserts them, tools/sim3_parity.py records them in profiles/sim3_parity.md) ----

def float64_solution(P1, P2):
    """an independent float64 solution of one triple: Horn with numpy.linalg.eigh on N -> (s, R [3, 3], t) f64"""
    P1, P2 = np.asarray(P1, D), np.asarray(P2, D)
    O1, O2 = P1.mean(axis=1), P2.mean(axis=1)
    Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
    M = Pr2 @ Pr1.T
    N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                  [M[1, 2] - M[2, 1], M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                  [M[2, 0] - M[0, 2], M[0, 1] + M[1, 0], -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                  [M[0, 1] - M[1, 0], M[2, 0] + M[0, 2], M[1, 2] + M[2, 1], -M[0, 0] - M[1, 1] + M[2, 2]]], D)
    w, x, y, z = np.linalg.eigh(N)[1][:, -1]
    Rm = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], D)
    P3 = Rm @ Pr2
    s = (Pr1 * P3).sum() / (P3 * P3).sum()
    return s, Rm, O1 - s * Rm @ O2


def measure_float64(sc, refs):
    """the rules' s, R, t beside float64_solution over every iteration of the scene -> the largest |difference| of (s, an entry of R, an entry of t)"""
    worst = np.zeros(3, D)
    for j, ref in zip(sc["jobs"], refs):
        sv = ref["solver"]
        for it in range(ref["iterations"]):
            idx = np.asarray(j["sets"], np.int32).reshape(-1, 3)[it]
            s, Rm, t = float64_solution(sv.c1[idx].T, sv.c2[idx].T)
            assert np.isfinite(ref["s"][it])
            worst = np.maximum(worst, [abs(D(ref["s"][it]) - s), np.abs(ref["R"][it].astype(D).reshape(3, 3) - Rm).max(), np.abs(ref["t"][it].astype(D) - t).max()])
    return worst


def rotation_by_angle_axis(q):
    """the reference's route for Z4, evaluated in float64: quaternion -> atan2 -> angle-axis -> Rodrigues, rounded to float32 once"""
    w, v = D(q[0]), np.asarray(q[1:4], D)
    with np.errstate(all="ignore"):
        n = np.sqrt((v * v).sum())
        dead = not (n > 0) or not np.isfinite(n)
        r = D(2.0) * np.arctan2(n, w) * v / n
        theta = np.sqrt((r * r).sum())
        k = r / theta if theta > 0 else np.zeros(3, D)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]], D)
        Rm = np.cos(theta) * np.eye(3) + (1 - np.cos(theta)) * np.outer(k, k) + np.sin(theta) * Kx
    return Rm.astype(F), dead


def measure_angle_axis(sc, refs):
    """Z4 beside the angle-axis route over every iteration of the scene -> (the largest entry difference of R, the inlier verdicts that differ,
    the verdicts compared)"""
    worst, differ, total = D(0.0), 0, 0
    for j, ref in zip(sc["jobs"], refs):
        if not ref["iterations"]:
            continue
        opts = {k: v for k, v in sc["opts"].items() if k in ("probability", "min_inliers", "max_iterations", "fix_scale")}
        other = R.Solver(sc["xyz"], j, rotation=rotation_by_angle_axis, **opts)
        while other.n_iterations < other.max_its:
            other.iterate(other.max_its)
        for it in range(ref["iterations"]):
            worst = max(worst, np.abs(other.hyps[it]["R"].astype(D).reshape(-1) - ref["R"][it].astype(D)).max())
            differ += int((other.inliers[it] != ref["inlier"][it]).sum())
            total += ref["n"]
    return worst, differ, total

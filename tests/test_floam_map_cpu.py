"""CPU tier of the F-LOAM scan-to-map block: pins tests/floam_map_ref.py itself (the yardstick of tests/test_gpu_floam_map.py). Jacobians against
central differences under Exp(delta) T, known answers of the two fits, Plus against a matrix exponential, the room scene's recovery, the long-double
yardstick of the records, and the gate margins of EVERY seeded scene the GPU tests use (STEP_SCENES / REGISTER_SCENES / nn_clouds below are what they
import). With
IBA_FLOAM_MAP_PARITY_OUT=<file> the measured figures are written there (profiles/floam_map_parity.md is such a run)."""
import math
import os

import numpy as np
import pytest

import floam_map_ref as F

MARGIN = 1e-6


# ---- the seeded scenes of the GPU tests: (name, room seed, perturbation seed, rotation in degrees, translation in metres). A scene whose margins
#      fall below MARGIN is re-seeded HERE, never skipped at run time. ----
ROOM_SEED = 1
STEP_SCENES = [("room-2deg", ROOM_SEED, 5, 2.0, 0.2), ("room-knee", ROOM_SEED, 9, 1.0, 0.12)]
REGISTER_SCENES = [("reg-a", ROOM_SEED, 5, 2.0, 0.2), ("reg-b", ROOM_SEED, 6, 1.0, 0.1), ("reg-c", ROOM_SEED, 7, 1.5, 0.15)]

# the neighbour test's clouds: a map of more than 12288 points has a node table above 6 KB and runs the search in four-wave blocks
NN_SEED, BIG_MAP = 11, 13000
NN_SIZES = (1, 63, 64, 65, 130)
NN_T = F.rigid([0.01, -0.02, 0.03], [0.05, -0.02, 0.01])

_cache = {}


def nn_max_dist2(map_name):
    """the 5-point maps are searched without a distance gate, so that their few points are found at all"""
    return 1e9 if map_name in ("four", "five", "six") else 1.0


def nn_clouds():
    """(maps, sources) of the neighbour test, built once"""
    if "nn" not in _cache:
        rng = np.random.default_rng(NN_SEED)
        base = rng.uniform(-3, 3, (400, 3)).astype(np.float32)                       # 400 points: 32 leaves, 7 chunk boxes
        dup = np.vstack([base[:60], base[:60], base[:60], base[60:200]]).astype(np.float32)   # every one of 60 points three times: ties
        big = rng.uniform(-6, 6, (BIG_MAP, 3)).astype(np.float32)
        maps = dict(four=base[:4], five=base[:5], six=base[:6], tiles=base, dup=dup, big=big)
        srcs = {n: (rng.uniform(-3, 3, (n, 3)) + rng.normal(0, 0.02, (n, 3))).astype(np.float32) for n in NN_SIZES}
        srcs[130][:40] = dup[:40] + np.float32(0.001)                                # queries beside triplicated points
        srcs[65][-1] = [40.0, 0.0, 0.0]                                              # more than 1 m outside every box: everything pruned
        _cache["nn"] = (maps, srcs)
    return _cache["nn"]


def reference_nn(map_name, n):
    """(query, idx, d2, ok) of one map and one source size of the neighbour test, computed once"""
    if ("nn", map_name, n) not in _cache:
        maps, srcs = nn_clouds()
        q = F.transform(NN_T, srcs[n])
        _cache[("nn", map_name, n)] = (q,) + F.knn5(q, maps[map_name], nn_max_dist2(map_name))
    return _cache[("nn", map_name, n)]


def room():
    if "room" not in _cache:
        _cache["room"] = F.room_scene(ROOM_SEED)
    return _cache["room"]


def scene_start(sc, pseed, rot, tr):
    return F.perturbed(sc["T_gt"], pseed, rot, tr)


def clouds(sc):
    return sc["src_edge"], sc["src_surf"], sc["map_edge"], sc["map_surf"]


def reference_step(name):
    """(moments, association) of a STEP_SCENES entry, computed once"""
    if ("step", name) not in _cache:
        _, seed, ps, rot, tr = next(s for s in STEP_SCENES if s[0] == name)
        sc = room()
        _cache[("step", name)] = F.step(scene_start(sc, ps, rot, tr), *clouds(sc))
    return _cache[("step", name)]


def reference_register(name):
    if ("reg", name) not in _cache:
        _, seed, ps, rot, tr = next(s for s in REGISTER_SCENES if s[0] == name)
        sc = room()
        _cache[("reg", name)] = F.register(scene_start(sc, ps, rot, tr), *clouds(sc))
    return _cache[("reg", name)]


def record_yardstick(name):
    """(edge, surf) of a STEP_SCENES entry: the reference's own per-entry error on that scene's records, f64 against long double"""
    if ("yard", name) not in _cache:
        _, seed, ps, rot, tr = next(s for s in STEP_SCENES if s[0] == name)
        sc = room()
        _cache[("yard", name)] = F.record_yardstick(scene_start(sc, ps, rot, tr), *clouds(sc))
    return _cache[("yard", name)]


# ---- Jacobians ----
def _numeric_J(T, pt, kind, v, h=1e-6):
    J = np.zeros(6)
    for k in range(6):
        d = np.zeros(6); d[k] = h
        rp, _ = F.residuals((F.plus(T, d) @ np.r_[pt, 1.0])[None, :3], np.array([kind]), v[None])
        rm, _ = F.residuals((F.plus(T, -d) @ np.r_[pt, 1.0])[None, :3], np.array([kind]), v[None])
        J[k] = (rp[0] - rm[0]) / (2 * h)
    return J


@pytest.mark.parametrize("kind", [1, 2])
def test_jacobians_match_central_differences(kind):
    rng = np.random.default_rng(3)
    for _ in range(20):
        T = F.rigid(rng.normal(size=3) * 0.4, rng.normal(size=3) * 3)
        pt = rng.normal(size=3) * 5
        if kind == 1:
            c, u = rng.normal(size=3) * 4, rng.normal(size=3); u /= np.linalg.norm(u)
            v = np.r_[c + 0.1 * u, c - 0.1 * u, 0.0]
        else:
            n = rng.normal(size=3); n /= np.linalg.norm(n)
            v = np.r_[n, rng.normal() * 3, 0, 0, 0]
        lp = (T @ np.r_[pt, 1.0])[None, :3]
        _, J = F.residuals(lp, np.array([kind]), v[None])
        Jn = _numeric_J(T, pt, kind, v)
        assert np.max(np.abs(J[0] - Jn)) <= 1e-6 * max(1.0, np.max(np.abs(Jn))), (kind, J[0], Jn)


# ---- known answers ----
def test_five_collinear_points_give_the_line_and_the_point_line_distance():
    p0, u = np.array([1.0, 2.0, -0.5]), np.array([2.0, -1.0, 2.0]) / 3.0
    P = np.stack([p0 + s * u for s in (-0.4, -0.1, 0.0, 0.25, 0.5)])[None]
    keep, a, b, lam = F.fit_edge(P, 3.0, 0.1)
    assert keep[0]
    d = (a[0] - b[0]) / np.linalg.norm(a[0] - b[0])
    assert abs(abs(d @ u) - 1) < 1e-12 and abs(np.linalg.norm(a[0] - b[0]) - 0.2) < 1e-12
    x = np.array([3.0, 0.5, 1.0])
    r, _ = F.residuals(x[None], np.array([1]), np.r_[a[0], b[0], 0.0][None])
    w = x - p0
    assert abs(r[0] - np.linalg.norm(w - (w @ u) * u)) < 1e-12


def test_five_coplanar_points_give_the_plane():
    n = np.array([1.0, 2.0, 2.0]) / 3.0; d = 1.7
    e1 = np.cross(n, [1, 0, 0]); e1 /= np.linalg.norm(e1); e2 = np.cross(n, e1)
    P = np.stack([-d * n + a * e1 + b * e2 for a, b in ((0.5, 0.5), (-0.5, 0.5), (-0.5, -0.5), (0.5, -0.5), (0.05, -0.02))])[None]   # a square and a point near its centre
    keep, nv, dd, _ = F.fit_surf(P, 0.2)
    assert keep[0] and np.max(np.abs(nv[0] - n)) < 1e-12 and abs(dd[0] - d) < 1e-12
    Q = P.copy(); Q[0, 4] += 0.3 * n                       # four coplanar points and the central one 0.3 m off: its residual stays at 0.248 > 0.2, rejected
    assert not F.fit_surf(Q, 0.2)[0][0]


def test_isotropic_blob_is_no_edge():
    P = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1.2]], float)[None] * 0.3 + 5.0
    assert not F.fit_edge(P, 3.0, 0.1)[0][0]


def test_plus_is_the_matrix_exponential():
    try:
        from scipy.linalg import expm
    except Exception:
        def expm(M):
            out, term = np.eye(4), np.eye(4)
            for k in range(1, 30):
                term = term @ M / k; out = out + term
            return out
    rng = np.random.default_rng(4)
    for scale in (1e-12, 1e-3, 0.5):
        d = rng.normal(size=6) * scale
        X = np.zeros((4, 4)); X[:3, :3] = F.skew(d[:3]); X[:3, 3] = d[3:]
        assert np.max(np.abs(F.exp_se3(d) - expm(X))) < 1e-9 * max(scale, 1e-6), scale     # (the reference's small-angle series is truncated: 1e-9 relative)


def test_ties_go_to_the_lowest_index_and_the_gate_is_strict():
    m = np.array([[0, 0, 0]] * 3 + [[1, 0, 0]] * 4, np.float32)
    idx, d2, ok = F.knn5(np.array([[0.5, 0, 0]]), m, 0.25)
    assert list(idx[0]) == [0, 1, 2, 3, 4] and not ok[0]          # d5^2 == 0.25 is not < 0.25
    assert F.knn5(np.array([[0.5, 0, 0]]), m, 0.2500001)[2][0]


# ---- the room: recovery, yardsticks, margins ----
def test_room_recovers_the_truth_and_figures_are_recorded():
    assert F.have_longdouble()                                     # LDBL_MANT_DIG >= 64: the yardstick means something
    sc = room()
    lines = []
    for name, _, ps, rot, tr in REGISTER_SCENES:
        r = reference_register(name)
        e0 = F.pose_error(scene_start(sc, ps, rot, tr), sc["T_gt"]); e1 = F.pose_error(r["T"], sc["T_gt"])
        print("floam-map-figures", name, "start", e0, "end", e1, {k: v for k, v in r.items() if k != "T"})
        assert r["status"] == 0 and r["passes"] == 2
        assert e1[0] < 0.05 * e0[0] and e1[1] < 0.05 * e0[1], (name, e0, e1)    # back at the truth: what is left is the map's 3 mm noise and 2 x 4 iterations
        assert r["final_cost"] < 0.05 * r["initial_cost"]
        lines.append("| %s | %.1f deg / %.2f m | %.3e rad / %.3e m | %d / %d / %d | %d / %d |" % (name, rot, tr, e1[0], e1[1], r["passes"], r["iterations"], r["evaluations"], r["n_edge"], r["n_surf"]))
    yards = []
    for name, _, ps, rot, tr in STEP_SCENES:                      # every scene whose records the GPU tests compare has a yardstick of its own
        ye, ys = record_yardstick(name)
        print("floam-map-figures yardstick %s edge %.3e surf %.3e" % (name, ye, ys))
        assert 0 < ye < 1e-13 and 0 < ys < 1e-10                  # f64 against long double on 5-point fits of coordinates up to 12 m
        yards.append("| %s | %.1f deg / %.2f m | %.3e | %.3e | %.3e | %.3e |" % (name, rot, tr, ye, 4 * ye, ys, 4 * ys))
    out = os.environ.get("IBA_FLOAM_MAP_PARITY_OUT")
    if out:
        with open(out, "w") as f:
            f.write("# F-LOAM scan-to-map: measured yardsticks\n\nWritten by `IBA_FLOAM_MAP_PARITY_OUT=<this file> python -m pytest tests/test_floam_map_cpu.py` "
                    "(CPU only, tests/floam_map_ref.py). The GPU tests recompute the same figures from the same seeds and hold the device to them.\n\n"
                    "## Records: the reference's own error (rule 9)\n\nLargest |f64 entry - long-double entry| over the kept records of each scene whose records "
                    "the GPU tests compare (room seed %d, 300 edge / 2000 surf source points). The f64 line fit is numpy.linalg.eigh, its long-double twin a "
                    "cyclic Jacobi (numpy has no long-double eigh); the plane fit is the same Householder QR in both. The device is allowed 4x the yardstick "
                    "of the scene per entry against the long-double evaluation.\n\n| scene | start | edge (a, b) yardstick, up to the swap | edge bar (4x) | surf (n, d) yardstick | surf bar (4x) |\n"
                    "|---|---|---|---|---|---|\n%s\n\n"
                    "## Registration: what the reference reaches\n\nRoom scene, defaults (2 passes x 4 iterations). The device must reach the truth within 2x the "
                    "residual error of its row and the reference's T within 1e-8.\n\n| scene | start | residual error | passes / iterations / evaluations | edge / surf factors |\n|---|---|---|---|---|\n%s\n"
                    % (ROOM_SEED, "\n".join(yards), "\n".join(lines)))


def test_every_gpu_scene_keeps_its_margins():
    sc = room()
    for name, _, ps, rot, tr in STEP_SCENES:
        m, rec = reference_step(name)
        mg = rec["margins"]
        print("floam-map-figures margins", name, mg, "kept", m[:4])
        assert min(mg["nn"], mg["edge"], mg["surf"], mg["huber"]) > MARGIN, (name, mg)
        assert m[1] > 0.5 * len(sc["src_edge"]) and m[3] > 0.5 * len(sc["src_surf"])
    # the knee scene has residuals on both sides of huber_delta
    T = scene_start(sc, *next(s[2:] for s in STEP_SCENES if s[0] == "room-knee"))
    _, rec = reference_step("room-knee")
    r, _ = F.residuals(F.transform_unfused(T, np.vstack([sc["src_edge"], sc["src_surf"]])), rec["kind"], rec["v"])
    a = np.abs(r[rec["kind"] != 0])
    assert (a <= 0.1).sum() > 100 and (a > 0.1).sum() > 100
    for name, _, ps, rot, tr in REGISTER_SCENES:                  # the first association of every registration
        _, rec = F.step(scene_start(sc, ps, rot, tr), *clouds(sc))
        mg = rec["margins"]
        assert min(mg["nn"], mg["edge"], mg["surf"], mg["huber"]) > MARGIN, (name, mg)


def test_the_neighbour_clouds_keep_their_distance_gate_margin():
    """the random clouds of the GPU neighbour test: the 5th distance of every query stays clear of max_nn_dist2, so `ok` cannot flip on a rounding"""
    maps, srcs = nn_clouds()
    for mn in maps:
        for n in NN_SIZES:
            _, idx, d2, ok = reference_nn(mn, n)
            if len(maps[mn]) < 5:
                assert not ok.any()
                continue
            mg = float(np.min(np.abs(d2[:, 4] - nn_max_dist2(mn))))
            assert mg > MARGIN, (mn, n, mg)
    assert reference_nn("big", 130)[3].sum() > 0 and not reference_nn("tiles", 65)[3][-1]


def test_small_maps_and_few_factors_are_degenerate():
    sc = room()
    T0 = scene_start(sc, 5, 2.0, 0.2)
    r = F.register(T0, sc["src_edge"], sc["src_surf"], sc["map_edge"][:10], sc["map_surf"])      # exactly min_map_edge points: not enough
    assert r["status"] == 1 and r["passes"] == 0 and np.array_equal(r["T"], T0)
    m, rec = F.step(T0, sc["src_edge"], sc["src_surf"], sc["map_edge"][:10], sc["map_surf"])
    assert not m.any() and not rec["kind"].any() and np.all(rec["nn"] == F.NONE)
    far = F.rigid([0, 0, 0], [100.0, 0, 0]) @ T0                                                  # no neighbour within 1 m: fewer than 6 factors
    r = F.register(far, *clouds(sc))
    assert r["status"] == 1 and r["passes"] == 1 and r["iterations"] == 0 and np.array_equal(r["T"], far)

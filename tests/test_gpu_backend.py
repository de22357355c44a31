"""Device tier of the back end's loop-closure run (include/iba_mi355x.h, iba_backend_run) against tests/backend_ref.py, which composes sc_ref,
submap_ref, scan_ref and smooth_ref. One synthetic closed circuit: 30 frames on a circle of 20, so that frames 20 .. 29 drive over frames 0 .. 9 again
with the same heading; raw poses are the truth plus seeded drift. The seed was chosen on the CPU from the reference alone; its margins are asserted.
Gates: keyframes, queries, detections (with their Scan Context distances) and accepted flags equal the INDEPENDENT reference run exactly. Then every
stage is held on the device's own inputs: with keep_update_poses the run hands out the estimates after every update, and a second reference run poses
its sub-maps by them, starts every update from them and takes the device's measured T into its loop factors. (The voxel averages of a sub-map are
narrowed to float32: a difference of one rounding in a pose or in out12 can flip single points by a float32 ulp and move a registration by 1e-9, so
the stages are compared on identical inputs, and the restatement forms out12 = [R^T, -R^T t] exactly as the library does.) Per loop, the gates of
tests/test_gpu_scan_edges.py: |T - long double| <= 4 x that of the float64 restatement, fitness to 1e-15, rmse to 1e-12 relative. Per update, the
optimise gate of tests/test_gpu_smooth.py: the same counts and stop, poses within 4 x the float64 reference's distance from its two long-double twins."""
import importlib

import numpy as np
import pytest

import backend_ref as B
import sc_ref as SC
import smooth_ref as S

pytestmark = pytest.mark.gpu
PKG = "spatial-temporal-lidar-camera-calibration_amd"
SEED = 2
SCENE = B.SCENE
SC_KW = dict(num_exclude_recent=3, tree_period=2, lidar_height=SCENE["lidar_height"])
ICP = dict(coarse=dict(gate=1.0, max_iter=30, rel_fitness=1e-4, rel_rmse=1e-4), refine=dict(gate=0.3, max_iter=30, rel_fitness=1e-6, rel_rmse=1e-6))
REF_KW = dict(voxel=0.2, lc_submap_size=2, loop_overlap_thre=0.5, loop_inlier_rmse_thre=0.2, sc=SC.options(**SC_KW), cloud_lag=0, **ICP)
DEV_KW = dict(voxel=0.2, lc_submap_size=2, loop_overlap_thre=0.5, loop_inlier_rmse_thre=0.2, cloud_lag=0, scan_coarse_max_iter=30, scan_refine_max_iter=30,
              **{"sc_" + k: v for k, v in SC_KW.items()})


# ---- tests ----
@pytest.fixture(scope="module")
def be(pkg):
    return importlib.import_module(PKG + ".backend")


@pytest.fixture(scope="module")
def world(pkg, abi, synth):
    scans, truth, raw = B.circuit(synth, SEED)
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    yield dict(scans=scans, raw=raw, h=h, ref=B.run(scans, raw[:, :3], **REF_KW))
    h.close()


def test_the_scene_has_margins(world):
    """from the reference alone: an accepted loop, a query that finds none, and every decision off its threshold"""
    ref = world["ref"]
    o = REF_KW["sc"]
    assert any(d["accepted"] for d in ref["detections"]) and any(hit["loop_node"] < 0 for hit in ref["sc"])
    for hit in ref["sc"]:
        assert abs(hit["min_dist"] - o["dist_thres"]) >= 1e-9
    for d in ref["detections"]:
        assert abs(d["fitness"] - REF_KW["loop_overlap_thre"]) >= 1e-6 and abs(d["rmse"] - REF_KW["loop_inlier_rmse_thre"]) >= 1e-6
    for value, gap in ref["plan"]["accumulators"]:
        assert abs(value - gap) >= 1e-9


def test_run_equals_the_reference(be, world):
    ind, raw = world["ref"], world["raw"]
    a = be.backend_run(world["h"], raw[:, :3], keep_update_poses=1, **DEV_KW)
    b = be.backend_run(world["h"], raw[:, :3], **DEV_KW)
    assert a["poses"].tobytes() == b["poses"].tobytes() and [d["T"].tobytes() for d in a["detections"]] == [d["T"].tobytes() for d in b["detections"]]
    assert all(p is None for p in b["update_poses"]) and a["poses"].tobytes() == a["update_poses"][-1].tobytes()
    # the decisions, against the independent reference run
    assert a["keyframes"].tolist() == ind["plan"]["keyframes"]
    assert [(d["query"], d["history"], d["accepted"]) for d in a["detections"]] == [(d["query"], d["history"], d["accepted"]) for d in ind["detections"]]
    assert [d["sc_dist"] for d in a["detections"]] == [d["sc_dist"] for d in ind["detections"]]
    assert len(a["updates"]) == len(ind["updates"]) == sum(d["accepted"] for d in ind["detections"]) + 1
    # every stage on the device's own inputs
    ref = B.run(world["scans"], raw[:, :3], measured={(d["history"], d["query"]): d["T"] for d in a["detections"]}, estimates=a["update_poses"], twins=True, **REF_KW)
    assert len(ref["detections"]) == len(a["detections"]) == 5
    for d, r in zip(a["detections"], ref["detections"]):
        truth = r["T_ld"]
        d_ref = float(np.max(np.abs(r["T"].astype(np.longdouble) - truth))); d_dev = float(np.max(np.abs(d["T"].astype(np.longdouble) - truth)))
        print("backend-figures loop", d["query"], d["history"], d["sc_dist"], d["fitness"], r["fitness"], d["rmse"], r["rmse"], d_dev, d_ref, r["iterations"], r["n_corr"], r["n_target"])
        assert (d["query"], d["history"], d["accepted"]) == (r["query"], r["history"], r["accepted"])
        assert abs(d["fitness"] - r["fitness"]) <= 1e-15 and abs(d["rmse"] - r["rmse"]) <= 1e-12 * r["rmse"]
        assert d_dev <= 4.0 * d_ref, (d["query"], d_dev, d_ref)
    for k, (u, r) in enumerate(zip(a["updates"], ref["updates"])):
        assert (u.iterations, u.trials, u.stop, u.n_nodes) == (r["iterations"], r["trials"], r["stop"], len(r["nodes"]))
        twins = [S.optimize(r["graph"], nodes=r["start"], ld=ld) for ld in ("lin", "solve")]
        assert all(t["trace"] == r["trace"] for t in twins)
        tol = 4.0 * max(float(np.max(np.abs(r["nodes"] - t["nodes"]))) for t in twins)
        err = float(np.max(np.abs(a["update_poses"][k] - r["nodes"][:, :3])))
        print("backend-figures update", k, u.n_nodes, u.trials, u.stop, err, tol)
        assert err <= tol, (k, err, tol)
    moved = float(np.max(np.abs(a["poses"] - raw[:, :3])))
    print("backend-figures poses", moved, float(np.max(np.abs(a["poses"] - ind["poses"]))))
    assert moved > 1e-4          # the loops moved something


def test_without_an_accepted_loop_the_poses_are_the_raw_poses(be, world):
    """loop_overlap_thre = 0.999: nothing is accepted; the odometry factors and the prior are at their optimum at the raw poses"""
    raw = world["raw"]
    a = be.backend_run(world["h"], raw[:, :3], **dict(DEV_KW, loop_overlap_thre=0.999))
    assert a["detections"] and not any(d["accepted"] for d in a["detections"]) and len(a["updates"]) == 1
    assert (a["updates"][0].stop, a["updates"][0].trials) == (S.STOP_RIGHT_TERM, 0)
    assert np.max(np.abs(a["poses"] - raw[:, :3])) <= 1e-10


def test_cloud_lag_describes_other_frames(be, world):
    raw = world["raw"]
    p0, p1 = be.backend_plan(raw[:, :3], cloud_lag=0), be.backend_plan(raw[:, :3], cloud_lag=1)
    assert p0["keyframes"].tolist() == p1["keyframes"].tolist() and p0["described"].tolist() == p0["keyframes"].tolist()
    assert p1["described"].tolist() == [0] + [k - 1 for k in p1["keyframes"].tolist()[1:]]
    a = be.backend_run(world["h"], raw[:, :3], **dict(DEV_KW, cloud_lag=1))
    ref = B.run(world["scans"], raw[:, :3], **dict(REF_KW, cloud_lag=1))
    assert [(d["query"], d["history"], d["accepted"]) for d in a["detections"]] == [(d["query"], d["history"], d["accepted"]) for d in ref["detections"]]


def test_argument_checks(be, world):
    import ctypes as C
    L = be._lib()
    raw = world["raw"]
    for kw, word in ((dict(cloud_lag=3), "cloud_lag"), (dict(struct_size=1), "struct_size"), (dict(voxel=-1.0), "voxel")):
        with pytest.raises(be.IbaError) as e:
            be.backend_run(world["h"], raw[:, :3], **kw)
        assert e.value.status == 1 and "iba_backend_run" in str(e.value) and word in str(e.value)
    with pytest.raises(be.IbaError) as e:          # more poses than resident scans: the composed call's message, this function's name in front
        be.backend_run(world["h"], np.concatenate([raw[:, :3]] * 2), **DEV_KW)
    assert "iba_backend_run: iba_submap_handle" in str(e.value)
    L.iba_backend_result_free(None)

"""bench.py's GPU-count contract, checked without a GPU: `--gpus N` is what the number will be labelled with, so a run that
cannot drive N devices must stop with a message instead of measuring something smaller (round 2's bench.py parsed the flag and
ignored it)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env_extra=None):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IBA_FORCE_DIST")}
    env.update(env_extra or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True, timeout=300)


def test_more_gpus_than_devices_is_refused():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("this box has the devices")
    for launch in ("auto", "group"):
        r = _run(["--gpus", "2", "--launch", launch, "--steps", "1", "--warmup", "0"])
        assert r.returncode != 0
        assert "--gpus 2 asked for" in r.stderr and "visible" in r.stderr, r.stderr
        assert "{" not in r.stdout            # no JSON line under a wrong label


def test_gpus_flag_must_agree_with_the_launcher():
    r = _run(["--gpus", "2"], {"WORLD_SIZE": "4", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "disagrees with WORLD_SIZE=4" in r.stderr
    r = _run(["--gpus", "0"])
    assert r.returncode != 0
    r = _run(["--gpus", "2", "--launch", "group"], {"WORLD_SIZE": "2", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "one process for all GPUs" in r.stderr


def test_default_is_the_metrics_own_problem_and_value_is_never_multiplied_by_the_gpu_count():
    """BASELINE.json's metric is the 2 M-point x 200-keyframe problem at 1 / 2 / 4 / 8 GPUs: strong scaling. Round 3's bench.py
    defaulted to weak scaling and multiplied candidates/s by N."""
    sys.path.insert(0, ROOT)
    import bench
    a = bench.build_parser().parse_args(["--gpus", "8"])
    assert a.scaling == "strong" and a.frames == 200 and a.pts == 10000 and a.batch == 64
    for scaling in ("strong", "weak"):
        for n in (1, 2, 8):
            assert bench.job_value(64 * 20, 0.01, n, scaling) == 64 * 20 / 0.01
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "units * evals" not in src and "n_gpus * evals" not in src


def test_steps_must_be_positive():
    r = _run(["--steps", "0"])
    assert r.returncode != 0 and "--steps must be >= 1" in r.stderr
    assert "{" not in r.stdout


def test_plain_run_is_the_headline_and_outputs_are_float64_rows_per_candidate(tmp_path):
    """--full (off by default) brings back everything beyond the headline; --dump-outputs writes the structs one iba_eval_full call
    returns as float64 arrays, one row per candidate, copied out of the reused output buffers."""
    import importlib
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    a = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.full is False and a.dump_outputs is None and (a.steps, a.warmup) == (7, 2)
    a = bench.build_parser().parse_args(["--full", "--dump-outputs", str(tmp_path)])
    assert a.full is True and a.dump_outputs == str(tmp_path)
    abi = importlib.import_module("spatial-temporal-lidar-camera-calibration_amd.abi")
    B = 3
    cost, nrm = (abi.IbaCostOut * B)(), (abi.IbaNormalOut * B)()
    for i in range(B):
        cost[i].f1, cost[i].C, cost[i].n_corr = 1.25 + i, float("nan") if i == 2 else 0.5, 100 + i
        nrm[i].H[:] = [float(v) for v in np.arange(49) + 100 * i]
        nrm[i].b[:] = [float(v) for v in -np.arange(7) - i]
        nrm[i].cost, nrm[i].n_factor_p2pl = 2.0 ** -40 * (i + 1), 7 * i
    arr = bench.output_arrays(cost, nrm)
    for i in range(B):   # the copies outlive the buffers
        cost[i].f1, nrm[i].H[0] = -1.0, -1.0
    assert set(arr) == {"cost_" + f for f, _ in abi.IbaCostOut._fields_} | {"normal_" + f for f, _ in abi.IbaNormalOut._fields_}
    assert all(v.dtype == np.float64 and len(v) == B for v in arr.values())
    assert arr["normal_H"].shape == (B, 7, 7) and arr["normal_b"].shape == (B, 7) and arr["cost_f1"].shape == (B,)
    assert np.array_equal(arr["cost_f1"], [1.25, 2.25, 3.25]) and np.array_equal(arr["cost_n_corr"], [100, 101, 102]) and np.isnan(arr["cost_C"][2])
    assert np.array_equal(arr["normal_H"][1], np.arange(49).reshape(7, 7) + 100) and np.array_equal(arr["normal_b"][2], -np.arange(7) - 2)
    assert np.array_equal(arr["normal_cost"], 2.0 ** -40 * np.arange(1, B + 1)) and np.array_equal(arr["normal_n_factor_p2pl"], [0, 7, 14])
    bench.dump_outputs(str(tmp_path / "out"), arr)
    for name, v in arr.items():
        got = np.load(tmp_path / "out" / (name + ".npy"))
        assert got.dtype == np.float64 and np.array_equal(got, v, equal_nan=True)

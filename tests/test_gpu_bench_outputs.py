"""bench.py's plain run on a small scene: the record holds the headline alone (roofline, extras and the CPU baseline are --full's), --steps
is the number of timed steps, and --dump-outputs writes what the last timed step returned — the same cost tuples and normal equations a
caller of iba_eval_full gets for those candidates (bench.py's seeded scene and xs_all[(steps - 1) % 4])."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu


def test_plain_run_dumps_its_last_timed_step(tmp_path, pkg, synth, abi):
    frames, pts, steps = 8, 3000, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "IBA_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--frames", str(frames), "--pts", str(pts), "--steps", str(steps),
                        "--warmup", "1", "--settle", "0", "--dump-outputs", str(tmp_path)], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    rec = json.loads(r.stdout.strip().splitlines()[-1])
    assert rec["steps"] == steps and rec["ms_per_step"] > 0 and rec["dtype"] == "f64" and rec["higher_is_better"] is True
    assert abs(rec["value"] - bench.BATCH * steps / (rec["ms_per_step"] * 1e-3 * steps)) <= 1e-9 * rec["value"]
    assert not {"roofline", "extras", "cpu_baseline", "large_batch"} & set(rec), sorted(rec)

    prob, meta = synth.make_scene(n_frames=frames, pts_per_frame=pts, n_keypoints=bench.KEYPOINTS, seed=0)
    rng = np.random.default_rng(0)
    xs_all = [synth.perturb(meta["x_gt"], rng, n=bench.BATCH) for _ in range(4)]
    h = pkg.IbaHandle(prob, abi.reference_yaml_params())
    want = bench.output_arrays(*h.eval_full(xs_all[(steps - 1) % 4]))
    h.close()
    got = {f[:-4]: np.load(tmp_path / f) for f in os.listdir(tmp_path)}
    assert set(got) == set(want)
    for name, w in want.items():
        g = got[name]
        assert g.dtype == np.float64 and g.shape == w.shape, name
        if name in ("cost_f1", "cost_f2", "cost_C", "normal_H", "normal_b", "normal_cost", "normal_chi2"):
            scale = np.nanmax(np.abs(w), initial=0.0)
            assert np.array_equal(np.isnan(g), np.isnan(w)) and np.nanmax(np.abs(g - w), initial=0.0) <= 1e-9 * scale, name
        else:   # counters: exact
            assert np.array_equal(g, w), name
    assert np.all(got["cost_n_corr"] > 0)

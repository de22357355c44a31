"""What the resident, fused ICP pass buys: one ICP iteration done two ways in the same process on the same inputs (120 k-point target; 5 k and
100 k sources), and the whole iba_icp_register at B = 1, 8, 64.
  (a) iba_geo_correspondences + the numpy Umeyama on the returned pairs: the only way before iba_icp_step existed (the baseline);
  (b) iba_icp_step without the pair output + the Umeyama on its 21 moments.
Warm-up, then medians of alternating repetitions, the host clock around blocking calls. Prints one JSON line; --md FILE appends a table.
  python tools/icp_bench.py [--reps 15] [--md build/icp_bench.md] [--quick]"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np

import icp_ref as R

PKG = "spatial-temporal-lidar-camera-calibration_amd"


def umeyama_from_moments(m):
    n = m[0]; mq, mp = m[2:5] / n, m[5:8] / n
    var = m[8] / n - mq @ mq
    U, d, Vt = np.linalg.svd(m[9:18].reshape(3, 3) / n - np.outer(mp, mq))
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    Rm = (U * S) @ Vt; c = (d * S).sum() / var
    T = np.eye(4); T[:3, :3] = c * Rm; T[:3, 3] = (m[18:21] + mp) - c * Rm @ (m[18:21] + mq)
    return T


def med(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--md", default=None)
    ap.add_argument("--quick", action="store_true", help="one small size (the kernel-trace run)")
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi")
    rng = np.random.default_rng(3)
    n_tgt = 120000
    tgt = (rng.normal(size=(n_tgt, 3)) * [25, 10, 1.5]).astype(np.float32)
    h = pkg.IbaHandle(abi.Problem.from_scans([tgt]), abi.reference_yaml_params())
    gate = 0.5
    T = np.eye(4); T[:3, :3] = 1.002 * R.rotvec([0, 0, 1e-3]); T[:3, 3] = [0.02, -0.01, 0.01]
    out = {"n_tgt": n_tgt, "gate": gate, "reps": a.reps, "sizes": {}}
    for n_src in ((5000,) if a.quick else (5000, 100000)):
        src = (tgt[rng.integers(0, n_tgt, n_src)].astype(np.float64) + rng.normal(0, 0.05, (n_src, 3)) - T[:3, 3]) @ T[:3, :3] / 1.002 ** 2
        tgt64 = tgt.astype(np.float64)

        def way_a():
            q = R.transform(T, src)
            s, t = h.geo_correspondences(0, q, gate * gate)   # (<= against the squared gate: GeoCalib's own comparison)
            return R.umeyama(q[s], tgt64[t]) @ T, len(s)

        def way_b():
            m = h.icp_step(src, T, gate)[0]
            return umeyama_from_moments(m) @ T, int(m[0])

        (Ta, na), (Tb, nb) = way_a(), way_b()
        assert na == nb and np.max(np.abs(Ta - Tb)) < 1e-9, (na, nb, np.max(np.abs(Ta - Tb)))
        for _ in range(3):
            way_a(); way_b()
        ta, tb = [], []
        for _ in range(a.reps):   # alternating
            t0 = time.perf_counter(); way_a(); ta.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); way_b(); tb.append(time.perf_counter() - t0)
        rec = {"kept": na, "a_geo_plus_numpy_ms": med(ta) * 1e3, "b_icp_step_ms": med(tb) * 1e3, "a_min_ms": min(ta) * 1e3, "b_min_ms": min(tb) * 1e3}
        for B in ((1,) if a.quick else (1, 8, 64)):
            starts = np.stack([R.perturb(T, np.random.default_rng(b), rot=(1e-3, 2e-3), trans=(0.01, 0.02), scale=0.001) for b in range(B)])
            res = h.icp_register(src, starts, max_corr_dist=gate)
            h.icp_register(src, starts, max_corr_dist=gate)
            tr = []
            for _ in range(max(3, a.reps // 3)):
                t0 = time.perf_counter(); res = h.icp_register(src, starts, max_corr_dist=gate); tr.append(time.perf_counter() - t0)
            its = [r.iterations for r in res]
            rec["register_B%d" % B] = {"ms": med(tr) * 1e3, "iterations_total": int(sum(its)), "passes": int(max(its)) + 1, "converged": int(sum(r.converged == 1 for r in res)),
                                       "ms_per_start_iteration": med(tr) * 1e3 / max(1, sum(its) + B)}
        out["sizes"][str(n_src)] = rec
    h.close()
    print(json.dumps(out))
    if a.md:
        with open(a.md, "a") as f:
            f.write("| source points | kept | (a) geo_correspondences + numpy Umeyama, ms | (b) iba_icp_step + Umeyama, ms | a / b |\n|---|---|---|---|---|\n")
            for k, r in out["sizes"].items():
                f.write("| %s | %d | %.3f | %.3f | %.2f |\n" % (k, r["kept"], r["a_geo_plus_numpy_ms"], r["b_icp_step_ms"], r["a_geo_plus_numpy_ms"] / r["b_icp_step_ms"]))
            f.write("\n| source points | B | iba_icp_register, ms | passes | start-evaluations | ms per start-evaluation |\n|---|---|---|---|---|---|\n")
            for k, r in out["sizes"].items():
                for key, v in r.items():
                    if key.startswith("register_B"):
                        f.write("| %s | %s | %.3f | %d | %d | %.4f |\n" % (k, key[10:], v["ms"], v["passes"], v["iterations_total"] + int(key[10:]), v["ms_per_start_iteration"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())

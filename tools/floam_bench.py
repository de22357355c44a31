"""F-LOAM feature extraction on the device beside the numpy restatement on the same box: iba_floam_extract for 200 scans x 120 k points (64 rings of
1875) and for one such scan. Nothing is gated: it records what is seen, a first measurement. On a GPU it writes profiles/floam_bench.md; the
per-kernel split comes from running this tool under `rocprofv3 --kernel-trace --stats -- python tools/floam_bench.py --reps 1`.
    python tools/floam_bench.py [--out profiles/floam_bench.md] [--reps 5] [--scans 200]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import floam_ref as F  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
RESOURCES = """| kernel | VGPRs | SGPRs | LDS bytes / block | scratch bytes / lane | occupancy (waves / SIMD) |
|---|---|---|---|---|---|
| iba_floam_classify_kernel | 18 | 34 | 272 | 0 | 8 |
| iba_floam_ring_points_kernel | 10 | 18 | 0 | 0 | 8 |
| iba_floam_sector_kernel | 53 | 57 | 16 static + 10 B per sorted entry + the mark words (5.2 KB at 512 entries, 80.3 KB at 8192) | 0 | 8 by registers; the LDS bounds it for long sectors |
| iba_floam_gather_kernel | 26 | 36 | 0 | 0 | 8 |"""


def best_ms(f, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floam_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--scans", type=int, default=200)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi")
    base = [F.room_scan(64, 1933, seed=40 + k) for k in range(4)]          # about 120 k points each after the dropouts
    rng = np.random.default_rng(2)
    scans = []
    for k in range(a.scans):                                              # the four rooms turned about z: 200 different scans without 200 ray casts
        c, s = np.cos(0.031 * k), np.sin(0.031 * k)
        scans.append((base[k % 4] @ np.array([[c, s, 0], [-s, c, 0], [0, 0, 1.0]], np.float32)).astype(np.float32))
    h = pkg.IbaHandle(abi.Problem.from_scans(scans), abi.reference_yaml_params(0))
    rows = []
    for name, fr in (("%d scans x %d points" % (a.scans, len(scans[0])), list(range(a.scans))), ("1 scan x %d points" % len(scans[0]), [0])):
        h.floam_extract(fr)                                               # warm-up
        keep = []
        dev = best_ms(lambda: keep.append(h.floam_extract(fr)), a.reps)
        t0 = time.perf_counter(); ref = F.extract(scans[0], F.options()); cpu = (time.perf_counter() - t0) * 1e3 * len(fr)
        got = keep[-1][0]
        same = all(np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(ref[k]).tobytes() for k in ("edge_index", "edge_xyz", "surf_index", "surf_xyz"))
        rows.append((name, dev[0], dev[1], cpu, same, len(ref["edge_index"]), len(ref["surf_index"])))
    h.close()
    lines = ["# F-LOAM feature extraction on the device: a first measurement", "",
             "`python tools/floam_bench.py` on one MI355X: wall time of the whole `iba_floam_extract` call from Python (the launch chain, its three synchronisations, the work buffers",
             "it allocates and frees, and the copies of both clouds to the host), best and median of %d; the numpy restatement `tests/floam_ref.py` on the same box, timed on" % a.reps,
             "one scan and scaled. Nothing comparable existed before this entry point, so there is no target and nothing here is gated. The per-kernel split is not recorded",
             "here: take it with `rocprofv3 --kernel-trace --stats` around this tool.", "",
             "| call | device best ms | device median ms | numpy restatement ms (scaled) | scan 0: same bytes | scan 0: edges | scan 0: surfs |", "|---|---|---|---|---|---|---|"]
    lines += ["| %s | %.3f | %.3f | %.0f | %s | %d | %d |" % (n, b, m, c, "yes" if s else "NO", e, u) for n, b, m, c, s, e, u in rows]
    lines += ["", "## Compiler resource report (hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage)", "", RESOURCES, "",
              "No kernel uses scratch. No block shape or occupancy was tuned: 256 threads everywhere, one block per sector."]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

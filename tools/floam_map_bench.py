"""F-LOAM scan-to-map on the device: iba_floam_map_step and iba_floam_map_register at B = 1 / 8 / 64 on a synthetic KITTI-sized pair (about 1.5 k edge
and 12 k surf source points against a 20 k edge / 100 k surf map; the pairs of a batch share the clouds and differ in their start pose). Nothing is
gated: nobody has measured these numbers before, the file records them. On a GPU it writes profiles/floam_map_bench.md.
Timing: both entry points block until their results are on the host and run on the handle's private stream, so a call is timed as the host sees it
(perf_counter around the call, after warm-up calls; best and median of --reps). The per-kernel split comes from running this tool under
`rocprofv3 --kernel-trace --stats -- python tools/floam_map_bench.py --reps 1`. The tool rewrites the timing part of the file only: everything from the
"Compiler resource report" heading on is kept as it stands, a table entered by hand from the compiler's report after a kernel changes.
    python tools/floam_map_bench.py [--out profiles/floam_map_bench.md] [--reps 10] [--warmup 3]"""
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
import floam_map_ref as F  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
RES_HEADING = "## Compiler resource report"   # from this heading on the file is kept by hand (as profiles/floam_bench.md is): this tool never writes figures it did not measure


def timed(f, warmup, reps):
    for _ in range(warmup):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "floam_map_bench.md"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi")
    rng = np.random.default_rng(7)
    map_edge, map_surf = F.room_clouds(rng, 0.0546, 0.00084, 0.003)
    se, ss = F.room_clouds(rng, 0.158, 0.0112, 0.0)
    T_gt = F.rigid([0.02, -0.015, 0.3], [1.2, -0.7, 0.15]); Ti = np.linalg.inv(T_gt)
    to_scan = lambda p: (p @ Ti[:3, :3].T + Ti[:3, 3]).astype(np.float32)
    clouds = [to_scan(se), to_scan(ss), map_edge.astype(np.float32), map_surf.astype(np.float32)]
    h = pkg.IbaHandle(abi.Problem.from_scans(clouds), abi.reference_yaml_params(0))
    rows = []
    for B in (1, 8, 64):
        pairs = [(0, 1, 2, 3, F.perturbed(T_gt, 100 + b, 1.0 + (b % 5) * 0.25, 0.1 + (b % 4) * 0.03)) for b in range(B)]
        st = timed(lambda: h.floam_map_step(pairs), a.warmup, a.reps)
        keep = []
        rg = timed(lambda: keep.append(h.floam_map_register(pairs)), a.warmup, a.reps)
        res = keep[-1]
        ev = sum(r["evaluations"] for r in res)
        worst = max(F.pose_error(r["T"], T_gt)[1] for r in res)
        rows.append((B, st[0], st[1], rg[0], rg[1], ev, sum(r["status"] == 0 for r in res), worst))
    h.close()
    sizes = " / ".join(str(len(c)) for c in clouds)
    lines = ["# F-LOAM scan-to-map on the device: resources and a first measurement", "",
             "`python tools/floam_map_bench.py` on one MI355X. Clouds (source edge / source surf / map edge / map surf points): %s. The pairs of a batch share the" % sizes,
             "clouds and start 1 .. 2 degrees / 0.10 .. 0.19 m from the truth. All times are HOST WALL TIME of the whole blocking call from Python (argument marshalling, the" ,
             "copies of poses and results, every launch and every synchronise of the LM loop), NOT kernel time: after %d warm-up calls, best and median of %d. The per-kernel" % (a.warmup, a.reps),
             "split is not recorded here: take it with `rocprofv3 --kernel-trace --stats` around this tool. Nothing comparable existed before, so there is no target and",
             "nothing here is gated.", "",
             "| B | step best ms | step median ms | register best ms | register median ms | evaluations of the batch | pairs ok | worst translation error m |", "|---|---|---|---|---|---|---|---|"]
    lines += ["| %d | %.3f | %.3f | %.3f | %.3f | %d | %d | %.4f |" % r for r in rows]
    tail = ""
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = f.read()
        if RES_HEADING in old:
            tail = old[old.index(RES_HEADING):]
    if not tail:
        tail = RES_HEADING + "\n\nNot recorded yet: compile csrc with -Rpass-analysis=kernel-resource-usage and enter the table here by hand.\n"
    text = "\n".join(lines) + "\n\n" + tail
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

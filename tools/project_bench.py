#!/usr/bin/env python3
"""Times the scan-to-image projection (iba_project_run and the colourise / overlay accessors) on one GPU and writes profiles/project_bench.md: the four
kernel times from HIP events (IBA_PROJECT_TIMING), the wall time of the whole call, the splat's achieved bytes per second beside the HBM figure, the
atomics per point, and the compiler's resource report of the projection kernels. Nothing is gated.

    python tools/project_bench.py --json runs.json --no-resources     on the GPU: measure, keep the numbers
    python tools/project_bench.py --from-json runs.json               anywhere hipcc is: format them, add the resource report (`make -C csrc asm`)
    python tools/project_bench.py                                     both in one go"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
os.environ.setdefault("IBA_DEBUG_ENV", "1")
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
KITTI = (718.856, 718.856, 607.1928, 185.2157, 1241.0, 376.0)
HBM_TBS = 6.29   # measured float4 copy on an MI355X (8.0 TB/s spec)
X = np.array([0.01, -0.02, 0.015, 0.05, -0.03, 0.08, 1.0])


def scans_of(rng, frames, pts):
    """points in and around the camera's frustum, 2 .. 80 m deep: about two thirds project inside a 1241 x 376 image"""
    out = []
    for _ in range(frames):
        z = rng.uniform(2.0, 80.0, pts)
        out.append(np.stack([rng.uniform(-1.0, 1.0, pts) * z, rng.uniform(-0.32, 0.32, pts) * z, z], axis=1).astype(np.float32))
    return out


def measure(reps):
    pkg = importlib.import_module(PKG); abi = importlib.import_module(PKG + ".abi"); pj = importlib.import_module(PKG + ".project")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (376, 1241, 3), dtype=np.uint8)
    rows = []
    for pts in (10000, 120000):
        h = pkg.IbaHandle(abi.Problem.from_scans(scans_of(rng, 200, pts), intr=KITTI), abi.reference_yaml_params(0))
        frames, xs = list(range(200)), np.tile(X, (200, 1))
        for r in (0, 1):
            o = pj.project_options(splat=r)
            pj.run(h, xs, frames, o).close()                       # warm-up: module load, first allocations
            wall = []
            for _ in range(reps):
                t0 = time.perf_counter(); p = pj.run(h, xs, frames, o); wall.append((time.perf_counter() - t0) * 1e3); p.close()
            os.environ["IBA_PROJECT_TIMING"] = "1"
            p = pj.run(h, xs, frames, o)
            p.colorize(0, img); p.overlay(0, img)
            del os.environ["IBA_PROJECT_TIMING"]
            ms = [float(v) for v in p.kernel_ms]
            c = [p.counts(j) for j in range(200)]
            uv, _, fl = p.points(0)
            ins = (fl & pj.INSIDE) > 0
            iu, iv = np.floor(uv[ins, 0]), np.floor(uv[ins, 1])
            atomics0 = float(((np.minimum(iu + r, 1240) - np.maximum(iu - r, 0) + 1) * (np.minimum(iv + r, 375) - np.maximum(iv - r, 0) + 1)).sum())
            n = sum(x["n_points"] for x in c)
            rows.append(dict(frames=200, points=pts, splat=r, chunks=p.n_chunks, wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)), splat_ms=ms[0], resolve_ms=ms[1],
                             visible_ms=ms[2], colourise_ms=ms[3], overlay_ms=ms[4], n_points=n, n_inside=sum(x["n_inside"] for x in c), n_visible=sum(x["n_visible"] for x in c),
                             n_pixels=sum(x["n_pixels"] for x in c), atomics_per_point_job0=atomics0 / max(c[0]["n_points"], 1),
                             splat_tbs=40.0 * n / (ms[0] * 1e-3) / 1e12 if ms[0] > 0 else 0.0))
            p.close()
            print(json.dumps(rows[-1]), flush=True)
        h.close()
    return rows


def resources():
    import resource_usage
    lines = resource_usage.table("project", "asm")
    return lines[2:4] + [ln for ln in lines[4:] if "iba_project" in ln]


def write(rows, res, out):
    with open(out, "w") as fh:
        fh.write("# Scan-to-image projection on the device: what one run saw\n\n")
        if rows:
            fh.write("`python tools/project_bench.py` on one MI355X. 200 jobs (one per frame, one extrinsic) at KITTI's 1241 x 376; points uniform in and around the\n"
                     "frustum, 2 .. 80 m. `wall`: the whole iba_project_run from Python — poses, job table, allocations of the result, the launch chain, one\n"
                     "synchronise. Kernel times are HIP events on the stream (IBA_PROJECT_TIMING), summed over the chunks of the call; colourise and overlay are\n"
                     "one job's launch each. The splat's bytes are 16 read + 24 written per point; the HBM figure beside them is the measured float4 copy rate,\n"
                     "%.2f TB/s. Atomics per point: job 0's clipped footprints over its points. Nothing here is gated.\n\n" % HBM_TBS)
            fh.write("| frames x points | r | chunks | wall ms (min / median) | splat ms | resolve ms | visible ms | colourise ms (1 job) | overlay ms (1 job) | splat TB/s | of HBM copy | atomics / point | inside | visible | pixels held |\n")
            fh.write("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                fh.write("| %d x %d | %d | %d | %.2f / %.2f | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f %% | %.2f | %.1f %% | %.1f %% | %d |\n" % (
                    r["frames"], r["points"], r["splat"], r["chunks"], r["wall_min_ms"], r["wall_median_ms"], r["splat_ms"], r["resolve_ms"], r["visible_ms"], r["colourise_ms"],
                    r["overlay_ms"], r["splat_tbs"], 100.0 * r["splat_tbs"] / HBM_TBS, r["atomics_per_point_job0"], 100.0 * r["n_inside"] / r["n_points"],
                    100.0 * r["n_visible"] / r["n_points"], r["n_pixels"]))
            fh.write("\nThe splat's 64-bit atomic mins per second, from job 0's atomics per point over all points: " + "; ".join(
                "%d x %d, r = %d: %.1f G/s" % (r["frames"], r["points"], r["splat"], r["atomics_per_point_job0"] * r["n_points"] / (r["splat_ms"] * 1e-3) / 1e9) for r in rows if r["splat_ms"] > 0) +
                ".\nAt r = 0 the splat moves points and records (no LDS tile, no merging of lanes that share a pixel: DESIGN.md 9); at r = 1 the nine mins per inside\n"
                "point are its cost. The resolve pass reads and writes every pixel of every job (16 bytes each) whatever the scans hold.\n")
        else:
            fh.write("The timings are UNMEASURED: this file was written without a GPU run and holds the compiler's resource report only.\n")
        if res:
            fh.write("\n## Resource report of the projection kernels (`make -C csrc asm`, hipcc --offload-arch=gfx950 -O3)\n\n" + "\n".join(res) + "\n\n"
                     "Scratch is 0 for all of them. iba_project_visible_kernel<true> is the colourise form of the visible kernel.\n")
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "project_bench.md"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None, help="keep the measured rows here")
    ap.add_argument("--from-json", default=None, help="format rows measured earlier instead of measuring")
    ap.add_argument("--no-resources", action="store_true", help="skip the compiler's resource report")
    a = ap.parse_args()
    rows = json.load(open(a.from_json)) if a.from_json else measure(a.reps)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    write(rows, None if a.no_resources else resources(), a.out)


if __name__ == "__main__":
    main()

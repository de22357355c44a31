#!/usr/bin/env python3
"""Times the ORB extraction (iba_orb_extract) on one GPU and writes profiles/orb_bench.md: seeded 1241 x 376 images at batch 1 / 8 / 64 with 2000
features; per stage the time (HIP events for the kernels, the steady clock for the host's share: IBA_ORB_TIMING), the bytes the stage must move computed
from the shapes, images per second from the wall time of whole calls, and the share of a call spent in the host distribution. Nothing is gated.

    python tools/orb_bench.py --json runs.json        on the GPU: measure, keep the numbers, write the file
    python tools/orb_bench.py --from-json runs.json   anywhere: format numbers measured earlier"""
import argparse
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault("IBA_DEBUG_ENV", "1")
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    pass
import numpy as np  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
W, H = 1241, 376
STAGES = ("resize", "score", "cell", "host distribution + copies", "orientation", "blur", "descriptor")
PATCH_PIXELS = sum(2 * u + 1 for u in (15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3)) * 2 - 31


def pattern(seed=7):
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < 512:
        x, y = (int(v) for v in rng.integers(-18, 19, 2))
        if x * x + y * y <= 324:
            pts.append((x, y))
    return np.array(pts, np.int8).reshape(256, 4)


def image(seed):
    """a street-scene stand-in: 600 rectangles of random size and grey level over a vertical ramp, and 40 patches of two-valued texture"""
    rng = np.random.default_rng(seed)
    img = np.tile(np.linspace(60, 160, H)[:, None], (1, W))
    for _ in range(600):
        x, y, w, h = int(rng.integers(0, W)), int(rng.integers(0, H)), int(rng.integers(4, 90)), int(rng.integers(4, 60))
        img[y:y + h, x:x + w] = rng.integers(20, 236)
    for _ in range(40):
        x, y = int(rng.integers(0, W - 40)), int(rng.integers(0, H - 40))
        img[y:y + 40, x:x + 40] += np.where(rng.integers(0, 2, (40, 40)) == 1, 25, 0)
    return np.clip(img, 0, 255).astype(np.uint8)


def stage_bytes(orb, opt, counts):
    """the bytes each stage must move for the images behind `counts`, from the shapes alone"""
    p = orb.plan(W, H, opt)
    px = [int(w) * int(h) for w, h in p["level_wh"]]
    n = len(counts)
    region = [max(int(w) - 38, 0) * max(int(h) - 38, 0) if c[0] else 0 for (w, h), c in zip(p["level_wh"], p["cells"])]
    cand = sum(int(c["candidates_per_level"].sum()) for c in counts)
    kp = sum(c["n_keypoints"] for c in counts)
    blurred = sum(px[l] for c in counts for l in range(len(px)) if c["per_level"][l] > 0)
    return {"resize": n * sum(px[l - 1] + px[l] + 8 * int(sum(p["level_wh"][l])) for l in range(1, len(px))), "score": 2 * n * sum(px), "cell": 2 * n * sum(region) + 12 * cand,
            "host distribution + copies": 12 * cand + 16 * kp, "orientation": kp * (PATCH_PIXELS + 4), "blur": 2 * blurred, "descriptor": kp * (512 + 32 + 4)}


def measure(reps):
    orb = importlib.import_module(PKG + ".orb")
    pat = pattern()
    opt = orb.orb_options(pat, n_features=2000)
    rows = []
    for batch in (1, 8, 64):
        imgs = [image(100 + i) for i in range(batch)]
        for _ in range(2):
            orb.extract(imgs, opt).close()                      # warm-up: code objects, first allocations
        wall = []
        for _ in range(reps):
            t0 = time.perf_counter(); f = orb.extract(imgs, opt); wall.append((time.perf_counter() - t0) * 1e3); f.close()
        os.environ["IBA_ORB_TIMING"] = "1"
        stage = []
        for _ in range(reps):
            f = orb.extract(imgs, opt)
            stage.append([float(v) for v in f.stage_ms])
            counts = [f.counts(i) for i in range(batch)]
            chunks = f.n_chunks
            f.close()
        del os.environ["IBA_ORB_TIMING"]
        ms = np.median(np.array(stage), axis=0)
        by = stage_bytes(orb, opt, counts)
        rows.append(dict(batch=batch, chunks=chunks, reps=reps, wall_min_ms=min(wall), wall_median_ms=float(np.median(wall)), stage_ms={s: float(m) for s, m in zip(STAGES, ms)},
                         stage_bytes=by, keypoints=sum(c["n_keypoints"] for c in counts), candidates=sum(int(c["candidates_per_level"].sum()) for c in counts),
                         fallback_cells=sum(int(c["fallback_cells_per_level"].sum()) for c in counts)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def write(rows, out):
    with open(out, "w") as fh:
        fh.write("# ORB extraction on the device: what the first run saw\n\n")
        fh.write("`python tools/orb_bench.py` on one MI355X. Seeded %d x %d images (rectangles over a ramp, patches of two-valued texture), 2000 features, 8 levels,\n"
                 "scale 1.2, thresholds 20 / 7. `wall`: the whole iba_orb_extract from Python — plans, tables, allocations, level 0 up, the launch chain, O6 on the\n"
                 "host, the results down — after two warm-up calls. Stage times are the median over the timed calls of a second set of calls with IBA_ORB_TIMING:\n"
                 "HIP events around the kernels, the steady clock around the host's share (both candidate copies, O6 over images and levels on up to 16\n"
                 "threads, the keypoints up). Bytes are what a stage must move, computed from the shapes and counts; GB/s is those bytes over the stage's time. No target is\n"
                 "set and nothing is gated.\n\n" % (W, H))
        fh.write("| batch | chunks | wall ms (min / median) | images / s (median) | keypoints | candidates | fallback cells | host share of the stages |\n|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            tot = sum(r["stage_ms"].values())
            fh.write("| %d | %d | %.2f / %.2f | %.1f | %d | %d | %d | %.1f %% |\n" % (r["batch"], r["chunks"], r["wall_min_ms"], r["wall_median_ms"], 1e3 * r["batch"] / r["wall_median_ms"],
                                                                                 r["keypoints"], r["candidates"], r["fallback_cells"], 100.0 * r["stage_ms"][STAGES[3]] / tot if tot > 0 else 0.0))
        for r in rows:
            fh.write("\n## Batch %d\n\n| stage | ms | bytes it must move | GB/s |\n|---|---|---|---|\n" % r["batch"])
            for s in STAGES:
                ms, by = r["stage_ms"][s], r["stage_bytes"][s]
                fh.write("| %s | %.3f | %d | %s |\n" % (s, ms, by, "%.1f" % (by / (ms * 1e-3) / 1e9) if ms > 0 else "-"))
        if rows:
            big = rows[-1]
            tot = sum(big["stage_ms"].values())
            fh.write("\nAt batch %d the host distribution with its copies takes %.1f %% of the summed stage time (%.2f of %.2f ms): that share is what moving O6 to the\n"
                     "device could remove. The rest of the wall time (%.2f ms of the median %.2f) is the host around the chain and is not split further here: plans and\n"
                     "tables, the pinned staging copy of level 0, the allocations of a call, the assembly of the result.\n" % (
                         big["batch"], 100.0 * big["stage_ms"][STAGES[3]] / tot, big["stage_ms"][STAGES[3]], tot, big["wall_median_ms"] - tot, big["wall_median_ms"]))
    print(open(out).read())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "orb_bench.md"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default=None, help="keep the measured rows here")
    ap.add_argument("--from-json", default=None, help="format rows measured earlier instead of measuring")
    a = ap.parse_args()
    rows = json.load(open(a.from_json)) if a.from_json else measure(a.reps)
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)
    write(rows, a.out)


if __name__ == "__main__":
    main()

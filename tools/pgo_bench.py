"""Pose-graph optimisation on the device beside the dense float64 trial of tests/pgo_ref.py: N = 512 with 8 loops and N = 4541 with 60 loops
(KITTI-00-sized, synthetic), segment K in {8, 16, 32, 64, 128}. Nothing is gated: it records what is seen, and the default K is chosen from it.
On a GPU it writes profiles/pgo_bench.md (the kernels' register / LDS report first: that part needs the compiler only).
    python tools/pgo_bench.py [--out profiles/pgo_bench.md] [--reps 7]"""
import argparse
import importlib
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
try:
    import torch  # noqa: F401  (one HIP runtime per process: torch's first)
except Exception:
    torch = None
import pgo_ref as R  # noqa: E402
import resource_usage  # noqa: E402

PKG = "spatial-temporal-lidar-camera-calibration_amd"
KS = (8, 16, 32, 64, 128)


def timed(f, reps, warm=2):
    for _ in range(warm):
        f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return min(t), float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgo_bench.md"))
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    lines = ["# Pose-graph optimisation on the device: what one run saw", ""]
    lines += ["## Kernels as compiled", ""] + resource_usage.table("iba_pgo.hip", "asm-pgo")[2:] + [""]
    have_gpu = torch is not None and torch.cuda.is_available()
    if not have_gpu:
        lines += ["## Timings", "", "not recorded: no GPU in this run."]
    else:
        pgo = importlib.import_module(PKG + ".pgo")
        lines += ["## Timings", "",
                  "`python tools/pgo_bench.py` on one MI355X: wall time of the whole C-ABI call from Python (launch chain + synchronise + the copies the call makes), 2 warm-up",
                  "calls, then best / median of %d. `linearise` = iba_pgo_linearize without outputs, `solve` = iba_pgo_solve at lambda_0 (delta N x 6 comes back)," % a.reps,
                  "`optimise` = iba_pgo_create + iba_pgo_optimize (both passes), per trial = that time over the LM trials it ran. Nothing here is gated.", "",
                  "| N | loops | K | K used | separators | linearise ms (best / median) | solve ms (best / median) | optimise ms | LM trials | ms per trial | pruned |", "|---|---|---|---|---|---|---|---|---|---|---|"]
        for N, loops in ((512, 8), (4541, 60)):
            g = R.make_graph(N, loops=loops, seed=7)
            edges = pgo.pgo_edges(g.edge_tuples())
            for K in KS:
                plan = pgo.pgo_plan(N, edges, segment=K)
                pg = pgo.PoseGraph(g.nodes, edges, segment=K)
                lin = timed(lambda: pg._chk(pg.lib.iba_pgo_linearize(pg.h, None, None, None, None, None)), a.reps)
                lam = 1e-5 * float(np.max(np.abs(pg.linearize()["A"])))
                sol = timed(lambda: pg.solve(lam), a.reps)
                pg.close()

                def whole():
                    p = pgo.PoseGraph(g.nodes, edges, segment=K)
                    r = p.optimize()
                    p.close()
                    return r
                whole()
                t0 = time.perf_counter(); r = whole(); opt_ms = (time.perf_counter() - t0) * 1e3
                trials = r.passes[0].trials + r.passes[1].trials
                lines.append("| %d | %d | %d | %d | %d | %.3f / %.3f | %.3f / %.3f | %.1f | %d | %.3f | %d |" % (N, loops, K, plan["K"], len(plan["separators"]), lin[0], lin[1], sol[0], sol[1],
                                                                                                       opt_ms, trials, opt_ms / max(trials, 1), r.n_pruned))
        # the dense float64 trial on the CPU at N = 512
        g = R.make_graph(512, loops=8, seed=7)
        w = np.ones(g.E)
        t0 = time.perf_counter(); lin = R.linearize(g.nodes, g, w); t_lin = (time.perf_counter() - t0) * 1e3
        H, b = R.dense_system(g.N, g, lin["A"], lin["b"])
        lam = 1e-5 * float(np.max(np.diag(H)))
        t_sol = timed(lambda: R.dense_solve(H, b, lam), 3, warm=1)[0]
        scale = (4541.0 / 512.0) ** 3
        lines += ["", "## The dense form on the CPU (tests/pgo_ref.py, numpy, this box's CPU)", "",
                  "| N | linearise ms | dense 6N x 6N solve ms | note |", "|---|---|---|---|",
                  "| 512 | %.1f | %.1f | measured |" % (t_lin, t_sol),
                  "| 4541 | — | %.0f | EXTRAPOLATED from N = 512 by (4541 / 512)^3; the matrix alone is 5.9 GB and was not formed |" % (t_sol * scale)]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()

"""bench.py — IBA residual+Jacobian evaluations/sec on the BASELINE.json workload.

One "step" = one batch of B candidate extrinsics x in R^7, each evaluated against every keyframe the job holds, producing
BOTH the BAError tuple (iba_global.cpp:169-344) AND the Gauss-Newton normal equations of the iba_local problem re-associated
at x (iba_local.cpp:145-323 + IBACalib2.hpp factors). Frames shard across GPUs; one sum all-reduce of the partial blocks per
call (RCCL over xGMI).

  --scaling strong (default) the 200-keyframe / 2 M-point problem of the metric itself (BASELINE.json: "2M pts x 200 KF @1/2/4/8
                   GPU") split N ways; value = candidates / s of THAT problem, whatever the GPU count.
  --scaling weak   every GPU holds configs[1]'s shape — 200 keyframes x 10 k points — so the map grows with the GPU count
                   (configs[2], [3]: N x 200 keyframes); value = candidates / s of that N-times-larger problem (NOT multiplied
                   by N: the record says how many keyframes a candidate covered).

A plain run sets up, warms up, times --steps steps and prints the record (metric, value, unit, ms_per_step, config). Everything
else the benchmark measures — the repeated timed regions, the 512-candidate step, the per-kernel times and the roofline, the
extras (batch sweeps, wide candidates, shard emulation, plane refit, KITTI-sized scans, calibrations, MADS replay, ORB-only BA,
sustained regions) and the CPU baseline — runs only with --full (--no-extras / --no-cpu-baseline then trim it as before).

  --dump-outputs DIR  after the timed steps, what the last timed step returned to its caller (the cost tuples and the normal
                      equations of the B candidates) as DIR/<struct>_<field>.npy, float64, one row per candidate. The scene and
                      the candidates are seeded: the same arguments give the same inputs in every run.
"""
import argparse
import hashlib
import importlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
PKG = "spatial-temporal-lidar-camera-calibration_amd"

FRAMES = 200
PTS_PER_FRAME = 10000
KEYPOINTS = 2000
BATCH = 64
HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: 8.0 TB/s spec
N_SIMD = 256 * 4        # MI355X: 256 CUs x 4 SIMDs


def algorithmic_bytes(n_points, n_frames, n_keypoints, n_corr, n_corr3, n_covis):
    """minimum traffic of ONE evaluation of the reference's formulation with float32 points, each datum
    touched once."""
    return (12.0 * n_points + 8.0 * n_keypoints + 8.0 * n_corr + n_corr3 * (12.0 * 31 + 24) + n_corr * n_covis * 12.0
            + n_frames * (256.0 + 96.0 * n_covis) + 640.0)


def source_stamp():
    """sha256 over the kernel sources: profiles/pmc_latest.json is only quoted when it was taken on these sources."""
    d = os.path.join(ROOT, PKG, "csrc")
    hsh = hashlib.sha256()
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".hpp", ".cpp")):
            hsh.update(open(os.path.join(d, f), "rb").read())
    return hsh.hexdigest()[:16]


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--settle", type=int, default=300, help="untimed steps BEFORE the warmup steps: a 10 ms timed region on a GPU that has only just left idle measures the clock ramp (config.untimed_steps_before_warmup)")
    ap.add_argument("--batch", type=int, default=BATCH)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--pts", type=int, default=PTS_PER_FRAME)
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--plane-cache", type=int, default=1, help="1 = memoise the x-independent local-plane fits (default), 0 = refit inside every evaluation")
    ap.add_argument("--full", action="store_true", help="also measure everything beyond the headline: repeated regions, the 512-candidate step, per-kernel times and roofline, "
                                                         "extras and the CPU baseline (off by default: a plain run times the headline only)")
    ap.add_argument("--no-extras", action="store_true", help="with --full: timed region and roofline only (profiling runs)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None, help="write what the last timed step computed as DIR/<name>.npy (float64)")
    ap.add_argument("--launch", choices=("auto", "ranks", "group"), default="auto",
                    help="how N GPUs are driven: ranks = one process per GPU over torch.distributed / RCCL (what the driver's torchrun line gives; "
                         "without WORLD_SIZE in the environment bench.py starts the N ranks itself), group = ONE process, iba_group_* with one issuing "
                         "thread and one RCCL communicator per device; auto = ranks")
    return ap


def job_value(evals, seconds, n_gpus, scaling):
    """The record's `value`: candidates evaluated against EVERY keyframe of the job per second — the whole-job aggregate. Never
    multiplied by the GPU count: in strong scaling the job is BASELINE's 200-keyframe problem at every N, in weak scaling it is
    N x 200 keyframes and the record says so (config.total_frames)."""
    assert scaling in ("strong", "weak") and n_gpus >= 1
    return evals / seconds


def output_arrays(cost, nrm):
    """The outputs of one iba_eval_full call as float64 arrays, one row per candidate: cost_<field> from the iba_cost_out
    structs, normal_<field> from the iba_normal_out structs (H as B x 7 x 7, b as B x 7; the counters are exact in float64).
    Copies: the step's output structs are reused by the next call."""
    arrays = {}
    for prefix, seq in (("cost", cost), ("normal", nrm)):
        for name, _ in type(seq[0])._fields_:
            arrays["%s_%s" % (prefix, name)] = np.array([np.array(getattr(s, name)) for s in seq], dtype=np.float64)
    arrays["normal_H"] = arrays["normal_H"].reshape(-1, 7, 7)
    return arrays


def dump_outputs(directory, arrays):
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), a)


SUSTAIN_S = 10.0   # seconds per sustained region of extras.sustained


def main():
    args = build_parser().parse_args()

    # ---- how many GPUs, really: --gpus is the contract, WORLD_SIZE what a launcher gave us; they must agree ----
    env_world = os.environ.get("WORLD_SIZE")
    if args.gpus < 1:
        sys.exit("bench.py: --gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        sys.exit("bench.py: --steps must be >= 1 and --warmup >= 0")
    if env_world is not None and int(env_world) != args.gpus and not os.environ.get("IBA_FORCE_DIST"):
        sys.exit("bench.py: --gpus %d disagrees with WORLD_SIZE=%s of the launcher: refusing to report a number for the wrong GPU count" % (args.gpus, env_world))
    if args.launch == "group" and env_world is not None and int(env_world) > 1:
        sys.exit("bench.py: --launch group is one process for all GPUs; do not start it under torchrun")
    if env_world is None and args.gpus > 1:
        import torch   # device_count() does not initialise the GPU: the ranks below are started from a process that never touched it
        have = torch.cuda.device_count()
        if have < args.gpus:
            sys.exit("bench.py: --gpus %d asked for, %d GPU(s) visible: not measuring a smaller job under that label" % (args.gpus, have))
        if args.launch != "group":
            import socket
            with socket.socket() as sk:
                sk.bind(("127.0.0.1", 0))
                port = sk.getsockname()[1]
            cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1", "--master-port", str(port),
                   os.path.abspath(__file__)] + sys.argv[1:]
            env = dict(os.environ, IBA_BENCH_SPAWNED="1")
            sys.exit(subprocess.call(cmd, env=env))

    t_start = time.perf_counter()
    # stdout carries ONE line, the JSON record: RCCL prints a version banner to stdout when its first communicator is made,
    # so everything but the record goes to stderr's descriptor
    sys.stdout.flush()
    fd_record = os.dup(1)
    os.dup2(2, 1)

    def stage(msg):
        if int(os.environ.get("RANK", "0")) == 0:
            print("[bench %7.1fs] %s" % (time.perf_counter() - t_start, msg), file=sys.stderr, flush=True)

    import torch
    import torch.distributed as dist
    stage("torch imported")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    use_dist = world > 1 or bool(os.environ.get("IBA_FORCE_DIST"))   # IBA_FORCE_DIST: exercise the RCCL path with one rank
    group_mode = args.launch == "group"
    n_gpus = args.gpus if group_mode else world
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))
    stage("process group ready" if use_dist else "single process")
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # everything of this process runs on ONE explicit stream: torch's default stream has the handle 0, which the C-ABI reads as
    # "the handle's own stream" — the kernels and torch's all-reduce / copies would then sit on unrelated streams
    work_stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(work_stream)
    assert torch.cuda.current_stream().cuda_stream != 0

    pkg = importlib.import_module(PKG)
    synth = importlib.import_module(PKG + ".synth")
    abi = importlib.import_module(PKG + ".abi")

    # ---- workload ----
    base, meta = synth.make_scene(n_frames=args.frames, pts_per_frame=args.pts, n_keypoints=KEYPOINTS, seed=0)
    params = abi.reference_yaml_params(plane_cache=args.plane_cache)
    if args.scaling == "weak":     # configs[1]'s shape on every GPU, tiled once per rank
        prob = base if n_gpus == 1 else synth.tile_scene(base, meta, n_gpus)[0]
        f0, f1 = rank * args.frames, (rank + 1) * args.frames
    else:                          # the 200-keyframe problem split over the ranks (contiguous ranges balanced by points)
        prob = base
        f0, f1 = pkg.shard_frames(prob.n_frames, n_gpus, rank, np.diff(prob.arrays["pt_offset"].astype(np.int64)))
    grp = None
    if group_mode:   # ONE process: every device's shard, issuing thread and communicator inside the library
        grp = pkg.IbaGroup(prob, params, devices=tuple(range(n_gpus)))
        f0, f1 = grp.frame_range(0)
        if grp.comm_ranks != n_gpus:
            sys.exit("bench.py: the group's communicator has %d ranks, %d GPUs were asked for" % (grp.comm_ranks, n_gpus))
    # (in group mode this handle only serves the per-kernel timing of device 0's shard after the timed region)
    h = pkg.IbaHandle(prob, params, device=local_rank, frame_begin=f0, frame_end=f1)
    stage("scene generated, handle created (static indices + plane memo)")
    h.set_timing(False)   # the library's per-phase event timing (a debug facility: four event records per chain, ~8 us of a step) is switched on only
                          # for the calls whose kernel times are read (phases() below), never inside a timed region
    stride = pkg.partial_stride()
    B = args.batch
    rng = np.random.default_rng(0)
    xs_all = [synth.perturb(meta["x_gt"], rng, n=B) for _ in range(4)]   # x0 +- seeded perturbations (0.5 mrad / 5 mm / 0.1 %)
    BIG = 8 * B   # the batch of extras.large_batch: one launch chain of 512 candidates (iba_create_options.max_chain_batch)
    d_part = torch.zeros(BIG * stride, dtype=torch.float64, device=dev)
    h_part = torch.zeros(BIG * stride, dtype=torch.float64).pin_memory()

    import ctypes as C
    lean_out = {}

    def eval_full_lean(xs, hh=None):
        """iba_eval_full through ctypes with the output arrays kept between calls (the wrapper's per-call allocations and list
        conversions cost ~30 us of a 0.6 ms step)"""
        hh = h if hh is None else hh
        n = len(xs)
        if n not in lean_out:
            lean_out[n] = ((pkg.IbaCostOut * n)(), (pkg.IbaNormalOut * n)())
        cost, nrm = lean_out[n]
        xs = np.ascontiguousarray(xs, np.float64)
        st_ = hh.lib.iba_eval_full(hh.h, xs.ctypes.data_as(C.c_void_p), C.c_int32(n), cost, nrm)
        if st_ != 0:
            raise pkg.IbaError(st_, hh.lib.iba_last_error(hh.h).decode())
        return cost, nrm

    def step(i, xsrc=xs_all):
        xs = xsrc[i % len(xsrc)]
        if grp is not None:   # candidate block once, the devices issued concurrently, one ncclAllReduce, device 0's copy finalised
            return grp.eval_full(xs)
        if not use_dist:   # one GPU: the C entry point does it all (launch chain, D2H of the 64-double blocks, host finalisation)
            return eval_full_lean(xs)
        # one process per GPU: the partial entry point enqueues on this process's stream and returns; ONE sum all-reduce of the
        # 64-double blocks (RCCL over xGMI); the block lands in pinned memory; the host finalises into arrays kept between calls
        st = torch.cuda.current_stream().cuda_stream
        n = len(xs)
        xs = np.ascontiguousarray(xs, np.float64)
        st_ = h.lib.iba_eval_full_partial(h.h, xs.ctypes.data_as(C.c_void_p), C.c_int32(n), C.c_void_p(d_part.data_ptr()), C.c_void_p(st))
        if st_ != 0:
            raise pkg.IbaError(st_, h.lib.iba_last_error(h.h).decode())
        dist.all_reduce(d_part[: n * stride])   # (a view of the first n blocks: the buffer also serves the 512-candidate region)
        h_part[: n * stride].copy_(d_part[: n * stride], non_blocking=True)
        cs = torch.cuda.current_stream()
        t_spin = time.perf_counter()
        while not cs.query():   # poll like the library's own wait (a blocking wait wakes up 10-20 us late on a 0.5 ms step)
            if time.perf_counter() - t_spin > 2e-3:
                cs.synchronize()
                break
        if n not in lean_out:
            lean_out[n] = ((pkg.IbaCostOut * n)(), (pkg.IbaNormalOut * n)())
        cost, nrm = lean_out[n]
        if h.lib.iba_finalize_cost(C.byref(params), C.c_void_p(h_part.data_ptr()), C.c_int32(n), cost) != 0 or \
           h.lib.iba_finalize_normal(C.byref(params), C.c_void_p(h_part.data_ptr()), C.c_int32(n), nrm) != 0:
            raise pkg.IbaError(-1, "iba_finalize_*")
        return cost, nrm

    def sync():
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    for i in range(args.settle):
        out = step(i)
    stage("settled")   # (no print, no allocation between the warm-up steps and the timed region: a write() to the log pipe right before t0 showed as a slow first region)
    for i in range(args.warmup):
        out = step(i)
    sync()
    t0 = time.perf_counter()
    for i in range(args.steps):
        out = step(i)
    sync()
    dt = time.perf_counter() - t0
    if use_dist:
        t = torch.tensor([dt], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
    stage("timed steps done")
    if args.dump_outputs and rank == 0:   # (before any later call reuses the step's output structs)
        dump_outputs(args.dump_outputs, output_arrays(*out))
        stage("outputs of the last timed step written to " + args.dump_outputs)
    # the timed region is ~10 ms at the default 20 steps: four more regions of the same K steps (AFTER the one the record's value
    # comes from) give its spread — a regression of a few per cent is otherwise inside the noise of one region
    region_rates = [B * args.steps / dt]
    for _ in range(4 if args.full else 0):
        sync()
        t0r = time.perf_counter()
        for i in range(args.steps):
            out = step(i)
        sync()
        dtr = time.perf_counter() - t0r
        if use_dist:
            tr_ = torch.tensor([dtr], dtype=torch.float64, device=dev)
            dist.all_reduce(tr_, op=dist.ReduceOp.MAX)
            dtr = float(tr_.item())
        region_rates.append(B * args.steps / dtr)

    # ---- the same step with 512 candidates per call: ONE launch chain (one pair search, one anchor plan, one set of launches), every rank
    #      on its shard, one all-reduce of 512 x 64 doubles. Not the headline (an optimiser's poll is tens of candidates); what the path
    #      gives a caller that has that many — and what keeps a small shard's GPU full in a multi-GPU job. Same bracket as the headline. ----
    #      (--full only; skipped with --no-extras: a profiling run then sees launches of ONE shape.)
    dt_big, n_big = None, max(4, args.steps // 2)
    if args.full and not args.no_extras:
        xs_big = [np.vstack([xs_all[(k + j) % len(xs_all)] for j in range(BIG // B)]) for k in range(2)]
        for i in range(3):
            step(i, xs_big)
        sync()
        t0b = time.perf_counter()
        for i in range(n_big):
            step(i, xs_big)
        sync()
        dt_big = time.perf_counter() - t0b
        if use_dist:
            tb_ = torch.tensor([dt_big], dtype=torch.float64, device=dev)
            dist.all_reduce(tb_, op=dist.ReduceOp.MAX)
            dt_big = float(tb_.item())
        for i in range(2):   # (the record's counts below come from the headline's candidates)
            out = step(i)

    if args.full:
        # ---- dominant kernels, timed with HIP events on their launch stream ----
        L = pkg.load_library()
        L.iba_last_phase_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]

        def phases():
            a, n, r = C.c_float(0), C.c_float(0), C.c_float(0)
            L.iba_last_phase_ms(h.h, C.byref(a), C.byref(n), C.byref(r))
            return a.value, n.value, r.value

        xs = xs_all[0]
        kms = []
        h.set_timing(True)
        for _ in range(5):
            h.eval_full_partial(xs, d_part.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            kms.append(phases())
        h.set_timing(False)
        assoc_ms, nn_ms, rest_ms = (float(v) for v in np.median(np.array(kms), axis=0))
        pair_ms = assoc_ms + nn_ms   # the two kernels that do what the reference's BAError / BuildProblem association does
        cost0 = pkg.finalize_cost(params, d_part[: B * stride].cpu().numpy())   # this rank's partial: the counts one launch processes
        n_slots = len(prob.arrays["covis_frame"]) / prob.n_frames
        per_eval = float(np.mean([algorithmic_bytes(h.n_points, f1 - f0, h.n_keypoints, c.n_corr, c.cnt_3d_3d, n_slots) for c in cost0]))
        achieved = B * per_eval / (pair_ms * 1e-3) / 1e9

    evals = B * args.steps
    units = 1            # one unit = one candidate against every keyframe of the job (never multiplied by the GPU count)
    value = job_value(evals, dt, n_gpus, args.scaling)
    if group_mode:
        launch, rccl_ranks = "group: one process, iba_group_* (one issuing thread + one RCCL communicator per device)", grp.comm_ranks
    elif use_dist:
        launch = "ranks: one process per GPU, torch.distributed backend nccl (= RCCL)" + (", started by bench.py itself" if os.environ.get("IBA_BENCH_SPAWNED") else ", started by the caller's launcher")
        rccl_ranks = dist.get_world_size()
    else:
        launch, rccl_ranks = "single process, no collective", 0
    res = {
        "metric": "IBA residual+Jacobian evals/sec",
        "value": value,
        "unit": "evals/s",
        "n_gpus": n_gpus,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": dt / args.steps * 1e3,
        "higher_is_better": True,
        "scaling": args.scaling,
        "vs_baseline": None,
        "dtype": "f64",
        "data": "synthetic",
        "config": {
            "workload": ("configs[1]-shaped synthetic street scene %s: %d keyframes x %d pts (%.1fM pts), %d keypoints/KF, IBACalib cost (3d-2d + 3d-3d plane + hand-eye) "
                         "+ iba_local normal equations per candidate") % ("per GPU (the job holds N x this)" if (args.scaling == "weak" and n_gpus > 1) else "split over the GPUs", args.frames, args.pts, args.frames * args.pts / 1e6, KEYPOINTS),
            "frames_this_rank": f1 - f0, "points_per_frame": args.pts, "keypoints_per_frame": KEYPOINTS,
            "candidates_per_step": B, "total_frames": prob.n_frames, "total_points": prob.n_points,
            "candidate_spread": "x_gt + N(0, 0.5 mrad), N(0, 5 mm), N(0, 0.1 %) per component (see extras.wide_candidates for a MADS-box-wide batch)",
            "plane_cache": int(params.plane_cache),
            "mean_n_corr": float(np.mean([c.n_corr for c in out[0]])), "mean_cnt_3d_3d": float(np.mean([c.cnt_3d_3d for c in out[0]])),
            "mean_factors": float(np.mean([n.n_factor_3d2d + n.n_factor_p2pl + n.n_factor_p2pt for n in out[1]])),
            "parallelism": "frames sharded over %d GPU(s), 1 all-reduce of %d doubles per call" % (n_gpus, B * stride),
            "untimed_steps_before_warmup": args.settle,
            "launch": launch, "rccl_ranks": rccl_ranks,
            "unit_definition": ("weak scaling: 1 eval = one candidate x against ALL %d keyframes of the job (%d per GPU), cost tuple + normal equations; "
                                "value = candidates/s, not multiplied by the GPU count" % (prob.n_frames, args.frames)) if args.scaling == "weak" else
                               "strong scaling: 1 eval = one candidate x against the whole %d-keyframe / %.1fM-point problem (cost tuple + normal equations), whatever the GPU count" % (args.frames, args.frames * args.pts / 1e6),
        },
    }
    if args.full:
        res["roofline"] = {
            # PHYSICAL figures only (round 3's `frac` was an effective rate against the reference's formulation and exceeded 1):
            #   achieved = HBM bytes the dominant kernels really moved per launch (FETCH_SIZE x2 + WRITE_SIZE, separate --pmc passes,
            #              profiles/pmc_latest.json, stamped with the kernel sources' hash) / their launch time measured HERE with HIP
            #              events on the launch stream;  hbm_frac = achieved / 8 TB/s.
            #   frac     = the fraction of the roof that BINDS these kernels: vector-instruction issue (bound "issue"): the share of
            #              SIMD cycles that issue a VALU instruction (4 x SQ_ACTIVE_INST_VALU / (1024 SIMDs x GRBM_GUI_ACTIVE / 8)).
            # The old effective figure lives on under effective_vs_reference_formulation (it is not a roofline fraction).
            "bound": "issue", "kernel": "association (iba_pairs_kernel + iba_assoc2_kernel) + search (iba_nn_kernel)", "achieved": None, "peak": HBM_PEAK_GBS, "unit": "GB/s",
            "frac": None, "frac_is": "valu_issue_share (4 x SQ_ACTIVE_INST_VALU / SIMD cycles) of the kernels named in `kernel`: NOT bytes / time / peak — that is hbm_frac", "hbm_frac": None, "traffic": None, "issue_frac": None,
            "launch_ms": pair_ms, "evals_per_launch": B, "shared_pair_search": bool(h.last_path),
            "kernel_ms": {"association (pairs + assoc2)": assoc_ms, "iba_nn_kernel": nn_ms, "factor + sums": rest_ms},
            "kernel_ms_how": "HIP events of the library on the launch stream (iba_set_timing), median of 5 launches of the headline's candidates right after the timed regions; the timed regions themselves run with the event timing off, as a caller's do",
            "effective_vs_reference_formulation": {
                "what": "algorithmic bytes of SURVEY 8(d) (every candidate streams every scan, gathers 31 points per MapPoint) x candidates per launch / (association + search kernel time): "
                        "an effective rate against the uncached, unbatched formulation. The kernels do not move those bytes (planes memoised, one pair search per batch, 1-NN memoised around an anchor), "
                        "so it may exceed the HBM peak; like_for_like = the same ratio with the planes fitted inside every evaluation (plane_cache = 0), over the whole step",
                "algorithmic_bytes_per_eval": per_eval, "effective_GBs": achieved, "ratio_to_hbm_peak": achieved / HBM_PEAK_GBS, "like_for_like": None},
        }
        # measured HBM traffic and VALU issue share of the same launch shape from the committed counter passes (tools/prof_run.sh +
        # tools/summarize_prof.py stamp them with the kernel sources' hash). Counters taken on OTHER sources of the same shape are
        # still quoted, flagged pmc_stale (a physical figure of a nearby kernel version beats none); another shape is not quoted.
        pmc_file = os.path.join(ROOT, "profiles", "pmc_latest.json")
        if os.path.exists(pmc_file):
            try:
                pmc = json.load(open(pmc_file))
                same_shape = (pmc.get("frames"), pmc.get("pts"), pmc.get("batch")) == (f1 - f0, args.pts, B)
                if same_shape:
                    rf = res["roofline"]
                    rf["traffic"] = pmc.get("hbm_bytes_per_launch")
                    rf["issue_frac"] = pmc.get("valu_issue_frac")
                    rf["achieved"] = rf["traffic"] / (pair_ms * 1e-3) / 1e9
                    rf["hbm_frac"] = rf["achieved"] / HBM_PEAK_GBS
                    rf["frac"] = rf["issue_frac"]
                    rf["pmc_stale"] = pmc.get("source_stamp") != source_stamp()
                    if pmc.get("hbm_bytes_per_step"):
                        rf["whole_step"] = {"hbm_bytes": pmc["hbm_bytes_per_step"], "hbm_frac": pmc["hbm_bytes_per_step"] / (dt / args.steps) / 1e9 / HBM_PEAK_GBS,
                                            "issue_frac": pmc.get("valu_issue_frac_step")}
                    rf["pmc_provenance"] = {k: pmc.get(k) for k in ("round", "git_head", "source_stamp", "taken_on", "counters")}
                    # per kernel of one step, from the same counter passes and the committed rocprofv3 summary: duration, share of the HBM peak, VALU-active share
                    pk = pmc.get("per_kernel") or {}
                    step_kernels = {k: v for k, v in pk.items() if not any(t in k for t in ("anchor", "plane_kernel", "verdict"))}
                    if step_kernels:
                        rf["per_kernel"] = {k: {"avg_us": v.get("avg_us"), "hbm_frac": ((v.get("hbm_read_bytes", 0) + v.get("hbm_write_bytes", 0)) / (v["avg_us"] * 1e-6) / 1e9 / HBM_PEAK_GBS) if v.get("avg_us") else None,
                                                "valu_active": v.get("valu_active_share"), "wait_any": v.get("wait_any_share"), "l2_requests": v.get("l2_requests")} for k, v in step_kernels.items()}
                        rf["longest_kernel"] = max(step_kernels, key=lambda k: step_kernels[k].get("avg_us") or 0.0)
                else:
                    res["roofline"]["pmc_provenance"] = "profiles/pmc_latest.json was taken on another launch shape (%s frames x %s pts x %s candidates): not quoted" % (pmc.get("frames"), pmc.get("pts"), pmc.get("batch"))
            except Exception:
                pass

    if dt_big is not None:
        res["large_batch"] = {"candidates_per_step": BIG, "steps": n_big, "ms_per_step": dt_big / n_big * 1e3, "evals_per_s": BIG * n_big / dt_big,
                              "note": "512 candidates per call = one launch chain; same scene, same candidate spread, same bracket (barrier + synchronize on both sides, max over ranks) as the headline, which stays at 64 per step"}
    if group_mode:
        res["config"]["group_issue_us_last_call"] = grp.last_issue_us
    if args.full and not args.no_extras and group_mode:
        stage("extras are measured in the default launch mode: skipped with --launch group")
    if args.full and not args.no_extras and not group_mode:
        extras = {}
        extras["timed_region_repeats"] = {"regions": len(region_rates), "steps_each": args.steps, "evals_per_s": region_rates, "min": float(np.min(region_rates)), "median": float(np.median(region_rates)),
                                          "max": float(np.max(region_rates)), "note": "region 0 is the record's value; the others follow it back to back"}
        st = torch.cuda.current_stream().cuda_stream
        # (1) batch-size sweep: wall and device time per call (NOMAD polls 8..14 points, the BAError shim calls B = 1)
        sweep = {}
        for b in (1, 8, 14, 64):
            xb = xs_all[1][:b]
            for _ in range(3):
                step(0, [xb])
            sync()
            ts = []
            for _ in range(50):   # (median of the calls' own wall times: a mean over 20 calls = 4 ms was at the mercy of one hiccup)
                t0 = time.perf_counter()
                step(0, [xb])
                ts.append(time.perf_counter() - t0)
            sync()
            wall = float(np.median(ts))
            h.set_timing(True); step(0, [xb]); sync(); a, n, r = phases(); h.set_timing(False)
            sweep[str(b)] = {"wall_ms": wall * 1e3, "assoc_ms": a, "nn_ms": n, "factor_sums_ms": r, "evals_per_s": units * b / wall}
        extras["batch_sweep"] = sweep
        # (1b) the same sweep for the entry points the reference's callers use alone: the cost tuple (BALoss::eval_x / NOMAD's poll
        # block: iba_eval_cost) and the frozen problem's normal equations (one LM step of iba_local: iba_eval_factors)
        h.build_problem(xs_all[0][0])
        sweep2 = {}
        for b in (1, 8, 14, 64):
            xb = xs_all[1][:b]
            row = {}
            for name, fn in (("cost", h.eval_cost), ("frozen_factors", h.eval_factors)):
                for _ in range(3):
                    fn(xb)
                ts = []
                for _ in range(50):
                    t0 = time.perf_counter()
                    fn(xb)
                    ts.append(time.perf_counter() - t0)
                row[name + "_wall_ms"] = float(np.median(ts)) * 1e3
                row[name + "_evals_per_s"] = units * b / float(np.median(ts))
                # the same calls in a C loop (iba_debug_call_latency): what the reference's own caller — C++, one candidate per call — sees
                row[name + "_wall_ms_c_caller"] = h.call_latency(xb, "cost" if name == "cost" else "factors", 100)[0]
            sweep2[str(b)] = row
        extras["batch_sweep_cost_and_factors"] = sweep2
        # (2) a batch as wide as the reference's search box (iba_calib_global.yml:39-40: +-0.1 rad, +-0.3 m, +-1 on the scale)
        xw = meta["x_gt"][None, :] + np.random.default_rng(7).uniform(-1, 1, (B, 7)) * np.array([0.1, 0.1, 0.1, 0.3, 0.3, 0.3, 1.0])
        for _ in range(2):
            step(0, [xw])
        sync()
        t0 = time.perf_counter()
        for _ in range(10):
            ow = step(0, [xw])
        sync()
        tw = (time.perf_counter() - t0) / 10
        h.set_timing(True); step(0, [xw]); sync(); a, n, r = phases(); h.set_timing(False)
        extras["wide_candidates"] = {"spread": "uniform over the yml search box around x_gt", "evals_per_s": units * B / tw, "ms_per_step": tw * 1e3, "assoc_ms": a, "nn_ms": n,
                                     "factor_sums_ms": r, "mean_n_corr": float(np.mean([c.n_corr for c in ow[0]]))}
        # (2b) strong-scaling prediction on ONE GPU: the frame shard a rank of a 2 / 4 / 8-GPU job holds (100 / 50 / 25 keyframes of the
        # 200), timed as a rank's step: iba_eval_full_partial (one launch chain of up to 512 candidates: iba_create_options.max_chain_batch),
        # ONE ncclAllReduce of the B x 64 doubles on a one-rank RCCL communicator made by the library (iba_comm_init_all: the launch and
        # kernel latency of the collective are in the figure, the xGMI hops of a real 8-rank ring are not), the D2H of the block into pinned
        # memory, a polled wait. Speed-up = candidates/s of the shard / candidates/s of the 200-keyframe handle timed the same way.
        if world == 1 and args.scaling == "strong" and args.frames >= 64:
            emu = {}
            comm = (C.c_void_p * 1)()
            devs = (C.c_int32 * 1)(local_rank)
            L.iba_comm_init_all.argtypes = [C.POINTER(C.c_void_p), C.POINTER(C.c_int32), C.c_int32]
            L.iba_comm_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
            L.iba_comm_destroy.argtypes = [C.c_void_p]
            have_comm = L.iba_comm_init_all(comm, devs, 1) == 0
            t_full = {}
            for nsh in (1, 2, 4, 8):
                fe = args.frames // nsh
                hs = h if nsh == 1 else pkg.IbaHandle(prob, params, device=local_rank, frame_begin=0, frame_end=fe)
                row = {"frames": fe}
                for mult in (1, 2, 4, 8):
                    Bm = B * mult
                    xm = np.vstack([xs_all[i % len(xs_all)] for i in range(mult)])
                    dm = torch.zeros(Bm * stride, dtype=torch.float64, device=dev)
                    hm = torch.zeros(Bm * stride, dtype=torch.float64).pin_memory()
                    cs_ = torch.cuda.current_stream()

                    def one(with_collective):
                        hs.eval_full_partial(xm, dm.data_ptr(), st)
                        if with_collective and have_comm:
                            L.iba_comm_allreduce(comm[0], C.c_void_p(dm.data_ptr()), C.c_int32(Bm), C.c_void_p(st))
                        hm.copy_(dm, non_blocking=True)
                        t_spin = time.perf_counter()
                        while not cs_.query():
                            if time.perf_counter() - t_spin > 5e-3:
                                cs_.synchronize()
                                break
                    res_row = {}
                    for tag, wc in (("", False), ("_with_allreduce", True)):
                        for _ in range(5):
                            one(wc)
                        ts = []
                        for _ in range(20):
                            t0 = time.perf_counter(); one(wc); ts.append(time.perf_counter() - t0)
                        res_row["ms_per_call" + tag] = float(np.median(ts)) * 1e3
                    res_row["candidates_per_s_this_shard"] = Bm / (res_row["ms_per_call_with_allreduce"] * 1e-3)
                    row["B%d" % Bm] = res_row
                    if nsh == 1:
                        t_full[Bm] = res_row["ms_per_call_with_allreduce"] * 1e-3
                emu[str(nsh)] = row
                if nsh > 1:
                    hs.close()
            base_rate = B / t_full[B]
            for nsh in (2, 4, 8):
                r_ = emu[str(nsh)]
                r_["predicted_speedup_same_batch_64"] = r_["B%d" % B]["candidates_per_s_this_shard"] / base_rate
                r_["predicted_speedup_batch_64N"] = r_["B%d" % (B * nsh)]["candidates_per_s_this_shard"] / base_rate
                r_["predicted_speedup_batch_512"] = r_["B%d" % (B * 8)]["candidates_per_s_this_shard"] / base_rate
            emu["note"] = ("speed-ups against the 200-keyframe handle at 64 candidates per call, the one-rank all-reduce and the D2H included on both sides" if have_comm
                           else "librccl could not be loaded: the all-reduce is missing from these figures")
            emu["single_gpu_rate_by_batch"] = {str(k): k / v for k, v in t_full.items()}
            if have_comm:
                L.iba_comm_destroy(comm[0])
            extras["strong_shard_emulation"] = emu
        # (3) same workload with the local planes refitted inside every evaluation, as the reference does
        other = abi.reference_yaml_params(plane_cache=1 - args.plane_cache)
        h.set_params(other)
        for i in range(2):
            h.eval_full_partial(xs_all[i], d_part.data_ptr(), st)
        sync()
        t0 = time.perf_counter()
        nrep = 5
        for i in range(nrep):
            h.eval_full_partial(xs_all[i % len(xs_all)], d_part.data_ptr(), st)
            if use_dist:
                dist.all_reduce(d_part[: B * stride])
            d_part[: B * stride].cpu()
        sync()
        t_other = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([t_other], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            t_other = float(t.item())
        res["value_plane_refit" if args.plane_cache else "value_plane_cache"] = units * B * nrep / t_other
        if args.plane_cache:   # the like-for-like roofline figure: what the reference computes per evaluation, over the whole step's time
            res["roofline"]["effective_vs_reference_formulation"]["like_for_like"] = (B * nrep * per_eval / t_other / 1e9) / HBM_PEAK_GBS
        h.set_params(params)
        # (3b) the plane memo itself: what a change of a plane parameter costs (every scan point of this rank refitted)
        moved = abi.reference_yaml_params(plane_cache=1)
        moved.norm_radius = params.norm_radius * 1.01; moved.neigh_radius = params.neigh_radius * 1.01
        h.set_params(moved); h.set_params(abi.reference_yaml_params(plane_cache=1))   # warm
        t0 = time.perf_counter(); h.set_params(moved); tm = time.perf_counter() - t0
        extras["plane_memo"] = {"ms": tm * 1e3, "fits": int(prob.n_points // max(world, 1)) if args.scaling == "weak" else int(prob.n_points), "note": "iba_set_params with a changed norm_radius: iba_plane_kernel over every scan point, synchronous"}
        h.set_params(params)
        if world == 1:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import lm_ref
            # (3c) the reference's real scan size: iba_global loads FULL KITTI scans (readPointCloud without skip /
            # only_positive_x, iba_global.cpp:490-502; ~120 k points): the same keyframes and keypoints over 120 k-point scans
            # (kd depth is capped at 11: 59-point leaves). 40 keyframes: the per-keyframe cost is what is measured.
            # (r05: the whole 200 keyframes on the device — 24 M points — instead of 40 scaled by 5. The scene generator ray-casts 40 of
            # them (its cost is minutes beyond that) and the trajectory is tiled 5 x: every keyframe has its own scan, tree, planes and
            # anchored lists in HBM; only the geometry repeats.)
            kf0 = 40
            big40, bmeta = synth.make_scene(n_frames=kf0, pts_per_frame=120000, n_keypoints=KEYPOINTS, seed=0)
            big = synth.tile_scene(big40, bmeta, 5)[0]
            kf = big.n_frames
            del big40
            hb = pkg.IbaHandle(big, params, device=local_rank)
            # the headline's own step (r05: this region used to go through the partial entry point and a torch D2H copy per step, ~50 us
            # of harness on a 1.6 ms step): iba_eval_full — launch chain, D2H of the 64-double blocks, host finalisation — on 4 candidate
            # sets of the headline's spread used in turn, 8 settling steps, K = 20 timed ones between two synchronisations
            rk = np.random.default_rng(2)
            xk_all = [synth.perturb(bmeta["x_gt"], rk, n=B) for _ in range(4)]
            for i in range(8):
                eval_full_lean(xk_all[i % 4], hb)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(20):
                ck, _nk = eval_full_lean(xk_all[i % 4], hb)
            torch.cuda.synchronize()
            tk = (time.perf_counter() - t0) / 20
            hb.set_timing(True); eval_full_lean(xk_all[0], hb); torch.cuda.synchronize()
            pa, pn, pr = C.c_float(0), C.c_float(0), C.c_float(0)
            L.iba_last_phase_ms(hb.h, C.byref(pa), C.byref(pn), C.byref(pr))
            per_eval_k = float(np.mean([algorithmic_bytes(hb.n_points, kf, hb.n_keypoints, c.n_corr, c.cnt_3d_3d, n_slots) for c in ck]))
            extras["kitti_raw_shape"] = {
                "keyframes": kf, "points_per_scan": 120000, "total_points": int(hb.n_points), "ms_per_step": tk * 1e3, "evals_per_s": B / tk,
                "kernel_ms": {"association (pairs + assoc2)": pa.value, "iba_nn_kernel": pn.value, "factor + sums": pr.value},
                "algorithmic_bytes_per_eval": per_eval_k, "effective_vs_reference_formulation_ratio_to_hbm_peak": (B * per_eval_k / ((pa.value + pn.value) * 1e-3) / 1e9) / HBM_PEAK_GBS,
                "mean_n_corr": float(np.mean([c.n_corr for c in ck])), "shared_pair_search": bool(hb.last_path),
                "note": "measured at the full 200 keyframes x 120 k points (40 ray-cast keyframes tiled 5 x), not scaled; the headline's step (iba_eval_full, 4 candidate sets in turn, 20 timed steps)"}
            hb.close()
            del big
            # (4a) distance from the PLANTED extrinsic needs a scene whose optimum is the planted one: no keypoint noise, no range noise
            clean, cmeta = synth.make_scene(n_frames=60, pts_per_frame=args.pts, n_keypoints=KEYPOINTS, seed=0, kp_noise=0.0, range_noise=0.0)
            hc_ = pkg.IbaHandle(clean, params, device=local_rank)
            xc0 = synth.perturb(cmeta["x_gt"], np.random.default_rng(5), rot=1e-3, trans=0.01, scale_rel=3e-3, n=1)[0]
            xcf, lrc = hc_.calibrate_lm(xc0, max_outer_iterations=10)
            ec0 = lm_ref.se3_error(xc0, cmeta["x_gt"], synth.sim3_exp)
            ec1 = lm_ref.se3_error(xcf, cmeta["x_gt"], synth.sim3_exp)
            res["final_se3_noise_free_scene"] = {"keyframes": 60, "start_err_rad_m": [ec0[0], ec0[1]], "final_err_rad_m_vs_planted": [ec1[0], ec1[1]],
                                                  "outer_iterations": lrc.outer_iterations, "evaluations": lrc.evaluations,
                                                  "note": "keypoints = exact projections, scans without range noise. The end point is still 0.2 mrad / 3 mm from the planted extrinsic: the objective is not zero there "
                                                          "(tools/clean_scene_probe.py: cost 3.1e3, |b| 2.5e4 at x_gt) because a MapPoint is a scan point of the keyframe that created it and lies BETWEEN the scan points of "
                                                          "the other keyframes that observe it - the 3d-3d point-to-point factors (1.4 k of 19 k) and the nearest-projection association carry that sampling offset. "
                                                          "Distance from the planted extrinsic therefore measures the objective on a sampled scene, not the solver; device = CPU is asserted in the tests"}
            hc_.close()
            # (4) final SE(3): iba_local's outer loop + LM on the device path from a perturbed start
            x0 = synth.perturb(meta["x_gt"], np.random.default_rng(5), rot=1e-3, trans=0.01, scale_rel=3e-3, n=1)[0]
            t0 = time.perf_counter()
            xf, lr = h.calibrate_lm(x0, max_outer_iterations=10)
            e0 = lm_ref.se3_error(x0, meta["x_gt"], synth.sim3_exp)
            e1 = lm_ref.se3_error(xf, meta["x_gt"], synth.sim3_exp)
            res["final_se3"] = {"start_err_rad_m": [e0[0], e0[1]], "final_err_rad_m_vs_planted": [e1[0], e1[1]], "outer_iterations": lr.outer_iterations,
                                "evaluations": lr.evaluations, "seconds": time.perf_counter() - t0, "initial_cost": lr.initial_cost, "final_cost": lr.final_cost,
                                "note": "parity of the final SE(3) with the CPU path (1e-4 rad / 1e-3 m) is asserted in tests/test_gpu_calibrate.py and, at 300 keyframes, tests/test_gpu_golden_and_shapes.py"}
            # (5) time-to-calibration of the two-stage pipeline (README steps 3 + 4): batch-aware MADS on the cost path from a
            # start as far off as a hand-eye initialiser may be inside the reference's search box, then the LM polish
            xg0 = meta["x_gt"] + np.array([0.009, -0.006, 0.005, 0.06, -0.04, 0.05, 0.4])
            t0 = time.perf_counter()
            xg, mr, mtr, mbs = h.calibrate_mads(xg0, record=True, max_bb_eval=100000)
            t_mads = time.perf_counter() - t0
            xl, lr2 = h.calibrate_lm(xg, max_outer_iterations=10)
            t_all = time.perf_counter() - t0
            eg0 = lm_ref.se3_error(xg0, meta["x_gt"], synth.sim3_exp)
            eg1 = lm_ref.se3_error(xg, meta["x_gt"], synth.sim3_exp)
            eg2 = lm_ref.se3_error(xl, meta["x_gt"], synth.sim3_exp)
            res["global_then_local"] = {"start_err_rad_m": [eg0[0], eg0[1]], "after_mads_err_rad_m": [eg1[0], eg1[1]], "after_lm_err_rad_m": [eg2[0], eg2[1]],
                                        "scale_start_mads_lm_planted": [float(xg0[6]), float(xg[6]), float(xl[6]), float(meta["x_gt"][6])],
                                        "mads_evaluations": mr.evaluations, "mads_batches": mr.batches, "mads_restarts": mr.restarts, "mads_feasible": mr.feasible,
                                        "mads_f": mr.f, "mads_seconds": t_mads, "total_seconds": t_all,
                                        "note": "reference budget: 5000 NOMAD evaluations on one CPU thread (iba_calib_global.yml:42) at ~2 evals/s"}
            res["_lm_check_start"] = [float(v) for v in xg]
            # (5a) the REFERENCE's experiment: the same start under the budget the reference's yml gives NOMAD
            # (config/calib/00/iba_calib_global.yml:40-47: max_bbeval 5000, lb / ub, init_frame, min_mesh, seed — read through
            # iba_run_config_mads from the committed values of that file), then the LM polish; what 5000 evaluations reach, how long
            # they take here, and how long they take the reference's one CPU thread at the rate measured below
            try:
                gold = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_configs.json")))["calib"]["00"]["values"]["runtime"]
                t0 = time.perf_counter()
                xb, mb = h.calibrate_mads(xg0, max_bb_eval=int(gold["max_bbeval"]), lb=xg0 + np.array(gold["lb"]), ub=xg0 + np.array(gold["ub"]), init_frame=np.array(gold["init_frame"]),
                                          min_mesh=float(gold["min_mesh"]), he_threshold=float(gold["he_threshold"]), valid_rate=float(gold["valid_rate"]), seed=int(gold["seed"]))
                t_mb = time.perf_counter() - t0
                xbl, lrb = h.calibrate_lm(xb, max_outer_iterations=10)
                t_ab = time.perf_counter() - t0
                eb1 = lm_ref.se3_error(xb, meta["x_gt"], synth.sim3_exp)
                eb2 = lm_ref.se3_error(xbl, meta["x_gt"], synth.sim3_exp)
                extras["global_then_local_ref_budget"] = {
                    "max_bb_eval": int(gold["max_bbeval"]), "start_err_rad_m": [eg0[0], eg0[1]], "after_mads_err_rad_m": [eb1[0], eb1[1]], "after_lm_err_rad_m": [eb2[0], eb2[1]],
                    "scale_start_mads_lm_planted": [float(xg0[6]), float(xb[6]), float(xbl[6]), float(meta["x_gt"][6])],
                    "mads_evaluations": mb.evaluations, "mads_batches": mb.batches, "mads_feasible": mb.feasible, "mads_stop_reason": mb.stop_reason, "mads_f": mb.f,
                    "mads_seconds": t_mb, "total_seconds": t_ab,
                    "config": "runtime keys of config/calib/00/iba_calib_global.yml (tests/golden/reference_configs.json): lb / ub around the start, init_frame, min_mesh, he_threshold, valid_rate, seed"}
            except Exception as e:   # (the extras never take the record down)
                extras["global_then_local_ref_budget"] = {"error": repr(e)}
            # (5b) what an optimiser really gets: the recorded black-box calls of that MADS run (every x, every batch boundary)
            # replayed through iba_eval_bbo on a FRESH handle, every cross-call mechanism live and inside the clock (pair searches,
            # pair-list reuse, anchor rebuilds, clustering of multi-centre batches): evaluations/s over the whole trace and the
            # share of calls / time per association path
            hr = pkg.IbaHandle(prob, params, device=local_rank)
            mo = pkg.mads_options(xg0)
            Lr = hr.lib
            Lr.iba_debug_last_path.argtypes = [C.c_void_p]
            bbo_buf = (pkg.IbaBbo * pkg.IBA_MAX_BATCH)()
            xr = np.ascontiguousarray(mtr[:, :7])
            at = 0
            t_by_path, n_by_path, e_by_path = {}, {}, {}
            t0 = time.perf_counter()
            for nb_ in mbs:
                nb_ = int(nb_)
                t1 = time.perf_counter()
                st_ = Lr.iba_eval_bbo(hr.h, C.c_void_p(xr[at:at + nb_].ctypes.data), C.c_int32(nb_), C.c_double(mo.he_threshold), C.c_double(mo.valid_rate), bbo_buf)
                t2 = time.perf_counter()
                if st_ != 0:
                    raise pkg.IbaError(st_, Lr.iba_last_error(hr.h).decode())
                pth = int(Lr.iba_debug_last_path(hr.h))
                t_by_path[pth] = t_by_path.get(pth, 0.0) + (t2 - t1); n_by_path[pth] = n_by_path.get(pth, 0) + 1; e_by_path[pth] = e_by_path.get(pth, 0) + nb_
                at += nb_
            t_rep = time.perf_counter() - t0
            names = {0: "per-candidate association (iba_assoc_kernel)", 1: "one shared pair search", 2: "clustered: one pair search per tight group"}
            extras["mads_trace_replay"] = {
                "evaluations": int(at), "batches": int(len(mbs)), "mean_batch": float(np.mean(mbs)), "seconds": t_rep, "evals_per_s": at / t_rep,
                "by_path": {names.get(k, str(k)): {"batches": n_by_path[k], "evaluations": e_by_path[k], "seconds": t_by_path[k], "evals_per_s": e_by_path[k] / t_by_path[k]} for k in sorted(t_by_path)},
                "anchor_builds": hr.anchor_builds, "pair_searches": hr.pairs_builds,
                "what": "cost tuple only (iba_eval_bbo = what BALoss::eval_x returns, iba_global.cpp:377-396); compare config.candidate_spread of the headline: "
                        "this is the optimiser's own sequence of batches from 11.8 mrad / 8.7 cm / 4x scale off down to the minimum mesh"}
            hr.close()
            # (6) ORB-only extrinsic BA on a planted edge list of the C2 scale: 200 keyframes x 600 observations
            import ba_scene
            ba = importlib.import_module(PKG + ".ba")
            bprob, bx_gt = ba_scene.make(n_frames=200, pts_per_frame=600, seed=1, ba=ba)
            bh = ba.BaHandle(bprob)
            bx0 = bx_gt + np.array([0.008, -0.006, 0.005, 0.03, -0.02, 0.02, 0.3])
            bh.eval(bx0, want_chi2=False)
            t0 = time.perf_counter()
            for _ in range(20):
                bh.eval(bx0, want_chi2=False)
            t_lin = (time.perf_counter() - t0) / 20
            t0 = time.perf_counter()
            bx, br = bh.optimize(bx0)
            t_opt = time.perf_counter() - t0
            res["orb_only_ba"] = {"edges": int(br.n_edges), "inliers": int(br.n_inliers), "linearisation_ms": t_lin * 1e3,
                                  "edges_per_s": br.n_edges / t_lin, "optimize_seconds": t_opt, "device_evaluations": int(br.evaluations),
                                  "err_vs_planted": {"rot_rad": float(np.linalg.norm(bx[:3] - bx_gt[:3])), "trans_m": float(np.linalg.norm(bx[3:6] - bx_gt[3:6])), "scale": float(abs(bx[6] - bx_gt[6]))}}
            bh.close()
        # (1c) SUSTAINED regions next to the headline: >= 10 s each (r06; 1.5 s in r05) of back-to-back steps, run LAST so that an outside sampler of GPU activity lands inside them, whose 64 candidates are drawn afresh
        # every step — (a) around the planted extrinsic (the headline's own workload without its four fixed candidate sets: every step
        # runs its own pair search on candidates it has never seen), (b) around a centre that DRIFTS (a random walk of 0.15 mrad / 1.5 mm
        # per step, reflected at 6 mrad / 6 cm from the planted extrinsic): the anchored lists are rebuilt as the centre leaves them.
        # A drifted centre is a LIGHTER workload, not a faster machine — away from the planted extrinsic fewer scan points meet a keypoint
        # within max_pixel_dist, so every later stage has less to do: the mean correspondence count is reported beside each rate, and only
        # (a) compares with the headline. evaluations/s over the whole region and min / median / max over windows of 100 steps.
        def sustained(drift, n_sets=40000):
            rs = np.random.default_rng(99)
            centre = meta["x_gt"].copy()
            sig = np.array([1.5e-4] * 3 + [1.5e-3] * 3 + [2e-4 * abs(meta["x_gt"][6])])
            box = np.array([6e-3] * 3 + [6e-2] * 3 + [0.02 * abs(meta["x_gt"][6])])
            sets = []
            for _ in range(n_sets):   # (generated BEFORE the clock: 60 us of numpy per set are not part of the path)
                if drift:
                    centre = centre + rs.normal(size=7) * sig
                    off = centre - meta["x_gt"]
                    centre = meta["x_gt"] + np.where(np.abs(off) > box, np.sign(off) * (2 * box - np.abs(off)), off)
                sets.append(synth.perturb(centre, rs, n=B))
            n_s, wins, ncs, ab0, pb0 = 0, [], [], h.anchor_builds, h.pairs_builds
            sync()
            t00 = time.perf_counter()
            tw0 = t00
            while n_s < n_sets:
                o_ = step(n_s, sets)
                n_s += 1
                if n_s % 100 == 0:
                    tnow = time.perf_counter()
                    wins.append(100 * B / (tnow - tw0))
                    ncs.append(float(np.mean([c.n_corr for c in o_[0]])))
                    tw0 = time.perf_counter()
                    if tnow - t00 > SUSTAIN_S and n_s >= 300:
                        break
            sync()
            t_s = time.perf_counter() - t00
            return {"seconds": t_s, "steps": n_s, "evals_per_s": n_s * B / t_s, "window_steps": 100,
                    "window_evals_per_s": {"min": float(np.min(wins)), "median": float(np.median(wins)), "max": float(np.max(wins))},
                    "mean_n_corr_sampled_every_100_steps": float(np.mean(ncs)), "anchor_builds": h.anchor_builds - ab0, "pair_searches": h.pairs_builds - pb0}
        extras["sustained"] = {"fresh_candidates_fixed_centre": sustained(False), "fresh_candidates_drifting_centre": sustained(True),
                               "headline_mean_n_corr": res["config"]["mean_n_corr"],
                               "what": "64 fresh candidates (0.5 mrad / 5 mm / 0.1 %) per step, every set generated before the clock starts and used once. The drifting "
                                       "centre wanders up to 6 mrad / 6 cm from the planted extrinsic: fewer correspondences, less work per evaluation (see mean_n_corr) - only the fixed centre compares with the headline"}
        res["extras"] = extras
    stage("extras done")

    if args.full and rank == 0 and n_gpus == 1 and not args.no_cpu_baseline:
        # ---- CPU baseline: the oracle — a port of the reference algorithm, per-evaluation 2-D tree rebuild included — on
        #      this box's host cores: x0 and 16 seeded perturbations, cost tuple + normal equations each; 1 warm-up, then the
        #      median over the 17 candidates on ONE thread (what the reference's NOMAD loop runs, iba_global.cpp:385) and the
        #      2 passes over them with OpenMP over keyframes (iba_func.cpp:203) at 8 and min(cores, 32) threads ----
        from oracle import binding as ob
        o = ob.Oracle(base)
        ncpu = ob.max_threads()
        cand = np.vstack([meta["x_gt"][None], synth.perturb(meta["x_gt"], np.random.default_rng(16), n=16)])

        def one(x, nt):
            t0 = time.perf_counter()
            o.eval_cost(params, x, nthreads=nt)
            o.eval_normal(params, x, nthreads=nt)
            return time.perf_counter() - t0

        one(cand[0], 1)                                      # warm-up (first touch of the trees and scans)
        t1 = [one(x, 1) for x in cand]
        single = 1.0 / float(np.median(t1))
        by_threads = {"1": single}
        best_nt, best = 1, single
        for nt in sorted(set([8, min(ncpu, 32)])):   # (r06: bounded to ~30 s — the pass with one thread per keyframe of r05 ran at 0.5 evals/s for three minutes)
            if nt <= 1 or nt > ncpu:
                continue
            one(cand[0], nt)
            reps = []
            for _ in range(2):
                t0 = time.perf_counter()
                for x in cand:
                    one(x, nt)
                reps.append((time.perf_counter() - t0) / len(cand))
            rate = 1.0 / float(np.median(reps))
            by_threads[str(nt)] = rate
            if rate > best:
                best_nt, best = nt, rate
        if "extras" in res and "mads_evaluations" in res["extras"].get("global_then_local_ref_budget", {}):
            rb = res["extras"]["global_then_local_ref_budget"]
            # (the cost tuple alone is what NOMAD's loop evaluates; the port's rate above is cost + normal equations: an upper bound of the time)
            rb["cpu_one_thread_projection_seconds"] = rb["mads_evaluations"] / single
            rb["cpu_projection_note"] = "evaluations / the one-thread rate of the CPU port measured in this run (cost tuple + normal equations per evaluation: the reference's loop evaluates the cost tuple alone, roughly half of it)"
        res["cpu_baseline"] = {
            "value": best, "unit": "evals/s", "cores": best_nt, "kind": "port",
            "sample": "x0 + 16 seeded perturbations (cost tuple + normal equations each), 1 warm-up; one thread: median over the 17 candidates; "
                      "OpenMP over keyframes with the reference's critical sections (iba_func.cpp:203, iba_global.cpp:239,318; iba_local.cpp:162): median of 2 passes at 8 and at min(host cores, 32) threads; best thread count reported",
            "evals_per_s_by_threads": by_threads, "single_thread_evals_per_s": single,
            "single_thread_note": "1 thread = what the reference's NOMAD loop runs (iba_global.cpp:385)", "host_cores": ncpu,
        }
        # the LM stage's shift on this scene: the SAME LM on the CPU oracle from the MADS end-point. If it lands
        # where the device LM lands, the shift is the iba_local objective's bias on this synthetic scene, not a parity defect.
        if "_lm_check_start" in res:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import lm_ref
            xg = np.array(res["_lm_check_start"])

            def ev(x):
                n = o.eval_factors(params, x)[0]
                return n.H_np(), n.b_np(), n.cost

            t0 = time.perf_counter()
            xc, sc = lm_ref.calibrate_lm(xg, lambda x: o.build_problem(params, x), ev, max_outer=10)
            ec = lm_ref.se3_error(xc, meta["x_gt"], synth.sim3_exp)
            xl2, _ = h.calibrate_lm(xg, max_outer_iterations=10)
            ed = lm_ref.se3_error(xl2, xc, synth.sim3_exp)
            res["global_then_local"]["cpu_lm_from_the_same_start"] = {
                "after_lm_err_rad_m_vs_planted": [ec[0], ec[1]], "device_vs_cpu_end_point_rad_m": [ed[0], ed[1]], "cpu_seconds": time.perf_counter() - t0,
                "reading": "device and CPU LM end at the same point: the shift away from the planted extrinsic is the iba_local objective's own optimum on this scene"}
    res.pop("_lm_check_start", None)
    if rank == 0:   # written (and flushed) before any teardown
        os.write(fd_record, (json.dumps(res) + "\n").encode())
    h.close()
    if grp is not None:
        grp.close()
    if use_dist:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

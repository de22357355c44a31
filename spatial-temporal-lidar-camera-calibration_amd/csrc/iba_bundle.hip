// Bundle adjustment (include/iba_mi355x.h, iba_bundle*): the C ABI, the result object's accessors and the launch chains of a call. The kernels are
// iba_bundle_kernels.hpp, the arithmetic iba_bundle_math.hpp, the host rules (argument checks, the plan, the flat tables, the host restatement)
// iba_bundle_host.hpp. A per-call unit (iba_call.hpp); per chunk of jobs: tables up, one launch chain per LM evaluation with ONE word read back per
// step, results down. The result is host memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_bundle_host.hpp"
#include "iba_bundle_kernels.hpp"
#include "iba_call.hpp"
#include "iba_device_buf.hpp"

using iba::DevBuf;
namespace bd = iba::bundle;
using bd::Ctl;
using bd::JobRec;

namespace {
thread_local iba::CallError t_err;

constexpr uint64_t kBudgetBytes = 1ull << 30;

struct Limits { uint64_t budget; bool timing; };
iba_status limits(int device, Limits* l) {
    IBA_CALL_TRY(iba::call_budget(device, kBudgetBytes, "IBA_BUNDLE_BUDGET", &l->budget));
    l->timing = iba::debug_env("IBA_BUNDLE_TIMING") != nullptr;
    return IBA_OK;
}
std::vector<int32_t> cut_jobs(const iba_bundle_job* jobs, const std::vector<bd::Plan>& plans, int32_t B, bool stages, bool eval, uint64_t budget) {
    std::vector<uint64_t> bytes((size_t)B);
    for (int32_t j = 0; j < B; ++j) bytes[(size_t)j] = bd::job_bytes(jobs[j], plans[(size_t)j], stages, eval);
    return iba::cut_chunks(bytes, budget);
}

struct DevTables {
#define X(type, name, up) DevBuf<type> name;
    IBA_BUNDLE_TABLES(X)
#undef X
};
// the chunk's tables on the device: what the builder filled is copied, the rest is zeroed
iba_status upload(const bd::HostTables& h, DevTables* d, bd::Tab* t, hipStream_t st) {
#define X(type, name, up)                                                                                                          \
    IBA_CALL_TRY(d->name.alloc(h.n.name));                                                                                         \
    if (up) { if (h.n.name) IBA_CALL_TRY(hipMemcpyAsync(d->name.p, h.name.data(), sizeof(type) * h.n.name, hipMemcpyHostToDevice, st)); } \
    else IBA_CALL_TRY(hipMemsetAsync(d->name.p, 0, sizeof(type) * std::max<size_t>(h.n.name, 1), st));                             \
    t->name = h.n.name ? d->name.p : nullptr;
    IBA_BUNDLE_TABLES(X)
#undef X
    return IBA_OK;
}
template <class T>
iba_status fetch(std::vector<T>* v, const DevBuf<T>& d, size_t n, hipStream_t st) {
    v->resize(n);
    if (n) IBA_CALL_TRY(hipMemcpyAsync(v->data(), d.p, sizeof(T) * n, hipMemcpyDeviceToHost, st));
    return IBA_OK;
}

inline uint32_t blocks(int n, int per) { return (uint32_t)((n + per - 1) / per); }

// the first part of a step's chain: the evaluation, its sums, the sequencer's first half, and the reduced system of the jobs that propose
iba_status launch_front(const bd::Tab& t, const bd::HostTables& h, const bd::DevOpt& o, hipStream_t st) {
    const dim3 th(bd::kThreads);
    if (h.nE) hipLaunchKernelGGL(bd::edge_kernel, dim3(blocks(h.nE, bd::kThreads)), th, 0, st, t, h.nE, o);
    if (h.nP) hipLaunchKernelGGL(bd::point_kernel, dim3(blocks(h.nP, bd::kThreads)), th, 0, st, t, h.nP);
    if (h.nC) hipLaunchKernelGGL(bd::camera_kernel, dim3(blocks(h.nC, bd::kThreads / bd::kWave)), th, 0, st, t, h.nC);
    hipLaunchKernelGGL(bd::front_kernel, dim3((uint32_t)std::min<int32_t>(h.nJ, bd::kMaxGrid)), th, 0, st, t, h.nJ, o);
    if (h.nP) hipLaunchKernelGGL(bd::inverse_kernel, dim3(blocks(h.nP, bd::kThreads)), th, 0, st, t, h.nP);
    if (h.nB) hipLaunchKernelGGL(bd::block_kernel, dim3(blocks(h.nB, bd::kThreads / bd::kWave)), th, 0, st, t, h.nB);
    IBA_CALL_TRY(hipGetLastError());
    return IBA_OK;
}
// the second part: the solve, the steps and trial estimates, the sequencer's second half
iba_status launch_back(const bd::Tab& t, const bd::HostTables& h, const bd::DevOpt& o, hipStream_t st) {
    const dim3 th(bd::kThreads);
    if (h.nB) hipLaunchKernelGGL(bd::solve_kernel, dim3((uint32_t)std::min<int32_t>(h.nJ, bd::kMaxGrid)), dim3(bd::kSolveThreads), 0, st, t, h.nJ);
    if (h.nP + h.nC) hipLaunchKernelGGL(bd::update_kernel, dim3(blocks(h.nP + h.nC, bd::kThreads)), th, 0, st, t, h.nP, h.nC);
    hipLaunchKernelGGL(bd::back_kernel, dim3(blocks(h.nJ, bd::kThreads)), th, 0, st, t, h.nJ, o);
    IBA_CALL_TRY(hipGetLastError());
    return IBA_OK;
}

iba_status optimize_chunk(iba_bundle_batch* res, const iba_bundle_job* jobs, const std::vector<bd::Plan>& plans, int32_t a, int32_t b, const Limits& lim) {
    hipStream_t st = nullptr;
    bd::HostTables h;
    iba::PinnedBuf<int32_t> running;
    DevTables d;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);
    const bool stages = res->opt.keep_stages != 0;
    if (!bd::build_tables(jobs, plans, a, b, nullptr, stages, false, &h)) return t_err.fail(IBA_ERR_UNSUPPORTED, "a chunk of 2^27 cameras, points or edges, or 2^31 blocks or items, or more");
    bd::Tab t{};
    if (const iba_status e = upload(h, &d, &t, st)) return e;
    IBA_CALL_TRY(running.alloc(1));
    const bd::DevOpt o = bd::dev_options(res->opt);
    if (lim.timing) { IBA_CALL_TRY(ev.create(2)); IBA_CALL_TRY(hipEventRecord(ev.e[0], st)); }
    const int bound = bd::max_steps(o);
    for (int s = 0; s < bound; ++s) {
        if (const iba_status e = launch_front(t, h, o, st)) return e;
        if (const iba_status e = launch_back(t, h, o, st)) return e;
        IBA_CALL_TRY(hipMemcpyAsync(running.p, d.running.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipStreamSynchronize(st));
        if (!running.p[0]) break;
    }
    if (lim.timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    if (const iba_status e = fetch(&h.ctl, d.ctl, h.n.ctl, st)) return e;
    if (const iba_status e = fetch(&h.T, d.T, h.n.T, st)) return e;
    if (const iba_status e = fetch(&h.X, d.X, h.n.X, st)) return e;
    if (const iba_status e = fetch(&h.outlier, d.outlier, h.n.outlier, st)) return e;
    if (const iba_status e = fetch(&h.chi2f, d.chi2f, h.n.chi2f, st)) return e;
    if (const iba_status e = fetch(&h.stT, d.stT, h.n.stT, st)) return e;
    if (const iba_status e = fetch(&h.stX, d.stX, h.n.stX, st)) return e;
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (lim.timing) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); res->kernel_ms += ms; }
    bd::collect(h, res->opt, a, res);
    return IBA_OK;
}

iba_status eval_chunk(const iba_bundle_job* jobs, const std::vector<bd::Plan>& plans, int32_t a, int32_t b, const uint8_t* const* active, const bd::DevOpt& o, iba_bundle_eval_out* outs) {
    hipStream_t st = nullptr;
    bd::HostTables h;
    std::vector<double> S_copy;
    DevTables d;
    iba::SyncOnExit sync(st);
    if (!bd::build_tables(jobs, plans, a, b, active, false, true, &h)) return t_err.fail(IBA_ERR_UNSUPPORTED, "a chunk of 2^27 cameras, points or edges, or 2^31 blocks or items, or more");
    bd::Tab t{};
    if (const iba_status e = upload(h, &d, &t, st)) return e;
    if (const iba_status e = launch_front(t, h, o, st)) return e;
    if (const iba_status e = fetch(&S_copy, d.S, h.n.S, st)) return e;
    if (const iba_status e = launch_back(t, h, o, st)) return e;
    if (const iba_status e = fetch(&h.ctl, d.ctl, h.n.ctl, st)) return e;
    if (const iba_status e = fetch(&h.cam_sums, d.cam_sums, h.n.cam_sums, st)) return e;
    if (const iba_status e = fetch(&h.cam_cnt, d.cam_cnt, h.n.cam_cnt, st)) return e;
    if (const iba_status e = fetch(&h.bs, d.bs, h.n.bs, st)) return e;
    if (const iba_status e = fetch(&h.dp, d.dp, h.n.dp, st)) return e;
    if (const iba_status e = fetch(&h.pt_sums, d.pt_sums, h.n.pt_sums, st)) return e;
    if (const iba_status e = fetch(&h.pt_cnt, d.pt_cnt, h.n.pt_cnt, st)) return e;
    if (const iba_status e = fetch(&h.dl, d.dl, h.n.dl, st)) return e;
    if (const iba_status e = fetch(&h.chi2d, d.chi2d, h.n.chi2d, st)) return e;
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    bd::collect_eval(h, S_copy, a, outs);
    return IBA_OK;
}

iba_status run(const char* name, const iba_bundle_job* jobs, int32_t B, const iba_bundle_options* opt, int device, bool on_host, iba_bundle_batch** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    std::vector<bd::Plan> plans;
    std::string why = bd::check_options(opt);
    if (why.empty()) why = bd::check_jobs(jobs, B, &plans);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_bundle_batch* res = new iba_bundle_batch();
    res->opt = *opt;
    res->job.resize((size_t)B);
    iba_status s = IBA_OK;
    if (on_host) {
        bd::host_call(jobs, plans, B, *opt, res);
    } else {
        Limits lim{};
        s = limits(device, &lim);
        const std::vector<int32_t> cut = cut_jobs(jobs, plans, B, opt->keep_stages != 0, false, lim.budget);
        for (size_t c = 0; c + 1 < cut.size() && s == IBA_OK; ++c) {
            s = optimize_chunk(res, jobs, plans, cut[c], cut[c + 1], lim);
            ++res->chunks;
        }
    }
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

iba_status check_eval(const std::string& who, const iba_bundle_job* jobs, int32_t B, double lambda, const iba_bundle_eval_out* outs, std::vector<bd::Plan>* plans) {
    if (!outs) return t_err.fail(IBA_ERR_INVALID_ARG, who + "outs is NULL");
    if (!std::isfinite(lambda) || lambda < 0.0) return t_err.fail(IBA_ERR_INVALID_ARG, who + "lambda is not finite or < 0");
    const std::string why = bd::check_jobs(jobs, B, plans);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    return IBA_OK;
}

iba_status check_job_index(const iba_bundle_batch* r, int32_t job, const std::string& who) {
    return t_err.check_index(!r, job, r ? r->job.size() : 0, who, "job");
}

}  // namespace

extern "C" {

const char* iba_bundle_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_bundle_options(iba_bundle_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_bundle_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->rounds = 2; opt->iterations[0] = 5; opt->iterations[1] = 10; opt->robust_rounds = 1;
    opt->chi2_threshold = 5.991f; opt->huber_delta = bd::local_delta(); opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_bundle_options_global(iba_bundle_options* opt, int32_t n_iterations, int32_t robust) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_bundle_options_global: opt is NULL");
    if (n_iterations < 1 || n_iterations > 100) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_bundle_options_global: n_iterations " + std::to_string(n_iterations) + " is outside 1..100");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->rounds = 1; opt->iterations[0] = n_iterations; opt->robust_rounds = robust ? 1 : 0;
    opt->chi2_threshold = 5.991f; opt->huber_delta = bd::global_delta(); opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_bundle_optimize(const iba_bundle_job* jobs, int32_t B, const iba_bundle_options* opt, int device, iba_bundle_batch** out) {
    return run("iba_bundle_optimize", jobs, B, opt, device, false, out);
}

iba_status iba_bundle_eval(const iba_bundle_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double lambda, int device, iba_bundle_eval_out* outs) {
    const std::string who = "iba_bundle_eval: ";
    std::vector<bd::Plan> plans;
    if (const iba_status s = check_eval(who, jobs, B, lambda, outs, &plans)) return s;
    Limits lim{};
    iba_status s = limits(device, &lim);
    const bd::DevOpt o = bd::eval_options(robust, lambda);
    const std::vector<int32_t> cut = cut_jobs(jobs, plans, B, false, true, lim.budget);
    for (size_t c = 0; c + 1 < cut.size() && s == IBA_OK; ++c) s = eval_chunk(jobs, plans, cut[c], cut[c + 1], active, o, outs);
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; return s; }
    return IBA_OK;
}

void iba_bundle_free(iba_bundle_batch* r) { delete r; }

int32_t iba_bundle_n_jobs(const iba_bundle_batch* r) { return r ? (int32_t)r->job.size() : 0; }

iba_status iba_bundle_read(const iba_bundle_batch* r, int32_t job, iba_bundle_result* result) {
    if (const iba_status s = check_job_index(r, job, "iba_bundle_read: ")) return s;
    if (!result) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_bundle_read: result is NULL");
    *result = r->job[(size_t)job].r;
    return IBA_OK;
}

iba_status iba_bundle_cameras(const iba_bundle_batch* r, int32_t job, double* Tcw12, float* Tcw12f) {
    if (const iba_status s = check_job_index(r, job, "iba_bundle_cameras: ")) return s;
    const std::vector<double>& T = r->job[(size_t)job].T;
    for (size_t k = 0; k < T.size(); ++k) { if (Tcw12) Tcw12[k] = T[k]; if (Tcw12f) Tcw12f[k] = (float)T[k]; }
    return IBA_OK;
}

iba_status iba_bundle_points(const iba_bundle_batch* r, int32_t job, double* xyz, float* xyzf) {
    if (const iba_status s = check_job_index(r, job, "iba_bundle_points: ")) return s;
    const std::vector<double>& X = r->job[(size_t)job].X;
    for (size_t k = 0; k < X.size(); ++k) { if (xyz) xyz[k] = X[k]; if (xyzf) xyzf[k] = (float)X[k]; }
    return IBA_OK;
}

iba_status iba_bundle_edges(const iba_bundle_batch* r, int32_t job, uint8_t* outlier, float* chi2) {
    if (const iba_status s = check_job_index(r, job, "iba_bundle_edges: ")) return s;
    const iba_bundle_job_out& o = r->job[(size_t)job];
    if (outlier && !o.outlier.empty()) std::memcpy(outlier, o.outlier.data(), o.outlier.size());
    if (chi2 && !o.chi2.empty()) std::memcpy(chi2, o.chi2.data(), sizeof(float) * o.chi2.size());
    return IBA_OK;
}

iba_status iba_bundle_stage(const iba_bundle_batch* r, int32_t job, int32_t round, double* Tcw12, double* xyz) {
    const std::string who = "iba_bundle_stage: ";
    if (const iba_status s = check_job_index(r, job, who)) return s;
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    const iba_bundle_job_out& o = r->job[(size_t)job];
    if (round < 0 || round >= o.r.rounds_run) return t_err.fail(IBA_ERR_INVALID_ARG, who + "round " + std::to_string(round) + " is outside the job's " + std::to_string(o.r.rounds_run) + " rounds");
    const size_t nT = 12 * (size_t)o.r.n_cameras, nX = 3 * (size_t)o.r.n_points;
    if (Tcw12 && nT) std::memcpy(Tcw12, o.stT.data() + (size_t)round * nT, sizeof(double) * nT);
    if (xyz && nX) std::memcpy(xyz, o.stX.data() + (size_t)round * nX, sizeof(double) * nX);
    return IBA_OK;
}

iba_status iba_bundle_plan(const iba_bundle_job* job, int32_t* point_offsets, int32_t* point_edges, int32_t* camera_offsets, int32_t* camera_edges, int32_t* n_blocks,
                           int32_t* n_items, int32_t* block_cameras, int32_t* block_offsets, int32_t* items) {
    const std::string who = "iba_bundle_plan: ";
    if (!job || !n_blocks || !n_items) return t_err.fail(IBA_ERR_INVALID_ARG, who + "job, n_blocks or n_items is NULL");
    bd::Plan pl;
    std::string why = bd::check_job(*job);
    if (why.empty()) why = bd::make_plan(*job, &pl);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    auto put = [](int32_t* dst, const std::vector<int32_t>& v) { if (dst && !v.empty()) std::memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    put(point_offsets, pl.pt_off); put(point_edges, pl.pt_edges); put(camera_offsets, pl.cam_off); put(camera_edges, pl.cam_edges); put(block_offsets, pl.blk_off);
    *n_blocks = (int32_t)pl.blk_a.size(); *n_items = (int32_t)pl.it_p.size();
    if (block_cameras) for (size_t k = 0; k < pl.blk_a.size(); ++k) { block_cameras[2 * k] = pl.blk_a[k]; block_cameras[2 * k + 1] = pl.blk_b[k]; }
    if (items) for (size_t k = 0; k < pl.it_p.size(); ++k) { items[3 * k] = pl.it_p[k]; items[3 * k + 1] = pl.it_ea[k]; items[3 * k + 2] = pl.it_eb[k]; }
    return IBA_OK;
}

iba_status iba_bundle_local_window(const int32_t* observations, int32_t n_observations, const uint8_t* point_bad, int32_t n_map_points, const uint8_t* keyframe_bad,
                                   int32_t n_keyframes, int32_t current, const int32_t* covisible, int32_t n_covisible, int32_t* camera_keyframe, uint8_t* fixed,
                                   int32_t* n_local, int32_t* n_cameras, int32_t* point_id, int32_t* n_points, int32_t* edge_point, int32_t* edge_camera,
                                   int32_t* edge_keypoint, int32_t* n_edges) {
    const std::string who = "iba_bundle_local_window: ";
    if (!n_local || !n_cameras || !n_points || !n_edges) return t_err.fail(IBA_ERR_INVALID_ARG, who + "a NULL count");
    *n_local = *n_cameras = *n_points = *n_edges = 0;
    bd::Window w;
    const std::string why = bd::local_window(observations, n_observations, point_bad, n_map_points, keyframe_bad, n_keyframes, current, covisible, n_covisible, &w);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    if ((!camera_keyframe || !fixed) || (!w.point_id.empty() && !point_id) || (!w.edge_point.empty() && (!edge_point || !edge_camera || !edge_keypoint)))
        return t_err.fail(IBA_ERR_INVALID_ARG, who + "a NULL output");
    auto put = [](int32_t* dst, const std::vector<int32_t>& v) { if (!v.empty()) std::memcpy(dst, v.data(), sizeof(int32_t) * v.size()); };
    put(camera_keyframe, w.camera_keyframe); put(point_id, w.point_id); put(edge_point, w.edge_point); put(edge_camera, w.edge_camera); put(edge_keypoint, w.edge_keypoint);
    std::memcpy(fixed, w.fixed.data(), w.fixed.size());
    *n_local = w.n_local; *n_cameras = (int32_t)w.camera_keyframe.size(); *n_points = (int32_t)w.point_id.size(); *n_edges = (int32_t)w.edge_point.size();
    return IBA_OK;
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_bundle_host(const iba_bundle_job* jobs, int32_t B, const iba_bundle_options* opt, iba_bundle_batch** out) {
    return run("iba_debug_bundle_host", jobs, B, opt, 0, true, out);
}

iba_status iba_debug_bundle_eval_host(const iba_bundle_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double lambda, iba_bundle_eval_out* outs) {
    std::vector<bd::Plan> plans;
    if (const iba_status s = check_eval("iba_debug_bundle_eval_host: ", jobs, B, lambda, outs, &plans)) return s;
    bd::host_eval(jobs, plans, B, active, robust != 0, lambda, outs);
    return IBA_OK;
}

int32_t iba_debug_bundle_big_steps(const iba_bundle_batch* r) { return r ? r->big_steps : 0; }

int32_t iba_debug_bundle_chunks(const iba_bundle_batch* r) { return r ? r->chunks : 0; }

float iba_debug_bundle_kernel_ms(const iba_bundle_batch* r) { return r ? r->kernel_ms : 0.f; }

}  // extern "C"

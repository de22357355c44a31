// Sim3 RANSAC between two keyframes (include/iba_mi355x.h, iba_sim3*): the C ABI, the result object's accessors and the launch chain of a call. The
// kernels are iba_sim3_kernels.hpp, the arithmetic iba_sim3_math.hpp, the host rules (argument checks, Z6, the helpers, the host restatement)
// iba_sim3_host.hpp. A per-call unit (iba_call.hpp): every job is prepared on the host; the chain of a chunk of jobs: tables up, five kernels,
// results down. The result is host memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_call.hpp"
#include "iba_device_buf.hpp"
#include "iba_sim3_host.hpp"
#include "iba_sim3_kernels.hpp"

using iba::DevBuf;
namespace z3 = iba::z3;

namespace {
thread_local iba::CallError t_err;

constexpr int kShippedForm = 1;    // 0: form (a), a lane per hypothesis; 1: form (b), a lane per correspondence (profiles/sim3_bench.md)

// device bytes of a job: per correspondence 32 (world points) + 8 (thresholds) + 48 (prepared) + the listed flags, per iteration 12 (set) + 52 + 96
// (hypothesis) + 4 (count) + 1 (cap), and with keep_stages a byte per (iteration, correspondence)
uint64_t job_bytes(const z3::JobPrep& q, const iba_sim3_options& o) {
    if (!q.I) return 0;
    return (uint64_t)q.N * (88ull + (uint64_t)(o.max_events + 1)) + (uint64_t)q.I * 165ull + (o.keep_stages ? (uint64_t)q.I * (uint64_t)q.N : 0ull) + sizeof(z3::JobRec) + 4 * z3::kSelInts + 8;
}

// one chain: the jobs [a, b) of the call, already prepared and their results started
iba_status run_chunk(iba_sim3_batch* res, const std::vector<z3::JobPrep>& prep, int32_t a, int32_t b, bool timing) {
    const iba_sim3_options& opt = res->opt;
    const int32_t nJ = b - a, E = opt.max_events;
    const bool keep = opt.keep_stages != 0;
    hipStream_t st = nullptr;
    // the host arrays of the chain first, then its device buffers, then the guard: it waits for the stream before any of them unwinds
    std::vector<z3::JobRec> recs((size_t)nJ);
    std::vector<float> h_w1, h_w2, h_th, h_srt;
    std::vector<int32_t> h_sets, h_counts, h_sel;
    std::vector<int64_t> h_itb((size_t)nJ, 0);
    std::vector<uint8_t> h_flags, h_itflags;
    DevBuf<z3::JobRec> d_jobs; DevBuf<float4> d_w1, d_w2, d_ca, d_cb, d_cc; DevBuf<float2> d_th; DevBuf<int32_t> d_sets, d_counts, d_sel; DevBuf<int64_t> d_itb;
    DevBuf<float> d_srt, d_T12, d_T21; DevBuf<uint8_t> d_cap, d_flags, d_itflags;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);
    size_t M = 0, H = 0, IN = 0;
    int32_t maxN = 0, maxI = 0;
    for (int32_t k = 0; k < nJ; ++k) {
        const z3::JobPrep& q = prep[(size_t)(a + k)];
        z3::JobRec& r = recs[(size_t)k];
        r.c_base = (int32_t)M; r.h_base = (int32_t)H; r.N = q.I ? q.N : 0; r.I = q.I;
        std::memcpy(r.K1, q.K1, sizeof(r.K1)); std::memcpy(r.K2, q.K2, sizeof(r.K2)); std::memcpy(r.T1, q.T1, sizeof(r.T1)); std::memcpy(r.T2, q.T2, sizeof(r.T2));
        h_itb[(size_t)k] = (int64_t)IN;
        M += (size_t)r.N; H += (size_t)r.I; IN += (size_t)r.N * (size_t)r.I;
        maxN = std::max(maxN, r.N); maxI = std::max(maxI, r.I);
        if ((uint64_t)(E + 1) * M >= (1ull << 31) || 13ull * H >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "a chunk of 2^31 per-hypothesis or per-correspondence entries or more");
    }
    if (H == 0) { sync.disarm(); return IBA_OK; }    // every job of the chunk has its status already: nothing was queued
    h_w1.resize(4 * M); h_w2.resize(4 * M); h_th.resize(2 * M); h_sets.resize(3 * H);
    for (int32_t k = 0; k < nJ; ++k) {
        const z3::JobPrep& q = prep[(size_t)(a + k)];
        const z3::JobRec& r = recs[(size_t)k];
        if (!r.I) continue;
        std::memcpy(&h_w1[4 * (size_t)r.c_base], q.w1.data(), sizeof(float) * 4 * (size_t)r.N); std::memcpy(&h_w2[4 * (size_t)r.c_base], q.w2.data(), sizeof(float) * 4 * (size_t)r.N);
        std::memcpy(&h_th[2 * (size_t)r.c_base], q.th.data(), sizeof(float) * 2 * (size_t)r.N);
        std::memcpy(&h_sets[3 * (size_t)r.h_base], q.sets.data(), sizeof(int32_t) * 3 * (size_t)r.I);
    }
    const size_t nF = (size_t)(E + 1) * M;
    IBA_CALL_TRY(d_jobs.alloc((size_t)nJ)); IBA_CALL_TRY(d_w1.alloc(M)); IBA_CALL_TRY(d_w2.alloc(M)); IBA_CALL_TRY(d_th.alloc(M)); IBA_CALL_TRY(d_ca.alloc(M)); IBA_CALL_TRY(d_cb.alloc(M));
    IBA_CALL_TRY(d_cc.alloc(M)); IBA_CALL_TRY(d_sets.alloc(3 * H)); IBA_CALL_TRY(d_counts.alloc(H)); IBA_CALL_TRY(d_sel.alloc((size_t)z3::kSelInts * (size_t)nJ)); IBA_CALL_TRY(d_itb.alloc((size_t)nJ));
    IBA_CALL_TRY(d_srt.alloc(13 * H)); IBA_CALL_TRY(d_T12.alloc(12 * H)); IBA_CALL_TRY(d_T21.alloc(12 * H)); IBA_CALL_TRY(d_cap.alloc(H)); IBA_CALL_TRY(d_flags.alloc(nF));
    if (keep) IBA_CALL_TRY(d_itflags.alloc(IN));
    IBA_CALL_TRY(hipMemcpyAsync(d_jobs.p, recs.data(), sizeof(z3::JobRec) * (size_t)nJ, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_w1.p, h_w1.data(), sizeof(float) * 4 * M, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_w2.p, h_w2.data(), sizeof(float) * 4 * M, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_th.p, h_th.data(), sizeof(float) * 2 * M, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_sets.p, h_sets.data(), sizeof(int32_t) * 3 * H, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_itb.p, h_itb.data(), sizeof(int64_t) * (size_t)nJ, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemsetAsync(d_counts.p, 0, sizeof(int32_t) * H, st)); IBA_CALL_TRY(hipMemsetAsync(d_sel.p, 0, sizeof(int32_t) * (size_t)z3::kSelInts * (size_t)nJ, st));
    IBA_CALL_TRY(hipMemsetAsync(d_flags.p, 0, std::max<size_t>(nF, 1), st));
    if (keep) IBA_CALL_TRY(hipMemsetAsync(d_itflags.p, 0, std::max<size_t>(IN, 1), st));
    if (timing) IBA_CALL_TRY(ev.create(6));
    int stage = 0;
#define Z3_STAGE() do { IBA_CALL_TRY(hipGetLastError()); if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[(size_t)++stage], st)); } while (0)
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    const uint32_t jobs_y = (uint32_t)nJ;
    hipLaunchKernelGGL(z3::z3_prep_kernel, dim3((uint32_t)((maxN + z3::kPrepThreads - 1) / z3::kPrepThreads), jobs_y), dim3(z3::kPrepThreads), 0, st, d_jobs.p, d_w1.p, d_w2.p, d_th.p, d_ca.p, d_cb.p,
                       d_cc.p);
    Z3_STAGE();
    hipLaunchKernelGGL(z3::z3_hyp_kernel, dim3((uint32_t)((maxI + z3::kHypThreads - 1) / z3::kHypThreads), jobs_y), dim3(z3::kHypThreads), 0, st, d_jobs.p, d_sets.p, d_ca.p, d_cb.p,
                       (int)opt.fix_scale, d_srt.p, d_T12.p, d_T21.p, d_cap.p);
    Z3_STAGE();
    if (res->form == 0)
        hipLaunchKernelGGL(z3::z3_count_a_kernel, dim3((uint32_t)((maxI + 63) / 64), jobs_y), dim3(64), 0, st, d_jobs.p, d_ca.p, d_cb.p, d_cc.p, d_T12.p, d_T21.p, d_counts.p);
    else
        hipLaunchKernelGGL(z3::z3_count_b_kernel, dim3((uint32_t)((maxI + 3) / 4), jobs_y), dim3(z3::kCountBThreads), 0, st, d_jobs.p, d_ca.p, d_cb.p, d_cc.p, d_T12.p, d_T21.p, d_counts.p);
    Z3_STAGE();
    hipLaunchKernelGGL(z3::z3_select_kernel, dim3((uint32_t)nJ), dim3(64), 0, st, d_jobs.p, (int)nJ, (int)opt.min_inliers, (int)E, d_counts.p, d_cap.p, d_sel.p);
    Z3_STAGE();
    const uint32_t flag_x = (uint32_t)((maxN + z3::kFlagThreads - 1) / z3::kFlagThreads);
    hipLaunchKernelGGL(z3::z3_flags_kernel, dim3(flag_x, (uint32_t)(E + 1), jobs_y), dim3(z3::kFlagThreads), 0, st, d_jobs.p, 0, (int)E, d_sel.p, d_itb.p, d_ca.p, d_cb.p, d_cc.p, d_T12.p, d_T21.p,
                       d_flags.p);
    if (keep) {
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(z3::z3_flags_kernel, dim3(flag_x, (uint32_t)maxI, jobs_y), dim3(z3::kFlagThreads), 0, st, d_jobs.p, 1, (int)E, d_sel.p, d_itb.p, d_ca.p, d_cb.p, d_cc.p, d_T12.p, d_T21.p,
                           d_itflags.p);
    }
    Z3_STAGE();
#undef Z3_STAGE
    // ---- everything down ----
    h_counts.resize(H); h_sel.resize((size_t)z3::kSelInts * (size_t)nJ); h_srt.resize(13 * H); h_flags.resize(nF); h_itflags.resize(keep ? IN : 0);
    IBA_CALL_TRY(hipMemcpyAsync(h_counts.data(), d_counts.p, sizeof(int32_t) * H, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_sel.data(), d_sel.p, sizeof(int32_t) * h_sel.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_srt.data(), d_srt.p, sizeof(float) * 13 * H, hipMemcpyDeviceToHost, st));
    if (nF) IBA_CALL_TRY(hipMemcpyAsync(h_flags.data(), d_flags.p, nF, hipMemcpyDeviceToHost, st));
    if (keep && IN) IBA_CALL_TRY(hipMemcpyAsync(h_itflags.data(), d_itflags.p, IN, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (timing)
        for (int k = 0; k < 5; ++k) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[(size_t)k], ev.e[(size_t)k + 1])); res->ms[k] += ms; }
    for (int32_t k = 0; k < nJ; ++k) {
        const z3::JobRec& r = recs[(size_t)k];
        if (!r.I) continue;
        z3::JobRes& o = res->job[(size_t)(a + k)];
        const int32_t* s = &h_sel[(size_t)z3::kSelInts * (size_t)k];
        const size_t N = (size_t)r.N, I = (size_t)r.I, hb = (size_t)r.h_base;
        o.counts.assign(h_counts.begin() + (ptrdiff_t)hb, h_counts.begin() + (ptrdiff_t)(hb + I));
        o.srt.assign(h_srt.begin() + (ptrdiff_t)(13 * hb), h_srt.begin() + (ptrdiff_t)(13 * (hb + I)));
        o.flags.assign(h_flags.begin() + (ptrdiff_t)((size_t)(E + 1) * (size_t)r.c_base), h_flags.begin() + (ptrdiff_t)((size_t)(E + 1) * ((size_t)r.c_base + N)));
        if (keep) o.it_flags.assign(h_itflags.begin() + (ptrdiff_t)h_itb[(size_t)k], h_itflags.begin() + (ptrdiff_t)((size_t)h_itb[(size_t)k] + I * N));
        o.r.sweep_cap_hits = s[3];
        z3::finish(opt, s + 4, s[0], s[1], s[2], o);
    }
    return IBA_OK;
}

// the chains of a call: consecutive jobs under the byte budget, at most 32768 and at least one per chunk
iba_status run_chunks(iba_sim3_batch* res, const std::vector<z3::JobPrep>& prep, int device, bool timing) {
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, IBA_SIM3_BUDGET_BYTES, "IBA_SIM3_BUDGET", &budget));
    std::vector<uint64_t> bytes(prep.size());
    for (size_t b = 0; b < prep.size(); ++b) bytes[b] = job_bytes(prep[b], res->opt);
    const std::vector<int32_t> cut = iba::cut_chunks(bytes, budget, 32768);
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        ++res->chunks;
        if (const iba_status s = run_chunk(res, prep, cut[c], cut[c + 1], timing)) return s;
    }
    return IBA_OK;
}

iba_status run(const char* name, const iba_map_points* points, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt, int device, bool on_host, iba_sim3_batch** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    const std::string why = z3::check_call(points, jobs, J, opt);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_sim3_batch* res = new iba_sim3_batch();
    res->opt = *opt;
    res->job.resize((size_t)J);
    res->form = kShippedForm;
    if (const char* e = iba::debug_env("IBA_SIM3_COUNT_FORM")) res->form = std::atoi(e) ? 1 : 0;
    std::vector<z3::JobPrep> prep((size_t)J);
    for (int32_t b = 0; b < J; ++b) z3::prepare(*points, jobs[b], *opt, prep[(size_t)b]);
    iba_status s = IBA_OK;
    if (on_host) {
        for (int32_t b = 0; b < J; ++b) z3::host_job(prep[(size_t)b], *opt, res->job[(size_t)b]);
    } else {
        for (int32_t b = 0; b < J; ++b) z3::start_result(prep[(size_t)b], *opt, res->job[(size_t)b]);
        s = run_chunks(res, prep, device, iba::debug_env("IBA_SIM3_TIMING") != nullptr);
    }
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

iba_status check_job_index(const iba_sim3_batch* r, int32_t job, const std::string& who) { return t_err.check_index(!r, job, r ? r->job.size() : 0, who, "job"); }

// s, R, t and the inlier bytes of one flag slot of a job
void put_hypothesis(const z3::JobRes& o, int32_t it, size_t slot, float* s, float* R, float* t, uint8_t* inlier) {
    const size_t N = (size_t)o.r.n;
    if (it < 0) {
        if (s) *s = 0.f;
        if (R) std::memset(R, 0, 9 * sizeof(float));
        if (t) std::memset(t, 0, 3 * sizeof(float));
        if (inlier && N) std::memset(inlier, 0, N);
        return;
    }
    const float* h = &o.srt[13 * (size_t)it];
    if (s) *s = h[0];
    if (R) std::memcpy(R, h + 1, 9 * sizeof(float));
    if (t) std::memcpy(t, h + 10, 3 * sizeof(float));
    if (inlier && N) std::memcpy(inlier, &o.flags[slot * N], N);
}

}  // namespace

extern "C" {

const char* iba_sim3_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_sim3_options(iba_sim3_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_sim3_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->probability = 0.99; opt->min_inliers = 20; opt->max_iterations = 300; opt->fix_scale = 0; opt->max_events = 1; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_sim3_solve(const iba_map_points* points, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt, int device, iba_sim3_batch** out) {
    return run("iba_sim3_solve", points, jobs, J, opt, device, false, out);
}

void iba_sim3_free(iba_sim3_batch* r) { delete r; }

int32_t iba_sim3_n_jobs(const iba_sim3_batch* r) { return r ? (int32_t)r->job.size() : 0; }

iba_status iba_sim3_read(const iba_sim3_batch* r, int32_t job, iba_sim3_result* result) {
    if (const iba_status s = check_job_index(r, job, "iba_sim3_read: ")) return s;
    if (!result) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_sim3_read: result is NULL");
    *result = r->job[(size_t)job].r;
    return IBA_OK;
}

iba_status iba_sim3_counts(const iba_sim3_batch* r, int32_t job, int32_t* n_inliers_per_iteration) {
    if (const iba_status s = check_job_index(r, job, "iba_sim3_counts: ")) return s;
    const z3::JobRes& o = r->job[(size_t)job];
    if (n_inliers_per_iteration && !o.counts.empty()) std::memcpy(n_inliers_per_iteration, o.counts.data(), sizeof(int32_t) * o.counts.size());
    return IBA_OK;
}

iba_status iba_sim3_event(const iba_sim3_batch* r, int32_t job, int32_t k, int32_t* iteration, int32_t* n_inliers, float* s, float R[9], float t[3], uint8_t* inlier) {
    const std::string who = "iba_sim3_event: ";
    if (const iba_status st = check_job_index(r, job, who)) return st;
    const z3::JobRes& o = r->job[(size_t)job];
    if (k < 0) return t_err.fail(IBA_ERR_INVALID_ARG, who + "event " + std::to_string(k) + " is negative");
    if (k >= r->opt.max_events) return t_err.fail(IBA_ERR_INVALID_ARG, who + "event " + std::to_string(k) + " is at or above max_events = " + std::to_string(r->opt.max_events) + ": raise max_events");
    if (k >= o.r.n_listed) return t_err.fail(IBA_ERR_INVALID_ARG, who + "event " + std::to_string(k) + " is outside the job's " + std::to_string(o.r.n_listed) + " events");
    const int32_t it = o.ev_it[(size_t)k];
    if (iteration) *iteration = it;
    if (n_inliers) *n_inliers = o.counts[(size_t)it];
    put_hypothesis(o, it, (size_t)k, s, R, t, inlier);
    return IBA_OK;
}

iba_status iba_sim3_best(const iba_sim3_batch* r, int32_t job, int32_t* iteration, int32_t* n_inliers, float* s, float R[9], float t[3], uint8_t* inlier) {
    if (const iba_status st = check_job_index(r, job, "iba_sim3_best: ")) return st;
    const z3::JobRes& o = r->job[(size_t)job];
    if (iteration) *iteration = o.r.best_it;
    if (n_inliers) *n_inliers = o.r.best_inliers;
    put_hypothesis(o, o.r.best_it, (size_t)r->opt.max_events, s, R, t, inlier);
    return IBA_OK;
}

iba_status iba_sim3_iterations(const iba_sim3_batch* r, int32_t job, float* s, float* R, float* t, uint8_t* inlier) {
    const std::string who = "iba_sim3_iterations: ";
    if (const iba_status st = check_job_index(r, job, who)) return st;
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    const z3::JobRes& o = r->job[(size_t)job];
    for (int32_t it = 0; it < o.r.iterations; ++it) {
        const float* h = &o.srt[13 * (size_t)it];
        if (s) s[it] = h[0];
        if (R) std::memcpy(R + 9 * (size_t)it, h + 1, 9 * sizeof(float));
        if (t) std::memcpy(t + 3 * (size_t)it, h + 10, 3 * sizeof(float));
    }
    if (inlier && !o.it_flags.empty()) std::memcpy(inlier, o.it_flags.data(), o.it_flags.size());
    return IBA_OK;
}

iba_status iba_sim3_correspondences(const iba_fuse_map* map, int32_t kf1, int32_t kf2, const int32_t* matches12, const int32_t* octave1, const int32_t* octave2,
                                    const float* level_sigma2_1, const float* level_sigma2_2, int32_t n_levels1, int32_t n_levels2, int32_t* index1, int32_t* point1,
                                    int32_t* point2, float* max_err1, float* max_err2, int32_t* n) {
    const std::string why = z3::correspondences(map, kf1, kf2, matches12, octave1, octave2, level_sigma2_1, level_sigma2_2, n_levels1, n_levels2, index1, point1, point2, max_err1, max_err2, n);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_sim3_correspondences: " + why);
}

iba_status iba_sim3_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out) {
    const std::string why = z3::make_sets(N, iterations, seed, out);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_sim3_sets: " + why);
}

iba_status iba_sim3_budget(int32_t N, const iba_sim3_options* opt, int32_t* iterations) {
    const std::string who = "iba_sim3_budget: ";
    const std::string why = z3::check_options(opt);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    if (N < 1 || !iterations) return t_err.fail(IBA_ERR_INVALID_ARG, who + "N < 1 or iterations is NULL");
    *iterations = z3::budget(N, *opt);
    return IBA_OK;
}

iba_status iba_sim3_iterate(const iba_sim3_batch* r, int32_t job, int32_t from_it, int32_t n, int32_t* next_it, int32_t* event, int32_t* no_more) {
    const std::string who = "iba_sim3_iterate: ";
    if (const iba_status st = check_job_index(r, job, who)) return st;
    if (!next_it || !event || !no_more) return t_err.fail(IBA_ERR_INVALID_ARG, who + "a NULL argument");
    const z3::JobRes& o = r->job[(size_t)job];
    if (from_it < 0 || from_it > o.r.iterations || n < 0) return t_err.fail(IBA_ERR_INVALID_ARG, who + "from_it is outside 0.." + std::to_string(o.r.iterations) + " or n < 0");
    z3::iterate(o, r->opt.min_inliers, from_it, n, next_it, event, no_more);
    return IBA_OK;
}

iba_status iba_sim3_compose(float s, const float R[9], const float t[3], const float* Tmw12, double* s_out, double R_out[9], double t_out[3]) {
    if (!R || !t || !Tmw12) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_sim3_compose: a NULL argument");
    z3::compose(s, R, t, Tmw12, s_out, R_out, t_out);
    return IBA_OK;
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_sim3_host(const iba_map_points* points, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt, iba_sim3_batch** out) {
    return run("iba_debug_sim3_host", points, jobs, J, opt, 0, true, out);
}

int32_t iba_debug_sim3_chunks(const iba_sim3_batch* r) { return r ? r->chunks : 0; }

iba_status iba_debug_sim3_stage_ms(const iba_sim3_batch* r, float ms[5]) {
    if (!r || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_sim3_stage_ms: a NULL argument");
    std::memcpy(ms, r->ms, sizeof(r->ms));
    return IBA_OK;
}

}  // extern "C"

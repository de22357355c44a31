// Motion-only pose optimisation (include/iba_mi355x.h, iba_pose*): the C ABI, the result object's accessors and the launch of a call. The kernels
// are iba_pose_kernels.hpp, the arithmetic iba_pose_math.hpp, the host rules (argument checks, the host restatement, the edges from matches)
// iba_pose_host.hpp. A per-call unit (iba_call.hpp); the chain of a chunk of jobs: edges up, ONE kernel, results down. The result is host memory.
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
#include "iba_pose_host.hpp"
#include "iba_pose_kernels.hpp"

using iba::DevBuf;
namespace ps = iba::pose;

namespace {
thread_local iba::CallError t_err;

constexpr uint64_t kBudgetBytes = 1ull << 30;
// device bytes of a job: per edge 24 (point, observation, information) + 1 (flag) + 4 (float chi2) + 8 (iba_pose_eval's chi2), and its records
uint64_t job_bytes(int32_t n) { return 37ull * (uint64_t)n + sizeof(ps::JobRec) + sizeof(ps::JobOut) + ps::kSums * sizeof(double); }

struct Limits { uint64_t budget; int cap; bool timing; };
// the chunk budget (1 GiB, or a quarter of the free device memory where that is less) and the on-chip capacity, with their debug overrides
iba_status limits(int device, Limits* l) {
    IBA_CALL_TRY(iba::call_budget(device, kBudgetBytes, "IBA_POSE_BUDGET", &l->budget));
    l->cap = ps::kCap;
    if (const char* e = iba::debug_env("IBA_POSE_ONCHIP")) { const int v = std::atoi(e); if (v >= 0 && v < ps::kCap) l->cap = v; }
    l->timing = iba::debug_env("IBA_POSE_TIMING") != nullptr;
    return IBA_OK;
}
// the chunks of a call: consecutive jobs under the budget, at least one each
std::vector<int32_t> cut_jobs(const iba_pose_job* jobs, int32_t B, uint64_t budget) {
    std::vector<uint64_t> bytes((size_t)B);
    for (int32_t j = 0; j < B; ++j) bytes[(size_t)j] = job_bytes(jobs[j].n);
    return iba::cut_chunks(bytes, budget);
}

// the edges of the jobs [a, b) side by side, and their records
struct Staged {
    std::vector<ps::JobRec> recs; std::vector<float> xyz, obs, w; size_t M = 0;
    DevBuf<ps::JobRec> d_recs; DevBuf<float> d_xyz, d_obs, d_w;
};
iba_status stage(const iba_pose_job* jobs, int32_t a, int32_t b, Staged* s, hipStream_t st) {
    const int32_t nJ = b - a;
    s->recs.resize((size_t)nJ);
    size_t M = 0;
    for (int32_t k = 0; k < nJ; ++k) {
        const iba_pose_job& q = jobs[a + k];
        ps::JobRec& r = s->recs[(size_t)k];
        r.base = (int32_t)M; r.n = q.n; r.fx = q.fx; r.fy = q.fy; r.cx = q.cx; r.cy = q.cy;
        std::memcpy(r.T, q.Tcw12, sizeof(r.T));
        M += (size_t)q.n;
    }
    if (M >= (1ull << 31) / 3) return t_err.fail(IBA_ERR_UNSUPPORTED, "a chunk of 2^31 / 3 edges or more");
    s->M = M;
    s->xyz.resize(3 * M); s->obs.resize(2 * M); s->w.resize(M);
    for (int32_t k = 0; k < nJ; ++k) {
        const iba_pose_job& q = jobs[a + k];
        const size_t base = (size_t)s->recs[(size_t)k].base, n = (size_t)q.n;
        if (!n) continue;
        std::memcpy(&s->xyz[3 * base], q.xyz, sizeof(float) * 3 * n); std::memcpy(&s->obs[2 * base], q.obs, sizeof(float) * 2 * n); std::memcpy(&s->w[base], q.inv_sigma2, sizeof(float) * n);
    }
    IBA_CALL_TRY(s->d_recs.alloc((size_t)nJ)); IBA_CALL_TRY(s->d_xyz.alloc(3 * M)); IBA_CALL_TRY(s->d_obs.alloc(2 * M)); IBA_CALL_TRY(s->d_w.alloc(M));
    IBA_CALL_TRY(hipMemcpyAsync(s->d_recs.p, s->recs.data(), sizeof(ps::JobRec) * (size_t)nJ, hipMemcpyHostToDevice, st));
    if (M) {
        IBA_CALL_TRY(hipMemcpyAsync(s->d_xyz.p, s->xyz.data(), sizeof(float) * 3 * M, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(s->d_obs.p, s->obs.data(), sizeof(float) * 2 * M, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(s->d_w.p, s->w.data(), sizeof(float) * M, hipMemcpyHostToDevice, st));
    }
    return IBA_OK;
}

iba_status optimize_chunk(iba_pose_batch* res, const iba_pose_job* jobs, int32_t a, int32_t b, const Limits& lim) {
    hipStream_t st = nullptr;
    const int32_t nJ = b - a;
    Staged s;
    std::vector<uint8_t> h_out;
    std::vector<float> h_chi2;
    DevBuf<uint8_t> d_out; DevBuf<float> d_chi2; DevBuf<ps::JobOut> d_res;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);
    if (const iba_status e = stage(jobs, a, b, &s, st)) return e;
    const size_t M = s.M;
    IBA_CALL_TRY(d_out.alloc(M)); IBA_CALL_TRY(d_chi2.alloc(M)); IBA_CALL_TRY(d_res.alloc((size_t)nJ));
    IBA_CALL_TRY(hipMemsetAsync(d_out.p, 0, std::max<size_t>(M, 1), st)); IBA_CALL_TRY(hipMemsetAsync(d_chi2.p, 0, sizeof(float) * std::max<size_t>(M, 1), st));
    IBA_CALL_TRY(hipMemcpyAsync(d_res.p, &res->job[(size_t)a], sizeof(ps::JobOut) * (size_t)nJ, hipMemcpyHostToDevice, st));
    const iba_pose_options& opt = res->opt;
    const ps::DevOpt o{opt.rounds, opt.iterations, opt.robust_rounds, opt.chi2_threshold, (double)opt.huber_delta};
    if (lim.timing) { IBA_CALL_TRY(ev.create(2)); IBA_CALL_TRY(hipEventRecord(ev.e[0], st)); }
    hipLaunchKernelGGL(ps::pose_optimize_kernel, dim3((uint32_t)std::min<int32_t>(nJ, ps::kMaxGrid)), dim3(ps::kThreads), 0, st, s.d_recs.p, (int)nJ, s.d_xyz.p, s.d_obs.p, s.d_w.p, d_out.p, d_chi2.p,
                       d_res.p, o, lim.cap);
    IBA_CALL_TRY(hipGetLastError());
    if (lim.timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    h_out.resize(M); h_chi2.resize(M);
    IBA_CALL_TRY(hipMemcpyAsync(&res->job[(size_t)a], d_res.p, sizeof(ps::JobOut) * (size_t)nJ, hipMemcpyDeviceToHost, st));
    if (M) {
        IBA_CALL_TRY(hipMemcpyAsync(h_out.data(), d_out.p, M, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(h_chi2.data(), d_chi2.p, sizeof(float) * M, hipMemcpyDeviceToHost, st));
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (lim.timing) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); res->kernel_ms += ms; }
    for (int32_t k = 0; k < nJ; ++k) {
        const size_t base = (size_t)s.recs[(size_t)k].base, n = (size_t)s.recs[(size_t)k].n;
        res->outlier[(size_t)(a + k)].assign(h_out.begin() + (ptrdiff_t)base, h_out.begin() + (ptrdiff_t)(base + n));
        res->chi2[(size_t)(a + k)].assign(h_chi2.begin() + (ptrdiff_t)base, h_chi2.begin() + (ptrdiff_t)(base + n));
    }
    return IBA_OK;
}

iba_status run(const char* name, const iba_pose_job* jobs, int32_t B, const iba_pose_options* opt, int device, bool on_host, iba_pose_batch** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    std::string why = ps::check_options(opt);
    if (why.empty()) why = ps::check_jobs(jobs, B);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_pose_batch* res = new iba_pose_batch();
    res->opt = *opt;
    res->job.resize((size_t)B); res->outlier.resize((size_t)B); res->chi2.resize((size_t)B);
    iba_status s = IBA_OK;
    if (on_host) {
        for (int32_t j = 0; j < B; ++j) {
            res->outlier[(size_t)j].assign((size_t)jobs[j].n, 0); res->chi2[(size_t)j].assign((size_t)jobs[j].n, 0.f);
            ps::host_job(jobs[j], *opt, res->job[(size_t)j], res->outlier[(size_t)j].data(), res->chi2[(size_t)j].data());
        }
    } else {
        for (int32_t j = 0; j < B; ++j) ps::start_out(jobs[j], res->job[(size_t)j]);
        Limits lim{};
        s = limits(device, &lim);
        const std::vector<int32_t> cut = cut_jobs(jobs, B, lim.budget);
        for (size_t c = 0; c + 1 < cut.size() && s == IBA_OK; ++c) {
            s = optimize_chunk(res, jobs, cut[c], cut[c + 1], lim);
            ++res->chunks;
        }
    }
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

iba_status eval_chunk(const iba_pose_job* jobs, int32_t a, int32_t b, const uint8_t* const* active, int32_t robust, const Limits& lim, double* sums, double* const* chi2_edges) {
    hipStream_t st = nullptr;
    const int32_t nJ = b - a;
    Staged s;
    std::vector<uint8_t> h_bad;
    std::vector<double> h_chi2;
    DevBuf<uint8_t> d_bad; DevBuf<double> d_sums, d_chi2;
    iba::SyncOnExit sync(st);
    if (const iba_status e = stage(jobs, a, b, &s, st)) return e;
    const size_t M = s.M;
    h_bad.assign(M, 0);
    bool want_chi2 = false;
    for (int32_t k = 0; k < nJ; ++k) {
        const size_t base = (size_t)s.recs[(size_t)k].base, n = (size_t)s.recs[(size_t)k].n;
        if (active && active[a + k]) for (size_t i = 0; i < n; ++i) h_bad[base + i] = active[a + k][i] ? 0 : 1;
        want_chi2 = want_chi2 || (chi2_edges && chi2_edges[a + k]);
    }
    IBA_CALL_TRY(d_bad.alloc(M)); IBA_CALL_TRY(d_sums.alloc((size_t)nJ * ps::kSums));
    if (want_chi2) IBA_CALL_TRY(d_chi2.alloc(M));
    if (M) IBA_CALL_TRY(hipMemcpyAsync(d_bad.p, h_bad.data(), M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ps::pose_eval_kernel, dim3((uint32_t)std::min<int32_t>(nJ, ps::kMaxGrid)), dim3(ps::kThreads), 0, st, s.d_recs.p, (int)nJ, s.d_xyz.p, s.d_obs.p, s.d_w.p, d_bad.p, (int)(robust != 0),
                       (double)ps::default_delta(), d_sums.p, want_chi2 ? d_chi2.p : (double*)nullptr, lim.cap);
    IBA_CALL_TRY(hipGetLastError());
    h_chi2.resize(want_chi2 ? M : 0);
    IBA_CALL_TRY(hipMemcpyAsync(sums, d_sums.p, sizeof(double) * (size_t)nJ * ps::kSums, hipMemcpyDeviceToHost, st));
    if (want_chi2 && M) IBA_CALL_TRY(hipMemcpyAsync(h_chi2.data(), d_chi2.p, sizeof(double) * M, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (want_chi2)
        for (int32_t k = 0; k < nJ; ++k) {
            const size_t base = (size_t)s.recs[(size_t)k].base, n = (size_t)s.recs[(size_t)k].n;
            if (chi2_edges[a + k] && n) std::memcpy(chi2_edges[a + k], &h_chi2[base], sizeof(double) * n);
        }
    return IBA_OK;
}

void spread(const double* sums, double* H, double* b, double* chi2) {
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) H[r * 6 + c] = sums[r <= c ? ps::hidx(r, c) : ps::hidx(c, r)];
    for (int k = 0; k < 6; ++k) b[k] = sums[21 + k];
    *chi2 = sums[27];
}

iba_status check_eval(const std::string& who, const iba_pose_job* jobs, int32_t B, const double* H, const double* b, const double* chi2_robust) {
    if (!H || !b || !chi2_robust) return t_err.fail(IBA_ERR_INVALID_ARG, who + "H, b or chi2_robust is NULL");
    const std::string why = ps::check_jobs(jobs, B);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    return IBA_OK;
}

iba_status check_job_index(const iba_pose_batch* r, int32_t job, const std::string& who) {
    return t_err.check_index(!r, job, r ? r->job.size() : 0, who, "job");
}

}  // namespace

extern "C" {

const char* iba_pose_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_pose_options(iba_pose_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_pose_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->rounds = 4; opt->iterations = 10; opt->chi2_threshold = 5.991f; opt->huber_delta = ps::default_delta(); opt->robust_rounds = 3; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_pose_optimize(const iba_pose_job* jobs, int32_t B, const iba_pose_options* opt, int device, iba_pose_batch** out) {
    return run("iba_pose_optimize", jobs, B, opt, device, false, out);
}

iba_status iba_pose_eval(const iba_pose_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, int device, double* H, double* b, double* chi2_robust,
                         double* const* chi2_edges) {
    const std::string who = "iba_pose_eval: ";
    if (const iba_status s = check_eval(who, jobs, B, H, b, chi2_robust)) return s;
    Limits lim{};
    iba_status s = limits(device, &lim);
    std::vector<double> sums((size_t)B * ps::kSums);
    const std::vector<int32_t> cut = cut_jobs(jobs, B, lim.budget);
    for (size_t c = 0; c + 1 < cut.size() && s == IBA_OK; ++c) s = eval_chunk(jobs, cut[c], cut[c + 1], active, robust, lim, &sums[(size_t)cut[c] * ps::kSums], chi2_edges);
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; return s; }
    for (int32_t j = 0; j < B; ++j) spread(&sums[(size_t)j * ps::kSums], H + 36 * (size_t)j, b + 6 * (size_t)j, chi2_robust + j);
    return IBA_OK;
}

void iba_pose_free(iba_pose_batch* r) { delete r; }

int32_t iba_pose_n_jobs(const iba_pose_batch* r) { return r ? (int32_t)r->job.size() : 0; }

iba_status iba_pose_read(const iba_pose_batch* r, int32_t job, iba_pose_result* result) {
    if (const iba_status s = check_job_index(r, job, "iba_pose_read: ")) return s;
    if (!result) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_pose_read: result is NULL");
    *result = r->job[(size_t)job].r;
    return IBA_OK;
}

iba_status iba_pose_edges(const iba_pose_batch* r, int32_t job, uint8_t* outlier, float* chi2) {
    if (const iba_status s = check_job_index(r, job, "iba_pose_edges: ")) return s;
    const size_t n = r->outlier[(size_t)job].size();
    if (outlier && n) std::memcpy(outlier, r->outlier[(size_t)job].data(), n);
    if (chi2 && n) std::memcpy(chi2, r->chi2[(size_t)job].data(), sizeof(float) * n);
    return IBA_OK;
}

iba_status iba_pose_stage(const iba_pose_batch* r, int32_t job, int32_t round, double Tcw12[12]) {
    const std::string who = "iba_pose_stage: ";
    if (const iba_status s = check_job_index(r, job, who)) return s;
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    const ps::JobOut& o = r->job[(size_t)job];
    if ((round < 0 || round >= o.r.rounds_run)) return t_err.fail(IBA_ERR_INVALID_ARG, who + "round " + std::to_string(round) + " is outside the job's " + std::to_string(o.r.rounds_run) + " rounds");
    if (!Tcw12) return t_err.fail(IBA_ERR_INVALID_ARG, who + "Tcw12 is NULL");
    std::memcpy(Tcw12, o.stage + 12 * round, 12 * sizeof(double));
    return IBA_OK;
}

iba_status iba_pose_edges_from_matches(const int32_t* match, const int32_t* query_index, int32_t n_queries, const float* last_world_xyz, int32_t n_last, const float* cur_xy,
                                       const int32_t* cur_octave, int32_t n_cur, const float* inv_level_sigma2, int32_t n_levels, float* xyz, float* obs, float* inv_sigma2,
                                       int32_t* keypoint_index, int32_t* n) {
    const std::string why = ps::edges_from_matches(match, query_index, n_queries, last_world_xyz, n_last, cur_xy, cur_octave, n_cur, inv_level_sigma2, n_levels, xyz, obs, inv_sigma2, keypoint_index, n);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_pose_edges_from_matches: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_pose_host(const iba_pose_job* jobs, int32_t B, const iba_pose_options* opt, iba_pose_batch** out) {
    return run("iba_debug_pose_host", jobs, B, opt, 0, true, out);
}

iba_status iba_debug_pose_eval_host(const iba_pose_job* jobs, int32_t B, const uint8_t* const* active, int32_t robust, double* H, double* b, double* chi2_robust,
                                    double* const* chi2_edges) {
    if (const iba_status s = check_eval("iba_debug_pose_eval_host: ", jobs, B, H, b, chi2_robust)) return s;
    for (int32_t j = 0; j < B; ++j)
        ps::host_eval(jobs[j], active ? active[j] : nullptr, robust != 0, H + 36 * (size_t)j, b + 6 * (size_t)j, chi2_robust + j, chi2_edges ? chi2_edges[j] : nullptr);
    return IBA_OK;
}

iba_status iba_debug_pose_series(double s, double out[3]) {
    if (!out || !(s >= 0.0) || !(s <= ps::kPi2)) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_pose_series: out is NULL or s is outside [0, pi^2]");
    for (int k = 0; k < 3; ++k) out[k] = ps::series(s, k + 1);
    return IBA_OK;
}

iba_status iba_debug_pose_exp(const double dx[6], const double T[12], double Tn[12], int32_t* big) {
    if (!dx || !T || !Tn) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_pose_exp: a NULL argument");
    const int g = ps::exp_update(dx, T, Tn);
    if (big) *big = g;
    return IBA_OK;
}

int32_t iba_debug_pose_big_steps(const iba_pose_batch* r) {
    int32_t t = 0;
    if (r) for (const ps::JobOut& o : r->job) t += o.big_steps;
    return t;
}

int32_t iba_debug_pose_chunks(const iba_pose_batch* r) { return r ? r->chunks : 0; }

float iba_debug_pose_kernel_ms(const iba_pose_batch* r) { return r ? r->kernel_ms : 0.f; }

}  // extern "C"

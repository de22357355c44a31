// Two-view initialisation (include/iba_mi355x.h, iba_twoview*): the C ABI, the result object's accessors and the launch chain of a call. The kernels
// are iba_twoview_kernels.hpp, the arithmetic iba_twoview_math.hpp, the host rules (argument checks, T1, the set generator, the host restatement, the
// last step with acos) iba_twoview_host.hpp. A per-call unit (iba_call.hpp): every pair is prepared on the host; the chain of a chunk of pairs:
// tables up, seven kernels, results down. The result is host memory.
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
#include "iba_twoview_host.hpp"
#include "iba_twoview_kernels.hpp"

using iba::DevBuf;
namespace tv = iba::tv;

namespace {
thread_local iba::CallError t_err;

constexpr uint64_t kBudgetBytes = 1ull << 30;
// device bytes of a pair: per match 32 (coordinates) + 2 (flags) + 8 x 17 (points, cosine, verdict per hypothesis) + 17 (the candidate's), per iteration 32 (set) + 116
uint64_t pair_bytes(int32_t N, int32_t I) { return 187ull * (uint64_t)N + 148ull * (uint64_t)I + sizeof(tv::PairRec) + sizeof(iba_twoview_result) + 8 * sizeof(tv::Cam); }

// one chain: the pairs [a, b) of the call, already prepared and their results started
iba_status run_chunk(iba_twoview_batch* res, const std::vector<tv::PairPrep>& prep, int32_t a, int32_t b, bool timing) {
    const iba_twoview_options& opt = res->opt;
    const int32_t nP = b - a, I = opt.iterations;
    hipStream_t st = nullptr;
    // the host arrays of the chain first, then its device buffers, then the guard: it waits for the stream before any of them unwinds
    std::vector<tv::PairRec> recs((size_t)nP);
    std::vector<float> h_mxy, h_mn, h_pts, h_cos, h_Hi, h_H12i, h_Fi, h_sH, h_sF;
    std::vector<int32_t> h_sets, h_aux;
    std::vector<iba_twoview_result> h_res;
    std::vector<tv::Cam> h_cams;
    std::vector<uint8_t> h_inl, h_verdict;
    int32_t hits = 0;
    DevBuf<tv::PairRec> d_pairs; DevBuf<float4> d_mxy, d_mn; DevBuf<int32_t> d_sets, d_aux, d_hits; DevBuf<float> d_Hi, d_H12i, d_Fi, d_sH, d_sF, d_pts, d_cos;
    DevBuf<uint8_t> d_inl, d_verdict, d_sel_verdict; DevBuf<iba_twoview_result> d_res; DevBuf<tv::Cam> d_cams; DevBuf<float> d_sel_pts, d_sel_cos;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);
    size_t M = 0;
    int32_t maxN = 0;
    for (int32_t k = 0; k < nP; ++k) {
        const tv::PairPrep& q = prep[(size_t)(a + k)];
        tv::PairRec& r = recs[(size_t)k];
        r.m_base = (int32_t)M; r.N = q.N >= 8 ? q.N : 0;
        r.fx = q.fx; r.fy = q.fy; r.cx = q.cx; r.cy = q.cy;
        std::memcpy(r.T1, q.T1, sizeof(r.T1)); std::memcpy(r.T2inv, q.T2inv, sizeof(r.T2inv)); std::memcpy(r.T2t, q.T2t, sizeof(r.T2t));
        M += (size_t)r.N; maxN = std::max(maxN, r.N);
    }
    if (maxN == 0) { sync.disarm(); return IBA_OK; }  // every pair of the chunk has its status already: nothing was queued
    if (8ull * M >= (1ull << 31) || (uint64_t)nP * (uint64_t)I * 9ull >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "a chunk of 2^31 per-hypothesis entries or more");
    const size_t nI = (size_t)nP * (size_t)I;
    h_mxy.resize(4 * M); h_mn.resize(4 * M);
    h_sets.assign(8 * nI, 0);
    for (int32_t k = 0; k < nP; ++k) {
        const tv::PairPrep& q = prep[(size_t)(a + k)];
        const tv::PairRec& r = recs[(size_t)k];
        if (!r.N) continue;
        std::memcpy(&h_mxy[4 * (size_t)r.m_base], q.mxy.data(), sizeof(float) * 4 * (size_t)r.N); std::memcpy(&h_mn[4 * (size_t)r.m_base], q.mn.data(), sizeof(float) * 4 * (size_t)r.N);
        std::memcpy(&h_sets[8 * (size_t)k * (size_t)I], q.sets.data(), sizeof(int32_t) * 8 * (size_t)I);
    }
    IBA_CALL_TRY(d_pairs.alloc((size_t)nP)); IBA_CALL_TRY(d_mxy.alloc(M)); IBA_CALL_TRY(d_mn.alloc(M)); IBA_CALL_TRY(d_sets.alloc(8 * nI)); IBA_CALL_TRY(d_aux.alloc(4 * (size_t)nP)); IBA_CALL_TRY(d_hits.alloc(1));
    IBA_CALL_TRY(d_Hi.alloc(9 * nI)); IBA_CALL_TRY(d_H12i.alloc(9 * nI)); IBA_CALL_TRY(d_Fi.alloc(9 * nI)); IBA_CALL_TRY(d_sH.alloc(nI)); IBA_CALL_TRY(d_sF.alloc(nI));
    IBA_CALL_TRY(d_pts.alloc(24 * M)); IBA_CALL_TRY(d_cos.alloc(8 * M)); IBA_CALL_TRY(d_inl.alloc(2 * M)); IBA_CALL_TRY(d_verdict.alloc(8 * M)); IBA_CALL_TRY(d_res.alloc((size_t)nP)); IBA_CALL_TRY(d_cams.alloc(8 * (size_t)nP));
    const bool keep = opt.keep_stages != 0;
    if (!keep) { IBA_CALL_TRY(d_sel_pts.alloc(3 * M)); IBA_CALL_TRY(d_sel_cos.alloc(M)); IBA_CALL_TRY(d_sel_verdict.alloc(M)); }
    h_res.resize((size_t)nP);
    for (int32_t k = 0; k < nP; ++k) h_res[(size_t)k] = res->pair[(size_t)(a + k)].r;
    IBA_CALL_TRY(hipMemcpyAsync(d_pairs.p, recs.data(), sizeof(tv::PairRec) * (size_t)nP, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_mxy.p, h_mxy.data(), sizeof(float) * 4 * M, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_mn.p, h_mn.data(), sizeof(float) * 4 * M, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_sets.p, h_sets.data(), sizeof(int32_t) * 8 * nI, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(d_res.p, h_res.data(), sizeof(iba_twoview_result) * (size_t)nP, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemsetAsync(d_aux.p, 0, sizeof(int32_t) * 4 * (size_t)nP, st)); IBA_CALL_TRY(hipMemsetAsync(d_hits.p, 0, sizeof(int32_t), st));
    IBA_CALL_TRY(hipMemsetAsync(d_Hi.p, 0, sizeof(float) * 9 * nI, st)); IBA_CALL_TRY(hipMemsetAsync(d_H12i.p, 0, sizeof(float) * 9 * nI, st)); IBA_CALL_TRY(hipMemsetAsync(d_Fi.p, 0, sizeof(float) * 9 * nI, st));
    IBA_CALL_TRY(hipMemsetAsync(d_sH.p, 0, sizeof(float) * nI, st)); IBA_CALL_TRY(hipMemsetAsync(d_sF.p, 0, sizeof(float) * nI, st));
    IBA_CALL_TRY(hipMemsetAsync(d_pts.p, 0, sizeof(float) * 24 * M, st)); IBA_CALL_TRY(hipMemsetAsync(d_cos.p, 0, sizeof(float) * 8 * M, st));
    IBA_CALL_TRY(hipMemsetAsync(d_inl.p, 0, 2 * M, st)); IBA_CALL_TRY(hipMemsetAsync(d_verdict.p, 0, 8 * M, st)); IBA_CALL_TRY(hipMemsetAsync(d_cams.p, 0, sizeof(tv::Cam) * 8 * (size_t)nP, st));
    if (timing) IBA_CALL_TRY(ev.create(8));
    const float invs = tv::inv_sigma_square(opt.sigma), sigma2 = opt.sigma * opt.sigma, th2 = (float)(4.0 * (double)sigma2);
    const uint32_t pair_blocks = (uint32_t)((nP + 63) / 64);
    int stage = 0;
#define TV_STAGE() do { IBA_CALL_TRY(hipGetLastError()); if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[(size_t)++stage], st)); } while (0)
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(tv::tv_hyp_kernel, dim3((uint32_t)((nI + tv::kHypLanes - 1) / tv::kHypLanes), 2), dim3(tv::kHypLanes), 0, st, d_pairs.p, (int)I, (int)nI, d_sets.p, d_mn.p, d_Hi.p, d_H12i.p,
                       d_Fi.p, d_hits.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_score_kernel, dim3((uint32_t)((I + 63) / 64), 2, (uint32_t)nP), dim3(64), 0, st, d_pairs.p, (int)I, d_mxy.p, d_Hi.p, d_H12i.p, d_Fi.p, invs, d_sH.p, d_sF.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_select_kernel, dim3((uint32_t)nP), dim3(128), 0, st, d_pairs.p, (int)I, d_mxy.p, d_Hi.p, d_H12i.p, d_Fi.p, d_sH.p, d_sF.p, invs, opt.rh_threshold, d_inl.p, M, d_res.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_motion_kernel, dim3(pair_blocks), dim3(64), 0, st, d_pairs.p, (int)nP, d_res.p, d_cams.p, d_hits.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_checkrt_kernel, dim3((uint32_t)((maxN + tv::kRtThreads - 1) / tv::kRtThreads), 8, (uint32_t)nP), dim3(tv::kRtThreads), 0, st, d_pairs.p, d_mxy.p, d_inl.p, M, th2, d_res.p,
                       d_cams.p, d_pts.p, d_cos.p, d_verdict.p, d_hits.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_kth_kernel, dim3(8, (uint32_t)nP), dim3(256), 0, st, d_pairs.p, d_res.p, d_cos.p, d_verdict.p);
    TV_STAGE();
    hipLaunchKernelGGL(tv::tv_accept_kernel, dim3(pair_blocks), dim3(64), 0, st, d_pairs.p, (int)nP, (int)opt.min_triangulated, d_res.p, d_aux.p);
    if (!keep) {                                      // without the stages only the candidate hypothesis' entries come down
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(tv::tv_gather_kernel, dim3((uint32_t)((maxN + tv::kRtThreads - 1) / tv::kRtThreads), (uint32_t)nP), dim3(tv::kRtThreads), 0, st, d_pairs.p, d_res.p, d_aux.p, d_pts.p, d_cos.p,
                           d_verdict.p, d_sel_pts.p, d_sel_cos.p, d_sel_verdict.p);
    }
    TV_STAGE();
#undef TV_STAGE
    // ---- everything down ----
    h_aux.resize(4 * (size_t)nP);
    h_cams.resize(8 * (size_t)nP);
    h_inl.resize(2 * M); h_verdict.resize(keep ? 8 * M : M);                        // kept: per hypothesis; else the candidate's alone
    h_pts.resize(keep ? 24 * M : 3 * M); h_cos.resize(keep ? 8 * M : M);
    IBA_CALL_TRY(hipMemcpyAsync(h_res.data(), d_res.p, sizeof(iba_twoview_result) * (size_t)nP, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_aux.data(), d_aux.p, sizeof(int32_t) * 4 * (size_t)nP, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_cams.data(), d_cams.p, sizeof(tv::Cam) * 8 * (size_t)nP, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_inl.data(), d_inl.p, 2 * M, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_verdict.data(), keep ? d_verdict.p : d_sel_verdict.p, h_verdict.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_pts.data(), keep ? d_pts.p : d_sel_pts.p, sizeof(float) * h_pts.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(h_cos.data(), keep ? d_cos.p : d_sel_cos.p, sizeof(float) * h_cos.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(&hits, d_hits.p, sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (keep) {
        h_Hi.resize(9 * nI); h_H12i.resize(9 * nI); h_Fi.resize(9 * nI); h_sH.resize(nI); h_sF.resize(nI);
        IBA_CALL_TRY(hipMemcpyAsync(h_Hi.data(), d_Hi.p, sizeof(float) * 9 * nI, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(h_H12i.data(), d_H12i.p, sizeof(float) * 9 * nI, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(h_Fi.data(), d_Fi.p, sizeof(float) * 9 * nI, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(h_sH.data(), d_sH.p, sizeof(float) * nI, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(h_sF.data(), d_sF.p, sizeof(float) * nI, hipMemcpyDeviceToHost, st));
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (timing)
        for (int k = 0; k < 7; ++k) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[(size_t)k], ev.e[(size_t)k + 1])); res->ms[k] += ms; }
    res->sweeps30 += hits;
    for (int32_t k = 0; k < nP; ++k) {
        const tv::PairRec& r = recs[(size_t)k];
        if (!r.N) continue;
        tv::PairRes& o = res->pair[(size_t)(a + k)];
        const size_t N = (size_t)r.N, mb = (size_t)r.m_base, Is = (size_t)I;
        o.r = h_res[(size_t)k];
        o.cand = h_aux[4 * (size_t)k]; o.fail_before = h_aux[4 * (size_t)k + 1]; o.fail_after = h_aux[4 * (size_t)k + 2];
        o.inlier.assign(h_inl.begin() + (ptrdiff_t)((o.r.model ? 0 : M) + mb), h_inl.begin() + (ptrdiff_t)((o.r.model ? 0 : M) + mb + N));
        for (int hyp = 0; hyp < 8; ++hyp) {
            std::memcpy(o.hyp_R + 9 * hyp, h_cams[8 * (size_t)k + (size_t)hyp].R, 9 * sizeof(float)); std::memcpy(o.hyp_t + 3 * hyp, h_cams[8 * (size_t)k + (size_t)hyp].t, 3 * sizeof(float));
        }
        if (keep) {
            o.hyp_pts.assign(h_pts.begin() + (ptrdiff_t)(24 * mb), h_pts.begin() + (ptrdiff_t)(24 * (mb + N)));
            o.hyp_cos.assign(h_cos.begin() + (ptrdiff_t)(8 * mb), h_cos.begin() + (ptrdiff_t)(8 * (mb + N)));
            o.verdict.assign(h_verdict.begin() + (ptrdiff_t)(8 * mb), h_verdict.begin() + (ptrdiff_t)(8 * (mb + N)));
            tv::select_from_stages(o);
        } else if (o.r.status == 0 && o.fail_before == 0) {
            o.sel_pts.assign(h_pts.begin() + (ptrdiff_t)(3 * mb), h_pts.begin() + (ptrdiff_t)(3 * (mb + N)));
            o.sel_cos.assign(h_cos.begin() + (ptrdiff_t)mb, h_cos.begin() + (ptrdiff_t)(mb + N));
            o.sel_verdict.assign(h_verdict.begin() + (ptrdiff_t)mb, h_verdict.begin() + (ptrdiff_t)(mb + N));
        }
        if (keep) {
            o.Hi.assign(h_Hi.begin() + (ptrdiff_t)(9 * Is * (size_t)k), h_Hi.begin() + (ptrdiff_t)(9 * Is * ((size_t)k + 1)));
            o.H12i.assign(h_H12i.begin() + (ptrdiff_t)(9 * Is * (size_t)k), h_H12i.begin() + (ptrdiff_t)(9 * Is * ((size_t)k + 1)));
            o.Fi.assign(h_Fi.begin() + (ptrdiff_t)(9 * Is * (size_t)k), h_Fi.begin() + (ptrdiff_t)(9 * Is * ((size_t)k + 1)));
            o.sH.assign(h_sH.begin() + (ptrdiff_t)(Is * (size_t)k), h_sH.begin() + (ptrdiff_t)(Is * ((size_t)k + 1)));
            o.sF.assign(h_sF.begin() + (ptrdiff_t)(Is * (size_t)k), h_sF.begin() + (ptrdiff_t)(Is * ((size_t)k + 1)));
        }
    }
    return IBA_OK;
}

iba_status check_pair_index(const iba_twoview_batch* r, int32_t pair, const std::string& who) {
    return t_err.check_index(!r, pair, r ? r->pair.size() : 0, who, "pair");
}

// the chains of a call: consecutive pairs under the byte budget, at most 32768 and at least one per chunk
iba_status run_chunks(iba_twoview_batch* res, const std::vector<tv::PairPrep>& prep, int device, bool timing) {
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, kBudgetBytes, "IBA_TWOVIEW_BUDGET", &budget));
    std::vector<uint64_t> bytes(prep.size());
    for (size_t b = 0; b < prep.size(); ++b) bytes[b] = pair_bytes(prep[b].N, res->opt.iterations);
    const std::vector<int32_t> cut = iba::cut_chunks(bytes, budget, 32768);
    for (size_t c = 0; c + 1 < cut.size(); ++c) {
        ++res->chunks;
        if (const iba_status s = run_chunk(res, prep, cut[c], cut[c + 1], timing)) return s;
    }
    return IBA_OK;
}

iba_status run(const char* name, const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt, int device, bool on_host, iba_twoview_batch** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    const std::string why = tv::check_call(pairs, B, opt);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_twoview_batch* res = new iba_twoview_batch();
    res->opt = *opt;
    res->pair.resize((size_t)B);
    std::vector<tv::PairPrep> prep((size_t)B);
    for (int32_t b = 0; b < B; ++b) tv::prepare(pairs[b], opt->iterations, prep[(size_t)b]);
    iba_status s = IBA_OK;
    if (on_host) {
        for (int32_t b = 0; b < B; ++b) tv::host_pair(prep[(size_t)b], *opt, res->pair[(size_t)b], &res->sweeps30);
    } else {
        for (int32_t b = 0; b < B; ++b) tv::start_result(prep[(size_t)b], res->pair[(size_t)b]);
        const bool timing = iba::debug_env("IBA_TWOVIEW_TIMING") != nullptr;
        s = run_chunks(res, prep, device, timing);
        if (s == IBA_OK)
            for (int32_t b = 0; b < B; ++b) tv::finish(*opt, opt->keep_stages != 0, res->pair[(size_t)b]);
    }
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

}  // namespace

extern "C" {

const char* iba_twoview_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_twoview_options(iba_twoview_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_twoview_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->sigma = 1.0f; opt->iterations = 200; opt->min_parallax_deg = 1.0f; opt->min_triangulated = 50; opt->rh_threshold = 0.40f; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_twoview_init(const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt, int device, iba_twoview_batch** out) {
    return run("iba_twoview_init", pairs, B, opt, device, false, out);
}

void iba_twoview_free(iba_twoview_batch* r) { delete r; }

int32_t iba_twoview_n_pairs(const iba_twoview_batch* r) { return r ? (int32_t)r->pair.size() : 0; }

iba_status iba_twoview_read(const iba_twoview_batch* r, int32_t pair, iba_twoview_result* result) {
    if (const iba_status s = check_pair_index(r, pair, "iba_twoview_read: ")) return s;
    if (!result) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_twoview_read: result is NULL");
    *result = r->pair[(size_t)pair].r;
    return IBA_OK;
}

iba_status iba_twoview_matches(const iba_twoview_batch* r, int32_t pair, int32_t* list, uint8_t* inlier) {
    if (const iba_status s = check_pair_index(r, pair, "iba_twoview_matches: ")) return s;
    const tv::PairRes& o = r->pair[(size_t)pair];
    if (list && o.N) std::memcpy(list, o.list.data(), sizeof(int32_t) * 2 * (size_t)o.N);
    if (inlier && o.N) std::memcpy(inlier, o.inlier.data(), (size_t)o.N);
    return IBA_OK;
}

iba_status iba_twoview_points(const iba_twoview_batch* r, int32_t pair, float* points, uint8_t* triangulated) {
    if (const iba_status s = check_pair_index(r, pair, "iba_twoview_points: ")) return s;
    const tv::PairRes& o = r->pair[(size_t)pair];
    if (points && o.n1) std::memcpy(points, o.points.data(), sizeof(float) * 3 * (size_t)o.n1);
    if (triangulated && o.n1) std::memcpy(triangulated, o.tri.data(), (size_t)o.n1);
    return IBA_OK;
}

iba_status iba_twoview_iterations(const iba_twoview_batch* r, int32_t pair, float* Hi, float* H12i, float* Fi, float* score_H, float* score_F) {
    const std::string who = "iba_twoview_iterations: ";
    if (const iba_status s = check_pair_index(r, pair, who)) return s;
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    const tv::PairRes& o = r->pair[(size_t)pair];
    const size_t I = (size_t)r->opt.iterations;
    const auto put = [](float* dst, const std::vector<float>& src, size_t n) {
        if (!dst) return;
        if (src.size() == n) std::memcpy(dst, src.data(), sizeof(float) * n); else std::memset(dst, 0, sizeof(float) * n);
    };
    put(Hi, o.Hi, 9 * I); put(H12i, o.H12i, 9 * I); put(Fi, o.Fi, 9 * I); put(score_H, o.sH, I); put(score_F, o.sF, I);
    return IBA_OK;
}

iba_status iba_twoview_hypothesis(const iba_twoview_batch* r, int32_t pair, int32_t hyp, float R[9], float t[3], int32_t* n_good, float* points, uint8_t* verdict) {
    const std::string who = "iba_twoview_hypothesis: ";
    if (const iba_status s = check_pair_index(r, pair, who)) return s;
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    if (hyp < 0 || hyp >= 8) return t_err.fail(IBA_ERR_INVALID_ARG, who + "hypothesis " + std::to_string(hyp) + " is outside 0..7");
    const tv::PairRes& o = r->pair[(size_t)pair];
    const size_t N = (size_t)o.N;
    if (R) std::memcpy(R, o.hyp_R + 9 * hyp, 9 * sizeof(float));
    if (t) std::memcpy(t, o.hyp_t + 3 * hyp, 3 * sizeof(float));
    if (n_good) *n_good = o.r.n_good[hyp];
    const bool have = o.verdict.size() == 8 * N && N;
    if (points && N) { if (have) std::memcpy(points, &o.hyp_pts[3 * (size_t)hyp * N], sizeof(float) * 3 * N); else std::memset(points, 0, sizeof(float) * 3 * N); }
    if (verdict && N) { if (have) std::memcpy(verdict, &o.verdict[(size_t)hyp * N], N); else std::memset(verdict, 0, N); }
    return IBA_OK;
}

iba_status iba_twoview_normalize(const float* xy, int32_t n, float* out_xy, float T[9]) {
    if (n < 0 || !T || (n && (!xy || !out_xy))) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_twoview_normalize: n < 0 or a NULL argument");
    for (int32_t i = 0; i < 2 * n; ++i) if (!std::isfinite(xy[i])) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_twoview_normalize: position " + std::to_string(i / 2) + " is not finite");
    tv::normalize(xy, n, out_xy, T);
    return IBA_OK;
}

iba_status iba_twoview_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out) {
    const std::string why = tv::make_sets(N, iterations, seed, out);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_twoview_sets: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_twoview_host(const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt, iba_twoview_batch** out) {
    return run("iba_debug_twoview_host", pairs, B, opt, 0, true, out);
}

iba_status iba_debug_twoview_null_vector(const float* A, int32_t m, int32_t n, float* v, double* v64, int32_t* sweeps) {
    if (!A || !v || !sweeps) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_twoview_null_vector: a NULL argument");
    double G[144], V[81];
    for (int32_t i = 0; i < m * n && i < 144; ++i) G[i] = (double)A[i];
    if (m == 16 && n == 9) *sweeps = tv::null_vector<16, 9, 1, 0>(G, V, v);
    else if (m == 8 && n == 9) *sweeps = tv::null_vector<8, 9, 1, 0>(G, V, v);
    else if (m == 4 && n == 4) *sweeps = tv::null_vector<4, 4, 1, 1>(G, V, v);
    else if (m == 3 && n == 3) *sweeps = tv::null_vector<3, 3, 1, 1>(G, V, v);
    else return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_twoview_null_vector: the sizes are 16 x 9, 8 x 9, 4 x 4 and 3 x 3");
    if (v64)                                          // the column v was rounded from: the one of V that rounds to it
        for (int32_t c = 0; c < n; ++c) {
            bool is = true;
            for (int32_t i = 0; i < n; ++i) is = is && (float)V[i * n + c] == v[i];
            if (is) { for (int32_t i = 0; i < n; ++i) v64[i] = V[i * n + c]; break; }
        }
    return IBA_OK;
}

int32_t iba_debug_twoview_sweep_cap_hits(const iba_twoview_batch* r) { return r ? r->sweeps30 : 0; }

int32_t iba_debug_twoview_chunks(const iba_twoview_batch* r) { return r ? r->chunks : 0; }

iba_status iba_debug_twoview_stage_ms(const iba_twoview_batch* r, float ms[7]) {
    if (!r || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_twoview_stage_ms: a NULL argument");
    std::memcpy(ms, r->ms, sizeof(r->ms));
    return IBA_OK;
}

}  // extern "C"

// Two-view initialisation, the kernels of one launch chain (include/iba_mi355x.h, iba_twoview*; launched by iba_twoview.hip). All arithmetic is
// iba_twoview_math.hpp, the text the host restatement compiles too. The tables of a chunk of pairs are flat: a pair's matches start at m_base, its
// iterations at pair * I, its 8 x N per-hypothesis entries at 8 * m_base + hyp * N. A pair with fewer than 8 matches is on the device with N = 0
// and every kernel leaves it alone. Only integer counts are combined by atomics; no float is summed in an order that depends on arrival.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/iba_mi355x.h"
#include "iba_twoview_math.hpp"

namespace iba {
namespace tv {

constexpr int kHypLanes = 32;     // lanes of a hypothesis block: kWorkDoubles doubles each in a lane-minor slab, 57600 bytes of LDS
constexpr int kRtThreads = 256;

struct PairRec {
    int32_t m_base, N;
    float fx, fy, cx, cy;
    float T1[9], T2inv[9], T2t[9];
};

// 1. one lane per (pair, iteration); blockIdx.y = 0 builds H21i and H12i (T3), 1 builds F21i (T4). The work matrices of T2 (225 doubles for the
// 16 x 9 case) live in LDS, element e of lane l at slab[e * kHypLanes + l]: consecutive lanes on consecutive 8-byte words, no bank conflict.
__global__ __launch_bounds__(kHypLanes) void tv_hyp_kernel(const PairRec* __restrict__ pairs, int I, int n_items, const int32_t* __restrict__ sets, const float4* __restrict__ mn,
                                                           float* __restrict__ Hi, float* __restrict__ H12i, float* __restrict__ Fi, int32_t* cap_hits) {
    __shared__ double slab[kWorkDoubles * kHypLanes];
    const int g = (int)blockIdx.x * kHypLanes + (int)threadIdx.x;
    if (g >= n_items) return;
    const PairRec& pr = pairs[g / I];
    if (pr.N == 0) return;
    float pn[32];
    for (int j = 0; j < 8; ++j) {
        const float4 v = mn[pr.m_base + sets[8 * (size_t)g + j]];
        pn[4 * j] = v.x; pn[4 * j + 1] = v.y; pn[4 * j + 2] = v.z; pn[4 * j + 3] = v.w;
    }
    double* ws = slab + threadIdx.x;
    int sweeps;
    if (blockIdx.y == 0) {
        float H[9], Hinv[9];
        sweeps = h_hypothesis<kHypLanes>(pn, pr.T1, pr.T2inv, ws, H, Hinv);
        for (int k = 0; k < 9; ++k) { Hi[9 * (size_t)g + k] = canon(H[k]); H12i[9 * (size_t)g + k] = canon(Hinv[k]); }
    } else {
        float F[9];
        sweeps = f_hypothesis<kHypLanes>(pn, pr.T1, pr.T2t, ws, F);
        for (int k = 0; k < 9; ++k) Fi[9 * (size_t)g + k] = canon(F[k]);
    }
    if (sweeps == kMaxSweeps) atomicAdd(cap_hits, 1);
}

// 2. the hot kernel: one lane per hypothesis, a wave = 64 iterations of ONE pair and model (blockIdx.y: 0 = H, 1 = F), so the match coordinates are
// wave-uniform and come through scalar loads. The lane keeps T5's sequential float32 sum in a register; nothing is reduced across lanes.
__global__ __launch_bounds__(64) void tv_score_kernel(const PairRec* __restrict__ pairs, int I, const float4* __restrict__ mxy, const float* __restrict__ Hi, const float* __restrict__ H12i,
                                                      const float* __restrict__ Fi, float invSigmaSquare, float* __restrict__ sH, float* __restrict__ sF) {
    const int p = (int)blockIdx.z;
    const int N = pairs[p].N;
    if (N == 0) return;
    const float4* __restrict__ m = mxy + pairs[p].m_base;
    const int it = (int)blockIdx.x * 64 + (int)threadIdx.x;
    const bool live = it < I;
    const size_t h = (size_t)p * (size_t)I + (size_t)(live ? it : I - 1);
    float a[9], b[9], s = 0.f;
    if (blockIdx.y == 0) {
        for (int k = 0; k < 9; ++k) { a[k] = Hi[9 * h + k]; b[k] = H12i[9 * h + k]; }
        for (int i = 0; i < N; ++i) { const float4 v = m[i]; score_h_match(a, b, v.x, v.y, v.z, v.w, invSigmaSquare, s); }
        if (live) sH[h] = canon(s);
    } else {
        for (int k = 0; k < 9; ++k) a[k] = Fi[9 * h + k];
        for (int i = 0; i < N; ++i) { const float4 v = m[i]; score_f_match(a, v.x, v.y, v.z, v.w, invSigmaSquare, s); }
        if (live) sF[h] = canon(s);
    }
}

// 3. T6: one block per pair, wave 0 takes H and wave 1 takes F: the lowest iteration among the strictly greatest score above 0, then the winner's
// inlier flags (inl[which * M + match], which: 0 = H, 1 = F) and their count; thread 0 forms RH and the path.
__global__ __launch_bounds__(128) void tv_select_kernel(const PairRec* __restrict__ pairs, int I, const float4* __restrict__ mxy, const float* __restrict__ Hi, const float* __restrict__ H12i,
                                                        const float* __restrict__ Fi, const float* __restrict__ sH, const float* __restrict__ sF, float invSigmaSquare, float rh_threshold,
                                                        uint8_t* __restrict__ inl, size_t M, iba_twoview_result* __restrict__ res) {
    __shared__ float s_best[2];
    __shared__ int s_it[2], s_cnt[2];
    const int p = (int)blockIdx.x;
    const int N = pairs[p].N;
    if (N == 0) return;
    const int which = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const float* s = (which == 0 ? sH : sF) + (size_t)p * (size_t)I;
    float best = 0.0f;
    int bit = -1;
    for (int it = lane; it < I; it += 64) { const float v = s[it]; if (v > best) { best = v; bit = it; } }
    for (int off = 32; off >= 1; off >>= 1) {
        const float ob = __shfl_xor(best, off);
        const int oi = __shfl_xor(bit, off);
        if (ob > best || (ob == best && oi < bit)) { best = ob; bit = oi; }
    }
    int cnt = 0;
    if (bit >= 0) {
        const size_t h = (size_t)p * (size_t)I + (size_t)bit;
        const float4* m = mxy + pairs[p].m_base;
        uint8_t* flag = inl + (size_t)which * M + (size_t)pairs[p].m_base;
        float a[9], b[9], dummy = 0.f;
        for (int k = 0; k < 9; ++k) { a[k] = which == 0 ? Hi[9 * h + k] : Fi[9 * h + k]; b[k] = which == 0 ? H12i[9 * h + k] : 0.f; }
        for (int i = lane; i < N; i += 64) {
            const float4 v = m[i];
            const bool in = which == 0 ? score_h_match(a, b, v.x, v.y, v.z, v.w, invSigmaSquare, dummy) : score_f_match(a, v.x, v.y, v.z, v.w, invSigmaSquare, dummy);
            flag[i] = in ? 1 : 0;
            cnt += in ? 1 : 0;
        }
        if (lane < 9) { if (which == 0) res[p].H21[lane] = a[lane]; else res[p].F21[lane] = a[lane]; }
    }
    for (int off = 32; off >= 1; off >>= 1) cnt += __shfl_xor(cnt, off);
    if (lane == 0) { s_best[which] = best; s_it[which] = bit; s_cnt[which] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        iba_twoview_result& r = res[p];
        r.SH = s_best[0]; r.SF = s_best[1]; r.best_it_H = s_it[0]; r.best_it_F = s_it[1]; r.n_inliers_H = s_cnt[0]; r.n_inliers_F = s_cnt[1];
        const float SH = s_best[0], SF = s_best[1];
        r.RH = SH + SF > 0.f ? SH / (SH + SF) : 0.f;
        r.model = r.RH > rh_threshold ? 1 : 0;
    }
}

// 4. T7 / T8: one lane per pair; the cameras of T9 per hypothesis
__global__ __launch_bounds__(64) void tv_motion_kernel(const PairRec* __restrict__ pairs, int nP, iba_twoview_result* __restrict__ res, Cam* __restrict__ cams, int32_t* cap_hits) {
    const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (p >= nP || pairs[p].N == 0) return;
    iba_twoview_result& r = res[p];
    if ((r.model ? r.best_it_H : r.best_it_F) < 0) { r.status = kNoModel; return; }
    float K[9], R[72], t[24];
    make_K(pairs[p].fx, pairs[p].fy, pairs[p].cx, pairs[p].cy, K);
    int sweeps = 0, n_hyp;
    if (r.model == 0) { sweeps = motions_from_f(r.F21, K, R, t); n_hyp = 4; }
    else { n_hyp = motions_from_h(r.H21, K, R, t, &sweeps) ? 8 : 0; }
    if (sweeps == kMaxSweeps) atomicAdd(cap_hits, 1);
    if (n_hyp == 0) { r.status = kHDegenerate; return; }
    r.n_hyp = n_hyp;
    for (int k = 0; k < n_hyp; ++k) make_cam(K, R + 9 * k, t + 3 * k, cams[(size_t)p * 8 + (size_t)k]);
}

// 5. T9: one lane per (pair, hypothesis, match): grid (blocks over the longest list, 8, pairs)
__global__ __launch_bounds__(kRtThreads) void tv_checkrt_kernel(const PairRec* __restrict__ pairs, const float4* __restrict__ mxy, const uint8_t* __restrict__ inl, size_t M, float th2,
                                                                 iba_twoview_result* res, const Cam* __restrict__ cams, float* __restrict__ pts, float* __restrict__ cosv,
                                                                 uint8_t* __restrict__ verdict, int32_t* cap_hits) {
    const int p = (int)blockIdx.z, k = (int)blockIdx.y;
    const PairRec& pr = pairs[p];
    const int N = pr.N;
    if (N == 0 || res[p].status != 0 || k >= res[p].n_hyp) return;
    const int i = (int)blockIdx.x * kRtThreads + (int)threadIdx.x;
    bool good = false;
    if (i < N && inl[(size_t)(res[p].model ? 0 : 1) * M + (size_t)pr.m_base + (size_t)i]) {
        const Cam cam = cams[(size_t)p * 8 + (size_t)k];
        const float4 v = mxy[pr.m_base + i];
        float q[3], c;
        int sweeps = 0;
        const int verd = check_rt_match(cam, pr.fx, pr.fy, pr.cx, pr.cy, v.x, v.y, v.z, v.w, th2, q, &c, &sweeps);
        const size_t at = 8 * (size_t)pr.m_base + (size_t)k * (size_t)N + (size_t)i;
        verdict[at] = (uint8_t)verd; cosv[at] = canon(c);
        pts[3 * at] = q[0]; pts[3 * at + 1] = q[1]; pts[3 * at + 2] = q[2];
        good = verd == 6;
        if (sweeps == kMaxSweeps) atomicAdd(cap_hits, 1);
    }
    const unsigned long long ballot = __ballot(good);
    if (((int)threadIdx.x & 63) == 0 && ballot) atomicAdd(&res[p].n_good[k], (int32_t)__popcll(ballot));
}

// 6. the good cosines' value at sorted position min(50, n_good - 1): a radix select over the ordered keys, 8 bits a pass, integer histograms in LDS
__global__ __launch_bounds__(256) void tv_kth_kernel(const PairRec* __restrict__ pairs, iba_twoview_result* res, const float* __restrict__ cosv, const uint8_t* __restrict__ verdict) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_prefix, s_target;
    const int p = (int)blockIdx.y, k = (int)blockIdx.x;
    const int N = pairs[p].N;
    if (N == 0 || res[p].status != 0 || k >= res[p].n_hyp) return;
    const int n_good = res[p].n_good[k];
    if (n_good == 0) { if (threadIdx.x == 0) res[p].cos_parallax[k] = 1.0f; return; }
    const size_t base = 8 * (size_t)pairs[p].m_base + (size_t)k * (size_t)N;
    uint32_t prefix = 0, mask = 0, target = (uint32_t)(n_good - 1 < 50 ? n_good - 1 : 50);
    for (int shift = 24; shift >= 0; shift -= 8) {
        hist[threadIdx.x] = 0;
        __syncthreads();
        for (int i = (int)threadIdx.x; i < N; i += 256) {
            if (verdict[base + (size_t)i] != 6) continue;
            const uint32_t key = cos_key(cosv[base + (size_t)i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0, b = 0;
            for (; b < 255; ++b) { if (target < acc + hist[b]) break; acc += hist[b]; }
            s_prefix = prefix | (b << shift); s_target = target - acc;
        }
        __syncthreads();
        prefix = s_prefix; target = s_target; mask |= 255u << shift;
    }
    if (threadIdx.x == 0) res[p].cos_parallax[k] = canon(cos_unkey(prefix));
}

// 7. T10 up to the parallax test (acos is the host's): one lane per pair writes (cand, fail_before, fail_after)
__global__ __launch_bounds__(64) void tv_accept_kernel(const PairRec* __restrict__ pairs, int nP, int min_triangulated, const iba_twoview_result* __restrict__ res, int32_t* __restrict__ aux) {
    const int p = (int)blockIdx.x * 64 + (int)threadIdx.x;
    if (p >= nP || pairs[p].N == 0 || res[p].status != 0) return;
    const iba_twoview_result& r = res[p];
    const Accept a = r.model ? accept_h(r.n_good, r.n_inliers_H, min_triangulated) : accept_f(r.n_good, r.n_inliers_F, min_triangulated);
    aux[4 * p] = a.cand; aux[4 * p + 1] = a.fail_before; aux[4 * p + 2] = a.fail_after;
}

// 8. the candidate hypothesis' per-match entries, compact at the match's own index: all the host's last step reads where the stages are not kept
__global__ __launch_bounds__(kRtThreads) void tv_gather_kernel(const PairRec* __restrict__ pairs, const iba_twoview_result* __restrict__ res, const int32_t* __restrict__ aux,
                                                                const float* __restrict__ pts, const float* __restrict__ cosv, const uint8_t* __restrict__ verdict,
                                                                float* __restrict__ sel_pts, float* __restrict__ sel_cos, uint8_t* __restrict__ sel_verdict) {
    const int p = (int)blockIdx.y;
    const int N = pairs[p].N;
    if (N == 0 || res[p].status != 0 || aux[4 * p + 1] != 0) return;
    const int i = (int)blockIdx.x * kRtThreads + (int)threadIdx.x;
    if (i >= N) return;
    const size_t at = 8 * (size_t)pairs[p].m_base + (size_t)aux[4 * p] * (size_t)N + (size_t)i, to = (size_t)pairs[p].m_base + (size_t)i;
    sel_verdict[to] = verdict[at]; sel_cos[to] = cosv[at];
    sel_pts[3 * to] = pts[3 * at]; sel_pts[3 * to + 1] = pts[3 * at + 1]; sel_pts[3 * to + 2] = pts[3 * at + 2];
}

}  // namespace tv
}  // namespace iba

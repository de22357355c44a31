// Sim3 RANSAC, the kernels of a chunk's chain (include/iba_mi355x.h, iba_sim3* DEVICE): preparation, hypotheses, the count kernel in its two forms,
// selection, flags. The arithmetic is iba_sim3_math.hpp, the text the host restatement compiles too. Every kernel checks its bounds against the
// job record; blocks never straddle a job, so a job's pose, intrinsics and bases are uniform per block. Nothing is combined by an atomic.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_sim3_math.hpp"

namespace iba {
namespace z3 {

struct JobRec {
    int32_t c_base, N;           // the job's correspondences in the chunk's flat arrays; N == 0: nothing runs
    int32_t h_base, I;           // its hypotheses
    float K1[4], K2[4], T1[12], T2[12];
};
constexpr int kSelInts = 4 + IBA_SIM3_MAX_EVENTS;   // per job: n_events, best_it, best_n, sweep cap hits, the listed events' iterations
constexpr int kTile = IBA_SIM3_TILE;
constexpr int kPrepThreads = 256, kHypThreads = 64, kFlagThreads = 256, kCountBThreads = 256;

// Z2: grid (ceil(maxN / kPrepThreads), jobs). ca = (Xc1, u1), cb = (Xc2, v1), cc = (u2, v2, max_err1, max_err2)
__global__ __launch_bounds__(kPrepThreads) void z3_prep_kernel(const JobRec* __restrict__ jobs, const float4* __restrict__ w1, const float4* __restrict__ w2, const float2* __restrict__ th,
                                                                float4* __restrict__ ca, float4* __restrict__ cb, float4* __restrict__ cc) {
    const JobRec& J = jobs[blockIdx.y];
    const int i = (int)(blockIdx.x * kPrepThreads + threadIdx.x);
    if (i >= J.N) return;
    const size_t g = (size_t)J.c_base + (size_t)i;
    const float4 a = w1[g], b = w2[g];
    const float2 e = th[g];
    float c1[3], c2[3], u1, v1, u2, v2;
    to_camera(J.T1, a.x, a.y, a.z, c1); to_camera(J.T2, b.x, b.y, b.z, c2);
    to_image(J.K1, c1[0], c1[1], c1[2], &u1, &v1); to_image(J.K2, c2[0], c2[1], c2[2], &u2, &v2);
    ca[g] = make_float4(c1[0], c1[1], c1[2], u1); cb[g] = make_float4(c2[0], c2[1], c2[2], v1); cc[g] = make_float4(u2, v2, e.x, e.y);
}

// Z3 / Z4: grid (ceil(maxI / kHypThreads), jobs), one lane per iteration. cap[h] = 1 where the Jacobi ran to the cap.
__global__ __launch_bounds__(kHypThreads) void z3_hyp_kernel(const JobRec* __restrict__ jobs, const int32_t* __restrict__ sets, const float4* __restrict__ ca, const float4* __restrict__ cb,
                                                              int fix_scale, float* __restrict__ srt, float* __restrict__ T12, float* __restrict__ T21, uint8_t* __restrict__ cap) {
    const JobRec& J = jobs[blockIdx.y];
    const int it = (int)(blockIdx.x * kHypThreads + threadIdx.x);
    if (it >= J.I) return;
    const size_t h = (size_t)J.h_base + (size_t)it;
    float P1[9], P2[9];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        int idx = sets[3 * h + j];
        idx = idx < 0 ? 0 : (idx >= J.N ? J.N - 1 : idx);            // the host checked it; never read outside the job
        const float4 a = ca[(size_t)J.c_base + (size_t)idx], b = cb[(size_t)J.c_base + (size_t)idx];
        P1[j] = a.x; P1[3 + j] = a.y; P1[6 + j] = a.z; P2[j] = b.x; P2[3 + j] = b.y; P2[6 + j] = b.z;
    }
    float o_srt[13], o12[12], o21[12];
    const int sweeps = horn(P1, P2, fix_scale, o_srt, o12, o21);
#pragma unroll
    for (int k = 0; k < 13; ++k) srt[13 * h + k] = o_srt[k];
#pragma unroll
    for (int k = 0; k < 12; ++k) { T12[12 * h + k] = o12[k]; T21[12 * h + k] = o21[k]; }
    cap[h] = sweeps >= kMaxSweeps ? 1 : 0;
}

// Z5, form (a): grid (ceil(maxI / 64), jobs), one wave per block, a lane per hypothesis with its transforms in registers; the job's correspondences pass
// through LDS kTile at a time and every lane reads entry k at the same address (a broadcast). Lanes beyond I keep loading tiles and score nothing.
__global__ __launch_bounds__(64) void z3_count_a_kernel(const JobRec* __restrict__ jobs, const float4* __restrict__ ca, const float4* __restrict__ cb, const float4* __restrict__ cc,
                                                         const float* __restrict__ T12, const float* __restrict__ T21, int32_t* __restrict__ counts) {
    __shared__ float4 tile[3 * kTile];
    const JobRec& J = jobs[blockIdx.y];
    if ((int)(blockIdx.x * 64) >= J.I) return;                        // uniform per block
    const int it = (int)(blockIdx.x * 64 + threadIdx.x);
    const bool live = it < J.I;
    const size_t h = (size_t)J.h_base + (size_t)(live ? it : 0);
    float t12[12], t21[12], K1[4], K2[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) { t12[k] = T12[12 * h + k]; t21[k] = T21[12 * h + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { K1[k] = J.K1[k]; K2[k] = J.K2[k]; }
    int32_t n = 0;
    for (int base = 0; base < J.N; base += kTile) {
        const int len = min(kTile, J.N - base);
        __syncthreads();
        for (int k = (int)threadIdx.x; k < len; k += 64) {
            const size_t g = (size_t)J.c_base + (size_t)(base + k);
            tile[3 * k] = ca[g]; tile[3 * k + 1] = cb[g]; tile[3 * k + 2] = cc[g];
        }
        __syncthreads();
        for (int k = 0; k < len; ++k) {
            const float4 a = tile[3 * k], b = tile[3 * k + 1], c = tile[3 * k + 2];
            const float c1[3] = {a.x, a.y, a.z}, c2[3] = {b.x, b.y, b.z};
            n += is_inlier(t12, t21, K1, K2, c1, c2, a.w, b.w, c.x, c.y, c.z, c.w) ? 1 : 0;
        }
    }
    if (live) counts[h] = n;
}

// Z5, form (b): grid (ceil(maxI / 4), jobs), four waves per block, a wave per hypothesis (uniform: its transforms can sit in scalar registers), a lane
// per correspondence, 64 at a time; the count is the popcount of the wave's ballot.
__global__ __launch_bounds__(kCountBThreads) void z3_count_b_kernel(const JobRec* __restrict__ jobs, const float4* __restrict__ ca, const float4* __restrict__ cb, const float4* __restrict__ cc,
                                                                     const float* __restrict__ T12, const float* __restrict__ T21, int32_t* __restrict__ counts) {
    const JobRec& J = jobs[blockIdx.y];
    const int it = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kCountBThreads / 64) + threadIdx.x / 64));
    if (it >= J.I) return;                                            // uniform per wave; no barrier follows
    const int lane = (int)(threadIdx.x & 63);
    const size_t h = (size_t)J.h_base + (size_t)it;
    float t12[12], t21[12], K1[4], K2[4];
#pragma unroll
    for (int k = 0; k < 12; ++k) { t12[k] = T12[12 * h + k]; t21[k] = T21[12 * h + k]; }
#pragma unroll
    for (int k = 0; k < 4; ++k) { K1[k] = J.K1[k]; K2[k] = J.K2[k]; }
    int32_t n = 0;
    for (int base = 0; base < J.N; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < J.N) {
            const size_t g = (size_t)J.c_base + (size_t)i;
            const float4 a = ca[g], b = cb[g], c = cc[g];
            const float c1[3] = {a.x, a.y, a.z}, c2[3] = {b.x, b.y, b.z};
            in = is_inlier(t12, t21, K1, K2, c1, c2, a.w, b.w, c.x, c.y, c.z, c.w);
        }
        n += __popcll(__ballot(in));
    }
    if (lane == 0) counts[h] = n;
}

// Z7: one wave per job. The best before iteration `it` is the running maximum of the counts before it (it starts at 0 and is replaced iff n >= best),
// so the walk splits: lane l owns a run of consecutive iterations, an inclusive maximum scan over the lanes' run maxima gives the best before each
// run, and every lane walks its own run as the sequential rule does. Events are numbered by a sum scan of the lanes' event counts. All integer:
// the outputs of scan(). sel[job] = n_events, best_it, best_n, sweep cap hits, the listed events' iterations (-1: none)
__global__ __launch_bounds__(64) void z3_select_kernel(const JobRec* __restrict__ jobs, int n_jobs, int min_inliers, int max_events, const int32_t* __restrict__ counts,
                                                        const uint8_t* __restrict__ cap, int32_t* __restrict__ sel) {
    __shared__ int32_t ev[IBA_SIM3_MAX_EVENTS];
    const int j = (int)blockIdx.x, lane = (int)threadIdx.x;
    if (j >= n_jobs) return;                                          // uniform per block
    const JobRec& J = jobs[j];
    const int32_t* c = counts + J.h_base;
    const uint8_t* cp = cap + J.h_base;
    const int per = (J.I + 63) / 64, a = min(lane * per, J.I), b = min(a + per, J.I);
    if (lane < IBA_SIM3_MAX_EVENTS) ev[lane] = -1;
    int32_t mx = 0, hits = 0;
    for (int it = a; it < b; ++it) { mx = max(mx, c[it]); hits += cp[it]; }
    int32_t inc = mx;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(inc, d); if (lane >= d) inc = max(inc, o); }
    int32_t before = __shfl_up(inc, 1);
    if (lane == 0) before = 0;
    int32_t best = before, ne = 0, last = -1;
    for (int it = a; it < b; ++it) {
        const int32_t n = c[it];
        if (n >= best) { best = n; last = it; ne += n > min_inliers ? 1 : 0; }
    }
    int32_t sum = ne;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const int32_t o = __shfl_up(sum, d); if (lane >= d) sum += o; }
    __syncthreads();
    int32_t k = sum - ne;                                             // the number of this run's first event
    if (ne && k < max_events) {
        best = before;
        for (int it = a; it < b; ++it) {
            const int32_t n = c[it];
            if (n < best) continue;
            best = n;
            if (n > min_inliers) { if (k < max_events) ev[k] = it; ++k; }
        }
    }
    __syncthreads();
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) { last = max(last, __shfl_xor(last, d)); hits += __shfl_xor(hits, d); }
    const int32_t n_events = __shfl(sum, 63), best_n = __shfl(inc, 63);
    int32_t* o = sel + (size_t)kSelInts * (size_t)j;
    if (lane == 0) { o[0] = n_events; o[1] = last; o[2] = best_n; o[3] = hits; }
    if (lane < IBA_SIM3_MAX_EVENTS) o[4 + lane] = ev[lane];
}

// the inlier bytes. all == 0: grid (ceil(maxN / kFlagThreads), max_events + 1, jobs); slot y < max_events is the y-th listed event, slot max_events the
// best; out = (max_events + 1) * c_base + y * N + i. all == 1 (keep_stages): grid (.., maxI, jobs), slot y is iteration y; out = it_base[job] + y * N + i.
__global__ __launch_bounds__(kFlagThreads) void z3_flags_kernel(const JobRec* __restrict__ jobs, int all, int max_events, const int32_t* __restrict__ sel, const int64_t* __restrict__ it_base,
                                                                 const float4* __restrict__ ca, const float4* __restrict__ cb, const float4* __restrict__ cc, const float* __restrict__ T12,
                                                                 const float* __restrict__ T21, uint8_t* __restrict__ out) {
    const JobRec& J = jobs[blockIdx.z];
    const int y = (int)blockIdx.y, i = (int)(blockIdx.x * kFlagThreads + threadIdx.x);
    int it;
    if (all) it = y;
    else it = y < max_events ? sel[(size_t)kSelInts * blockIdx.z + 4 + y] : sel[(size_t)kSelInts * blockIdx.z + 1];
    if (it < 0 || it >= J.I || i >= J.N) return;
    const size_t h = (size_t)J.h_base + (size_t)it, g = (size_t)J.c_base + (size_t)i;
    float t12[12], t21[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) { t12[k] = T12[12 * h + k]; t21[k] = T21[12 * h + k]; }
    const float4 a = ca[g], b = cb[g], c = cc[g];
    const float c1[3] = {a.x, a.y, a.z}, c2[3] = {b.x, b.y, b.z};
    const bool in = is_inlier(t12, t21, J.K1, J.K2, c1, c2, a.w, b.w, c.x, c.y, c.z, c.w);
    const size_t at = all ? (size_t)it_base[blockIdx.z] + (size_t)y * (size_t)J.N + (size_t)i : (size_t)(max_events + 1) * (size_t)J.c_base + (size_t)y * (size_t)J.N + (size_t)i;
    out[at] = in ? 1 : 0;
}

}  // namespace z3
}  // namespace iba

// Map-point refresh, the device half (include/iba_mi355x.h, rules S2-S6): ONE kernel text in three shapes. A group of G lanes takes one listed
// point: G = 4, 8, 16 or 32 (narrow: 256 / G points per block, up to G observations), G = 64 (one wave per point, lane i owns row i) or G = 256 (one
// block per point, up to IBA_REFRESH_MAX_OBS observations, rows strided over the threads). The group gathers the descriptors, the terms of S4 and
// the keyframe of every observation of the FULL list into LDS once; a lane holds its own row's descriptor in four 64-bit registers and reads
// descriptor j at an address that is uniform across the group. The median of a row is S3's counting form in one of two ways (ROW): a 9-step binary
// search on v that recomputes the row's distances at every step, or one pass that keeps the row and searches there. The pick is the group minimum
// of (median << 32) | row by xor shuffles. Lane 0 of the group then adds the terms IN LIST ORDER and writes every output of its point by slot, so
// no byte depends on an arrival order; the only atomics are integer counts (ballot, LDS, one atomic per counter and block). The float decisions
// are the one text of iba_refresh_math.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_refresh_math.hpp"

namespace iba {
namespace rfr {

constexpr int kThreads = 256;
constexpr int kCounters = 8;            // desc_state 0..2, geo_state 0..3, n_desc_changed

// what the kernel reads: the flat keypoint tables of the call's frames, the keyframe tables, the point table, the observation lists (obs_kp
// indexes the FLAT keypoint tables) and per slot (position of the call's list) its point and, with keep_stages, its first median
struct Tables {
    const uint64_t* desc; const int32_t* octave;
    const KfRec* kf; const KfScale* sc;
    const float *xyz, *normal, *min_dist, *max_dist; const uint64_t* pdesc;
    const int32_t *ref_kf, *obs_off, *obs_kf, *obs_kp;
    const int32_t *slot_point, *med_off;
};

// what it writes, by slot; median is NULL without keep_stages
struct Outputs {
    uint8_t *desc_state, *geo_state;
    int32_t *best_obs, *best_median, *n_desc;
    float *normal, *min_dist, *max_dist; uint64_t* desc;
    int32_t* median;
    int32_t* counts;
};

template <int W>
__device__ inline uint64_t group_min_u64(uint64_t v) {
#pragma unroll
    for (int d = W / 2; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

__device__ inline int wave_sum_i32(int v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

template <int G, bool ROW>
__global__ __launch_bounds__(kThreads) void refresh_kernel(const Tables t, const Outputs o, const int32_t* __restrict__ work, int n_work) {
    constexpr int kGroups = kThreads / G;                       // points of a block
    constexpr int kCap = G == kThreads ? kMaxObs : G;           // observations a group holds: the host bins a point where its list fits
    constexpr int kEntries = kGroups * kCap;
    constexpr bool kWaveRows = ROW && G == kThreads;            // the kept row lies in the registers of a wave, 16 distances per lane
    __shared__ uint64_t s_desc[kEntries * 4];
    __shared__ float s_term[kEntries * 3];
    __shared__ int32_t s_kf[kEntries];
    __shared__ uint8_t s_flag[kEntries];                        // bit 0: a row of S2 (the keyframe is not bad); bit 1: |PO| == 0
    __shared__ uint16_t s_row[(ROW && G < kThreads) ? kThreads * G : 1];   // entry j of this lane's row at [j * kThreads + tid]
    __shared__ uint64_t s_red[kThreads / 64];
    __shared__ int32_t s_cnt[kCounters];
    const int tid = (int)threadIdx.x, sub = tid % G, grp = tid / G, lane = tid & 63, wave = tid >> 6;
    const int w = (int)blockIdx.x * kGroups + grp;
    const bool live = w < n_work;
    const int slot = live ? work[w] : 0;
    const int p = live ? t.slot_point[slot] : 0;
    const int e0 = live ? t.obs_off[p] : 0, len = live ? t.obs_off[p + 1] - e0 : 0;
    const int base = grp * kCap;
    const float X[3] = {live ? t.xyz[3 * (size_t)p] : 0.f, live ? t.xyz[3 * (size_t)p + 1] : 0.f, live ? t.xyz[3 * (size_t)p + 2] : 0.f};
    if (tid < kCounters) s_cnt[tid] = 0;
    // ---- the gather: descriptor, term, keyframe and flags of every observation of the full list ----
    for (int k = sub; k < len; k += G) {
        const int e = e0 + k, g = t.obs_kf[e];
        const KfRec kf = t.kf[g];
        const uint64_t* d = t.desc + 4 * (size_t)t.obs_kp[e];
        float tm[3];
        const bool ok = term(X, kf.Ow, tm);
#pragma unroll
        for (int c = 0; c < 4; ++c) s_desc[(size_t)(base + k) * 4 + c] = d[c];
        s_term[(base + k) * 3] = tm[0]; s_term[(base + k) * 3 + 1] = tm[1]; s_term[(base + k) * 3 + 2] = tm[2];
        s_kf[base + k] = g;
        s_flag[base + k] = (uint8_t)((kf.bad ? 0 : 1) | (ok ? 0 : 2));
    }
    __syncthreads();
    // ---- S2 / S3: N, the median of every row, the least (median, row) ----
    int N = 0;
    for (int k = 0; k < len; ++k) N += s_flag[base + k] & 1;
    const int need = median_rank(N) + 1;
    int32_t* med = (o.median && live) ? o.median + t.med_off[slot] : nullptr;
    uint64_t best = kNoKey;
    if constexpr (kWaveRows) {
        for (int i = wave; i < len; i += kThreads / 64) {
            if (!(s_flag[i] & 1)) {
                if (med && lane == 0) med[i] = -1;
                continue;
            }
            const uint64_t mine[4] = {s_desc[(size_t)i * 4], s_desc[(size_t)i * 4 + 1], s_desc[(size_t)i * 4 + 2], s_desc[(size_t)i * 4 + 3]};
            int d[kMaxObs / 64];                                 // (skipping the parts past the list behind a uniform branch measured slower)
#pragma unroll
            for (int u = 0; u < kMaxObs / 64; ++u) {
                const int j = lane + 64 * u;
                d[u] = (j < len && (s_flag[j] & 1)) ? hamming256(mine, &s_desc[(size_t)j * 4]) : 0x7FFF;
            }
            int lo = 0, hi = 256;
            for (int step = 0; step < 9; ++step) {
                const int mid = (lo + hi) >> 1;
                int c = 0;
#pragma unroll
                for (int u = 0; u < kMaxObs / 64; ++u) c += d[u] <= mid ? 1 : 0;
                c = wave_sum_i32(c);
                if (c >= need) hi = mid; else lo = mid + 1;
            }
            if (lane == 0) {
                const uint64_t key = pick_key(lo, (uint32_t)i);
                best = key < best ? key : best;
                if (med) med[i] = lo;
            }
        }
    } else {
        for (int i = sub; i < len; i += G) {
            if (!(s_flag[base + i] & 1)) {
                if (med) med[i] = -1;
                continue;
            }
            const uint64_t* own = &s_desc[(size_t)(base + i) * 4];
            const uint64_t mine[4] = {own[0], own[1], own[2], own[3]};
            if constexpr (ROW)
                for (int j = 0; j < len; ++j) s_row[j * kThreads + tid] = (uint16_t)((s_flag[base + j] & 1) ? hamming256(mine, &s_desc[(size_t)(base + j) * 4]) : 0x7FFF);
            int lo = 0, hi = 256;
            for (int step = 0; step < 9; ++step) {
                const int mid = (lo + hi) >> 1;
                int c = 0;
                if constexpr (ROW) {
                    for (int j = 0; j < len; ++j) c += (int)s_row[j * kThreads + tid] <= mid ? 1 : 0;
                } else {
                    for (int j = 0; j < len; ++j)
                        if (s_flag[base + j] & 1) c += hamming256(mine, &s_desc[(size_t)(base + j) * 4]) <= mid ? 1 : 0;
                }
                if (c >= need) hi = mid; else lo = mid + 1;
            }
            const uint64_t key = pick_key(lo, (uint32_t)i);
            best = key < best ? key : best;
            if (med) med[i] = lo;
        }
    }
    best = group_min_u64<(G < 64 ? G : 64)>(best);
    if constexpr (G == kThreads) {
        if (lane == 0) s_red[wave] = best;
        __syncthreads();
        best = s_red[0];
        for (int v = 1; v < kThreads / 64; ++v) best = s_red[v] < best ? s_red[v] : best;
    }
    // ---- lane 0 of the group: the outputs of the point, S4 in list order, S5 / S6 ----
    int ds = -1, gs = -1, changed = 0;
    if (live && sub == 0) {
        const uint64_t* given = t.pdesc + 4 * (size_t)p;
        const uint64_t* pick = given;
        if (N) {
            ds = IBA_REFRESH_DESC_PICKED;
            pick = &s_desc[(size_t)(base + (int)(uint32_t)best) * 4];
            changed = (pick[0] != given[0] || pick[1] != given[1] || pick[2] != given[2] || pick[3] != given[3]) ? 1 : 0;
            o.best_obs[slot] = (int32_t)(uint32_t)best; o.best_median[slot] = (int32_t)(best >> 32);
        } else {
            ds = IBA_REFRESH_DESC_KEPT;
            o.best_obs[slot] = -1; o.best_median[slot] = -1;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) o.desc[4 * (size_t)slot + c] = pick[c];
        o.n_desc[slot] = N;
        o.desc_state[slot] = (uint8_t)ds;
        float sum[3] = {0.f, 0.f, 0.f};
        bool degenerate = false;
        int kref = -1;
        const int ref = t.ref_kf[p];
        for (int k = 0; k < len; ++k) {
            sum[0] = sum[0] + s_term[(base + k) * 3]; sum[1] = sum[1] + s_term[(base + k) * 3 + 1]; sum[2] = sum[2] + s_term[(base + k) * 3 + 2];
            degenerate = degenerate || (s_flag[base + k] & 2);
            if (kref < 0 && s_kf[base + k] == ref) kref = k;
        }
        float nrm[3] = {t.normal[3 * (size_t)p], t.normal[3 * (size_t)p + 1], t.normal[3 * (size_t)p + 2]}, mn = t.min_dist[p], mx = t.max_dist[p];
        if (degenerate) gs = IBA_REFRESH_GEO_DEGENERATE;
        else {
            for (int c = 0; c < 3; ++c) nrm[c] = mean_of(sum[c], len);
            if (kref < 0) gs = IBA_REFRESH_GEO_NO_REF;
            else {
                gs = IBA_REFRESH_GEO_UPDATED;
                distances(X, t.kf[ref], t.sc[ref], t.octave[t.obs_kp[e0 + kref]], &mn, &mx);
            }
        }
        o.normal[3 * (size_t)slot] = nrm[0]; o.normal[3 * (size_t)slot + 1] = nrm[1]; o.normal[3 * (size_t)slot + 2] = nrm[2];
        o.min_dist[slot] = mn; o.max_dist[slot] = mx;
        o.geo_state[slot] = (uint8_t)gs;
    }
    for (int c = 0; c < kCounters; ++c) {
        const bool hit = c < 3 ? ds == c : c < 7 ? gs == c - 3 : changed != 0;
        const unsigned long long m = __ballot(hit);
        if (lane == 0 && m) atomicAdd(&s_cnt[c], __popcll(m));
    }
    __syncthreads();
    if (tid < kCounters && s_cnt[tid]) atomicAdd(&o.counts[tid], s_cnt[tid]);
}

}  // namespace rfr
}  // namespace iba

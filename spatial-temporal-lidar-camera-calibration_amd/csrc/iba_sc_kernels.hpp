// Device side of iba_sc_describe / iba_sc_distance / iba_sc_detect (include/iba_mi355x.h, "Scan Context"): the rules are stated there and restated in
// numpy in tests/sc_ref.py; the results are compared byte for byte. Every f64 expression below is written as separately rounded operations under
// `fp contract(off)`: no fma, so that numpy reproduces the bits. No floating-point atomics: the only atomics are integer max / add.
//
//  iba_sc_bins_kernel      flat grid over slices of kScSlice points of every node (ScBlock: node, first point). The slice is streamed coalesced from
//      the resident pts4 (16 B per lane; the kd order of the scan does not matter to a maximum). Thread = point: range, ring, angle, sector by the
//      rules, then an integer atomic max of the order-preserving key of its float32 z on the block's R x S bins in LDS (4 B each: 4.8 KB at 20 x 60,
//      64 KB at the largest shape). The block then merges its non-empty bins into the node's global bins by integer atomic max, and a wave's count of
//      non-finite points goes to the node by one integer atomic add. Key 0 = empty (below the key of every finite float).
//  iba_sc_finalize_kernel  one 64-thread block per node: keys -> doubles (+ lidar_height, empty = 0) row-major [ring][sector]; ring key (thread = ring,
//      sectors ascending) and its float narrowing; sector key and column norm (thread = sector, strided; rings ascending).
//  iba_sc_knn_kernel       one wave per query: num_candidates selection rounds over the float ring keys of [0, db_end). In a round every lane walks its
//      nodes (lane, lane + 64, ..), keeps the smallest (distance, node) pair that lies lexicographically ABOVE the previous round's winner, and the
//      wave takes the minimum of the lanes' pairs over xor shuffles. A lexicographic minimum over a set does not depend on the walk: the result is
//      the exact k nearest, nearest first, equal distances to the lower node, whatever the lane count. The distances are recomputed per round
//      (R subtractions, multiplications, additions per node and round) instead of being kept in a lane-local list: no indexed private array, no scratch.
//  iba_sc_distance_kernel  one one-wave block per (a, b) pair (iba_sc_distance: the caller's pairs; iba_sc_detect: query x candidate slot). Both
//      descriptors are staged in LDS when 16 R S bytes fit in 64 KB (19.2 KB at 20 x 60), otherwise read from global; sector keys and column norms
//      come from the database (computed once per descriptor). Alignment: lane = shift (strided), its sum over the sectors ascending, square root,
//      then the lexicographic (norm, shift) minimum over the wave = the first minimum. The window of shifts around it is listed ascending; per chunk
//      of kScChunk shifts the (shift, column) cosines are spread over the lanes (rings ascending per dot product) into LDS, lane w then adds the
//      columns of its shift ascending, skipping the columns with a zero norm, and the chunk's first minimum is taken in shift order.
//  iba_sc_pick_kernel      thread = query: the candidates in search order, first strict minimum from 10000000, threshold, yaw; writes iba_sc_result.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_types.hpp"

namespace iba {

constexpr int kScThreads = 256;
constexpr int kScItems = 16;                         // points per thread of the bins kernel
constexpr int kScSlice = kScThreads * kScItems;      // points per block
constexpr int kScChunk = 8;                          // window shifts evaluated together by the distance kernel
constexpr double kScNoWinner = IBA_SC_NO_WINNER;

struct ScBlock { int32_t node; uint32_t begin; };    // one slice of one node's scan
struct ScShape {                                      // what every kernel needs of the options
    int32_t R, S, k, radius;                          // rings, sectors, candidates, SEARCH_RADIUS
    double max_radius, lidar_height, dist_thres;
};

// order-preserving key of a float32: a < b  <=>  key(a) < key(b) for finite values, +0 above -0; 0 lies below every finite value
__host__ __device__ __forceinline__ uint32_t sc_z_key(float z) {
    uint32_t b;
    __builtin_memcpy(&b, &z, 4);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
__host__ __device__ __forceinline__ float sc_z_unkey(uint32_t k) {
    const uint32_t b = (k >> 31) ? (k & 0x7FFFFFFFu) : ~k;
    float z;
    __builtin_memcpy(&z, &b, 4);
    return z;
}

// rules 1 and 2 for one finite point: false = it does not enter a bin
__device__ __forceinline__ bool sc_bin_of(const ScShape& sh, double x, double y, double z, int& ring, int& sector) {
#pragma clang fp contract(off)
    const double zz = z + sh.lidar_height;
    const double xx = x * x, yy = y * y, z2 = zz * zz;
    const double sxy = xx + yy;
    const double range = sqrt(sxy + z2);
    if (range > sh.max_radius || !(zz > -1000.0)) return false;
    double ang = 0.0;
    if (!(x == 0.0 && y == 0.0)) {
        ang = atan2(y, x) * (180.0 / M_PI);
        if (ang < 0.0) ang = ang + 360.0;
    }
    const double ra = range / sh.max_radius * (double)sh.R;
    const double sa = ang / 360.0 * (double)sh.S;
    const int ri = (int)ceil(ra), si = (int)ceil(sa);
    ring = max(min(sh.R, ri), 1) - 1;
    sector = max(min(sh.S, si), 1) - 1;
    return true;
}

__global__ __launch_bounds__(kScThreads) void iba_sc_bins_kernel(const FrameHdr* __restrict__ frames, const float4* __restrict__ pts4, const int32_t* __restrict__ node_frame,
                                                                const ScBlock* __restrict__ blocks, ScShape sh, uint32_t* __restrict__ bins, uint32_t* __restrict__ skipped) {
    extern __shared__ uint32_t s_bins[];
    const int nb = sh.R * sh.S;
    for (int i = threadIdx.x; i < nb; i += kScThreads) s_bins[i] = 0u;
    __syncthreads();
    const ScBlock B = blocks[blockIdx.x];
    const FrameHdr& fh = frames[node_frame[B.node]];
    const float4* __restrict__ src = pts4 + fh.pt_base;
    const uint32_t end = min(fh.P, B.begin + (uint32_t)kScSlice);
    uint32_t bad = 0u;
    for (uint32_t i = B.begin + threadIdx.x; i < end; i += kScThreads) {
        const float4 p = src[i];
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) { ++bad; continue; }
        int ring, sector;
        if (sc_bin_of(sh, (double)p.x, (double)p.y, (double)p.z, ring, sector)) atomicMax(&s_bins[ring * sh.S + sector], sc_z_key(p.z));
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) bad += (uint32_t)__shfl_xor((int)bad, m, 64);
    if ((threadIdx.x & 63u) == 0u && bad) atomicAdd(&skipped[B.node], bad);
    __syncthreads();
    uint32_t* __restrict__ dst = bins + (size_t)B.node * (size_t)nb;
    for (int i = threadIdx.x; i < nb; i += kScThreads) {
        const uint32_t k = s_bins[i];
        if (k) atomicMax(&dst[i], k);
    }
}

__device__ __forceinline__ double sc_bin_value(uint32_t key, double lidar_height) {
#pragma clang fp contract(off)
    return key ? (double)sc_z_unkey(key) + lidar_height : 0.0;
}

__global__ __launch_bounds__(64) void iba_sc_finalize_kernel(const uint32_t* __restrict__ bins, ScShape sh, double* __restrict__ desc, double* __restrict__ ring_key, float* __restrict__ ring_key_f,
                                                            double* __restrict__ sector_key, double* __restrict__ col_norm) {
#pragma clang fp contract(off)
    const int R = sh.R, S = sh.S, nb = R * S;
    const size_t node = blockIdx.x;
    const uint32_t* __restrict__ b = bins + node * (size_t)nb;
    double* __restrict__ d = desc + node * (size_t)nb;
    for (int i = threadIdx.x; i < nb; i += 64) d[i] = sc_bin_value(b[i], sh.lidar_height);
    if ((int)threadIdx.x < R) {
        const int r = threadIdx.x;
        double acc = 0.0;
        for (int c = 0; c < S; ++c) acc = acc + sc_bin_value(b[r * S + c], sh.lidar_height);
        const double mean = acc / (double)S;
        ring_key[node * (size_t)R + r] = mean;
        ring_key_f[node * (size_t)R + r] = (float)mean;
    }
    for (int c = threadIdx.x; c < S; c += 64) {
        double acc = 0.0, sq = 0.0;
        for (int r = 0; r < R; ++r) {
            const double v = sc_bin_value(b[r * S + c], sh.lidar_height);
            const double vv = v * v;
            acc = acc + v;
            sq = sq + vv;
        }
        sector_key[node * (size_t)S + c] = acc / (double)R;
        col_norm[node * (size_t)S + c] = sqrt(sq);
    }
}

// the lexicographic minimum of (value, index) over the wave; every lane gets it. A lane without a pair passes idx = INT_MAX (its value is then ignored).
__device__ __forceinline__ void sc_wave_min(double& v, int& idx) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(v, m, 64);
        const int oi = __shfl_xor(idx, m, 64);
        const bool take = oi != 0x7FFFFFFF && (idx == 0x7FFFFFFF || ov < v || (ov == v && oi < idx));
        if (take) { v = ov; idx = oi; }
    }
}

__global__ __launch_bounds__(64) void iba_sc_knn_kernel(const float* __restrict__ ring_key_f, const iba_sc_query* __restrict__ queries, ScShape sh, int32_t* __restrict__ cand) {
#pragma clang fp contract(off)
    __shared__ double s_q[IBA_SC_MAX_RING];
    const int R = sh.R, lane = threadIdx.x;
    const iba_sc_query q = queries[blockIdx.x];
    if (lane < R) s_q[lane] = (double)ring_key_f[(size_t)q.node * (size_t)R + lane];
    __syncthreads();
    double prev_d = -1.0;   // a squared distance is never below 0: every pair lies above (-1, any node)
    int prev_j = 0x7FFFFFFF;
    for (int round = 0; round < sh.k; ++round) {
        double best_d = 0.0;
        int best_j = 0x7FFFFFFF;
        for (int j = lane; j < q.db_end; j += 64) {
            const float* __restrict__ kj = ring_key_f + (size_t)j * (size_t)R;
            double d2 = 0.0;
            for (int r = 0; r < R; ++r) {
                const double t = (double)kj[r] - s_q[r];
                const double tt = t * t;
                d2 = d2 + tt;
            }
            const bool above = d2 > prev_d || (d2 == prev_d && j > prev_j);
            if (above && (best_j == 0x7FFFFFFF || d2 < best_d)) { best_d = d2; best_j = j; }   // (ascending j per lane: an equal distance keeps the lower node)
        }
        sc_wave_min(best_d, best_j);
        if (lane == 0) cand[(size_t)blockIdx.x * (size_t)sh.k + round] = best_j == 0x7FFFFFFF ? -1 : best_j;
        if (best_j == 0x7FFFFFFF) {   // the set is exhausted: the remaining slots are -1
            if (lane == 0) for (int r2 = round + 1; r2 < sh.k; ++r2) cand[(size_t)blockIdx.x * (size_t)sh.k + r2] = -1;
            break;
        }
        prev_d = best_d; prev_j = best_j;
    }
}

// bytes of dynamic LDS of the distance kernel: [descriptors 2 R S doubles when staged] [vk1 vk2 n1 n2: 4 S doubles] [cosines kScChunk S doubles] [cosine
// validity kScChunk S bytes] [window S ints]
__host__ __device__ __forceinline__ size_t sc_distance_lds(int R, int S, bool staged) {
    return (staged ? 2 * (size_t)R * S * 8 : 0) + 4 * (size_t)S * 8 + (size_t)kScChunk * S * 8 + (((size_t)kScChunk * S + 7) & ~(size_t)7) + (size_t)S * 4;
}

template <bool kStaged>
__global__ __launch_bounds__(64) void iba_sc_distance_kernel(const double* __restrict__ desc, const double* __restrict__ sector_key, const double* __restrict__ col_norm,
                                                            const int32_t* __restrict__ pairs, const iba_sc_query* __restrict__ queries, const int32_t* __restrict__ cand, ScShape sh,
                                                            double* __restrict__ out_dist, int32_t* __restrict__ out_shift) {
#pragma clang fp contract(off)
    extern __shared__ double s_mem[];
    const int R = sh.R, S = sh.S, nb = R * S, lane = threadIdx.x;
    int a, b;
    if (pairs) { a = pairs[2 * (size_t)blockIdx.x]; b = pairs[2 * (size_t)blockIdx.x + 1]; }
    else { a = queries[blockIdx.x / (unsigned)sh.k].node; b = cand[blockIdx.x]; }
    if (b < 0) {   // an empty candidate slot (uniform over the block)
        if (lane == 0) { out_dist[blockIdx.x] = __builtin_nan(""); out_shift[blockIdx.x] = -1; }
        return;
    }
    double* s_p = s_mem;
    const double* A = desc + (size_t)a * (size_t)nb;
    const double* B = desc + (size_t)b * (size_t)nb;
    if (kStaged) {
        for (int i = lane; i < nb; i += 64) { s_p[i] = A[i]; s_p[nb + i] = B[i]; }
        A = s_p; B = s_p + nb;
        s_p += 2 * nb;
    }
    double* s_vk1 = s_p; double* s_vk2 = s_vk1 + S; double* s_n1 = s_vk2 + S; double* s_n2 = s_n1 + S;
    double* s_cos = s_n2 + S;
    unsigned char* s_ok = (unsigned char*)(s_cos + kScChunk * S);
    int* s_win = (int*)(s_ok + ((kScChunk * S + 7) & ~7));
    for (int c = lane; c < S; c += 64) {
        s_vk1[c] = sector_key[(size_t)a * S + c]; s_vk2[c] = sector_key[(size_t)b * S + c];
        s_n1[c] = col_norm[(size_t)a * S + c]; s_n2[c] = col_norm[(size_t)b * S + c];
    }
    __syncthreads();

    // ---- fastAlignUsingVkey: lane = shift ----
    double al_v = 0.0;
    int al_s = 0x7FFFFFFF;
    for (int s = lane; s < S; s += 64) {
        double acc = 0.0;
        int c2 = s == 0 ? 0 : S - s;               // (c - s) mod S at c = 0
        for (int c = 0; c < S; ++c) {
            const double t = s_vk1[c] - s_vk2[c2];
            const double tt = t * t;
            acc = acc + tt;
            c2 = c2 + 1 == S ? 0 : c2 + 1;
        }
        const double nrm = sqrt(acc);
        if (nrm < kScNoWinner && (al_s == 0x7FFFFFFF || nrm < al_v)) { al_v = nrm; al_s = s; }
    }
    sc_wave_min(al_v, al_s);
    const int argmin = al_s == 0x7FFFFFFF ? 0 : al_s;

    // ---- the window, ascending ----
    const int span = 2 * sh.radius + 1;
    const int nW = span >= S ? S : span;
    if (lane == 0) {
        int n = 0;
        for (int s = 0; s < S; ++s) {
            int off = (s - argmin + sh.radius) % S;
            if (off < 0) off += S;
            if (span >= S || off < span) s_win[n++] = s;
        }
    }
    __syncthreads();

    double best = kScNoWinner;
    int best_shift = 0;
    for (int w0 = 0; w0 < nW; w0 += kScChunk) {
        const int nw = min(kScChunk, nW - w0);
        for (int i = lane; i < nw * S; i += 64) {
            const int w = i / S, c = i - w * S;
            int c2 = c - s_win[w0 + w];
            if (c2 < 0) c2 += S;
            const double n1 = s_n1[c], n2 = s_n2[c2];
            const bool ok = !(n1 == 0.0 || n2 == 0.0);
            double cs = 0.0;
            if (ok) {
                double dot = 0.0;
                for (int r = 0; r < R; ++r) {
                    const double pr = A[r * S + c] * B[r * S + c2];
                    dot = dot + pr;
                }
                const double den = n1 * n2;
                cs = dot / den;
            }
            s_cos[i] = cs; s_ok[i] = ok ? 1 : 0;
        }
        __syncthreads();
        double d = 0.0;
        int w_idx = 0x7FFFFFFF;
        if (lane < nw) {
            double sum = 0.0;
            int cnt = 0;
            for (int c = 0; c < S; ++c)
                if (s_ok[lane * S + c]) { sum = sum + s_cos[lane * S + c]; ++cnt; }
            const double mean = sum / (double)cnt;      // 0 / 0 = NaN without a common non-zero column
            d = 1.0 - mean;
            if (d < best) w_idx = lane;                 // a NaN and a distance that does not beat the earlier chunks never enter
        }
        sc_wave_min(d, w_idx);
        if (w_idx != 0x7FFFFFFF) { best = d; best_shift = s_win[w0 + w_idx]; }
        __syncthreads();
    }
    if (lane == 0) { out_dist[blockIdx.x] = best; out_shift[blockIdx.x] = best_shift; }
}

__global__ __launch_bounds__(256) void iba_sc_pick_kernel(const iba_sc_query* __restrict__ queries, const int32_t* __restrict__ cand, const double* __restrict__ dist, const int32_t* __restrict__ shift,
                                                         ScShape sh, int Q, iba_sc_result* __restrict__ out) {
#pragma clang fp contract(off)
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= Q) return;
    iba_sc_result r;
    r.struct_size = (int32_t)sizeof(iba_sc_result); r.reserved = 0;
    double best = kScNoWinner;
    int arg = 0, nn = -1, n = 0;
#pragma unroll
    for (int i = 0; i < IBA_SC_MAX_CANDIDATES; ++i) {
        int node = -1, s = -1;
        double d = __builtin_nan("");
        if (i < sh.k) {
            node = cand[(size_t)q * sh.k + i];
            if (node >= 0) {
                d = dist[(size_t)q * sh.k + i]; s = shift[(size_t)q * sh.k + i]; ++n;
                if (d < best) { best = d; arg = s; nn = node; }
            }
        }
        r.cand_node[i] = node; r.cand_shift[i] = s; r.cand_dist[i] = d;
    }
    r.loop_node = best < sh.dist_thres ? nn : -1;
    r.shift = arg; r.n_candidates = n; r.min_dist = best;
    const double deg = (double)arg * (360.0 / (double)sh.S);
    const double num = deg * M_PI;
    r.yaw_rad = (float)(num / 180.0);
    (void)queries;
    out[q] = r;
}

}  // namespace iba

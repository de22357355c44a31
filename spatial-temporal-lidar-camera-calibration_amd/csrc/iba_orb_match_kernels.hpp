// Windowed ORB matching, the device half (include/iba_mi355x.h, rules M2-M8). Every launch runs over flat tables of the whole call: keypoints of all
// frames, queries of all jobs. The float decisions (a keypoint's cell, a window's cell range) are written once in iba_orb_match_host.hpp; everything
// else is integer. No order depends on atomic arrival: the only atomics are integer counts.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "iba_orb_match_host.hpp"

namespace iba {
namespace orbm {

constexpr int kThreads = 256;
constexpr uint16_t kFree = 0xFFFFu;          // held_dist of a train keypoint nobody holds (INT_MAX in the rule); a claimed one holds 0
constexpr uint32_t kNoPos = 0xFFFFFFFFu;

struct FrameRec { int32_t kp_base, n; float min_x, min_y, inv_w, inv_h; };
struct QueryRec {
    float u, v, r;
    int32_t min_level, max_level;
    int32_t kp;        // the flat keypoint that supplies descriptor and angle
    int32_t train;     // the train frame
    int32_t valid;
};
struct JobRec {
    int32_t q0, nq;            // the job's queries in the call's flat table
    int32_t rule;
    int32_t train_base, n_train;
    int32_t state_base;        // into the global per-train state, or -1: the state is in LDS
};
struct JobOut { int32_t n_matches, n_displaced, n_rot_removed, hist[kHisto], ind[3]; };

// M2: one thread per keypoint of any frame: its cell (px * 48 + py, the order M3 walks; -1: none) and the count of its (frame, cell)
__global__ __launch_bounds__(kThreads) void orbm_cell_kernel(const FrameRec* __restrict__ frames, const int32_t* __restrict__ kp_frame, const float2* __restrict__ xy, int n_kp,
                                                             int32_t* __restrict__ kp_cell, int32_t* __restrict__ cell_cnt) {
    const int i = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (i >= n_kp) return;
    const int f = kp_frame[i];
    const FrameRec fr = frames[f];
    const float2 p = xy[i];
    const int px = cell_of(p.x, fr.min_x, fr.inv_w, kCols), py = cell_of(p.y, fr.min_y, fr.inv_h, kRows);
    const int c = (px < 0 || py < 0) ? -1 : px * kRows + py;
    kp_cell[i] = c;
    if (c >= 0) atomicAdd(&cell_cnt[(size_t)f * kCells + (size_t)c], 1);
}

// the ordered fill: one wave per frame takes 64 keypoints per trip in ascending index; a lane's place inside its cell is the cell's cursor plus the
// number of lower lanes of the trip in the same cell; the highest lane of each cell moves the cursor
__global__ __launch_bounds__(64) void orbm_fill_kernel(const FrameRec* __restrict__ frames, const int32_t* __restrict__ kp_cell, const int32_t* __restrict__ cell_off, int32_t* __restrict__ list) {
    __shared__ int32_t cursor[kCells];
    const FrameRec fr = frames[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int32_t* __restrict__ off = cell_off + (size_t)blockIdx.x * kCells;
    for (int c = lane; c < kCells; c += 64) cursor[c] = off[c];
    __syncthreads();
    for (int i0 = 0; i0 < fr.n; i0 += 64) {          // (uniform trip count)
        const int i = i0 + lane;
        const int c = i < fr.n ? kp_cell[fr.kp_base + i] : -1;
        int rank = 0, last = 1;
        for (int l = 0; l < 64; ++l) {
            const int cl = __shfl(c, l, 64);
            if (cl == c) { if (l < lane) ++rank; if (l > lane) last = 0; }
        }
        if (c >= 0) {
            const int at = cursor[c] + rank;          // global positions: cell_off is scanned over the call's (frame, cell) table
            list[at] = i;
            if (last) cursor[c] = at + 1;
        }
        __syncthreads();
    }
}

// exclusive scan of n counts by one block: off[0 .. n], off[n] = the total (the extraction's orb_scan_kernel, which lives in another translation unit)
__global__ __launch_bounds__(1024) void orbm_scan_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ off, int n) {
    __shared__ int32_t part[1024];
    const int per = (n + 1023) / 1024, a = min((int)threadIdx.x * per, n), b = min(a + per, n);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += cnt[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int at = part[threadIdx.x] - sum;
    for (int i = a; i < b; ++i) { off[i] = at; at += cnt[i]; }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

// M4
__device__ inline int hamming256(const uint64_t (&a)[4], const uint64_t* __restrict__ b) {
    return __popcll(a[0] ^ b[0]) + __popcll(a[1] ^ b[1]) + __popcll(a[2] ^ b[2]) + __popcll(a[3] ^ b[3]);
}

// M3: one thread per query. WRITE = false counts the list; WRITE = true writes the candidates (indices inside the train frame) in M3's order at the
// query's offset, each with its M4 distance. With cell = px * 48 + py the cells iy = c0y .. c1y of a column are one run of the frame's list.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void orbm_list_kernel(const FrameRec* __restrict__ frames, const QueryRec* __restrict__ queries, int q0, int nq, const float2* __restrict__ xy,
                                                             const int32_t* __restrict__ octave, const uint64_t* __restrict__ desc, const int32_t* __restrict__ cell_off,
                                                             const int32_t* __restrict__ list, int32_t* __restrict__ cnt, const int32_t* __restrict__ off, int32_t* __restrict__ cand,
                                                             uint16_t* __restrict__ cand_dist) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (k >= nq) return;
    const QueryRec q = queries[q0 + k];
    int n = 0;
    if (q.valid) {
        const FrameRec fr = frames[q.train];
        const int c0x = window_first(q.u, fr.min_x, q.r, fr.inv_w, kCols), c1x = window_last(q.u, fr.min_x, q.r, fr.inv_w, kCols);
        const int c0y = window_first(q.v, fr.min_y, q.r, fr.inv_h, kRows), c1y = window_last(q.v, fr.min_y, q.r, fr.inv_h, kRows);
        if (c0x < kCols && c1x >= 0 && c0y < kRows && c1y >= 0) {
            const bool check = q.min_level > 0 || q.max_level >= 0;
            const int32_t* __restrict__ coff = cell_off + (size_t)q.train * kCells;
            uint64_t d[4] = {0, 0, 0, 0};
            size_t at = 0;
            if (WRITE) {
                for (int w = 0; w < 4; ++w) d[w] = desc[4 * (size_t)q.kp + (size_t)w];
                at = (size_t)off[k];
            }
            for (int ix = c0x; ix <= c1x; ++ix) {
                // (the table has one entry past the call's last cell, so [cell + 1] is the run's end also for the last cell of the last frame)
                const int a = coff[ix * kRows + c0y], b = coff[ix * kRows + c1y + 1];
                for (int e = a; e < b; ++e) {
                    const int i = list[e];
                    if (check) {
                        const int o = octave[fr.kp_base + i];
                        if (o < q.min_level) continue;
                        if (q.max_level >= 0 && o > q.max_level) continue;
                    }
                    const float2 p = xy[fr.kp_base + i];
                    if (!(fabsf(p.x - q.u) < q.r && fabsf(p.y - q.v) < q.r)) continue;
                    if (WRITE) {
                        cand[at + (size_t)n] = i;
                        cand_dist[at + (size_t)n] = (uint16_t)hamming256(d, desc + 4 * (size_t)(fr.kp_base + i));
                    }
                    ++n;
                }
            }
        }
    }
    if (!WRITE) cnt[k] = n;
}

__device__ inline uint64_t wave_min_u64(uint64_t v) {
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d, 64), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline int wave_min_i32(int v) {
    for (int d = 32; d >= 1; d >>= 1) v = min(v, __shfl_xor(v, d, 64));
    return v;
}

// M8's bin of a rotation difference
__device__ inline int rot_bin(float rot) {
    if (rot < 0.0f) rot += 360.0f;
    int bin = (int)roundf(rot * (1.0f / (float)kHisto));
    if (bin == kHisto) bin = 0;
    return bin;
}

// M6 / M7 / M8: ONE wave per job walks the job's queries in order. Per query the lanes stride over its segment, skipping a candidate whose
// held_dist <= dist (a claimed candidate of rule CLAIM holds 0, a free one 0xFFFF); a lane keeps (best, its first list position, best2); the wave takes the
// minimum of (best, position) and, for best2, the least of the winner lane's best2 and the other lanes' best: the second order statistic of the
// multiset. Lane 0 applies the rule. The per-train state is in LDS up to IBA_ORB_MATCH_LDS_TRAIN train keypoints, else in global memory.
__global__ __launch_bounds__(64) void orbm_resolve_kernel(const JobRec* __restrict__ jobs, const QueryRec* __restrict__ queries, const float* __restrict__ angle, int chunk_q0,
                                                          const int32_t* __restrict__ off, const int32_t* __restrict__ cand, const uint16_t* __restrict__ cand_dist,
                                                          uint16_t* __restrict__ g_held, int32_t* __restrict__ g_holder, int th_low, int th_high, float nn_ratio, int check_orientation,
                                                          int32_t* __restrict__ match, int32_t* __restrict__ dist, int8_t* __restrict__ qbin, JobOut* __restrict__ out) {
    __shared__ uint16_t s_held[IBA_ORB_MATCH_LDS_TRAIN];
    __shared__ int32_t s_holder[IBA_ORB_MATCH_LDS_TRAIN];
    __shared__ int32_t s_hist[kHisto];
    __shared__ int32_t s_ind[3];
    const JobRec job = jobs[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const bool init = job.rule == IBA_ORB_MATCH_INIT;
    uint16_t* held = job.state_base < 0 ? s_held : g_held + job.state_base;
    int32_t* holder = job.state_base < 0 ? s_holder : g_holder + job.state_base;
    for (int c = lane; c < job.n_train; c += 64) { held[c] = kFree; holder[c] = -1; }
    if (lane < kHisto) s_hist[lane] = 0;
    const int qa = job.q0 - chunk_q0;                 // the job's queries in the chunk's arrays
    for (int k = lane; k < job.nq; k += 64) { match[qa + k] = -1; dist[qa + k] = -1; qbin[qa + k] = -1; }
    __syncthreads();
    const int sentinel = init ? INT_MAX : 256;
    int n_matches = 0, n_displaced = 0;               // lane 0's
    for (int k = 0; k < job.nq; ++k) {
        const int a = off[qa + k], b = off[qa + k + 1];
        if (a == b) continue;                         // (uniform)
        int best = sentinel, best2 = INT_MAX;
        uint32_t pos = kNoPos;
        for (int e = a + lane; e < b; e += 64) {
            const int d = (int)cand_dist[e];
            if ((int)held[cand[e]] <= d) continue;
            if (d < best) { best2 = best; best = d; pos = (uint32_t)(e - a); }
            else if (d < best2) best2 = d;
        }
        const uint64_t key = wave_min_u64(((uint64_t)(uint32_t)best << 32) | pos);
        const uint32_t wpos = (uint32_t)key;
        if (wpos == kNoPos) continue;                 // (uniform) nothing left to take
        const int wbest = (int)(key >> 32);
        // (a lane without the winner has best >= wbest; one that never took a candidate offers its sentinel, which CLAIM does not use and which is
        // INT_MAX under INIT)
        const int wbest2 = wave_min_i32(pos == wpos ? best2 : (init ? best : INT_MAX));
        if (lane == 0) {
            const bool accept = init ? (wbest <= th_low && (float)wbest < (float)wbest2 * nn_ratio) : wbest <= th_high;
            if (accept) {
                const int c = cand[a + (int)wpos];
                if (init) {
                    const int h = holder[c];
                    if (h >= 0) { match[qa + h] = -1; dist[qa + h] = -1; --n_matches; ++n_displaced; }
                    holder[c] = k;
                }
                held[c] = init ? (uint16_t)wbest : (uint16_t)0;
                match[qa + k] = c; dist[qa + k] = wbest; ++n_matches;
                if (check_orientation) {
                    const int bin = rot_bin(angle[queries[job.q0 + k].kp] - angle[job.train_base + c]);
                    qbin[qa + k] = (int8_t)bin;
                    s_hist[bin] += 1;
                }
            }
        }
        __syncthreads();                              // the state lane 0 changed, before the next query's walk
    }
    // M8: ComputeThreeMaxima on lane 0, then every lane takes its share of the queries
    if (lane == 0) {
        int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
        if (check_orientation) {
            for (int i = 0; i < kHisto; ++i) {
                const int s = s_hist[i];
                if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
                else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
                else if (s > max3) { max3 = s; i3 = i; }
            }
            if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
            else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
        }
        s_ind[0] = i1; s_ind[1] = i2; s_ind[2] = i3;
    }
    __syncthreads();
    int removed = 0;
    if (check_orientation) {
        const int i1 = s_ind[0], i2 = s_ind[1], i3 = s_ind[2];
        for (int k = lane; k < job.nq; k += 64) {
            const int bin = qbin[qa + k];
            if (bin < 0 || bin == i1 || bin == i2 || bin == i3) continue;
            if (match[qa + k] >= 0) { match[qa + k] = -1; dist[qa + k] = -1; ++removed; }
        }
        for (int d = 32; d >= 1; d >>= 1) removed += __shfl_xor(removed, d, 64);
    }
    JobOut* __restrict__ o = out + blockIdx.x;
    if (lane == 0) { o->n_matches = n_matches - removed; o->n_displaced = n_displaced; o->n_rot_removed = removed; }
    if (lane < kHisto) o->hist[lane] = s_hist[lane];
    if (lane < 3) o->ind[lane] = s_ind[lane];
}

}  // namespace orbm
}  // namespace iba

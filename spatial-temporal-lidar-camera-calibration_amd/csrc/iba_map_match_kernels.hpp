// Local-map point matching, the device half (include/iba_mi355x.h, rules L1-L5): the frustum kernel and the resolve kernel. The grid and the
// candidate lists are the matcher's kernels as they are (iba_orb_match_kernels.hpp: cell, scan, fill, list); the float decisions are the one text of
// iba_map_match_math.hpp. No floating-point atomics and no order that depends on atomic arrival: the only atomics are integer counts.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "iba_map_match_host.hpp"      // (with iba_orb_match_host.hpp: everything the matcher's kernels header includes is included here, at file scope, first)

// The matcher's kernels header defines its __global__ functions without `inline`, for the one translation unit that is iba_orb_match.hip. This
// unit launches the same text as kernels of its own: the header is included, unedited, inside iba::mapm::matcher, so its kernels are
// iba::mapm::matcher::iba::orbm::orbm_*_kernel here and no symbol is defined twice in the library. The using-directive hands the header's
// unqualified lookups the host half's names (cell_of, window_first, window_last, the grid constants), which live in ::iba::orbm.
namespace iba {
namespace mapm {
namespace matcher {
namespace iba { namespace orbm { using namespace ::iba::orbm; } }
#include "iba_orb_match_kernels.hpp"
}  // namespace matcher
namespace orbk = matcher::iba::orbm;
}  // namespace mapm
}  // namespace iba

namespace iba {
namespace mapm {

constexpr int kBitmapWords = IBA_ORB_MATCH_MAX_KEYPOINTS / 32;      // 4 KB of LDS: every frame fits, there is no global fallback

struct BlockRec { int32_t job, first; };          // a frustum block: its job and its first list position (blocks do not straddle a job)
struct JobOut { int32_t n_matches; };

// L1 / L2: one lane per slot (job, list position). The job's camera is uniform per block. Writes the status, the view and the slot's QueryRec (the
// point's descriptor lies behind the keypoints' in the flat descriptor table: kp = n_kp + point). The status counts go by wave ballot into LDS and
// from there with one integer atomic per counter and block.
__global__ __launch_bounds__(orbk::kThreads) void mapm_frustum_kernel(const BlockRec* __restrict__ blocks, const JobRec* __restrict__ jobs, const int32_t* __restrict__ slot_point,
                                                                      const uint8_t* __restrict__ slot_skip, const float* __restrict__ xyz, const float* __restrict__ normal,
                                                                      const float* __restrict__ min_dist, const float* __restrict__ max_dist, int n_kp, uint8_t* __restrict__ status,
                                                                      float* __restrict__ view_cos, int32_t* __restrict__ level, orbk::QueryRec* __restrict__ queries,
                                                                      int32_t* __restrict__ job_counts) {
    __shared__ int32_t s_cnt[kStatuses];
    const BlockRec blk = blocks[blockIdx.x];
    const JobRec& job = jobs[blk.job];
    const int tid = (int)threadIdx.x, k = blk.first + tid;
    if (tid < kStatuses) s_cnt[tid] = 0;
    __syncthreads();
    const bool live = k < job.nq;
    int st = -1;
    if (live) {
        const size_t slot = (size_t)job.q0 + (size_t)k;
        View w{IBA_MAP_MATCH_SKIPPED, 0.f, 0.f, 0.f, 0};
        const int32_t p = slot_point[slot];
        if (!slot_skip[slot]) {
            const float P[3] = {xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2]};
            const float N[3] = {normal[3 * (size_t)p], normal[3 * (size_t)p + 1], normal[3 * (size_t)p + 2]};
            w = frustum(job.cam, P, N, min_dist[p], max_dist[p]);
        }
        st = w.status;
        const bool in_view = st == IBA_MAP_MATCH_IN_VIEW;
        const float r = in_view ? query_radius(w.view_cos, job.cam.th, job.cam.sf[w.level]) : 0.f;
        status[slot] = (uint8_t)st;
        view_cos[slot] = w.view_cos; level[slot] = w.level;
        queries[slot] = orbk::QueryRec{w.u, w.v, r, in_view ? w.level - 1 : 0, in_view ? w.level : 0, n_kp + p, job.frame, in_view ? 1 : 0};
    }
    for (int s = 0; s < kStatuses; ++s) {
        const unsigned long long m = __ballot(st == s);
        if ((tid & 63) == 0 && m) atomicAdd(&s_cnt[s], __popcll(m));
    }
    __syncthreads();
    if (tid < kStatuses && s_cnt[tid]) atomicAdd(&job_counts[(size_t)blk.job * kStatuses + (size_t)tid], s_cnt[tid]);
}

// L4: ONE wave per job walks the job's points in order. The claimed state is a bitmap in LDS seeded from `occupied`. Per point the lanes stride over
// its segment and each keeps its two least (distance, position) keys among the candidates below 256 that are not claimed; the wave's first is the
// 64-bit key minimum, its second the least of the winner lane's second and the other lanes' firsts (keys are distinct: a position occurs once). Lane 0
// reads the two octaves and applies the acceptance. One barrier follows each point with a non-empty segment.
__global__ __launch_bounds__(64) void mapm_resolve_kernel(const JobRec* __restrict__ jobs, int job0, int chunk_q0, int chunk_kpo0, const int32_t* __restrict__ octave,
                                                          const uint8_t* __restrict__ occupied, const int32_t* __restrict__ off, const int32_t* __restrict__ cand,
                                                          const uint16_t* __restrict__ cand_dist, int th_high, float nn_ratio, int32_t* __restrict__ match, int32_t* __restrict__ dist,
                                                          int32_t* __restrict__ point_of, JobOut* __restrict__ out) {
    __shared__ uint32_t s_claimed[kBitmapWords];
    const JobRec& job = jobs[job0 + (int)blockIdx.x];
    const int lane = (int)threadIdx.x;
    const int n_kp = job.n_kp, n_words = (n_kp + 31) >> 5;
    for (int w = lane; w < n_words; w += 64) {
        uint32_t bits = 0;
        if (job.occ_base >= 0) {
            const uint8_t* __restrict__ occ = occupied + (size_t)job.occ_base;
            for (int b = 0; b < 32 && 32 * w + b < n_kp; ++b) bits |= occ[32 * w + b] ? (1u << b) : 0u;
        }
        s_claimed[w] = bits;
    }
    const int qa = job.q0 - chunk_q0, ka = job.kpo_base - chunk_kpo0;      // the job's slots and keypoints in the chunk's arrays
    for (int k = lane; k < job.nq; k += 64) { match[qa + k] = -1; dist[qa + k] = -1; }
    for (int c = lane; c < n_kp; c += 64) point_of[ka + c] = -1;
    __syncthreads();
    int n_matches = 0;                                // lane 0's
    for (int k = 0; k < job.nq; ++k) {
        const int a = off[qa + k], b = off[qa + k + 1];
        if (a == b) continue;                         // (uniform)
        uint64_t k1 = kNoKey, k2 = kNoKey;
        for (int e = a + lane; e < b; e += 64) {
            const int d = (int)cand_dist[e];
            const int c = cand[e];
            if (d >= 256 || ((s_claimed[c >> 5] >> (c & 31)) & 1u)) continue;
            const uint64_t key = ((uint64_t)(uint32_t)d << 32) | (uint32_t)(e - a);
            if (key < k1) { k2 = k1; k1 = key; }
            else if (key < k2) k2 = key;
        }
        const uint64_t w1 = orbk::wave_min_u64(k1);
        if (w1 != kNoKey) {                           // (uniform)
            const uint64_t w2 = orbk::wave_min_u64(k1 == w1 ? k2 : k1);
            if (lane == 0) {
                const int c1 = cand[a + (int)(uint32_t)w1], c2 = w2 != kNoKey ? cand[a + (int)(uint32_t)w2] : -1;
                const int best = (int)(w1 >> 32), best2 = c2 >= 0 ? (int)(w2 >> 32) : 256;
                if (accept(true, best, octave[job.kp_base + c1], best2, c2 >= 0 ? octave[job.kp_base + c2] : -1, th_high, nn_ratio)) {
                    s_claimed[c1 >> 5] |= 1u << (c1 & 31);
                    match[qa + k] = c1; dist[qa + k] = best; point_of[ka + c1] = k;
                    ++n_matches;
                }
            }
        }
        __syncthreads();                              // the bitmap lane 0 changed, before the next point's walk
    }
    if (lane == 0) out[blockIdx.x].n_matches = n_matches;
}

}  // namespace mapm
}  // namespace iba

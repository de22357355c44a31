// Map-point fusion, the device half (include/iba_mi355x.h, rules F1-F5): the frustum kernel and the pick kernel. The grid and the candidate lists
// are the matcher's kernels as they are (iba_orb_match_kernels.hpp: cell, scan, fill, list); the float decisions are the one text of
// iba_fuse_math.hpp. Both kernels run on the call's table of blocks: a block is up to 256 consecutive list positions of ONE job, so the job's camera
// and tables are uniform per block. No floating-point atomics and no byte that depends on atomic arrival: the only atomics are integer counts.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "iba_fuse_host.hpp"           // (with iba_orb_match_host.hpp: everything the matcher's kernels header includes is included here, at file scope, first)

// The matcher's kernels header defines its __global__ functions without `inline`; as iba_map_match_kernels.hpp does, this unit includes it,
// unedited, inside a namespace of its own, so its kernels are iba::fuse::matcher::iba::orbm::orbm_*_kernel here and no symbol is defined twice.
namespace iba {
namespace fuse {
namespace matcher {
namespace iba { namespace orbm { using namespace ::iba::orbm; } }
#include "iba_orb_match_kernels.hpp"
}  // namespace matcher
namespace orbk = matcher::iba::orbm;
}  // namespace fuse
}  // namespace iba

namespace iba {
namespace fuse {

struct BlockRec { int32_t job, first; };          // a block: its job and its first list position (blocks do not straddle a job)

// F1-F4: one lane per slot (job, list position). Writes the status (IBA_FUSE_PICKED stands for "in view" until the pick kernel settles it), the
// level, match = dist = -1 and the slot's QueryRec (the point's descriptor lies behind the keypoints' in the flat descriptor table: kp = n_kp +
// point). The counts of the statuses that end here go by wave ballot into LDS and from there with one integer atomic per counter and block.
__global__ __launch_bounds__(orbk::kThreads) void fuse_frustum_kernel(const BlockRec* __restrict__ blocks, const JobRec* __restrict__ jobs, const int32_t* __restrict__ slot_point,
                                                                      const uint8_t* __restrict__ slot_skip, const float* __restrict__ xyz, const float* __restrict__ normal,
                                                                      const float* __restrict__ min_dist, const float* __restrict__ max_dist, int n_kp, uint8_t* __restrict__ status,
                                                                      int32_t* __restrict__ level, int32_t* __restrict__ match, int32_t* __restrict__ dist,
                                                                      orbk::QueryRec* __restrict__ queries, int32_t* __restrict__ job_counts) {
    __shared__ int32_t s_cnt[kStatuses];
    const BlockRec blk = blocks[blockIdx.x];
    const JobRec& job = jobs[blk.job];
    const int tid = (int)threadIdx.x, k = blk.first + tid;
    if (tid < kStatuses) s_cnt[tid] = 0;
    __syncthreads();
    int st = -1;
    if (k < job.nq) {
        const size_t slot = (size_t)job.q0 + (size_t)k;
        View w{IBA_FUSE_SKIPPED, 0.f, 0.f, 0.f, 0};
        const int32_t p = slot_point[slot];
        if (p >= 0 && !slot_skip[slot]) {
            const float P[3] = {xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2]};
            const float N[3] = {normal[3 * (size_t)p], normal[3 * (size_t)p + 1], normal[3 * (size_t)p + 2]};
            w = frustum(job.cam, P, N, min_dist[p], max_dist[p]);
        }
        st = w.status;
        const bool in_view = st == IBA_FUSE_PICKED;
        status[slot] = (uint8_t)st;
        level[slot] = w.level; match[slot] = -1; dist[slot] = -1;
        queries[slot] = orbk::QueryRec{w.u, w.v, w.radius, in_view ? w.level - 1 : 0, in_view ? w.level : 0, in_view ? n_kp + p : 0, job.frame, in_view ? 1 : 0};
    }
    for (int s = IBA_FUSE_SKIPPED; s <= IBA_FUSE_ANGLE; ++s) {
        const unsigned long long m = __ballot(st == s);
        if ((tid & 63) == 0 && m) atomicAdd(&s_cnt[s], __popcll(m));
    }
    __syncthreads();
    if (tid < kStatuses && s_cnt[tid]) atomicAdd(&job_counts[(size_t)blk.job * kStatuses + (size_t)tid], s_cnt[tid]);
}

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

// F5: W lanes per slot, 256 / W slots per round, W rounds per block. The lanes stride over the slot's segment of (candidate, distance) entries; a
// lane gathers position and octave only of a candidate whose key would improve its own; the group's minimum comes from xor shuffles that stay
// inside the aligned group of W lanes. Every lane of the block reaches every shuffle and ballot. Lane 0 of the group writes status, match, dist.
// off, cand and cand_dist are the chunk's (off is indexed from chunk_q0); status, match, dist and queries the call's.
template <int W>
__global__ __launch_bounds__(orbk::kThreads) void fuse_pick_kernel(const BlockRec* __restrict__ blocks, const JobRec* __restrict__ jobs, int chunk_q0,
                                                                   const orbk::QueryRec* __restrict__ queries, const float2* __restrict__ xy, const int32_t* __restrict__ octave,
                                                                   const int32_t* __restrict__ off, const int32_t* __restrict__ cand, const uint16_t* __restrict__ cand_dist, int th_low,
                                                                   float chi2_mono, int check_reprojection, uint8_t* __restrict__ status, int32_t* __restrict__ match,
                                                                   int32_t* __restrict__ dist, int32_t* __restrict__ job_counts) {
    __shared__ int32_t s_cnt[3];
    const BlockRec blk = blocks[blockIdx.x];
    const JobRec& job = jobs[blk.job];
    const int tid = (int)threadIdx.x, sub = tid % W, grp = tid / W;
    constexpr int kPerRound = orbk::kThreads / W;
    if (tid < 3) s_cnt[tid] = 0;
    __syncthreads();
    for (int r = 0; r < W; ++r) {
        const int k = blk.first + r * kPerRound + grp;
        const bool live = k < job.nq;
        const size_t slot = (size_t)job.q0 + (size_t)(live ? k : 0);
        const bool in_view = live && status[slot] == IBA_FUSE_PICKED;
        uint64_t best = kNoKey;
        int a = 0, b = 0;
        if (in_view) {
            a = off[slot - (size_t)chunk_q0]; b = off[slot - (size_t)chunk_q0 + 1];
            const float u = queries[slot].u, v = queries[slot].v;
            for (int e = a + sub; e < b; e += W) {
                const int d = (int)cand_dist[e];
                if (d >= 256) continue;
                const uint64_t key = pick_key(d, (uint32_t)(e - a));
                if (key >= best) continue;
                if (check_reprojection) {
                    const int c = job.kp_base + cand[e];
                    const float2 p = xy[c];
                    if (!gate_passes(u, v, p.x, p.y, job.cam.inv_sigma2[octave[c]], chi2_mono)) continue;
                }
                best = key;
            }
        }
        best = group_min_u64<W>(best);
        int st = -1;
        if (in_view && sub == 0) {
            st = a == b ? IBA_FUSE_NO_CANDIDATE : (best == kNoKey || (int)(best >> 32) > th_low) ? IBA_FUSE_NO_MATCH : IBA_FUSE_PICKED;
            if (st == IBA_FUSE_PICKED) { match[slot] = cand[a + (int)(uint32_t)best]; dist[slot] = (int32_t)(best >> 32); }
            else status[slot] = (uint8_t)st;
        }
        const unsigned long long m0 = __ballot(st == IBA_FUSE_PICKED), m1 = __ballot(st == IBA_FUSE_NO_CANDIDATE), m2 = __ballot(st == IBA_FUSE_NO_MATCH);
        if ((tid & 63) == 0) {
            if (m0) atomicAdd(&s_cnt[0], __popcll(m0));
            if (m1) atomicAdd(&s_cnt[1], __popcll(m1));
            if (m2) atomicAdd(&s_cnt[2], __popcll(m2));
        }
    }
    __syncthreads();
    if (tid < 3 && s_cnt[tid]) atomicAdd(&job_counts[(size_t)blk.job * kStatuses + (size_t)(tid == 0 ? IBA_FUSE_PICKED : tid == 1 ? IBA_FUSE_NO_CANDIDATE : IBA_FUSE_NO_MATCH)], s_cnt[tid]);
}

}  // namespace fuse
}  // namespace iba

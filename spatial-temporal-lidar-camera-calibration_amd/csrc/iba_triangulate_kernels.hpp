// New-map-point creation, the device half (include/iba_mi355x.h, rules R1-R8): prologue, segments, pick, compaction, triangulation, resolve,
// counts and gather. The float decisions are the one text of iba_triangulate_math.hpp; the block scan is the matcher's (iba_orb_match_kernels.hpp,
// included and not edited). Every kernel but the prologue and the triangulation runs on the call's table of blocks: a block is up to 256
// consecutive keypoints of ONE (job, neighbour) pair, so the pair's geometry, keyframes and job are uniform per block. No floating-point atomics
// and no result that depends on atomic arrival: the atomics are integer counts, and the one list whose order they decide is read back by slot.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "iba_triangulate_host.hpp"    // (with iba_orb_match_host.hpp: everything the matcher's kernels header includes is included here, at file scope, first)

// The matcher's kernels header defines its __global__ functions without `inline`; as iba_map_match_kernels.hpp does, this unit includes it,
// unedited, inside a namespace of its own, so its kernels are iba::trg::matcher::iba::orbm::orbm_*_kernel here and no symbol is defined twice.
namespace iba {
namespace trg {
namespace matcher {
namespace iba { namespace orbm { using namespace ::iba::orbm; } }
#include "iba_orb_match_kernels.hpp"
}  // namespace matcher
namespace orbk = matcher::iba::orbm;
}  // namespace trg
}  // namespace iba

namespace iba {
namespace trg {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// the tables of a chunk, by value to every kernel
struct ChunkView {
    const KfRec* __restrict__ kfs; const PairRec* __restrict__ pairs; const JobRec* __restrict__ jobs; const BlockRec* __restrict__ blocks;
    const float2* __restrict__ xy; const int32_t* __restrict__ octave; const uint64_t* __restrict__ desc;          // per keypoint of a frame
    const int32_t* __restrict__ kf_node; const uint8_t* __restrict__ kf_has;                                       // per keypoint of a keyframe
    const int32_t* __restrict__ skey; const int32_t* __restrict__ sidx;                                            // the node order of a keyframe
    int32_t slot0, pair0, block0, job0;            // the chunk's first slot, pair, block and job in the call's tables
    int32_t n_slots, n_pairs, n_blocks, n_jobs;
    Gates gt;
};

// R1: one lane per pair of the chunk
__global__ __launch_bounds__(kThreads) void trg_prologue_kernel(ChunkView c, PairGeom* __restrict__ geom) {
    const int p = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (p >= c.n_pairs) return;
    const PairRec pr = c.pairs[c.pair0 + p];
    PairGeom g;
    pair_prologue(c.kfs[pr.cur].kf, c.kfs[pr.nb].kf, c.gt.min_baseline_ratio, g);
    geom[p] = g;
}

// R2: one lane per slot. Where the slot ends here it gets its status; otherwise kPending and its segment [a, b) in the neighbour's node order.
__global__ __launch_bounds__(kThreads) void trg_segment_kernel(ChunkView c, const PairGeom* __restrict__ geom, uint8_t* __restrict__ status, int32_t* __restrict__ match,
                                                               int32_t* __restrict__ dist, float* __restrict__ xyz, int32_t* __restrict__ seg_a, int32_t* __restrict__ seg_b) {
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    const int i = blk.first + (int)threadIdx.x;
    if (i >= pr.n_cur) return;
    const KfRec& k1 = c.kfs[pr.cur];
    const KfRec& k2 = c.kfs[pr.nb];
    const size_t slot = (size_t)(pr.slot_base - c.slot0) + (size_t)i;
    const bool skipped = geom[blk.pair - c.pair0].skipped != 0;
    const bool has = c.kf_has[k1.kn_base + i] != 0;
    const int node = c.kf_node[k1.kn_base + i];
    int a = 0, b = 0;
    if (!skipped && !has && node >= 0) {
        const int32_t* __restrict__ key = c.skey + k2.kn_base;
        int lo = 0, hi = k2.n_keys;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] < node) lo = m + 1; else hi = m; }
        a = lo; hi = k2.n_keys;
        while (lo < hi) { const int m = (lo + hi) >> 1; if (key[m] <= node) lo = m + 1; else hi = m; }
        b = lo;
    }
    const int st = skipped ? IBA_TRIANGULATE_PAIR_SKIPPED : has ? IBA_TRIANGULATE_HAS_POINT : a == b ? IBA_TRIANGULATE_NO_NODE : (int)kPending;
    status[slot] = (uint8_t)st;
    match[slot] = -1; dist[slot] = -1;
    xyz[3 * slot] = 0.f; xyz[3 * slot + 1] = 0.f; xyz[3 * slot + 2] = 0.f;
    seg_a[slot] = a; seg_b[slot] = b;
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

// R3: W lanes per query, 256 / W queries per round, W rounds per block. The query's 256 bits and its epipolar line sit in registers; the lanes
// stride over the segment, each keeps its least (distance, descending position) key among the candidates that pass, the group's minimum comes from
// xor shuffles that stay inside the aligned group of W lanes. Every lane of the block reaches every shuffle. A pending slot leaves with NO_MATCH,
// or stays pending with its match and distance for the triangulation.
template <int W>
__global__ __launch_bounds__(kThreads) void trg_pick_kernel(ChunkView c, const PairGeom* __restrict__ geom, const int32_t* __restrict__ seg_a, const int32_t* __restrict__ seg_b,
                                                            uint8_t* __restrict__ status, int32_t* __restrict__ match, int32_t* __restrict__ dist) {
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    const KfRec& k1 = c.kfs[pr.cur];
    const KfRec& k2 = c.kfs[pr.nb];
    const PairGeom& g = geom[blk.pair - c.pair0];
    const Scales& sc = c.jobs[pr.job].sc;
    const int sub = (int)threadIdx.x % W, grp = (int)threadIdx.x / W;
    constexpr int kPerRound = kThreads / W;
    const int32_t* __restrict__ sidx = c.sidx + k2.kn_base;
    for (int r = 0; r < W; ++r) {
        const int i = blk.first + r * kPerRound + grp;
        const bool live = i < pr.n_cur;
        const size_t slot = (size_t)(pr.slot_base - c.slot0) + (size_t)(live ? i : 0);
        const bool pending = live && status[slot] == kPending;
        uint64_t best = kNoKey;
        int a = 0;
        if (pending) {
            a = seg_a[slot];
            const int b = seg_b[slot];
            uint64_t d1[4];
            for (int w = 0; w < 4; ++w) d1[w] = c.desc[4 * (size_t)(k1.kp_base + i) + (size_t)w];
            const float2 p1 = c.xy[k1.kp_base + i];
            const Line l = epipolar_line(g.F12, p1.x, p1.y);
            for (int p = a + sub; p < b; p += W) {
                const int i2 = sidx[p];
                if (i2 < 0) continue;                                        // it has a point
                const int d = orbk::hamming256(d1, c.desc + 4 * (size_t)(k2.kp_base + i2));
                if (d > c.gt.th_low) continue;
                const uint64_t key = pick_key(d, (uint32_t)(p - a));
                if (key >= best) continue;
                const float2 p2 = c.xy[k2.kp_base + i2];
                const int o2 = c.octave[k2.kp_base + i2];
                if (candidate_passes(l, g.ex, g.ey, p2.x, p2.y, sc.sf[o2], sc.sigma2[o2], c.gt.epipole_gate, c.gt.chi2_line)) best = key;
            }
        }
        best = group_min_u64<W>(best);
        if (pending && sub == 0) {
            if (best == kNoKey) status[slot] = (uint8_t)IBA_TRIANGULATE_NO_MATCH;
            else { match[slot] = sidx[a + (int)pick_pos(best)]; dist[slot] = (int32_t)(best >> 32); }
        }
    }
}

// the exclusive prefix of a flag inside the block and the block's total; s_wave: kWaves + 1 ints of LDS. Every lane of the block calls it.
__device__ inline int block_prefix(bool flag, int* s_wave, int* total) {
    const unsigned long long m = __ballot(flag);
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) s_wave[wave] = __popcll(m);
    __syncthreads();
    int base = 0, sum = 0;
    for (int w = 0; w < kWaves; ++w) { const int n = s_wave[w]; if (w < wave) base += n; sum += n; }
    *total = sum;
    return base + before;
}

// the matched slots as a list, so that the lanes of the triangulation are all busy: ballot prefix inside the block, one integer atomic per block
// for the base. The list's order depends on the atomics' arrival; nothing else does, because the triangulation writes by slot.
__global__ __launch_bounds__(kThreads) void trg_compact_kernel(ChunkView c, const uint8_t* __restrict__ status, int32_t* __restrict__ n_list, int32_t* __restrict__ list_slot,
                                                               int32_t* __restrict__ list_pair) {
    __shared__ int s_wave[kWaves + 1];
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    const int i = blk.first + (int)threadIdx.x;
    const int slot = pr.slot_base - c.slot0 + i;
    const bool flag = i < pr.n_cur && status[slot] == kPending;
    int total = 0;
    const int at = block_prefix(flag, s_wave, &total);
    if (threadIdx.x == 0) s_wave[kWaves] = total ? atomicAdd(n_list, total) : 0;
    __syncthreads();
    if (flag) { const int k = s_wave[kWaves] + at; list_slot[k] = slot; list_pair[k] = blk.pair; }
}

// R4-R6: one lane per matched slot of the list
__global__ __launch_bounds__(kThreads) void trg_triangulate_kernel(ChunkView c, const int32_t* __restrict__ n_list, const int32_t* __restrict__ list_slot,
                                                                   const int32_t* __restrict__ list_pair, const int32_t* __restrict__ match, uint8_t* __restrict__ status,
                                                                   float* __restrict__ xyz) {
    const int k = (int)blockIdx.x * kThreads + (int)threadIdx.x;
    if (k >= *n_list) return;
    const int slot = list_slot[k];
    const PairRec pr = c.pairs[list_pair[k]];
    const KfRec& k1 = c.kfs[pr.cur];
    const KfRec& k2 = c.kfs[pr.nb];
    const int i = slot - (pr.slot_base - c.slot0), i2 = match[slot];
    const float2 p1 = c.xy[k1.kp_base + i], p2 = c.xy[k2.kp_base + i2];
    const Outcome o = triangulate(k1.kf, k2.kf, c.jobs[pr.job].sc, c.gt, p1.x, p1.y, c.octave[k1.kp_base + i], p2.x, p2.y, c.octave[k2.kp_base + i2]);
    status[slot] = (uint8_t)o.status;
    xyz[3 * (size_t)slot] = o.x[0]; xyz[3 * (size_t)slot + 1] = o.x[1]; xyz[3 * (size_t)slot + 2] = o.x[2];
}

// R7: one lane per (job, keypoint of the current keyframe): the blocks of a job's first pair cover exactly those; the others leave at once
__global__ __launch_bounds__(kThreads) void trg_resolve_kernel(ChunkView c, uint8_t* __restrict__ status, int32_t* __restrict__ match, int32_t* __restrict__ dist, float* __restrict__ xyz) {
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    if (pr.pos != 0) return;
    const int i = blk.first + (int)threadIdx.x;
    if (i >= pr.n_cur) return;
    const int n_nb = c.jobs[pr.job].n_nb;
    bool got = false;
    for (int pos = 0; pos < n_nb; ++pos) {
        const size_t slot = (size_t)(pr.slot_base - c.slot0) + (size_t)pos * (size_t)pr.n_cur + (size_t)i;
        if (got) {
            status[slot] = (uint8_t)IBA_TRIANGULATE_SUPERSEDED;
            match[slot] = -1; dist[slot] = -1;
            xyz[3 * slot] = 0.f; xyz[3 * slot + 1] = 0.f; xyz[3 * slot + 2] = 0.f;
        } else if (status[slot] == IBA_TRIANGULATE_CREATED) got = true;
    }
}

// the counts: per job and status, per pair the matches and the created points (wave ballots into LDS, one integer atomic per counter and block),
// and per block the created points, for the scan
__global__ __launch_bounds__(kThreads) void trg_count_kernel(ChunkView c, const uint8_t* __restrict__ status, const int32_t* __restrict__ match, int32_t* __restrict__ job_counts,
                                                             int32_t* __restrict__ pair_counts, int32_t* __restrict__ blk_cnt) {
    __shared__ int32_t s_cnt[kStatuses + 1];
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    const int tid = (int)threadIdx.x, i = blk.first + tid;
    if (tid <= kStatuses) s_cnt[tid] = 0;
    __syncthreads();
    int st = -1;
    bool matched = false;
    if (i < pr.n_cur) {
        const int slot = pr.slot_base - c.slot0 + i;
        st = status[slot]; matched = match[slot] >= 0;
    }
    for (int s = 0; s <= kStatuses; ++s) {
        const unsigned long long m = __ballot(s < kStatuses ? st == s : matched);
        if ((tid & 63) == 0 && m) atomicAdd(&s_cnt[s], __popcll(m));
    }
    __syncthreads();
    if (tid < kStatuses && s_cnt[tid]) atomicAdd(&job_counts[(size_t)(pr.job - c.job0) * kStatuses + (size_t)tid], s_cnt[tid]);
    if (tid == 0) {
        if (s_cnt[kStatuses]) atomicAdd(&pair_counts[2 * (size_t)(blk.pair - c.pair0)], s_cnt[kStatuses]);
        if (s_cnt[IBA_TRIANGULATE_CREATED]) atomicAdd(&pair_counts[2 * (size_t)(blk.pair - c.pair0) + 1], s_cnt[IBA_TRIANGULATE_CREATED]);
        blk_cnt[blockIdx.x] = s_cnt[IBA_TRIANGULATE_CREATED];
    }
}

// R8: the created points in creation order. The blocks run job after job, neighbour after neighbour, keypoints ascending, so a point's place is the
// scan of the blocks' counts plus its prefix inside the block.
__global__ __launch_bounds__(kThreads) void trg_gather_kernel(ChunkView c, const uint8_t* __restrict__ status, const int32_t* __restrict__ match, const float* __restrict__ xyz,
                                                              const int32_t* __restrict__ blk_off, int32_t* __restrict__ p_idx1, int32_t* __restrict__ p_nb, int32_t* __restrict__ p_idx2,
                                                              float* __restrict__ p_xyz, float* __restrict__ p_normal, float* __restrict__ p_min, float* __restrict__ p_max,
                                                              uint64_t* __restrict__ p_desc) {
    __shared__ int s_wave[kWaves + 1];
    const BlockRec blk = c.blocks[c.block0 + (int)blockIdx.x];
    const PairRec pr = c.pairs[blk.pair];
    const int i = blk.first + (int)threadIdx.x;
    const int slot = pr.slot_base - c.slot0 + i;
    const bool flag = i < pr.n_cur && status[slot] == IBA_TRIANGULATE_CREATED;
    int total = 0;
    const int at = block_prefix(flag, s_wave, &total);
    if (!flag) return;
    const size_t k = (size_t)blk_off[blockIdx.x] + (size_t)at;
    const KfRec& k1 = c.kfs[pr.cur];
    const KfRec& k2 = c.kfs[pr.nb];
    const float x[3] = {xyz[3 * (size_t)slot], xyz[3 * (size_t)slot + 1], xyz[3 * (size_t)slot + 2]};
    float nrm[3], mn, mx;
    new_point(k1.kf, k2.kf, c.jobs[pr.job].sc, x, c.octave[k1.kp_base + i], nrm, &mn, &mx);
    p_idx1[k] = i; p_nb[k] = pr.pos; p_idx2[k] = match[slot];
    for (int d = 0; d < 3; ++d) { p_xyz[3 * k + (size_t)d] = x[d]; p_normal[3 * k + (size_t)d] = nrm[d]; }
    p_min[k] = mn; p_max[k] = mx;
    for (int w = 0; w < 4; ++w) p_desc[4 * k + (size_t)w] = c.desc[4 * (size_t)(k1.kp_base + i) + (size_t)w];
}

}  // namespace trg
}  // namespace iba

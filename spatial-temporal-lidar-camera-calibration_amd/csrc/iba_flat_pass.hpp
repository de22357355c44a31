// The skeleton the correspondence passes share (iba_icp_*, iba_scan_*, iba_floam_map_*: iba_{icp,scan,floam_map}_{kernels,host}.hpp). A pass
// is a search kernel whose lanes own one source point each and whose waves write ONE partial of NS doubles, then a sum kernel that adds the
// partials of an item. The rules stated here are what makes an item's output the same bytes whatever else is in the batch and whichever
// block shape the batch selects:
//
//  * The flat grid. A job with P source positions (kd-leaf order of its source cloud) owns ceil(P / THREADS) consecutive blocks and
//    ceil(P / 64) partials, one per 64-position chunk; the host places the jobs in ascending order (flat_take) and a block finds its job by
//    bisection over the jobs' first blocks (flat_job). A 256-thread block is four chunks of ONE job, so the chunk -> partial map does not
//    depend on the block shape; a wave of such a block beyond the job's last chunk has no partial.
//  * The block shape (pass_shape): one-wave blocks while the largest node table of the pass is at most kOneWaveLdsMax bytes
//    (a CU then holds 16 of them), else four waves per block. The block stages the table in LDS (stage_nodes; the barrier is the caller's).
//  * The sums. A wave adds its lanes' terms by DPP (wave_sum_f64: fixed order) and lane 63 writes the partial (wave_sum_store). The sum kernel
//    runs 256 threads per item: thread t takes the partials t, t + 256, ..; the 64 threads of a wave by DPP; the four waves in order
//    (block_sum_partials, wave_totals). No atomics. A launch of its own: folded into the pass kernel's last block it would wait on a
//    completion counter (that serialises).
//  * Ties. nn_merge keeps the lowest original index inside a tile; across the tiles of a target a later tile replaces the best only when
//    STRICTLY closer, and the tiles are searched in ascending order: the lowest (frame, index) wins. The box test (box_dist2) is exact.
//
// The host half (PassWork, pass_shape, flat_take) is plain C++ beside the kernels' helpers: one staging rule, one shape rule, one placement.
#pragma once
#include "iba_device_buf.hpp"
#include "iba_kernels.hpp"
#include "iba_split_kernels.hpp"

namespace iba {

constexpr uint32_t kOneWaveLdsMax = 6144u;   // bytes of node table up to which a pass runs one-wave blocks (also iba_handle::nn_small)

// ---- device ----

// the last job whose first block (the member FIRST) is not beyond blk; the jobs' first blocks ascend (uniform over the block)
template <auto FIRST, class Job>
__device__ __forceinline__ int flat_job(const Job* __restrict__ jobs, int nj, uint32_t blk) {
    int lo = 0, hi = nj - 1;
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (jobs[mid].*FIRST <= blk) lo = mid; else hi = mid - 1; }
    return lo;
}

// the kd node table of frame h into LDS, by the whole block
template <int THREADS>
__device__ __forceinline__ void stage_nodes(const DevProblem& dp, const FrameHdr& h, TreeNode* s_nodes) {
    const uint32_t nn = (1u << h.depth) - 1u;
    for (uint32_t i = threadIdx.x; i < nn; i += THREADS) s_nodes[i] = dp.nodes[h.node_base + i];
}

// d^2 of q to the box bx = (min xyz, -, max xyz, -). Exact as a bound: it is formed with the operations of the point distance (a difference
// per axis, its square, the same order of additions), each monotone in its operand after rounding, and per axis |q - face| <= |q - p| for
// every p inside the box: the result never exceeds the COMPUTED distance of a point inside the box. A test `box_dist2 > bound` therefore
// skips no point that could replace the bound's holder, and `box_dist2 < bound` searches whenever a point within the bound can exist.
__device__ __forceinline__ double box_dist2(const float* __restrict__ bx, double q0, double q1, double q2) {
    const double lx = (double)bx[0], ly = (double)bx[1], lz = (double)bx[2], hx = (double)bx[4], hy = (double)bx[5], hz = (double)bx[6];
    const double dx = q0 < lx ? q0 - lx : (q0 > hx ? q0 - hx : 0.0), dy = q1 < ly ? q1 - ly : (q1 > hy ? q1 - hy : 0.0), dz = q2 < lz ? q2 - lz : (q2 > hz ? q2 - hz : 0.0);
    return (dx * dx + dy * dy) + dz * dz;
}

// the 18 point-to-point terms of one kept pair about the pivot: 1, d^2, dq (3), dt (3), |dq|^2, dt dq^T (9); q the moved source point, t its target
__device__ __forceinline__ void p2p_terms(double* __restrict__ v, double d2, double q0, double q1, double q2, double t0, double t1, double t2, const double* __restrict__ piv) {
    const double dq[3] = {q0 - piv[0], q1 - piv[1], q2 - piv[2]};
    const double dp_[3] = {t0 - piv[0], t1 - piv[1], t2 - piv[2]};
    v[0] = 1.0; v[1] = d2;
    v[2] = dq[0]; v[3] = dq[1]; v[4] = dq[2];
    v[5] = dp_[0]; v[6] = dp_[1]; v[7] = dp_[2];
    v[8] = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) v[9 + 3 * i + j] = dp_[i] * dq[j];
}

// v added over the wave (the total in lane 63); lane 63 of a wave that `writes` stores it as the partial at out. Every lane of the wave calls.
template <int NS>
__device__ __forceinline__ void wave_sum_store(double (&v)[NS], bool writes, double* __restrict__ out) {
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = wave_sum_f64(v[k]);
    if ((threadIdx.x & 63u) == 63u && writes) {
#pragma unroll
        for (int k = 0; k < NS; ++k) out[k] = v[k];
    }
}

// the nw partials from first, added by a 256-thread block: the four wave totals are left in s_w (the barrier before they are read is the caller's)
template <int NS>
__device__ __forceinline__ void block_sum_partials(const double* __restrict__ first, int nw, double (*s_w)[NS]) {
    const int t = (int)threadIdx.x;
    double a[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = 0.0;
    for (int w = t; w < nw; w += 256) {
        const double* p = first + (size_t)w * NS;
#pragma unroll
        for (int k = 0; k < NS; ++k) a[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < NS; ++k) a[k] = wave_sum_f64(a[k]);
    if ((t & 63) == 63) {
#pragma unroll
        for (int k = 0; k < NS; ++k) s_w[t >> 6][k] = a[k];
    }
}
template <int NS>
__device__ __forceinline__ double wave_totals(const double (*s_w)[NS], int k) { return ((s_w[0][k] + s_w[1][k]) + s_w[2][k]) + s_w[3][k]; }

// ---- host ----

// threads per block and bytes of dynamic LDS of a pass whose largest node table has max_nodes entries
struct PassShape { int threads; size_t lds; };
inline PassShape pass_shape(uint32_t max_nodes) {
    const size_t lds = 8u * (size_t)std::max(max_nodes, 1u);
    return {lds <= kOneWaveLdsMax ? 64 : 256, lds};
}
inline uint32_t tree_nodes(const FrameHdr& f) { return (1u << f.depth) - 1u; }

// a job of P positions takes its ceil(P / per) blocks (per = threads) or chunks (per = 64) at `next`: its first one is returned
inline uint32_t flat_take(uint64_t& next, uint32_t P, int per) {
    const uint32_t first = (uint32_t)next;
    next += (P + (uint32_t)per - 1u) / (uint32_t)per;
    return first;
}

// The buffers every pass has: its items (transforms / edges / jobs) staged in pinned memory and on the device, the partials, the moment
// blocks on the device and in pinned memory. They live in the handle and only grow (PinnedBuf::grow, DevBuf::grow).
template <class Item>
struct PassWork {
    DevBuf<Item> d_item; PinnedBuf<Item> h_item;
    DevBuf<double> d_part, d_mom; PinnedBuf<double> h_mom;
    hipError_t reserve(size_t n_items, size_t n_mom) {
        hipError_t e = d_item.grow(n_items);
        if (e == hipSuccess) e = h_item.grow(n_items);
        if (e == hipSuccess) e = d_mom.grow(n_mom);
        if (e == hipSuccess) e = h_mom.grow(n_mom);
        return e;
    }
    hipError_t upload(size_t n_items, hipStream_t st) { return hipMemcpyAsync(d_item.p, h_item.p, sizeof(Item) * n_items, hipMemcpyHostToDevice, st); }
    // after the sum kernel's launch: its launch status, the moments to pinned memory, the pass's ONE synchronise
    hipError_t finish(size_t n_mom, hipStream_t st) {
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(h_mom.p, d_mom.p, sizeof(double) * n_mom, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        return e;
    }
};

}  // namespace iba

// Device side of iba_icp_step / iba_icp_register (include/iba_mi355x.h): one correspondence pass of point-to-point ICP per (transform, source
// chunk), the sums of the kept pairs formed where the search runs.
//
//  iba_icp_pass_kernel<THREADS>   grid (ceil(n / THREADS), B). A lane owns one source point: it transforms the point in f64 (three fused
//      multiply-adds per row, icp_transform), runs the evaluation path's own exact 1-NN lane search (lane_nn_begin / lane_nn_visit<1>, what
//      iba_nn_probe_kernel drives) against every tile of the target — the tile's kd nodes staged in LDS by the block, the lane's best distance
//      carried into the next tile's search as its pruning bound, a tile whose bounding box is further away than that skipped by the lane —,
//      applies the gate d^2 < r^2 and forms its 18 terms in registers. A wave adds its lanes' terms by DPP (wave_sum_f64: fixed order) and its
//      last lane writes ONE partial of kIcpSums doubles. No atomics, no scratch outside the tree search.
//  iba_icp_sum_kernel             grid (B), 256 threads: the partials of a transform added in an order fixed by position (thread t takes the
//      waves t, t + 256, ..; the 64 threads of a wave by DPP; the four waves in order), the pivot appended: IBA_ICP_NMOM doubles per transform.
//      A launch of its own: folded into the pass kernel's last block it would wait on a completion counter (that serialises).
//
// Ties: nn_merge keeps the lowest original index inside a tile; across tiles a later tile replaces the best only when STRICTLY closer, and the
// tiles are searched in ascending order: the lowest (frame, index) wins. The box test is exact: a box distance is formed with the operations of
// the point distance, each monotone in its operand after rounding, so it never exceeds the computed distance of a point inside the box.
// Block shape (the rule of DESIGN.md 5b): one-wave blocks while the largest tile's node table is at most 6 KB, else four waves per block.
#pragma once
#include "iba_kernels.hpp"
#include "iba_split_kernels.hpp"

namespace iba {

constexpr int kIcpSums = 18;   // doubles per partial: the summed part of the IBA_ICP_NMOM = 21 moments (the pivot is not summed)
constexpr int kIcpMom = 21;

struct IcpXf {          // one transform of a pass (host -> device)
    double T[12];       // rows 0-2 of the row-major 4x4
    double piv[3];      // the pivot the sums are taken about: T * centroid(source)
    double gate2;       // max_corr_dist^2
};

// q = T x: row r = fma(T[r][2], z, fma(T[r][1], y, fma(T[r][0], x, T[r][3])))  (fdot3c; the library is built -ffp-contract=off: only these fuse)
__device__ __forceinline__ void icp_transform(const double* __restrict__ T, double x, double y, double z, double& q0, double& q1, double& q2) {
    q0 = fdot3c(T[0], x, T[1], y, T[2], z, T[3]);
    q1 = fdot3c(T[4], x, T[5], y, T[6], z, T[7]);
    q2 = fdot3c(T[8], x, T[9], y, T[10], z, T[11]);
}

// frame_box: [frame][8] min xyz, -, max xyz, - of every local frame's scan (NaN for an empty one)
template <int THREADS>
__global__ __launch_bounds__(THREADS) void iba_icp_pass_kernel(DevProblem dp, const float* __restrict__ frame_box, int fb, int fe, const double* __restrict__ src, int n,
                                                               const IcpXf* __restrict__ xf, double* __restrict__ partials, uint32_t* __restrict__ pair_frame, uint32_t* __restrict__ pair_idx) {
    extern __shared__ __align__(16) unsigned char smem[];
    TreeNode* s_nodes = (TreeNode*)smem;
    const int e = (int)(blockIdx.x * THREADS + threadIdx.x);
    const bool act = e < n;
    const IcpXf& X = xf[blockIdx.y];
    double sx = 0.0, sy = 0.0, sz = 0.0;
    if (act) { sx = src[3 * (size_t)e]; sy = src[3 * (size_t)e + 1]; sz = src[3 * (size_t)e + 2]; }
    double q0, q1, q2;
    icp_transform(X.T, sx, sy, sz, q0, q1, q2);
    double gbest = INFINITY; uint32_t gfr = kNone; uint64_t gpt = 0;   // best so far: d^2, local frame, position in the flat point arrays
    IBA_LANE_NN_DECL;
    for (int f = fb; f < fe; ++f) {   // (every condition on the way to a barrier is uniform over the block)
        const FrameHdr& h = dp.frames[f];
        const uint32_t P = h.P, D = h.depth;
        if (P == 0) continue;
        for (uint32_t i = threadIdx.x; i < (1u << D) - 1u; i += THREADS) s_nodes[i] = dp.nodes[h.node_base + i];
        __syncthreads();
        bool look = act;
        if (look && gfr != kNone) {   // a later tile: is its box within reach at all?
            const float* bx = frame_box + 8 * (size_t)f;
            const double lx = (double)bx[0], ly = (double)bx[1], lz = (double)bx[2], hx = (double)bx[4], hy = (double)bx[5], hz = (double)bx[6];
            const double dx = q0 < lx ? q0 - lx : (q0 > hx ? q0 - hx : 0.0), dy = q1 < ly ? q1 - ly : (q1 > hy ? q1 - hy : 0.0), dz = q2 < lz ? q2 - lz : (q2 > hz ? q2 - hz : 0.0);
            look = !((dx * dx + dy * dy) + dz * dz > gbest);
        }
        if (look) {
            const float4* p4 = dp.pts4 + h.pt_base;
            const uint32_t* perm = dp.perm + h.pt_base;
            actA = true; actC = false; ax = q0; ay = q1; az = q2;
            lane_nn_begin(IBA_LANE_NN_PASS);
            bestA = gbest;   // the bound carried over (first tile: infinity, the plain search)
            do { lane_nn_visit<1>(IBA_LANE_NN_PASS, s_nodes, p4, perm, P, D); } while (go >= 0);
            if (bposA != kNone && bestA < gbest) { gbest = bestA; gfr = (uint32_t)f; gpt = h.pt_base + bposA; }
        }
        if (f + 1 < fe) __syncthreads();   // the node table is overwritten by the next tile
    }
    const bool keep = act && gfr != kNone && gbest < X.gate2;
    double v[kIcpSums];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) v[k] = 0.0;
    uint32_t gidx = kNone;
    if (keep) {
        const float4 pv = dp.pts4[gpt];
        gidx = dp.perm[gpt];
        const double dq[3] = {q0 - X.piv[0], q1 - X.piv[1], q2 - X.piv[2]};
        const double dp_[3] = {(double)pv.x - X.piv[0], (double)pv.y - X.piv[1], (double)pv.z - X.piv[2]};
        v[0] = 1.0; v[1] = gbest;
        v[2] = dq[0]; v[3] = dq[1]; v[4] = dq[2];
        v[5] = dp_[0]; v[6] = dp_[1]; v[7] = dp_[2];
        v[8] = (dq[0] * dq[0] + dq[1] * dq[1]) + dq[2] * dq[2];
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) v[9 + 3 * i + j] = dp_[i] * dq[j];
    }
    if (pair_idx && act) {
        const size_t o = (size_t)blockIdx.y * (size_t)n + (size_t)e;
        pair_frame[o] = keep ? gfr : kNone; pair_idx[o] = gidx;
    }
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) v[k] = wave_sum_f64(v[k]);   // (the total in lane 63)
    if ((threadIdx.x & 63u) == 63u) {
        const size_t nw = (size_t)gridDim.x * (THREADS / 64);
        double* o = partials + ((size_t)blockIdx.y * nw + (size_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6)) * kIcpSums;
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) o[k] = v[k];
    }
}

// nw: partials (waves) per transform
__global__ __launch_bounds__(256) void iba_icp_sum_kernel(const double* __restrict__ partials, int nw, const IcpXf* __restrict__ xf, double* __restrict__ out) {
    __shared__ double s_w[4][kIcpSums];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    double a[kIcpSums];
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) a[k] = 0.0;
    for (int w = t; w < nw; w += 256) {
        const double* p = partials + ((size_t)b * (size_t)nw + (size_t)w) * kIcpSums;
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) a[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < kIcpSums; ++k) a[k] = wave_sum_f64(a[k]);
    if ((t & 63) == 63) {
#pragma unroll
        for (int k = 0; k < kIcpSums; ++k) s_w[t >> 6][k] = a[k];
    }
    __syncthreads();
    if (t < kIcpSums) out[(size_t)b * kIcpMom + t] = ((s_w[0][t] + s_w[1][t]) + s_w[2][t]) + s_w[3][t];
    else if (t < kIcpMom) out[(size_t)b * kIcpMom + t] = xf[b].piv[t - kIcpSums];
}

}  // namespace iba

// Device side of iba_icp_step / iba_icp_register (include/iba_mi355x.h): one correspondence pass of point-to-point ICP per (transform, source
// chunk), the sums of the kept pairs formed where the search runs. The shared rules (sums, ties, block shape) are iba_flat_pass.hpp's.
//
//  iba_icp_pass_kernel<THREADS>   grid (ceil(n / THREADS), B): not a flat grid, every transform walks the same uploaded source. A lane owns
//      one source point: it transforms the point in f64 (three fused multiply-adds per row, icp_transform), runs the evaluation path's own
//      exact 1-NN lane search (lane_nn_begin / lane_nn_visit<1>, what iba_nn_probe_kernel drives) against every tile of the target — the lane's
//      best distance carried into the next tile's search as its pruning bound, a tile whose box is further away than that skipped by the
//      lane —, applies the gate d^2 < r^2 and forms its 18 terms in registers. Every wave writes a partial of kIcpSums doubles.
//  iba_icp_sum_kernel             grid (B): the partials of a transform added, the pivot appended: IBA_ICP_NMOM doubles per transform.
#pragma once
#include "iba_flat_pass.hpp"

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
        stage_nodes<THREADS>(dp, h, s_nodes);
        __syncthreads();
        bool look = act;
        if (look && gfr != kNone) look = !(box_dist2(frame_box + 8 * (size_t)f, q0, q1, q2) > gbest);   // a later tile: is its box within reach at all?
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
        p2p_terms(v, gbest, q0, q1, q2, (double)pv.x, (double)pv.y, (double)pv.z, X.piv);
    }
    if (pair_idx && act) {
        const size_t o = (size_t)blockIdx.y * (size_t)n + (size_t)e;
        pair_frame[o] = keep ? gfr : kNone; pair_idx[o] = gidx;
    }
    const size_t nw = (size_t)gridDim.x * (THREADS / 64);   // (every wave writes: the sum kernel reads nw partials per transform)
    wave_sum_store<kIcpSums>(v, true, partials + ((size_t)blockIdx.y * nw + (size_t)blockIdx.x * (THREADS / 64) + (threadIdx.x >> 6)) * kIcpSums);
}

// nw: partials (waves) per transform
__global__ __launch_bounds__(256) void iba_icp_sum_kernel(const double* __restrict__ partials, int nw, const IcpXf* __restrict__ xf, double* __restrict__ out) {
    __shared__ double s_w[4][kIcpSums];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    block_sum_partials<kIcpSums>(partials + (size_t)b * (size_t)nw * kIcpSums, nw, s_w);
    __syncthreads();
    if (t < kIcpSums) out[(size_t)b * kIcpMom + t] = wave_totals(s_w, t);
    else if (t < kIcpMom) out[(size_t)b * kIcpMom + t] = xf[b].piv[t - kIcpSums];
}

}  // namespace iba

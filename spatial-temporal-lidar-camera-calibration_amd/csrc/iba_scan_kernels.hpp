// Device side of iba_scan_step / iba_scan_register / iba_scan_information (include/iba_mi355x.h): one correspondence pass of scan-to-scan ICP
// for a BATCH OF EDGES (source scan -> target scan, both resident in the handle) on the flat grid of iba_flat_pass.hpp, a job = an edge.
//
//  iba_scan_pass_kernel<THREADS, MODE>   a lane reads its source point from the resident pts4 (float32, widened), transforms it in f64
//      (icp_transform), runs the evaluation path's exact 1-NN lane search (lane_nn_begin / lane_nn_visit<1>) against the edge's target tree,
//      applies the gate d^2 < r^2 and forms its terms in registers:
//        MODE 0  point-to-point: the 18 pivoted sums (p2p_terms), the pivot = T * centre of the source scan's box
//        MODE 1  point-to-plane: kept pairs, sum d^2, pairs that carry a normal, JtJ (21, upper triangle by rows), Jtr (6), sum r^2 — 31 sums,
//                about the origin of the target frame. The normal is the cost path's memoised plane of the target point (plane_cost); a record
//                with fewer than max(norm_min_pts, 3) kept neighbours or a non-finite normal carries none: such a pair counts in [0], [1] only
//        MODE 2  information: kept pairs, sum t (3), sum t t^T (6, upper triangle by rows), t the TARGET point — 10 sums about the origin
//      The terms are formed after the search has ended: none of them is live across it.
//  iba_scan_sum_kernel<MODE>             grid (edges): IBA_SCAN_NMOM doubles per edge.
#pragma once
#include "iba_icp_kernels.hpp"

namespace iba {

constexpr int kScanMom = 32;                         // IBA_SCAN_NMOM
constexpr int kScanP2P = 0, kScanP2L = 1, kScanInfo = 2;
template <int MODE> struct ScanSums { static constexpr int n = MODE == kScanP2P ? kIcpSums : (MODE == kScanP2L ? 31 : 10); };

struct ScanXf {          // one edge of a pass (host -> device)
    double T[12];        // rows 0-2 of the row-major 4x4
    double piv[3];       // MODE 0: the pivot the sums are taken about
    double gate2;        // max distance^2
    int32_t src, tgt;    // local frames
    uint32_t blk0;       // first block of the edge in the flat grid
    uint32_t part0;      // first partial (64-position chunk) of the edge
    uint64_t pair0;      // first entry of the edge in the pair output
};

template <int THREADS, int MODE>
__global__ __launch_bounds__(THREADS) void iba_scan_pass_kernel(DevProblem dp, const ScanXf* __restrict__ xf, int nb, int min_pts, double* __restrict__ partials, uint32_t* __restrict__ pair_idx) {
    constexpr int NS = ScanSums<MODE>::n;
    extern __shared__ __align__(16) unsigned char smem[];
    TreeNode* s_nodes = (TreeNode*)smem;
    const ScanXf& X = xf[flat_job<&ScanXf::blk0>(xf, nb, blockIdx.x)];
    const FrameHdr& hs = dp.frames[X.src];
    const FrameHdr& ht = dp.frames[X.tgt];
    const uint32_t pos = (blockIdx.x - X.blk0) * (uint32_t)THREADS + threadIdx.x;   // position in the source scan's tree order
    const bool act = pos < hs.P;
    const uint32_t P = ht.P, D = ht.depth;
    stage_nodes<THREADS>(dp, ht, s_nodes);
    __syncthreads();
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    uint32_t sidx = 0u;
    if (act) {
        const float4 sv = dp.pts4[hs.pt_base + pos];
        sidx = __float_as_uint(sv.w);
        icp_transform(X.T, (double)sv.x, (double)sv.y, (double)sv.z, q0, q1, q2);
    }
    IBA_LANE_NN_DECL;
    if (act && P > 0u) {
        actA = true; actC = false; ax = q0; ay = q1; az = q2;
        lane_nn_begin(IBA_LANE_NN_PASS);
        do { lane_nn_visit<1>(IBA_LANE_NN_PASS, s_nodes, dp.pts4 + ht.pt_base, dp.perm + ht.pt_base, P, D); } while (go >= 0);
    }
    const bool keep = act && bposA != kNone && bestA < X.gate2;
    double v[NS];
#pragma unroll
    for (int k = 0; k < NS; ++k) v[k] = 0.0;
    uint32_t gidx = kNone;
    if (keep) {
        const float4 pv = dp.pts4[ht.pt_base + bposA];
        gidx = __float_as_uint(pv.w);
        const double t[3] = {(double)pv.x, (double)pv.y, (double)pv.z};
        v[0] = 1.0;
        if (MODE == kScanP2P) {
            p2p_terms(v, bestA, q0, q1, q2, t[0], t[1], t[2], X.piv);
        } else if (MODE == kScanP2L) {
            v[1] = bestA;
            const PlaneRec& rec = dp.plane_cost[ht.pt_base + bposA];
            const double n[3] = {rec.nx, rec.ny, rec.nz};
            const bool has = rec.k >= min_pts && isfinite(n[0]) && isfinite(n[1]) && isfinite(n[2]);
            if (has) {
                const double r = ((q0 - t[0]) * n[0] + (q1 - t[1]) * n[1]) + (q2 - t[2]) * n[2];
                const double J[6] = {q1 * n[2] - q2 * n[1], q2 * n[0] - q0 * n[2], q0 * n[1] - q1 * n[0], n[0], n[1], n[2]};   // [q x n, n]
                v[2] = 1.0;
                int o = 3;
#pragma unroll
                for (int i = 0; i < 6; ++i)
#pragma unroll
                    for (int j = i; j < 6; ++j) v[o++] = J[i] * J[j];
#pragma unroll
                for (int i = 0; i < 6; ++i) v[24 + i] = J[i] * r;
                v[30] = r * r;
            }
        } else {
            v[1] = t[0]; v[2] = t[1]; v[3] = t[2];
            v[4] = t[0] * t[0]; v[5] = t[0] * t[1]; v[6] = t[0] * t[2];
            v[7] = t[1] * t[1]; v[8] = t[1] * t[2]; v[9] = t[2] * t[2];
        }
    }
    if (pair_idx && act) pair_idx[X.pair0 + sidx] = keep ? gidx : kNone;   // ORIGINAL order of the source scan
    const uint32_t chunk = (blockIdx.x - X.blk0) * (uint32_t)(THREADS / 64) + (threadIdx.x >> 6);
    wave_sum_store<NS>(v, chunk * 64u < hs.P, partials + ((size_t)X.part0 + (size_t)chunk) * NS);
}

template <int MODE>
__global__ __launch_bounds__(256) void iba_scan_sum_kernel(DevProblem dp, const double* __restrict__ partials, const ScanXf* __restrict__ xf, double* __restrict__ out) {
    constexpr int NS = ScanSums<MODE>::n;
    __shared__ double s_w[4][NS];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    const int nw = (int)((dp.frames[xf[b].src].P + 63u) / 64u);
    block_sum_partials<NS>(partials + (size_t)xf[b].part0 * NS, nw, s_w);
    __syncthreads();
    double* o = out + (size_t)b * kScanMom;
    if (t < NS) o[t] = wave_totals(s_w, t);
    else if (MODE == kScanP2P && t < kIcpMom) o[t] = xf[b].piv[t - kIcpSums];
    else if (t < kScanMom) o[t] = 0.0;
}

}  // namespace iba

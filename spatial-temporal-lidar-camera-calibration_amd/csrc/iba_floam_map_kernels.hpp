// Device side of iba_floam_map_step / iba_floam_map_register (include/iba_mi355x.h): the scan-to-map stage of F-LOAM for a BATCH OF PAIRS
// (edge / surf cloud of a scan -> edge / surf cloud of a map, all four resident frames of the handle).
//
// A pair is two JOBS, (pair, edge) and (pair, surf): a job's source cloud is searched against the job's map cloud. Both kernels run on the
// flat grid of iba_flat_pass.hpp (the search at the pass's block shape from blk_nn, the evaluation at 256 threads from blk_ev).
//
//  iba_floam_nn5_kernel<THREADS>   a lane owns one source point: widened, transformed in f64 (icp_transform), then an exact 5-NN search of
//      the map frame's implicit kd tree, its node table staged in LDS by the block. A frame of this library IS one kd tile (what
//      iba_icp_pass_kernel walks tile by tile are frames): the tile's box test (box_dist2) is against the bound the search starts from,
//      max_nn_dist2 — a query no closer than that to the map's box searches nothing. The walk is plain f64 and keeps NO path:
//      the plane distance of level L is re-read from the LDS node of the leaf's ancestor, the visited far sides are one bit per level. The
//      best list is five (d^2, original index, position) triples in named registers, kept ascending by (d^2, index) with four compare-and-
//      swap steps per insertion; the pruning bound is min(5th best, max_nn_dist2). A far child is entered iff its plane distance^2 is <= the
//      5th best and < max_nn_dist2: the plane distance is formed with the operations of the point distance, each monotone after rounding, so
//      it never exceeds the computed distance of a point behind the plane, and '<=' keeps an equally distant point of lower index reachable.
//      The lane then fits its own line (3x3 symmetric eigen problem, cyclic Jacobi on named scalars) or plane (5x3 Householder QR) in f64 and
//      writes ONE record; nn_idx only when asked. No scratch: nothing is indexed dynamically.
//  iba_floam_eval_kernel           a lane reads its source point, its record and the job's pose: r, J, the Huber weight and its 31 terms
//      (tried, kept, 21 of H, 6 of b, chi^2, sum r^2). A wave adds its lanes' terms by DPP (wave_sum_f64) and its last lane writes one partial.
//  iba_floam_sum_kernel            grid (pairs): the partials of the edge job, then of the surf job; the pair's IBA_FLOAM_NMOM moments are
//      composed from the two.
// No scratch, no atomics.
#pragma once
#include "iba_icp_kernels.hpp"

namespace iba {

constexpr int kFloamMom = 34;     // IBA_FLOAM_NMOM
constexpr int kFloamSums = 31;    // per job: tried, kept, H (21), b (6), chi^2, sum r^2

struct FloamRec {                 // = iba_floam_record
    int32_t kind;                 // 0 none, 1 edge, 2 surf
    int32_t tried;                // 1: the point passed the neighbour gate (rule 2)
    double v[7];                  // edge: a (3), b (3), 0; surf: n (3), d, 0, 0, 0
};

struct FloamJob {                 // one (pair, kind) of a launch (host -> device)
    double T[12];                 // rows 0-2 of the row-major 4x4
    int32_t src, map;             // local frames
    int32_t kind;                 // 1 edge, 2 surf
    int32_t enabled;              // the pair's maps are large enough (rule 2)
    uint32_t blk_nn, blk_ev;      // first block of the job in the flat grid of the search / the evaluation kernel
    uint32_t part0;               // first partial (64-position chunk) of the job
    uint32_t pad;
    uint64_t rec0;                // first record of the job (records and nn_idx are in the ORIGINAL order of the source cloud)
};

struct FloamFit { double max_nn_dist2, edge_eig_ratio, edge_half_len, plane_max_resid, huber_delta; };

// (d^2, index) ascending; a NaN distance is never less
#define IBA_NN5_LESS(da, ia, db, ib) ((da) < (db) || ((da) == (db) && (ia) < (ib)))
#define IBA_NN5_CSWAP(dl, il, pl, dh, ih, ph) \
    if (IBA_NN5_LESS(dh, ih, dl, il)) { const double td_ = dl; dl = dh; dh = td_; const uint32_t ti_ = il; il = ih; ih = ti_; const uint32_t tp_ = pl; pl = ph; ph = tp_; }

// one Jacobi rotation of the symmetric 3x3 (app, aqq, apq; the third index r) and of the eigenvector columns p, q
__device__ __forceinline__ void jacobi_rot(double& app, double& aqq, double& apq, double& arp, double& arq,
                                           double& v0p, double& v0q, double& v1p, double& v1q, double& v2p, double& v2q) {
    if (apq == 0.0) return;
    const double theta = (aqq - app) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    app = app - t * apq; aqq = aqq + t * apq; apq = 0.0;
    const double rp = c * arp - s * arq, rq = s * arp + c * arq; arp = rp; arq = rq;
    const double a0 = c * v0p - s * v0q, b0 = s * v0p + c * v0q; v0p = a0; v0q = b0;
    const double a1 = c * v1p - s * v1q, b1 = s * v1p + c * v1q; v1p = a1; v1q = b1;
    const double a2 = c * v2p - s * v2q, b2 = s * v2p + c * v2q; v2p = a2; v2q = b2;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void iba_floam_nn5_kernel(DevProblem dp, const float* __restrict__ frame_box, const FloamJob* __restrict__ jobs, int nj, FloamFit fit,
                                                                FloamRec* __restrict__ recs, uint32_t* __restrict__ nn_idx) {
    extern __shared__ __align__(16) unsigned char smem[];
    TreeNode* s_nodes = (TreeNode*)smem;
    const FloamJob& X = jobs[flat_job<&FloamJob::blk_nn>(jobs, nj, blockIdx.x)];
    const FrameHdr& hs = dp.frames[X.src];
    const FrameHdr& hm = dp.frames[X.map];
    const uint32_t pos = (blockIdx.x - X.blk_nn) * (uint32_t)THREADS + threadIdx.x;   // position in the source cloud's tree order
    const bool act = pos < hs.P;
    const uint32_t P = hm.P, D = hm.depth;
    stage_nodes<THREADS>(dp, hm, s_nodes);
    __syncthreads();
    if (!act) return;   // (no barrier and no wave operation below)
    const float4 sv = dp.pts4[hs.pt_base + pos];
    const uint32_t sidx = __float_as_uint(sv.w);
    double q0, q1, q2;
    icp_transform(X.T, (double)sv.x, (double)sv.y, (double)sv.z, q0, q1, q2);
    const float4* __restrict__ p4 = dp.pts4 + hm.pt_base;

    double d0 = INFINITY, d1 = INFINITY, d2 = INFINITY, d3 = INFINITY, d4 = INFINITY;
    uint32_t i0 = kNone, i1 = kNone, i2 = kNone, i3 = kNone, i4 = kNone, p0 = 0u, p1 = 0u, p2 = 0u, p3 = 0u, p4i = 0u;
    bool look = X.enabled != 0 && P >= 5u;
    if (look) look = box_dist2(frame_box + 8 * (size_t)X.map, q0, q1, q2) < fit.max_nn_dist2;   // the tile's box against the bound the search starts from
    if (look) {
        const uint32_t first_leaf = (1u << D) - 1u;
        uint32_t node = 0u, done = 0u;   // done bit L: the far child at level L of the current path needs no (further) visit
        int start = 0;
        for (;;) {
            for (int L = start; L < (int)D; ++L) {   // to the leaf on the near side
                const TreeNode n = s_nodes[node];
                const double qd = n.dim == 0u ? q0 : (n.dim == 1u ? q1 : q2);
                node = 2u * node + 1u + (qd - (double)n.split >= 0.0 ? 1u : 0u);
            }
            const uint32_t j = node - first_leaf;
            const uint32_t lo = (uint32_t)(((uint64_t)j * P) >> D), hi = (uint32_t)(((uint64_t)(j + 1) * P) >> D);
            for (uint32_t i = lo; i < hi; ++i) {
                const float4 pv = p4[i];
                const double dx = q0 - (double)pv.x, dy = q1 - (double)pv.y, dz = q2 - (double)pv.z;
                const double dd = (dx * dx + dy * dy) + dz * dz;
                const uint32_t id = __float_as_uint(pv.w);
                if (IBA_NN5_LESS(dd, id, d4, i4)) {
                    d4 = dd; i4 = id; p4i = i;
                    IBA_NN5_CSWAP(d3, i3, p3, d4, i4, p4i);
                    IBA_NN5_CSWAP(d2, i2, p2, d3, i3, p3);
                    IBA_NN5_CSWAP(d1, i1, p1, d2, i2, p2);
                    IBA_NN5_CSWAP(d0, i0, p0, d1, i1, p1);
                }
            }
            int go = -1;   // the deepest level whose far child is still within reach
            for (int L = (int)D - 1; L >= 0; --L) {
                if ((done >> L) & 1u) continue;
                done |= 1u << L;
                const TreeNode n = s_nodes[((node + 1u) >> (D - (uint32_t)L)) - 1u];
                const double qd = n.dim == 0u ? q0 : (n.dim == 1u ? q1 : q2);
                const double pd = qd - (double)n.split;
                const double pd2 = pd * pd;
                if (pd2 <= d4 && pd2 < fit.max_nn_dist2) { go = L; break; }
            }
            if (go < 0) break;
            const uint32_t anc = ((node + 1u) >> (D - (uint32_t)go)) - 1u;
            const uint32_t was = ((node + 1u) >> (D - (uint32_t)go - 1u)) & 1u;   // the child of anc the path went through
            node = 2u * anc + 1u + (was ^ 1u);
            done &= (2u << go) - 1u;   // the levels below start anew
            start = go + 1;
        }
    }
    const bool ok = look && i4 != kNone && d4 < fit.max_nn_dist2;
    int rkind = 0;   // the record in named registers (a local struct written by parts is kept in scratch)
    double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0, r4 = 0.0, r5 = 0.0;
    if (ok) {
        const float4 f0 = p4[p0], f1 = p4[p1], f2 = p4[p2], f3 = p4[p3], f4 = p4[p4i];
        const double x[5] = {(double)f0.x, (double)f1.x, (double)f2.x, (double)f3.x, (double)f4.x};
        const double y[5] = {(double)f0.y, (double)f1.y, (double)f2.y, (double)f3.y, (double)f4.y};
        const double z[5] = {(double)f0.z, (double)f1.z, (double)f2.z, (double)f3.z, (double)f4.z};
        if (X.kind == 1) {
            const double cx = ((((x[0] + x[1]) + x[2]) + x[3]) + x[4]) / 5.0, cy = ((((y[0] + y[1]) + y[2]) + y[3]) + y[4]) / 5.0, cz = ((((z[0] + z[1]) + z[2]) + z[3]) + z[4]) / 5.0;
            double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0;
#pragma unroll
            for (int k = 0; k < 5; ++k) {
                const double ex = x[k] - cx, ey = y[k] - cy, ez = z[k] - cz;
                a00 += ex * ex; a01 += ex * ey; a02 += ex * ez; a11 += ey * ey; a12 += ey * ez; a22 += ez * ez;
            }
            double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;   // v[row][column]
            for (int sweep = 0; sweep < 8; ++sweep) {   // cyclic Jacobi: (0,1), (0,2), (1,2); converged long before 8 sweeps
                jacobi_rot(a00, a11, a01, a02, a12, v00, v01, v10, v11, v20, v21);
                jacobi_rot(a00, a22, a02, a01, a12, v00, v02, v10, v12, v20, v22);
                jacobi_rot(a11, a22, a12, a01, a02, v01, v02, v11, v12, v21, v22);
            }
            // the largest eigenvalue, its column, and the middle one
            // (two selects with the values pinned between them: left to itself the compiler stores the nine entries to scratch and loads the column by index)
            const bool s1 = a11 > a00;
            double l2 = s1 ? a11 : a00, u0 = s1 ? v01 : v00, u1 = s1 ? v11 : v10, u2 = s1 ? v21 : v20;
            asm volatile("" : "+v"(l2), "+v"(u0), "+v"(u1), "+v"(u2));
            const bool s2 = a22 > l2;
            l2 = s2 ? a22 : l2; u0 = s2 ? v02 : u0; u1 = s2 ? v12 : u1; u2 = s2 ? v22 : u2;
            const double l1 = fmax(fmin(a00, a11), fmin(fmax(a00, a11), a22));   // the median of the diagonal: exact, no cancellation
            const double un = sqrt((u0 * u0 + u1 * u1) + u2 * u2);
            if (l2 > fit.edge_eig_ratio * l1 && un > 0.0) {
                u0 /= un; u1 /= un; u2 /= un;
                const double h = fit.edge_half_len;
                rkind = 1;
                r0 = cx + h * u0; r1 = cy + h * u1; r2 = cz + h * u2;
                r3 = cx - h * u0; r4 = cy - h * u1; r5 = cz - h * u2;
            }
        } else {
            // least squares A n0 = -1 by Householder QR of the 5x3 matrix of the neighbours (columns x, y, z)
            double A[4][5];   // columns x, y, z and the right-hand side
#pragma unroll
            for (int k = 0; k < 5; ++k) { A[0][k] = x[k]; A[1][k] = y[k]; A[2][k] = z[k]; A[3][k] = -1.0; }
            double diag[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                double s2 = 0.0;
#pragma unroll
                for (int k = c; k < 5; ++k) s2 += A[c][k] * A[c][k];
                const double nrm = sqrt(s2);
                const double alpha = A[c][c] >= 0.0 ? -nrm : nrm;
                double vv[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) vv[k] = k < c ? 0.0 : A[c][k];
                vv[c] -= alpha;
                double beta = 0.0;
#pragma unroll
                for (int k = c; k < 5; ++k) beta += vv[k] * vv[k];
                diag[c] = alpha;
#pragma unroll
                for (int cc = c + 1; cc < 4; ++cc) {   // the columns to the right, the right-hand side last
                    double dot = 0.0;
#pragma unroll
                    for (int k = c; k < 5; ++k) dot += vv[k] * A[cc][k];
                    const double f = 2.0 * dot / beta;
#pragma unroll
                    for (int k = c; k < 5; ++k) A[cc][k] -= f * vv[k];
                }
            }
            const double n2 = A[3][2] / diag[2];
            const double n1 = (A[3][1] - A[2][1] * n2) / diag[1];
            const double n0 = ((A[3][0] - A[1][0] * n1) - A[2][0] * n2) / diag[0];
            const double nn = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            const double d = 1.0 / nn, m0 = n0 / nn, m1 = n1 / nn, m2 = n2 / nn;
            bool fine = nn > 0.0 && isfinite(d) && isfinite(m0) && isfinite(m1) && isfinite(m2);
#pragma unroll
            for (int k = 0; k < 5; ++k) fine = fine && fabs(((m0 * x[k] + m1 * y[k]) + m2 * z[k]) + d) <= fit.plane_max_resid;
            if (fine) { rkind = 2; r0 = m0; r1 = m1; r2 = m2; r3 = d; }
        }
    }
    FloamRec* ro = recs + (X.rec0 + sidx);
    ro->kind = rkind; ro->tried = ok ? 1 : 0;
    ro->v[0] = r0; ro->v[1] = r1; ro->v[2] = r2; ro->v[3] = r3; ro->v[4] = r4; ro->v[5] = r5; ro->v[6] = 0.0;
    if (nn_idx) {
        uint32_t* o = nn_idx + 5u * (X.rec0 + sidx);
        o[0] = ok ? i0 : kNone; o[1] = ok ? i1 : kNone; o[2] = ok ? i2 : kNone; o[3] = ok ? i3 : kNone; o[4] = ok ? i4 : kNone;
    }
}

// r, the direction g of its gradient with respect to the transformed point (J = [lp x g, g]) of one record at lp; false: no factor
__device__ __forceinline__ bool floam_residual(const FloamRec& rec, double l0, double l1, double l2, double& r, double& g0, double& g1, double& g2) {
    if (rec.kind == 1) {
        const double ax = l0 - rec.v[0], ay = l1 - rec.v[1], az = l2 - rec.v[2], bx = l0 - rec.v[3], by = l1 - rec.v[4], bz = l2 - rec.v[5];
        const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;                       // nu = (lp - a) x (lp - b)
        const double ex = rec.v[0] - rec.v[3], ey = rec.v[1] - rec.v[4], ez = rec.v[2] - rec.v[5];                 // de = a - b
        const double den = sqrt((ex * ex + ey * ey) + ez * ez), nn = sqrt((nx * nx + ny * ny) + nz * nz);
        r = nn / den;
        if (nn > 0.0) {
            const double wx = nx / nn, wy = ny / nn, wz = nz / nn;
            g0 = (ey * wz - ez * wy) / den; g1 = (ez * wx - ex * wz) / den; g2 = (ex * wy - ey * wx) / den;        // (de x nu / |nu|) / |de|
        } else { g0 = 0.0; g1 = 0.0; g2 = 0.0; }
        return true;
    }
    if (rec.kind == 2) {
        r = ((rec.v[0] * l0 + rec.v[1] * l1) + rec.v[2] * l2) + rec.v[3];
        g0 = rec.v[0]; g1 = rec.v[1]; g2 = rec.v[2];
        return true;
    }
    return false;
}

template <int THREADS>
__global__ __launch_bounds__(THREADS) void iba_floam_eval_kernel(DevProblem dp, const FloamJob* __restrict__ jobs, int nj, double huber_delta, const FloamRec* __restrict__ recs,
                                                                 double* __restrict__ partials) {
    const FloamJob& X = jobs[flat_job<&FloamJob::blk_ev>(jobs, nj, blockIdx.x)];
    const FrameHdr& hs = dp.frames[X.src];
    const uint32_t pos = (blockIdx.x - X.blk_ev) * (uint32_t)THREADS + threadIdx.x;
    double v[kFloamSums];
#pragma unroll
    for (int k = 0; k < kFloamSums; ++k) v[k] = 0.0;
    if (pos < hs.P) {
        const float4 sv = dp.pts4[hs.pt_base + pos];
        const FloamRec rec = recs[X.rec0 + __float_as_uint(sv.w)];
        double l0, l1, l2;
        icp_transform(X.T, (double)sv.x, (double)sv.y, (double)sv.z, l0, l1, l2);
        double r = 0.0, g0 = 0.0, g1 = 0.0, g2 = 0.0;
        v[0] = (double)rec.tried;
        if (floam_residual(rec, l0, l1, l2, r, g0, g1, g2)) {
            const double J[6] = {l1 * g2 - l2 * g1, l2 * g0 - l0 * g2, l0 * g1 - l1 * g0, g0, g1, g2};   // [lp x g, g]
            const double ar = fabs(r);
            const bool in = ar <= huber_delta;
            const double w = in ? 1.0 : huber_delta / ar;
            v[1] = 1.0;
            int o = 2;
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                const double wj = w * J[i];
#pragma unroll
                for (int j = i; j < 6; ++j) v[o++] = wj * J[j];
                v[23 + i] = wj * r;
            }
            v[29] = in ? r * r : 2.0 * huber_delta * ar - huber_delta * huber_delta;
            v[30] = r * r;
        }
    }
    const uint32_t chunk = (blockIdx.x - X.blk_ev) * (uint32_t)(THREADS / 64) + (threadIdx.x >> 6);
    wave_sum_store<kFloamSums>(v, chunk * 64u < hs.P, partials + ((size_t)X.part0 + (size_t)chunk) * kFloamSums);
}

// jobs 2 b (edge) and 2 b + 1 (surf) are pair b of the launch
__global__ __launch_bounds__(256) void iba_floam_sum_kernel(DevProblem dp, const double* __restrict__ partials, const FloamJob* __restrict__ jobs, double* __restrict__ out) {
    __shared__ double s_w[2][4][kFloamSums];
    const int b = (int)blockIdx.x, t = (int)threadIdx.x;
    for (int side = 0; side < 2; ++side) {
        const FloamJob& X = jobs[2 * b + side];
        const int nw = (int)((dp.frames[X.src].P + 63u) / 64u);
        block_sum_partials<kFloamSums>(partials + (size_t)X.part0 * kFloamSums, nw, s_w[side]);
    }
    __syncthreads();
    if (t < kFloamMom) {
        const auto tot = [&](int side, int k) { return wave_totals(s_w[side], k); };
        double r;
        if (t < 4) r = tot(t >> 1, t & 1);               // edge tried, edge kept, surf tried, surf kept
        else if (t < 32) r = tot(0, t - 2) + tot(1, t - 2);   // H (21), b (6), chi^2: the edge job's sum + the surf job's
        else r = tot(t - 32, 30);                        // sum r^2 of the edges, of the surfs
        out[(size_t)b * kFloamMom + t] = r;
    }
}

}  // namespace iba

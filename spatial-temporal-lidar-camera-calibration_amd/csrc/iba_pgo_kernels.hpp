// Device side of the pose-graph optimiser (include/iba_mi355x.h, iba_pgo_*; the rules are numbered there). All arithmetic is f64 with
// -ffp-contract=off, no floating-point atomics, every sum in a fixed order; kernel boundaries are the only grid-wide synchronisation.
//   linearise   pgo_edge_kernel<true>: one lane per edge (rules 2-4: zeta, w, A = w Js^T L Js, g = w Js^T L zeta, c = w zeta^T L zeta);
//               pgo_node_kernel: one 64-lane block per node gathers D_i = sum A_e and b_i = sum -+ g_e over the node's incident edges in ascending edge
//               index (host-built CSR) and takes |vec6(pose_i)|^2, max |b_i|, max diag D_i; pgo_final_kernel sums / maxes the block partials
//               (a lane takes every 64th block in ascending order, the wave by DPP).
//   solve       pgo_run_forward_kernel: 16 lanes per interior run, 4 runs per one-wave block. Lane 0 factors D'_i = L D L^T in LDS (the 6x6 LDL^T of
//               iba_icp_math.hpp), lanes 0-5 solve one column each of G_i = D'^-1 C_i, lanes 6-11 of F_i = D'^-1 E_i (E_i the fill towards the run's
//               left separator), lane 12 y_i = D'^-1 b'_i; the same lanes form their column of the update of node i + 1 and of the Schur
//               contributions. pgo_sep_assemble_kernel sums every block of the separator system from a host-built list (diagonal, edges ascending,
//               runs ascending); pgo_chol_panel_kernel (one workgroup: the NB x NB diagonal block in LDS, then one thread per row below it) and
//               pgo_chol_update_kernel (32 x 32 tiles of the trailing lower triangle across the grid) are the blocked right-looking Cholesky;
//               pgo_sep_solve_kernel the two triangular solves with x in LDS; pgo_run_back_kernel one lane per run.
//   trial       pgo_update_kernel: one lane per node, trial pose = T(delta_i) pose_i and the partial sums of delta . (lambda delta + b), |delta|^2;
//               pgo_edge_kernel<false> the trial residual.
// The separator matrix is the lower triangle, column-major: entry (i, j), i >= j, at S[j * n + i].
// The kernels here have external linkage: this header goes into ONE unit (iba_pgo.hip). Other units reach them through iba_pgo_solve.hpp, and take the
// constants and the rigid algebra from iba_pgo_math.hpp, the wave reductions and the block tail behind them from iba_wave_sum.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_icp_math.hpp"
#include "iba_pgo_math.hpp"

namespace iba { namespace pgo {

struct EdgeDev {
    int E;
    const int32_t* src; const int32_t* tgt;
    const double* Xinv;        // E x 12
    const double* info;        // E x 36, mirrored
    const uint8_t* flags;      // bit 0 uncertain, bit 1 dropped
};

// FULL: zeta, w (recomputed with recompute_w), A, g, c. Otherwise c at `poses` with the weights as they are. Block partial: sum of c.
template <bool FULL>
__global__ __launch_bounds__(kThreads) void pgo_edge_kernel(EdgeDev d, const double* __restrict__ poses, double mu, int recompute_w, double* __restrict__ weight,
                                                            double* __restrict__ zeta_out, double* __restrict__ A_out, double* __restrict__ g_out, double* __restrict__ partial) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    double c = 0.0;
    if (e < d.E) {
        const int s = d.src[e], t = d.tgt[e];
        const uint8_t fl = d.flags[e];
        double zeta[6], Js[36], Lz[6];
        edge_zeta_js(d.Xinv + 12 * (size_t)e, poses + 16 * (size_t)t, poses + 16 * (size_t)s, zeta, FULL ? Js : nullptr);
        const double* L = d.info + 36 * (size_t)e;
        const double q = quad6(L, zeta, Lz);
        double w = weight[e];
        const bool dropped = (fl & 2) != 0;   // a dropped edge keeps the weight it was dropped with
        if (FULL && recompute_w && !dropped) { w = (fl & 1) ? line_weight(mu, q) : 1.0; weight[e] = w; }
        c = dropped ? 0.0 : w * q;
        if (FULL) {
            const double wa = dropped ? 0.0 : w;
#pragma unroll
            for (int i = 0; i < 6; ++i) zeta_out[6 * (size_t)e + i] = zeta[i];
            double LJ[36];
#pragma unroll
            for (int i = 0; i < 6; ++i)
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    double a = L[i * 6] * Js[k];
#pragma unroll
                    for (int j = 1; j < 6; ++j) a += L[i * 6 + j] * Js[j * 6 + k];
                    LJ[i * 6 + k] = a;
                }
            double* A = A_out + 36 * (size_t)e;
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int l = k; l < 6; ++l) {
                    double a = Js[k] * LJ[l];
#pragma unroll
                    for (int i = 1; i < 6; ++i) a += Js[i * 6 + k] * LJ[i * 6 + l];
                    a *= wa;
                    A[k * 6 + l] = a; A[l * 6 + k] = a;
                }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double a = Js[k] * Lz[0];
#pragma unroll
                for (int i = 1; i < 6; ++i) a += Js[i * 6 + k] * Lz[i];
                g_out[6 * (size_t)e + k] = wa * a;
            }
        }
    }
    const double tsum[1] = {wave_sum_f64(c)};
    block_sum_store<1, kThreads>(tsum, partial);
}

// One 64-lane block per node. Lanes 0-35: D_i entry, lanes 36-41: b_i entry, lane 42: |vec6(pose_i)|^2. partial[node] = {|x_i|^2, max |b_i|, max diag D_i}
__global__ __launch_bounds__(64) void pgo_node_kernel(int N, const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc_edge /* edge * 2 + (node is the target) */,
                                                      const double* __restrict__ A, const double* __restrict__ g, const double* __restrict__ poses,
                                                      double* __restrict__ D, double* __restrict__ b, double* __restrict__ partial) {
    const int i = blockIdx.x, l = threadIdx.x;
    const int lo = inc_off[i], hi = inc_off[i + 1];
    double v = 0.0, mb = 0.0, md = 0.0, xx = 0.0;
    if (l < 36) {
        for (int k = lo; k < hi; ++k) v += A[36 * (size_t)(inc_edge[k] >> 1) + l];
        D[36 * (size_t)i + l] = v;
        if (l % 7 == 0) md = fabs(v);
    } else if (l < 42) {
        for (int k = lo; k < hi; ++k) { const int ie = inc_edge[k]; const double ge = g[6 * (size_t)(ie >> 1) + (l - 36)]; v += (ie & 1) ? ge : -ge; }
        b[6 * (size_t)i + (l - 36)] = v;
        mb = fabs(v);
    } else if (l == 42) {
        double x[6];
        vec6_of(poses + 16 * (size_t)i, x);
        xx = x[0] * x[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) xx += x[k] * x[k];
    }
    mb = wave_max_f64(mb); md = wave_max_f64(md); xx = wave_sum_f64(xx);
    if (l == 63) { partial[3 * (size_t)i] = xx; partial[3 * (size_t)i + 1] = mb; partial[3 * (size_t)i + 2] = md; }
}

// out[k] = sum (k < nsum) or max (the next nmax) over the blocks of partial[block * (nsum + nmax) + k], one wave
__global__ __launch_bounds__(64) void pgo_final_kernel(const double* __restrict__ partial, int nblocks, int nsum, int nmax, double* __restrict__ out) {
    const int l = threadIdx.x, stride = nsum + nmax;
    for (int k = 0; k < stride; ++k) {
        double v = 0.0;
        if (k < nsum) { for (int blk = l; blk < nblocks; blk += 64) v += partial[(size_t)blk * stride + k]; v = wave_sum_f64(v); }
        else { for (int blk = l; blk < nblocks; blk += 64) v = fmax(v, partial[(size_t)blk * stride + k]); v = wave_max_f64(v); }
        if (l == 63) out[k] = v;
    }
}

struct RunDev {
    int n_runs;
    const int32_t* first; const int32_t* last;   // interior nodes first .. last; the left separator is first - 1
    const int32_t* chain;                        // [N]: the chain edge between i and i + 1, -1 without one
    int N;
};

// Forward block LDL^T along the runs (see the head of the file). G, F: N x 36, y: N x 6 (interior nodes only). run_S: n_runs x 3 x 36 (what the
// run ADDS to S_LL, S_RR and the block (R, L)), run_b: n_runs x 2 x 6 (to b_L, b_R).
__global__ __launch_bounds__(64) void pgo_run_forward_kernel(RunDev r, const double* __restrict__ D, const double* __restrict__ b, const double* __restrict__ A, double lambda,
                                                             double* __restrict__ G, double* __restrict__ F, double* __restrict__ y, double* __restrict__ run_S,
                                                             double* __restrict__ run_b, double* __restrict__ scal) {
    __shared__ double s_Dp[4][36], s_Ep[4][36], s_Cn[4][36], s_L[4][36], s_d[4][6], s_bp[4][6];
    const int sub = threadIdx.x >> 4, l = threadIdx.x & 15;
    const int run = blockIdx.x * 4 + sub;
    const bool live = run < r.n_runs;
    const int a = live ? r.first[run] : 0, z = live ? r.last[run] : -1;
    double* Dp = s_Dp[sub]; double* Ep = s_Ep[sub]; double* Cn = s_Cn[sub]; double* Lf = s_L[sub]; double* df = s_d[sub]; double* bp = s_bp[sub];
    int steps = z - a + 1, max_steps = steps;   // the four runs of a wave step together: every lane meets every barrier
    max_steps = max(max_steps, __shfl_xor(max_steps, 16)); max_steps = max(max_steps, __shfl_xor(max_steps, 32));
    if (live) {
        const int ce = r.chain[a - 1];
        for (int k = l; k < 36; k += 16) { Dp[k] = D[36 * (size_t)a + k] + ((k % 7 == 0) ? lambda : 0.0); Ep[k] = ce >= 0 ? -A[36 * (size_t)ce + k] : 0.0; }
        if (l < 6) bp[l] = b[6 * (size_t)a + l];
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // lanes 6-11: their column of the S_LL contribution; lane 12: the b_L contribution
    for (int st = 0; st < max_steps; ++st) {
        const bool on = live && st < steps;
        const int i = a + st;
        const bool at_end = i == z;
        if (on) {
            const int ce = (i + 1 < r.N) ? r.chain[i] : -1;
            for (int k = l; k < 36; k += 16) Cn[k] = ce >= 0 ? -A[36 * (size_t)ce + k] : 0.0;
        }
        __syncthreads();
        if (on && l == 0 && !icp::ldlt6_factor(Dp, Lf, df)) scal[7] = 1.0;
        __syncthreads();
        double x[6], u[6], nd[6];
        const int j = l < 6 ? l : l - 6;
        if (on && l < 13) {
            double rhs[6];
#pragma unroll
            for (int m = 0; m < 6; ++m) rhs[m] = l < 6 ? Cn[m * 6 + j] : (l < 12 ? Ep[m * 6 + j] : bp[m]);
            icp::ldlt6_apply(Lf, df, rhs, x);
            double* out = l < 6 ? G + 36 * (size_t)i : (l < 12 ? F + 36 * (size_t)i : y + 6 * (size_t)i);
#pragma unroll
            for (int m = 0; m < 6; ++m) { if (l < 12) out[m * 6 + j] = x[m]; else out[m] = x[m]; }
            // u = Cn^T x: this lane's column of what node i + 1 (or the right separator) loses; lanes 6-12 also Ep^T x towards the left separator
#pragma unroll
            for (int rr = 0; rr < 6; ++rr) {
                double s = Cn[rr] * x[0];
#pragma unroll
                for (int m = 1; m < 6; ++m) s += Cn[m * 6 + rr] * x[m];
                u[rr] = s;
                if (l >= 6) {
                    double t = Ep[rr] * x[0];
#pragma unroll
                    for (int m = 1; m < 6; ++m) t += Ep[m * 6 + rr] * x[m];
                    acc[rr] -= t;
                }
            }
            if (!at_end) {
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) {
                    if (l < 6) nd[rr] = (D[36 * (size_t)(i + 1) + rr * 6 + j] + (rr == j ? lambda : 0.0)) - u[rr];
                    else if (l < 12) nd[rr] = -u[rr];
                    else nd[rr] = b[6 * (size_t)(i + 1) + rr] - u[rr];
                }
            }
        }
        __syncthreads();
        if (on && l < 13) {
            if (!at_end) {
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) { if (l < 6) Dp[rr * 6 + j] = nd[rr]; else if (l < 12) Ep[rr * 6 + j] = nd[rr]; else bp[rr] = nd[rr]; }
            } else {
                double* S = run_S + 108 * (size_t)run; double* rb = run_b + 12 * (size_t)run;
#pragma unroll
                for (int rr = 0; rr < 6; ++rr) {
                    if (l < 6) S[36 + rr * 6 + j] = -u[rr];            // S_RR
                    else if (l < 12) { S[72 + rr * 6 + j] = -u[rr]; S[rr * 6 + j] = acc[rr]; }   // block (R, L) and S_LL
                    else { rb[6 + rr] = -u[rr]; rb[rr] = acc[rr]; }
                }
            }
        }
    }
}

// The separator system from the host-built list: block q covers (brow[q], bcol[q]), brow >= bcol, and sums items [off[q], off[q + 1]): kind 0 the
// diagonal block of node idx (+ lambda I; rhs b_node), 1 edge idx (-A), 2 / 3 / 4 run idx's S_LL / S_RR / (R, L) block (rhs of 2 / 3: its b_L / b_R).
__global__ __launch_bounds__(64) void pgo_sep_assemble_kernel(const int32_t* __restrict__ brow, const int32_t* __restrict__ bcol, const int32_t* __restrict__ off,
                                                              const int32_t* __restrict__ kind, const int32_t* __restrict__ idx, const double* __restrict__ D,
                                                              const double* __restrict__ b, const double* __restrict__ A, const double* __restrict__ run_S,
                                                              const double* __restrict__ run_b, double lambda, int n, double* __restrict__ S, double* __restrict__ rhs) {
    const int q = blockIdx.x, l = threadIdx.x;
    const int bi = brow[q], bj = bcol[q];
    if (l < 36) {
        double v = 0.0;
        for (int k = off[q]; k < off[q + 1]; ++k) {
            const int kd = kind[k], ix = idx[k];
            if (kd == 0) v += D[36 * (size_t)ix + l] + ((l % 7 == 0) ? lambda : 0.0);
            else if (kd == 1) v -= A[36 * (size_t)ix + l];
            else v += run_S[108 * (size_t)ix + 36 * (kd - 2) + l];
        }
        const int rr = l / 6, cc = l % 6;
        if (bi != bj || rr >= cc) S[(size_t)(6 * bj + cc) * n + 6 * bi + rr] = v;
    } else if (l < 42 && bi == bj) {
        double v = 0.0;
        for (int k = off[q]; k < off[q + 1]; ++k) {
            const int kd = kind[k], ix = idx[k];
            if (kd == 0) v += b[6 * (size_t)ix + (l - 36)];
            else if (kd == 2 || kd == 3) v += run_b[12 * (size_t)ix + 6 * (kd - 2) + (l - 36)];
        }
        rhs[6 * bi + (l - 36)] = v;
    }
}

// Panel [j0, j0 + w) of the right-looking Cholesky, one workgroup: the diagonal block in LDS, then L21 = A21 L11^-T, one thread per row
__global__ __launch_bounds__(kThreads) void pgo_chol_panel_kernel(double* __restrict__ S, int n, int j0, int w, double* __restrict__ scal) {
    __shared__ double s_a[kNB][kNB + 1];
    const int t = threadIdx.x;
    for (int k = t; k < w * w; k += kThreads) { const int i = k % w, j = k / w; if (i >= j) s_a[i][j] = S[(size_t)(j0 + j) * n + j0 + i]; }
    __syncthreads();
    for (int k = 0; k < w; ++k) {
        if (t == 0) {
            const double p = s_a[k][k];
            if (!(p > 0.0) || !(p <= 1.7976931348623157e308)) scal[7] = 1.0;
            s_a[k][k] = sqrt(p);
        }
        __syncthreads();
        if (t > k && t < w) s_a[t][k] /= s_a[k][k];
        __syncthreads();
        for (int m = t; m < w * w; m += kThreads) { const int i = m % w, j = m / w; if (j > k && i >= j) s_a[i][j] -= s_a[i][k] * s_a[j][k]; }
        __syncthreads();
    }
    for (int k = t; k < w * w; k += kThreads) { const int i = k % w, j = k / w; if (i >= j) S[(size_t)(j0 + j) * n + j0 + i] = s_a[i][j]; }
    for (int i = j0 + w + t; i < n; i += kThreads) {
        // the row is re-read from memory (this thread's own stores, coalesced over i): 48 values in registers spill
        for (int c = 0; c < w; ++c) {
            double v = S[(size_t)(j0 + c) * n + i];
            for (int k = 0; k < c; ++k) v -= S[(size_t)(j0 + k) * n + i] * s_a[c][k];
            S[(size_t)(j0 + c) * n + i] = v / s_a[c][c];
        }
    }
}

// A22 -= L21 L21^T on the lower triangle behind the panel: block (ti, tj), ti >= tj, of 32 x 32 tiles; a thread owns 2 x 2 entries
__global__ __launch_bounds__(kThreads) void pgo_chol_update_kernel(double* __restrict__ S, int n, int j0, int w) {
    if (blockIdx.y > blockIdx.x) return;
    __shared__ double s_i[kNB][kTile], s_j[kNB][kTile];
    const int j1 = j0 + w, t = threadIdx.x;
    const int i0 = j1 + blockIdx.x * kTile, c0 = j1 + blockIdx.y * kTile;
    for (int m = t; m < w * kTile; m += kThreads) {
        const int k = m / kTile, o = m % kTile;
        s_i[k][o] = (i0 + o < n) ? S[(size_t)(j0 + k) * n + i0 + o] : 0.0;
        s_j[k][o] = (c0 + o < n) ? S[(size_t)(j0 + k) * n + c0 + o] : 0.0;
    }
    __syncthreads();
    const int ii = t & 15, jj = t >> 4;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    for (int k = 0; k < w; ++k) {
        const double x0 = s_i[k][ii], x1 = s_i[k][ii + 16], y0 = s_j[k][jj], y1 = s_j[k][jj + 16];
        a00 += x0 * y0; a01 += x0 * y1; a10 += x1 * y0; a11 += x1 * y1;
    }
    const int r0 = i0 + ii, r1 = r0 + 16, q0 = c0 + jj, q1 = q0 + 16;
    if (r0 < n && q0 <= r0) S[(size_t)q0 * n + r0] -= a00;
    if (r0 < n && q1 <= r0) S[(size_t)q1 * n + r0] -= a01;
    if (r1 < n && q0 <= r1) S[(size_t)q0 * n + r1] -= a10;
    if (r1 < n && q1 <= r1) S[(size_t)q1 * n + r1] -= a11;
}

// L y = rhs, L^T x = y with the vector in LDS, one workgroup
__global__ __launch_bounds__(kThreads) void pgo_sep_solve_kernel(const double* __restrict__ S, int n, const double* __restrict__ rhs, double* __restrict__ x_out) {
    __shared__ double s_x[kMaxSepDim];
    __shared__ double s_w[kThreads / 64];
    const int t = threadIdx.x;
    for (int i = t; i < n; i += kThreads) s_x[i] = rhs[i];
    __syncthreads();
    for (int j = 0; j < n; ++j) {
        if (t == 0) s_x[j] /= S[(size_t)j * n + j];
        __syncthreads();
        const double xj = s_x[j];
        for (int i = j + 1 + t; i < n; i += kThreads) s_x[i] -= S[(size_t)j * n + i] * xj;
        __syncthreads();
    }
    for (int j = n - 1; j >= 0; --j) {
        double v = 0.0;
        for (int i = j + 1 + t; i < n; i += kThreads) v += S[(size_t)j * n + i] * s_x[i];
        v = wave_sum_f64(v);
        if ((t & 63) == 63) s_w[t >> 6] = v;
        __syncthreads();
        if (t == 0) { double s = s_w[0]; for (int k = 1; k < kThreads / 64; ++k) s += s_w[k]; s_x[j] = (s_x[j] - s) / S[(size_t)j * n + j]; }
        __syncthreads();
    }
    for (int i = t; i < n; i += kThreads) x_out[i] = s_x[i];
}

// delta of the separators, then back substitution along the runs: x_i = y_i - G_i x_(i+1) - F_i x_L. One lane per separator / per run.
__global__ __launch_bounds__(64) void pgo_run_back_kernel(RunDev r, int n_sep, const int32_t* __restrict__ sep_node, const int32_t* __restrict__ sep_of_node,
                                                          const double* __restrict__ xs, const double* __restrict__ G, const double* __restrict__ F,
                                                          const double* __restrict__ y, double* __restrict__ delta) {
    const int id = blockIdx.x * 64 + threadIdx.x;
    if (id < n_sep) {
#pragma unroll
        for (int k = 0; k < 6; ++k) delta[6 * (size_t)sep_node[id] + k] = xs[6 * (size_t)id + k];
    }
    if (id >= r.n_runs) return;
    const int a = r.first[id], z = r.last[id];
    double xl[6], xn[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) { xl[k] = xs[6 * (size_t)sep_of_node[a - 1] + k]; xn[k] = (z + 1 < r.N) ? xs[6 * (size_t)sep_of_node[z + 1] + k] : 0.0; }
    for (int i = z; i >= a; --i) {
        double xi[6];
#pragma unroll
        for (int rr = 0; rr < 6; ++rr) {
            double s = y[6 * (size_t)i + rr];
#pragma unroll
            for (int m = 0; m < 6; ++m) s -= G[36 * (size_t)i + rr * 6 + m] * xn[m];
#pragma unroll
            for (int m = 0; m < 6; ++m) s -= F[36 * (size_t)i + rr * 6 + m] * xl[m];
            xi[rr] = s;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) { xn[k] = xi[k]; delta[6 * (size_t)i + k] = xi[k]; }
    }
}

// trial pose_i = T(delta_i) pose_i; partial[block] = {sum delta . (lambda delta + b), sum |delta|^2}
__global__ __launch_bounds__(kThreads) void pgo_update_kernel(int N, const double* __restrict__ poses, const double* __restrict__ delta, const double* __restrict__ b, double lambda,
                                                              double* __restrict__ trial, double* __restrict__ partial) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    double dot = 0.0, dd = 0.0;
    if (i < N) {
        double dl[6], T[16], P[12];
#pragma unroll
        for (int k = 0; k < 6; ++k) dl[k] = delta[6 * (size_t)i + k];
        icp::vec6_to_mat4(dl, T);
        mul12(T, poses + 16 * (size_t)i, P);
#pragma unroll
        for (int k = 0; k < 12; ++k) trial[16 * (size_t)i + k] = P[k];
        trial[16 * (size_t)i + 12] = 0.0; trial[16 * (size_t)i + 13] = 0.0; trial[16 * (size_t)i + 14] = 0.0; trial[16 * (size_t)i + 15] = 1.0;
#pragma unroll
        for (int k = 0; k < 6; ++k) { dot += dl[k] * (lambda * dl[k] + b[6 * (size_t)i + k]); dd += dl[k] * dl[k]; }
    }
    const double tsum[2] = {wave_sum_f64(dot), wave_sum_f64(dd)};
    block_sum_store<2, kThreads>(tsum, partial);
}

// pose_i = C pose_i (the reference-node compensation of rule 6), C a rigid 3x4
struct Rigid12 { double m[12]; };
__global__ __launch_bounds__(kThreads) void pgo_left_mul_kernel(int N, Rigid12 C, double* __restrict__ poses) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= N) return;
    double P[12], O[12];
#pragma unroll
    for (int k = 0; k < 12; ++k) P[k] = poses[16 * (size_t)i + k];
    mul12(C.m, P, O);
#pragma unroll
    for (int k = 0; k < 12; ++k) poses[16 * (size_t)i + k] = O[k];
}

} }  // namespace iba::pgo

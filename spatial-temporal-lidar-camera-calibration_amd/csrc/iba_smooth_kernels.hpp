// Device side of the robust pose-graph smoother (include/iba_mi355x.h, iba_smooth_*; rules S1-S5 there). All arithmetic is f64 with
// -ffp-contract=off, no floating-point atomics, every sum in a fixed order; kernel boundaries are the only grid-wide synchronisation.
//   linearise   smooth_factor_kernel<true>: one lane per factor (S1-S3: r = Log(Z^-1 [P_i^-1] P_j), J = Jr^-1(r) Ad(P_j^-1), w, A = w J^T S^-1 J,
//               g = w J^T S^-1 r, the factor's term of F); smooth_node_kernel: one 64-lane block per node gathers D and b over the node's factors in
//               ascending factor index, the prior's among them, and takes |vec6(pose)|^2, max |b|, and the largest diagonal entry of the
//               between-factor part of D. iba_pgo's final kernel (pgo::final_launch) sums / maxes the block partials.
//   solve       the arrowhead chain of iba_pgo (iba_pgo_solve.hpp): nothing of it is restated here.
//   trial       smooth_update_kernel: one lane per node, trial pose = Exp(delta_i) P_i and the partial sums of delta . (lambda delta + b), |delta|^2;
//               smooth_factor_kernel<false>: F at the trial poses.
// The math of S1 / S2 is host-callable (IBA_ICP_HD): tests/smooth_ref.py restates it expression by expression.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_pgo_math.hpp"

namespace iba { namespace smooth {

using pgo::kThreads;
using pgo::mul12;
using pgo::inv12;

constexpr double kSeriesTh2 = 1e-2;     // theta^2 below which every coefficient is its series in theta^2
constexpr double kSeriesU2 = 2.5e-3;    // (|v| / w)^2 of the quaternion below which atan(u) / u is its series

// a = sin t / t, b = (1 - cos t) / t^2, c = (t - sin t) / t^3, e = (1 - (t / 2) cot(t / 2)) / t^2, c2 = (t^2 / 2 + cos t - 1) / t^4,
// k4 = (c2 + 3 (c - 1/6) / t^2) / 2
struct Coef { double a, b, c, e, c2, k4; };

IBA_ICP_HD inline Coef coeffs(double x) {
    Coef k;
    if (x < kSeriesTh2) {
        k.a = ((((-1.0 / 39916800.0 * x + 1.0 / 362880.0) * x - 1.0 / 5040.0) * x + 1.0 / 120.0) * x - 1.0 / 6.0) * x + 1.0;
        k.b = ((((-1.0 / 479001600.0 * x + 1.0 / 3628800.0) * x - 1.0 / 40320.0) * x + 1.0 / 720.0) * x - 1.0 / 24.0) * x + 1.0 / 2.0;
        k.c = ((((-1.0 / 6227020800.0 * x + 1.0 / 39916800.0) * x - 1.0 / 362880.0) * x + 1.0 / 5040.0) * x - 1.0 / 120.0) * x + 1.0 / 6.0;
        k.e = ((((691.0 / 1307674368000.0 * x + 1.0 / 47900160.0) * x + 1.0 / 1209600.0) * x + 1.0 / 30240.0) * x + 1.0 / 720.0) * x + 1.0 / 12.0;
        k.c2 = (((1.0 / 479001600.0 * x - 1.0 / 3628800.0) * x + 1.0 / 40320.0) * x - 1.0 / 720.0) * x + 1.0 / 24.0;
        k.k4 = (((1.0 / 1245404160.0 * x - 1.0 / 9979200.0) * x + 1.0 / 120960.0) * x - 1.0 / 2520.0) * x + 1.0 / 120.0;
    } else {
        const double t = sqrt(x), sh = sin(t * 0.5), ch = cos(t * 0.5), s = 2.0 * sh * ch;
        k.a = s / t;
        k.b = 2.0 * sh * sh / x;
        k.c = (t - s) / (x * t);
        k.e = (1.0 - (t * 0.5) * ch / sh) / x;
        k.c2 = (0.5 - k.b) / x;
        k.k4 = 0.5 * (k.c2 + 3.0 * (k.c - 1.0 / 6.0) / x);
    }
    return k;
}

IBA_ICP_HD inline void hat3(const double* v, double* W) {
    W[0] = 0.0; W[1] = -v[2]; W[2] = v[1];
    W[3] = v[2]; W[4] = 0.0; W[5] = -v[0];
    W[6] = -v[1]; W[7] = v[0]; W[8] = 0.0;
}
IBA_ICP_HD inline void mm3(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[r * 3 + c] = (A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c]) + A[r * 3 + 2] * B[6 + c];
}
IBA_ICP_HD inline void mv3(const double* A, const double* v, double* o) {
    for (int r = 0; r < 3; ++r) o[r] = (A[r * 3] * v[0] + A[r * 3 + 1] * v[1]) + A[r * 3 + 2] * v[2];
}
IBA_ICP_HD inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// S1: Exp([omega, upsilon]) as a rigid 3x4 (rows of 4)
IBA_ICP_HD inline void exp_se3(const double* xi, double* T) {
    const Coef k = coeffs(dot3(xi, xi));
    double W[9], W2[9], Wu[3], W2u[3];
    hat3(xi, W);
    mm3(W, W, W2);
    mv3(W, xi + 3, Wu);
    mv3(W2, xi + 3, W2u);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) T[r * 4 + c] = ((r == c ? 1.0 : 0.0) + k.a * W[r * 3 + c]) + k.b * W2[r * 3 + c];
        T[r * 4 + 3] = (xi[3 + r] + k.b * Wu[r]) + k.c * W2u[r];
    }
}

// the rotation of a rigid 3x4 -> omega, through the quaternion (largest component first); theta = 2 atan2(|v|, w) in [0, pi]
IBA_ICP_HD inline void log_so3(const double* M, double* om) {
    const double R00 = M[0], R01 = M[1], R02 = M[2], R10 = M[4], R11 = M[5], R12 = M[6], R20 = M[8], R21 = M[9], R22 = M[10];
    const double tr = (R00 + R11) + R22;
    double w, v[3];
    if (tr > 0.0) { const double S = sqrt(tr + 1.0) * 2.0; w = S * 0.25; v[0] = (R21 - R12) / S; v[1] = (R02 - R20) / S; v[2] = (R10 - R01) / S; }
    else if (R00 > R11 && R00 > R22) { const double S = sqrt(((1.0 + R00) - R11) - R22) * 2.0; w = (R21 - R12) / S; v[0] = S * 0.25; v[1] = (R01 + R10) / S; v[2] = (R02 + R20) / S; }
    else if (R11 > R22) { const double S = sqrt(((1.0 + R11) - R00) - R22) * 2.0; w = (R02 - R20) / S; v[0] = (R01 + R10) / S; v[1] = S * 0.25; v[2] = (R12 + R21) / S; }
    else { const double S = sqrt(((1.0 + R22) - R00) - R11) * 2.0; w = (R10 - R01) / S; v[0] = (R02 + R20) / S; v[1] = (R12 + R21) / S; v[2] = S * 0.25; }
    if (w < 0.0) { w = -w; v[0] = -v[0]; v[1] = -v[1]; v[2] = -v[2]; }
    const double s2 = dot3(v, v), u2 = s2 / (w * w);
    double k;
    if (u2 < kSeriesU2) k = (2.0 / w) * (((((-1.0 / 11.0 * u2 + 1.0 / 9.0) * u2 - 1.0 / 7.0) * u2 + 1.0 / 5.0) * u2 - 1.0 / 3.0) * u2 + 1.0);
    else { const double s = sqrt(s2); k = 2.0 * atan2(s, w) / s; }
    om[0] = k * v[0]; om[1] = k * v[1]; om[2] = k * v[2];
}

// S1: Log of a rigid 3x4 -> r = [omega, V(omega)^-1 t], V^-1 = I - W / 2 + e W^2
IBA_ICP_HD inline void log_se3(const double* M, double* r) {
    log_so3(M, r);
    const Coef k = coeffs(dot3(r, r));
    double W[9], Wt[3], WWt[3];
    const double t[3] = {M[3], M[7], M[11]};
    hat3(r, W);
    mv3(W, t, Wt);
    mv3(W, Wt, WWt);
    for (int a = 0; a < 3; ++a) r[3 + a] = (t[a] - 0.5 * Wt[a]) + k.e * WWt[a];
}

// S2: J = Jr^-1(r) Ad(P_j^-1), row-major 6x6. Jr^-1 = [[Ji, 0], [-Ji Q Ji, Ji]], Ji = I + W / 2 + e W^2,
// Q = -U / 2 + c (W U + U W + d W) - c2 (W W U + U W W + 3 d W) - 2 k4 d W W with W = [omega]x, U = [upsilon]x, d = omega . upsilon
IBA_ICP_HD inline void factor_jacobian(const double* r, const double* Pj, double* J) {
    const Coef k = coeffs(dot3(r, r));
    double W[9], U[9], W2[9], WU[9], WWU[9], Ji[9], Q[9], T1[9], B[9];
    hat3(r, W); hat3(r + 3, U);
    const double d = dot3(r, r + 3);
    mm3(W, W, W2);
    mm3(W, U, WU);
    mm3(W, WU, WWU);
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
            const int ac = a * 3 + c, ca = c * 3 + a;
            Ji[ac] = ((a == c ? 1.0 : 0.0) + 0.5 * W[ac]) + k.e * W2[ac];
            // U W = (W U)^T, U W W = -(W W U)^T
            Q[ac] = ((-0.5 * U[ac] + k.c * ((WU[ac] + WU[ca]) + d * W[ac])) - k.c2 * ((WWU[ac] + -WWU[ca]) + 3.0 * d * W[ac])) - (2.0 * k.k4) * (d * W2[ac]);
        }
    mm3(Ji, Q, T1);
    mm3(T1, Ji, B);
    double Jr[36], Ad[36], Pi[12], Rt[9], X[9], H[9];
    inv12(Pj, Pi);
    for (int a = 0; a < 3; ++a) for (int c = 0; c < 3; ++c) Rt[a * 3 + c] = Pi[a * 4 + c];
    const double tp[3] = {Pi[3], Pi[7], Pi[11]};
    hat3(tp, H);
    mm3(H, Rt, X);
    for (int a = 0; a < 3; ++a)
        for (int c = 0; c < 3; ++c) {
            Jr[a * 6 + c] = Ji[a * 3 + c]; Jr[a * 6 + 3 + c] = 0.0; Jr[(3 + a) * 6 + c] = -B[a * 3 + c]; Jr[(3 + a) * 6 + 3 + c] = Ji[a * 3 + c];
            Ad[a * 6 + c] = Rt[a * 3 + c]; Ad[a * 6 + 3 + c] = 0.0; Ad[(3 + a) * 6 + c] = X[a * 3 + c]; Ad[(3 + a) * 6 + 3 + c] = Rt[a * 3 + c];
        }
    for (int a = 0; a < 6; ++a)
        for (int c = 0; c < 6; ++c) {
            double v = Jr[a * 6] * Ad[c];
            for (int m = 1; m < 6; ++m) v += Jr[a * 6 + m] * Ad[m * 6 + c];
            J[a * 6 + c] = v;
        }
}

// r of a factor: Log(Z^-1 P_j) for a prior (Pi == nullptr), Log(Z^-1 P_i^-1 P_j) otherwise
IBA_ICP_HD inline void factor_residual(const double* Zi, const double* Pi, const double* Pj, double* r) {
    double M[12];
    if (Pi) { double Ti[12], B[12]; inv12(Pi, Ti); mul12(Zi, Ti, B); mul12(B, Pj, M); }
    else mul12(Zi, Pj, M);
    log_se3(M, r);
}

struct FactorDev {
    int F;
    const int32_t* fi; const int32_t* fj;   // fi < 0: a prior on fj
    const double* Zinv;        // F x 12
    const double* ivar;        // F x 6, 1 / var
    const uint8_t* robust;
};

// FULL: r, w, A, g and the factor's term of F. Otherwise the term alone. Block partial: the sum of the terms.
template <bool FULL>
__global__ __launch_bounds__(kThreads) void smooth_factor_kernel(FactorDev d, const double* __restrict__ poses, double* __restrict__ r_out, double* __restrict__ w_out,
                                                                 double* __restrict__ A_out, double* __restrict__ g_out, double* __restrict__ partial) {
    const int f = blockIdx.x * kThreads + threadIdx.x;
    double cost = 0.0;
    if (f < d.F) {
        const int i = d.fi[f], j = d.fj[f];
        const double* Pj = poses + 16 * (size_t)j;
        double r[6], iv[6];
        factor_residual(d.Zinv + 12 * (size_t)f, i >= 0 ? poses + 16 * (size_t)i : nullptr, Pj, r);
#pragma unroll
        for (int k = 0; k < 6; ++k) iv[k] = d.ivar[6 * (size_t)f + k];
        double q = r[0] * r[0] * iv[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) q += r[k] * r[k] * iv[k];
        const bool rob = d.robust[f] != 0;
        cost = rob ? log1p(q) : q;
        if (FULL) {
            const double w = rob ? 1.0 / (1.0 + q) : 1.0;
            double J[36];
            factor_jacobian(r, Pj, J);
            w_out[f] = w;
#pragma unroll
            for (int k = 0; k < 6; ++k) r_out[6 * (size_t)f + k] = r[k];
            double* A = A_out + 36 * (size_t)f;
#pragma unroll
            for (int k = 0; k < 6; ++k)
#pragma unroll
                for (int l = k; l < 6; ++l) {
                    double a = J[k] * iv[0] * J[l];
#pragma unroll
                    for (int m = 1; m < 6; ++m) a += J[m * 6 + k] * iv[m] * J[m * 6 + l];
                    a *= w;
                    A[k * 6 + l] = a; A[l * 6 + k] = a;
                }
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                double a = J[k] * iv[0] * r[0];
#pragma unroll
                for (int m = 1; m < 6; ++m) a += J[m * 6 + k] * iv[m] * r[m];
                g_out[6 * (size_t)f + k] = w * a;
            }
        }
    }
    const double tsum[1] = {wave_sum_f64(cost)};
    block_sum_store<1, kThreads>(tsum, partial);
}

// One 64-lane block per node. inc: factor * 2 + (the node is the factor's i), ascending factor. Lanes 0-35: D entry, lanes 36-41: b entry (+g for i,
// -g for j and for a prior), lane 42: |vec6(pose)|^2. partial[node] = {|x|^2, max |b|, max diagonal entry of the between-factor part of D}
__global__ __launch_bounds__(64) void smooth_node_kernel(int N, const int32_t* __restrict__ inc_off, const int32_t* __restrict__ inc, const int32_t* __restrict__ fi,
                                                         const double* __restrict__ A, const double* __restrict__ g, const double* __restrict__ poses,
                                                         double* __restrict__ D, double* __restrict__ b, double* __restrict__ partial) {
    const int i = blockIdx.x, l = threadIdx.x;
    const int lo = inc_off[i], hi = inc_off[i + 1];
    double v = 0.0, vb = 0.0, mb = 0.0, md = 0.0, xx = 0.0;
    if (l < 36) {
        for (int k = lo; k < hi; ++k) { const int f = inc[k] >> 1; const double a = A[36 * (size_t)f + l]; v += a; if (fi[f] >= 0) vb += a; }
        D[36 * (size_t)i + l] = v;
        if (l % 7 == 0) md = fabs(vb);
    } else if (l < 42) {
        for (int k = lo; k < hi; ++k) { const int e = inc[k]; const double ge = g[6 * (size_t)(e >> 1) + (l - 36)]; v += (e & 1) ? ge : -ge; }
        b[6 * (size_t)i + (l - 36)] = v;
        mb = fabs(v);
    } else if (l == 42) {
        double x[6];
        pgo::vec6_of(poses + 16 * (size_t)i, x);
        xx = x[0] * x[0];
#pragma unroll
        for (int k = 1; k < 6; ++k) xx += x[k] * x[k];
    }
    mb = wave_max_f64(mb); md = wave_max_f64(md); xx = wave_sum_f64(xx);
    if (l == 63) { partial[3 * (size_t)i] = xx; partial[3 * (size_t)i + 1] = mb; partial[3 * (size_t)i + 2] = md; }
}

// trial pose_i = Exp(delta_i) pose_i; partial[block] = {sum delta . (lambda delta + b), sum |delta|^2}
__global__ __launch_bounds__(kThreads) void smooth_update_kernel(int N, const double* __restrict__ poses, const double* __restrict__ delta, const double* __restrict__ b, double lambda,
                                                                 double* __restrict__ trial, double* __restrict__ partial) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    double dot = 0.0, dd = 0.0;
    if (i < N) {
        double dl[6], T[12], P[12];
#pragma unroll
        for (int k = 0; k < 6; ++k) dl[k] = delta[6 * (size_t)i + k];
        exp_se3(dl, T);
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

} }  // namespace iba::smooth

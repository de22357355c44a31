// Two-view initialisation, the arithmetic of rules T2-T5 and T7-T9 (include/iba_mi355x.h, iba_twoview*): ONE text for the kernels
// (iba_twoview_kernels.hpp), the host restatement (iba_twoview_host.hpp) and the stand-alone sanitizer self-test, which compiles this file with plain
// g++. Everything here is + - x / sqrt on float32 or float64, every operation rounded, left to right, no contraction; nothing calls libm beyond sqrt.
// A work matrix is addressed with an element stride S: 1 for a private array, the lane count of a block for a lane-minor LDS slab.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define IBA_TV_HD __host__ __device__ inline
#else
#define IBA_TV_HD inline
#endif

namespace iba {
namespace tv {

constexpr int kMaxSweeps = 30;
constexpr int kWorkDoubles = 16 * 9 + 9 * 9;      // the largest case of T2: G and V of the 16 x 9 design matrix

// a NaN that is stored into an output is stored as this one
IBA_TV_HD float canon(float x) {
    if (x == x) return x;
    const uint32_t b = 0x7FC00000u;
    float c;
    __builtin_memcpy(&c, &b, 4);
    return c;
}

// ---- T2: one-sided Jacobi on G (M x N, already holding the widened float32 matrix) with V = I; returns the sweeps that rotated (kMaxSweeps: all did) ----
template <int M, int N, int S, int UNROLL>
IBA_TV_HD int jacobi(double* G, double* V) {
#pragma unroll UNROLL ? N : 1
    for (int i = 0; i < N; ++i)
#pragma unroll UNROLL ? N : 1
        for (int j = 0; j < N; ++j) V[(i * N + j) * S] = i == j ? 1.0 : 0.0;
    // a column at the rounding level of the whole matrix is numerically null and is left alone: without this a matrix of rank below N (every
    // 8 x 9 one) never meets the relative test on its vanishing column and runs to the cap
    double fro = 0.0;
#pragma unroll UNROLL ? M * N : 1
    for (int i = 0; i < M * N; ++i) fro += G[i * S] * G[i * S];
    const double tiny = fro * 0x1p-104;
    int sweep = 0;
    for (; sweep < kMaxSweeps; ++sweep) {
        int rotated = 0;
#pragma unroll UNROLL ? N : 1
        for (int p = 0; p < N - 1; ++p) {
#pragma unroll UNROLL ? N : 1
            for (int q = p + 1; q < N; ++q) {
                double a = 0.0, b = 0.0, g = 0.0;
#pragma unroll UNROLL ? M : 1
                for (int r = 0; r < M; ++r) {
                    const double gp = G[(r * N + p) * S], gq = G[(r * N + q) * S];
                    a += gp * gp; b += gq * gq; g += gp * gq;
                }
                if (g * g <= a * b * 0x1p-104 || a <= tiny || b <= tiny) continue;
                const double zeta = (b - a) / (2.0 * g);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
#pragma unroll UNROLL ? M : 1
                for (int r = 0; r < M; ++r) {
                    const double gp = G[(r * N + p) * S], gq = G[(r * N + q) * S];
                    G[(r * N + p) * S] = c * gp - s * gq; G[(r * N + q) * S] = s * gp + c * gq;
                }
#pragma unroll UNROLL ? N : 1
                for (int r = 0; r < N; ++r) {
                    const double vp = V[(r * N + p) * S], vq = V[(r * N + q) * S];
                    V[(r * N + p) * S] = c * vp - s * vq; V[(r * N + q) * S] = s * vp + c * vq;
                }
                ++rotated;
            }
        }
        if (!rotated) break;
    }
    return sweep;
}

template <int M, int N, int S, int UNROLL>
IBA_TV_HD double col_norm2(const double* G, int c) {
    double n = 0.0;
#pragma unroll UNROLL ? M : 1
    for (int r = 0; r < M; ++r) { const double g = G[(r * N + c) * S]; n += g * g; }
    return n;
}

// the null vector: V's column under G's column of least squared norm, the first on a tie
template <int M, int N, int S, int UNROLL>
IBA_TV_HD int null_vector(double* G, double* V, float* v) {
    const int sweeps = jacobi<M, N, S, UNROLL>(G, V);
    int best = 0;
    double bn = col_norm2<M, N, S, UNROLL>(G, 0);
#pragma unroll UNROLL ? N : 1
    for (int c = 1; c < N; ++c) {
        const double n = col_norm2<M, N, S, UNROLL>(G, c);
        if (n < bn) { bn = n; best = c; }
    }
#pragma unroll UNROLL ? N : 1
    for (int i = 0; i < N; ++i) {
        double x = V[(i * N) * S];
#pragma unroll UNROLL ? N : 1
        for (int c = 1; c < N; ++c) x = c == best ? V[(i * N + c) * S] : x;
        v[i] = (float)x;
    }
    return sweeps;
}

IBA_TV_HD int null_vector_33(const float* A, float* v) {
    double G[9], V[9];
    for (int i = 0; i < 9; ++i) G[i] = (double)A[i];
    return null_vector<3, 3, 1, 1>(G, V, v);
}

// the 3 x 3 SVD of T2: w descending (stable on the squared norms), vt's ROWS and u's COLUMNS go with them; u3 = u1 x u2 where w3 <= 2^-23 w1
IBA_TV_HD int svd33(const float* A, float* U, float* w, float* Vt) {
    double G[9], V[9], n[3], ud[9], wd[3];
    for (int i = 0; i < 9; ++i) G[i] = (double)A[i];
    const int sweeps = jacobi<3, 3, 1, 1>(G, V);
    for (int c = 0; c < 3; ++c) n[c] = col_norm2<3, 3, 1, 1>(G, c);
    int o0 = 0, o1 = 1, o2 = 2, tmp;
    if (n[o1] > n[o0]) { tmp = o0; o0 = o1; o1 = tmp; }
    if (n[o2] > n[o1]) { tmp = o1; o1 = o2; o2 = tmp; if (n[o1] > n[o0]) { tmp = o0; o0 = o1; o1 = tmp; } }
    const int ord[3] = {o0, o1, o2};
    for (int k = 0; k < 3; ++k) {
        wd[k] = std::sqrt(n[ord[k]]);
        for (int r = 0; r < 3; ++r) { ud[r * 3 + k] = G[r * 3 + ord[k]] / wd[k]; Vt[k * 3 + r] = (float)V[r * 3 + ord[k]]; }
    }
    if (wd[2] <= 0x1p-23 * wd[0]) {
        ud[2] = ud[3] * ud[7] - ud[6] * ud[4];
        ud[5] = ud[6] * ud[1] - ud[0] * ud[7];
        ud[8] = ud[0] * ud[4] - ud[3] * ud[1];
    }
    for (int i = 0; i < 9; ++i) U[i] = (float)ud[i];
    for (int k = 0; k < 3; ++k) w[k] = (float)wd[k];
    return sweeps;
}

// ---- the cv::Mat operations, restated: float64 on the widened float32 entries, one rounding per result element ----
IBA_TV_HD void mul33(const float* A, const float* B, float* C) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            C[i * 3 + j] = (float)(((double)A[i * 3] * (double)B[j] + (double)A[i * 3 + 1] * (double)B[3 + j]) + (double)A[i * 3 + 2] * (double)B[6 + j]);
}
IBA_TV_HD void mul331(const float* A, const float* x, float* y) {
    for (int i = 0; i < 3; ++i) y[i] = (float)(((double)A[i * 3] * (double)x[0] + (double)A[i * 3 + 1] * (double)x[1]) + (double)A[i * 3 + 2] * (double)x[2]);
}
IBA_TV_HD void transpose33(const float* A, float* At) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) At[i * 3 + j] = A[j * 3 + i];
}
IBA_TV_HD double det33(const float* M) {
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    return (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
}
IBA_TV_HD void inv33(const float* M, float* Mi) {
    const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5], g = M[6], h = M[7], i = M[8];
    const double det = (a * (e * i - f * h) - b * (d * i - f * g)) + c * (d * h - e * g);
    Mi[0] = (float)((e * i - f * h) / det); Mi[1] = (float)((c * h - b * i) / det); Mi[2] = (float)((b * f - c * e) / det);
    Mi[3] = (float)((f * g - d * i) / det); Mi[4] = (float)((a * i - c * g) / det); Mi[5] = (float)((c * d - a * f) / det);
    Mi[6] = (float)((d * h - e * g) / det); Mi[7] = (float)((b * g - a * h) / det); Mi[8] = (float)((a * e - b * d) / det);
}
IBA_TV_HD double norm3(const float* x) { return std::sqrt(((double)x[0] * (double)x[0] + (double)x[1] * (double)x[1]) + (double)x[2] * (double)x[2]); }
// the inverse of T = [sx 0 tx; 0 sy ty; 0 0 1] in closed form (T3)
IBA_TV_HD void inv_affine_diag(const float* T, float* Ti) {
    for (int i = 0; i < 9; ++i) Ti[i] = 0.f;
    Ti[0] = (float)(1.0 / (double)T[0]); Ti[4] = (float)(1.0 / (double)T[4]);
    Ti[2] = (float)(-(double)T[2] / (double)T[0]); Ti[5] = (float)(-(double)T[5] / (double)T[4]); Ti[8] = 1.f;
}
IBA_TV_HD void make_K(float fx, float fy, float cx, float cy, float* K) {
    K[0] = fx; K[1] = 0.f; K[2] = cx; K[3] = 0.f; K[4] = fy; K[5] = cy; K[6] = 0.f; K[7] = 0.f; K[8] = 1.f;
}

// ---- T3: pn = the 8 normalised pairs (u1 v1 u2 v2 each); ws = kWorkDoubles doubles at stride S ----
template <int S>
IBA_TV_HD int h_hypothesis(const float* pn, const float* T1, const float* T2inv, double* ws, float* H21, float* H12) {
    double* G = ws;
    double* V = ws + 144 * S;
    for (int i = 0; i < 8; ++i) {
        const float u1 = pn[4 * i], v1 = pn[4 * i + 1], u2 = pn[4 * i + 2], v2 = pn[4 * i + 3];
        const float r0[9] = {0.0f, 0.0f, 0.0f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.0f, 0.0f, 0.0f, -u2 * u1, -u2 * v1, -u2};
        for (int j = 0; j < 9; ++j) { G[((2 * i) * 9 + j) * S] = (double)r0[j]; G[((2 * i + 1) * 9 + j) * S] = (double)r1[j]; }
    }
    float Hn[9], tmp[9];
    const int sweeps = null_vector<16, 9, S, 0>(G, V, Hn);
    mul33(T2inv, Hn, tmp);
    mul33(tmp, T1, H21);
    inv33(H21, H12);
    return sweeps;
}

// ---- T4 ----
template <int S>
IBA_TV_HD int f_hypothesis(const float* pn, const float* T1, const float* T2t, double* ws, float* F21) {
    double* G = ws;
    double* V = ws + 144 * S;
    for (int i = 0; i < 8; ++i) {
        const float u1 = pn[4 * i], v1 = pn[4 * i + 1], u2 = pn[4 * i + 2], v2 = pn[4 * i + 3];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        for (int j = 0; j < 9; ++j) G[(i * 9 + j) * S] = (double)r[j];
    }
    float Fpre[9], v3[3], Fn[9], tmp[9];
    int sweeps = null_vector<8, 9, S, 0>(G, V, Fpre);
    const int s2 = null_vector_33(Fpre, v3);
    sweeps = s2 > sweeps ? s2 : sweeps;
    for (int i = 0; i < 3; ++i) {
        const double y = ((double)Fpre[i * 3] * (double)v3[0] + (double)Fpre[i * 3 + 1] * (double)v3[1]) + (double)Fpre[i * 3 + 2] * (double)v3[2];
        for (int j = 0; j < 3; ++j) Fn[i * 3 + j] = (float)((double)Fpre[i * 3 + j] - y * (double)v3[j]);
    }
    mul33(T2t, Fn, tmp);
    mul33(tmp, T1, F21);
    return sweeps;
}

// ---- T5: one match of CheckHomography / CheckFundamental; score takes the match's two terms in order; returns bIn ----
IBA_TV_HD float inv_sigma_square(float sigma) { return (float)(1.0 / (double)(sigma * sigma)); }
IBA_TV_HD bool score_h_match(const float* h, const float* hi, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
    const float th = 5.991f;
    bool bIn = true;
    const float w2in1inv = (float)(1.0 / (double)(hi[6] * u2 + hi[7] * v2 + hi[8]));
    const float u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
    const float v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += th - chiSquare1;
    const float w1in2inv = (float)(1.0 / (double)(h[6] * u1 + h[7] * v1 + h[8]));
    const float u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
    const float v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += th - chiSquare2;
    return bIn;
}
IBA_TV_HD bool score_f_match(const float* f, float u1, float v1, float u2, float v2, float invSigmaSquare, float& score) {
    const float th = 3.841f, thScore = 5.991f;
    bool bIn = true;
    const float a2 = f[0] * u1 + f[1] * v1 + f[2];
    const float b2 = f[3] * u1 + f[4] * v1 + f[5];
    const float c2 = f[6] * u1 + f[7] * v1 + f[8];
    const float num2 = a2 * u2 + b2 * v2 + c2;
    const float squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = false; else score += thScore - chiSquare1;
    const float a1 = f[0] * u2 + f[3] * v2 + f[6];
    const float b1 = f[1] * u2 + f[4] * v2 + f[7];
    const float c1 = f[2] * u2 + f[5] * v2 + f[8];
    const float num1 = a1 * u1 + b1 * v1 + c1;
    const float squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = false; else score += thScore - chiSquare2;
    return bIn;
}

// ---- a motion hypothesis as T9 reads it ----
struct Cam { float R[9], t[3], P2[12], O2[3]; };
IBA_TV_HD void make_cam(const float* K, const float* R, const float* t, Cam& c) {
    for (int i = 0; i < 9; ++i) c.R[i] = R[i];
    for (int i = 0; i < 3; ++i) c.t[i] = t[i];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            const double m0 = j < 3 ? (double)R[j] : (double)t[0], m1 = j < 3 ? (double)R[3 + j] : (double)t[1], m2 = j < 3 ? (double)R[6 + j] : (double)t[2];
            c.P2[i * 4 + j] = (float)(((double)K[i * 3] * m0 + (double)K[i * 3 + 1] * m1) + (double)K[i * 3 + 2] * m2);
        }
    for (int i = 0; i < 3; ++i) c.O2[i] = (float)(-(((double)R[i] * (double)t[0] + (double)R[3 + i] * (double)t[1]) + (double)R[6 + i] * (double)t[2]));
}

// ---- T7: E = K^T F K, the four hypotheses (R1, t), (R2, t), (R1, -t), (R2, -t) ----
IBA_TV_HD int motions_from_f(const float* F, const float* K, float* R /* 4 x 9 */, float* t /* 4 x 3 */) {
    float Kt[9], tmp[9], E[9], U[9], w[3], Vt[9], W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f}, Wt[9], R1[9], R2[9], tt[3];
    transpose33(K, Kt);
    mul33(Kt, F, tmp);
    mul33(tmp, K, E);
    const int sweeps = svd33(E, U, w, Vt);
    const float u3[3] = {U[2], U[5], U[8]};
    const double n = norm3(u3);
    for (int i = 0; i < 3; ++i) tt[i] = (float)((double)u3[i] / n);
    mul33(U, W, tmp);
    mul33(tmp, Vt, R1);
    if (det33(R1) < 0.0) for (int i = 0; i < 9; ++i) R1[i] = -R1[i];
    transpose33(W, Wt);
    mul33(U, Wt, tmp);
    mul33(tmp, Vt, R2);
    if (det33(R2) < 0.0) for (int i = 0; i < 9; ++i) R2[i] = -R2[i];
    for (int i = 0; i < 9; ++i) { R[i] = R1[i]; R[9 + i] = R2[i]; R[18 + i] = R1[i]; R[27 + i] = R2[i]; }
    for (int i = 0; i < 3; ++i) { t[i] = tt[i]; t[3 + i] = tt[i]; t[6 + i] = -tt[i]; t[9 + i] = -tt[i]; }
    return sweeps;
}

// ---- T8: Faugeras' eight hypotheses; false = the early refusal ----
IBA_TV_HD bool motions_from_h(const float* H21, const float* K, float* R /* 8 x 9 */, float* t /* 8 x 3 */, int* sweeps_out) {
    float invK[9], tmp[9], A[9], U[9], w[3], Vt[9];
    inv33(K, invK);
    mul33(invK, H21, tmp);
    mul33(tmp, K, A);
    *sweeps_out = svd33(A, U, w, Vt);
    const float s = (float)(det33(U) * det33(Vt));
    const float d1 = w[0], d2 = w[1], d3 = w[2];
    if ((double)(d1 / d2) < 1.00001 || (double)(d2 / d3) < 1.00001) return false;
    const float aux1 = std::sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));
    const float aux3 = std::sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const float x1[4] = {aux1, aux1, -aux1, -aux1};
    const float x3[4] = {aux3, -aux3, aux3, -aux3};
    const float aux_stheta = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);
    const float ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const float stheta[4] = {aux_stheta, -aux_stheta, -aux_stheta, aux_stheta};
    const float aux_sphi = std::sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);
    const float cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    const float sphi[4] = {aux_sphi, -aux_sphi, -aux_sphi, aux_sphi};
    float sU[9];
    for (int i = 0; i < 9; ++i) sU[i] = s * U[i];
    for (int k = 0; k < 8; ++k) {
        const int i = k & 3;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f}, tp[3], tk[3];
        if (k < 4) {
            Rp[0] = ctheta; Rp[2] = -stheta[i]; Rp[6] = stheta[i]; Rp[8] = ctheta;
            tp[0] = x1[i] * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3[i] * (d1 - d3);
        } else {
            Rp[0] = cphi; Rp[2] = sphi[i]; Rp[4] = -1.f; Rp[6] = sphi[i]; Rp[8] = -cphi;
            tp[0] = x1[i] * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3[i] * (d1 + d3);
        }
        mul33(sU, Rp, tmp);
        mul33(tmp, Vt, R + 9 * k);
        mul331(U, tp, tk);
        const double n = norm3(tk);
        for (int j = 0; j < 3; ++j) t[3 * k + j] = (float)((double)tk[j] / n);
    }
    return true;
}

// ---- T9: one (motion hypothesis, inlier match). Verdicts: 1 not finite, 2 depth in camera 1, 3 depth in camera 2, 4 reprojection in image 1,
// 5 reprojection in image 2, 6 good (0 is kept for a match that is no inlier of the chosen model and was not evaluated). p and cosParallax are
// written for every verdict but 1. ----
IBA_TV_HD int check_rt_match(const Cam& c, float fx, float fy, float cx, float cy, float u1, float v1, float u2, float v2, float th2, float* p, float* cos_out, int* sweeps_out) {
    const float P1[12] = {fx, 0.f, cx, 0.f, 0.f, fy, cy, 0.f, 0.f, 0.f, 1.f, 0.f};
    double G[16], V[16];
    for (int j = 0; j < 4; ++j) {
        G[j] = (double)(u1 * P1[8 + j] - P1[j]);
        G[4 + j] = (double)(v1 * P1[8 + j] - P1[4 + j]);
        G[8 + j] = (double)(u2 * c.P2[8 + j] - c.P2[j]);
        G[12 + j] = (double)(v2 * c.P2[8 + j] - c.P2[4 + j]);
    }
    float x[4];
    *sweeps_out = null_vector<4, 4, 1, 1>(G, V, x);
    p[0] = x[0] / x[3]; p[1] = x[1] / x[3]; p[2] = x[2] / x[3];
    *cos_out = 0.f;
    if (!std::isfinite(p[0]) || !std::isfinite(p[1]) || !std::isfinite(p[2])) { p[0] = p[1] = p[2] = 0.f; return 1; }
    const float dist1 = (float)norm3(p);
    const float n2[3] = {p[0] - c.O2[0], p[1] - c.O2[1], p[2] - c.O2[2]};
    const float dist2 = (float)norm3(n2);
    const double dot = ((double)p[0] * (double)n2[0] + (double)p[1] * (double)n2[1]) + (double)p[2] * (double)n2[2];
    const float cosParallax = (float)(dot / (double)(dist1 * dist2));
    *cos_out = cosParallax;
    if (p[2] <= 0.f && (double)cosParallax < 0.99998) return 2;
    float p2[3];
    for (int i = 0; i < 3; ++i)
        p2[i] = (float)((((double)c.R[i * 3] * (double)p[0] + (double)c.R[i * 3 + 1] * (double)p[1]) + (double)c.R[i * 3 + 2] * (double)p[2]) + (double)c.t[i]);
    if (p2[2] <= 0.f && (double)cosParallax < 0.99998) return 3;
    const float invZ1 = (float)(1.0 / (double)p[2]);
    const float im1x = fx * p[0] * invZ1 + cx, im1y = fy * p[1] * invZ1 + cy;
    const float squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);
    if (squareError1 > th2) return 4;
    const float invZ2 = (float)(1.0 / (double)p2[2]);
    const float im2x = fx * p2[0] * invZ2 + cx, im2y = fy * p2[1] * invZ2 + cy;
    const float squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);
    if (squareError2 > th2) return 5;
    return 6;
}

// the order of the good cosines (T9): ascending float, every NaN last
IBA_TV_HD uint32_t cos_key(float c) {
    if (c != c) return 0xFFFFFFFFu;
    uint32_t b;
    __builtin_memcpy(&b, &c, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
IBA_TV_HD float cos_unkey(uint32_t k) {
    const uint32_t b = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k;
    float c;
    __builtin_memcpy(&c, &b, 4);
    return c;
}

// ---- T10 up to the parallax test: fail_before / fail_after are T11 codes or 0; cand = the hypothesis whose parallax decides (-1: none) ----
enum { kOK = 0, kTooFewMatches = 1, kNoModel = 2, kHDegenerate = 3, kNoClearWinner = 4, kTooFewPoints = 5, kLowParallax = 6 };
struct Accept { int cand, fail_before, fail_after; };
IBA_TV_HD Accept accept_f(const int* nGood, int N, int minTriangulated) {
    int maxGood = nGood[0];
    for (int k = 1; k < 4; ++k) maxGood = nGood[k] > maxGood ? nGood[k] : maxGood;
    const int n09 = (int)(0.9 * N);
    const int nMinGood = n09 > minTriangulated ? n09 : minTriangulated;
    int nsimilar = 0;
    for (int k = 0; k < 4; ++k) if ((double)nGood[k] > 0.7 * maxGood) nsimilar++;
    Accept a{-1, 0, 0};
    if (maxGood < nMinGood) { a.fail_before = kTooFewPoints; return a; }
    if (nsimilar > 1) { a.fail_before = kNoClearWinner; return a; }
    for (int k = 3; k >= 0; --k) if (nGood[k] == maxGood) a.cand = k;
    return a;
}
IBA_TV_HD Accept accept_h(const int* nGood, int N, int minTriangulated) {
    int bestGood = 0, secondBestGood = 0, best = -1;
    for (int k = 0; k < 8; ++k) {
        if (nGood[k] > bestGood) { secondBestGood = bestGood; bestGood = nGood[k]; best = k; }
        else if (nGood[k] > secondBestGood) secondBestGood = nGood[k];
    }
    Accept a{-1, 0, 0};
    if (!((double)secondBestGood < 0.75 * bestGood)) { a.fail_before = kNoClearWinner; return a; }
    a.cand = best;
    if (!(bestGood > minTriangulated) || !((double)bestGood > 0.9 * N)) a.fail_after = kTooFewPoints;
    return a;
}

}  // namespace tv
}  // namespace iba

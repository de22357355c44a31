// Sim3 RANSAC between two keyframes, the arithmetic of rules Z2-Z5 and Z7 (include/iba_mi355x.h, iba_sim3*): ONE text for the kernels
// (iba_sim3_kernels.hpp), the host restatement (iba_sim3_host.hpp) and the stand-alone sanitizer self-test, which compiles this file with plain g++.
// Everything here is + - x / sqrt on float32 or float64, every operation rounded, left to right, no contraction; nothing calls libm beyond sqrt.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define IBA_Z_HD __host__ __device__ inline
#else
#define IBA_Z_HD inline
#endif

namespace iba {
namespace z3 {

constexpr int kMaxSweeps = 30;

// a NaN that is stored into an output is stored as this one
IBA_Z_HD float canon(float x) {
    if (x == x) return x;
    const uint32_t b = 0x7FC00000u;
    float c;
    __builtin_memcpy(&c, &b, 4);
    return c;
}

// the product of a float32 matrix row with a float32 vector as a cv::Mat product gives it: float64 on the widened entries, one rounding
IBA_Z_HD float dot3(float a0, float a1, float a2, float b0, float b1, float b2) {
    return (float)((((double)a0 * (double)b0) + ((double)a1 * (double)b1)) + ((double)a2 * (double)b2));
}

// ---- Z2: a world point into a camera (L1's order of sums, float32) and its image point ----
IBA_Z_HD void to_camera(const float* T, float X, float Y, float Z, float* c) {
    for (int i = 0; i < 3; ++i) c[i] = ((T[4 * i] * X + T[4 * i + 1] * Y) + T[4 * i + 2] * Z) + T[4 * i + 3];
}
IBA_Z_HD void to_image(const float* K, float x, float y, float z, float* u, float* v) {
    const float invz = (float)(1.0 / (double)z);      // 1 / z in float32, correctly rounded; no test on z
    const float xn = x * invz, yn = y * invz;
    *u = K[0] * xn + K[2]; *v = K[1] * yn + K[3];
}

// ---- Z3 / Z4: Horn's closed form on three correspondences. P1, P2: 3 x 3 row-major, COLUMN j = point j in camera 1 / 2.
// out: srt[13] = s, R (row-major), t; T12[12], T21[12] (3 x 4 row-major). Returns the sweeps that rotated. ----
IBA_Z_HD int horn(const float* P1, const float* P2, int fix_scale, float* srt, float* T12, float* T21) {
    float O1[3], O2[3], Pr1[9], Pr2[9], M[9];
    for (int r = 0; r < 3; ++r) {
        const float s1 = (float)(((double)P1[3 * r] + (double)P1[3 * r + 1]) + (double)P1[3 * r + 2]);
        const float s2 = (float)(((double)P2[3 * r] + (double)P2[3 * r + 1]) + (double)P2[3 * r + 2]);
        O1[r] = (float)((double)s1 / 3.0); O2[r] = (float)((double)s2 / 3.0);
        for (int j = 0; j < 3; ++j) { Pr1[3 * r + j] = P1[3 * r + j] - O1[r]; Pr2[3 * r + j] = P2[3 * r + j] - O2[r]; }
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = dot3(Pr2[3 * i], Pr2[3 * i + 1], Pr2[3 * i + 2], Pr1[3 * j], Pr1[3 * j + 1], Pr1[3 * j + 2]);
    const double m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
    const float N11 = (float)((m00 + m11) + m22), N12 = (float)(m12 - m21), N13 = (float)(m20 - m02), N14 = (float)(m01 - m10), N22 = (float)((m00 - m11) - m22),
                N23 = (float)(m01 + m10), N24 = (float)(m20 + m02), N33 = (float)((-m00 + m11) - m22), N34 = (float)(m12 + m21), N44 = (float)((-m00 - m11) + m22);
    double A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    double V[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5 == 0) ? 1.0 : 0.0;
    // the cyclic two-sided Jacobi: pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); a pair at the rounding level of its diagonal is left alone
    int sweep = 0;
    for (; sweep < kMaxSweeps; ++sweep) {
        int rotated = 0;
#pragma unroll
        for (int p = 0; p < 3; ++p) {
#pragma unroll
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[4 * p + q], app = A[4 * p + p], aqq = A[4 * q + q];
                if (std::fabs(apq) <= 0x1p-53 * (std::fabs(app) + std::fabs(aqq))) continue;
                const double theta = (aqq - app) / (2.0 * apq);
                const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(1.0 + theta * theta));
                const double c = 1.0 / std::sqrt(1.0 + tt * tt), s = c * tt;
#pragma unroll
                for (int k = 0; k < 4; ++k) {             // columns p and q of A and of V
                    const double ap = A[4 * k + p], aq = A[4 * k + q], vp = V[4 * k + p], vq = V[4 * k + q];
                    A[4 * k + p] = c * ap - s * aq; A[4 * k + q] = s * ap + c * aq;
                    V[4 * k + p] = c * vp - s * vq; V[4 * k + q] = s * vp + c * vq;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {             // rows p and q of A
                    const double ap = A[4 * p + k], aq = A[4 * q + k];
                    A[4 * p + k] = c * ap - s * aq; A[4 * q + k] = s * ap + c * aq;
                }
                A[4 * p + q] = 0.0; A[4 * q + p] = 0.0;
                ++rotated;
            }
        }
        if (!rotated) break;
    }
    // the greatest eigenvalue, the first on a tie; its eigenvector narrowed: the quaternion (w, x, y, z)
    double ev = A[0], qd[4] = {V[0], V[4], V[8], V[12]};
#pragma unroll
    for (int c = 1; c < 4; ++c) {
        const bool take = A[5 * c] > ev;
        ev = take ? A[5 * c] : ev;
#pragma unroll
        for (int k = 0; k < 4; ++k) qd[k] = take ? V[4 * k + c] : qd[k];
    }
    const double w = (double)(float)qd[0], x = (double)(float)qd[1], y = (double)(float)qd[2], z = (double)(float)qd[3];
    // Z4: the reference divides by the norm of the imaginary part: 0 or not finite there is NaN everywhere
    const double vn = std::sqrt((x * x + y * y) + z * z);
    const bool dead = !(vn > 0.0) || !(vn <= 1.7976931348623157e308);
    const double n = ((w * w + x * x) + y * y) + z * z;
    float R[9];
    R[0] = (float)(1.0 - 2.0 * (y * y + z * z) / n); R[1] = (float)(2.0 * (x * y - w * z) / n); R[2] = (float)(2.0 * (x * z + w * y) / n);
    R[3] = (float)(2.0 * (x * y + w * z) / n); R[4] = (float)(1.0 - 2.0 * (x * x + z * z) / n); R[5] = (float)(2.0 * (y * z - w * x) / n);
    R[6] = (float)(2.0 * (x * z - w * y) / n); R[7] = (float)(2.0 * (y * z + w * x) / n); R[8] = (float)(1.0 - 2.0 * (x * x + y * y) / n);
    // the scale: P3 = R Pr2; nom = Pr1 . P3, den = the sum of P3's float32 squares, both double sums in row-major order
    float s = 1.0f;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float p3 = dot3(R[3 * i], R[3 * i + 1], R[3 * i + 2], Pr2[j], Pr2[3 + j], Pr2[6 + j]);
                nom += (double)Pr1[3 * i + j] * (double)p3;
                const float sq = p3 * p3;
                den += (double)sq;
            }
        s = (float)(nom / den);
    }
    float sR[9], t[3];
    for (int i = 0; i < 9; ++i) sR[i] = s * R[i];
    for (int i = 0; i < 3; ++i) t[i] = O1[i] - dot3(sR[3 * i], sR[3 * i + 1], sR[3 * i + 2], O2[0], O2[1], O2[2]);
    const double inv_s = 1.0 / (double)s;
    const float nan = canon(std::sqrt(-1.0f));
    srt[0] = dead ? nan : canon(s);
    for (int i = 0; i < 9; ++i) srt[1 + i] = dead ? nan : canon(R[i]);
    for (int i = 0; i < 3; ++i) srt[10 + i] = dead ? nan : canon(t[i]);
    for (int i = 0; i < 3; ++i) {
        float ri[3];
        for (int j = 0; j < 3; ++j) { ri[j] = (float)(inv_s * (double)R[3 * j + i]); T12[4 * i + j] = dead ? nan : canon(sR[3 * i + j]); T21[4 * i + j] = dead ? nan : canon(ri[j]); }
        T12[4 * i + 3] = dead ? nan : canon(t[i]);
        T21[4 * i + 3] = dead ? nan : canon(-dot3(ri[0], ri[1], ri[2], t[0], t[1], t[2]));
    }
    return sweep;
}

// ---- Z5: Project, then the squared distance to the image point ----
IBA_Z_HD float reproject_err(const float* T, const float* K, float X, float Y, float Z, float u0, float v0) {
    const float px = dot3(T[0], T[1], T[2], X, Y, Z) + T[3], py = dot3(T[4], T[5], T[6], X, Y, Z) + T[7], pz = dot3(T[8], T[9], T[10], X, Y, Z) + T[11];
    float u, v;
    to_image(K, px, py, pz, &u, &v);
    const float d0 = u0 - u, d1 = v0 - v;
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}
// c1, c2: the correspondence in camera 1 / 2; (u1, v1), (u2, v2) its image points there; a NaN passes neither test
IBA_Z_HD bool is_inlier(const float* T12, const float* T21, const float* K1, const float* K2, const float* c1, const float* c2, float u1, float v1, float u2, float v2, float e1, float e2) {
    const float err1 = reproject_err(T12, K1, c2[0], c2[1], c2[2], u1, v1);
    const float err2 = reproject_err(T21, K2, c1[0], c1[1], c1[2], u2, v2);
    return err1 < e1 && err2 < e2;
}

// ---- Z7: the sequential rule over a job's counts. ev_it takes max_events entries (-1 where there is no such event). ----
IBA_Z_HD void scan(const int32_t* counts, int32_t I, int32_t min_inliers, int32_t max_events, int32_t* ev_it, int32_t* n_events, int32_t* best_it, int32_t* best_n) {
    int32_t best = 0, bi = -1, ne = 0;
    for (int32_t k = 0; k < max_events; ++k) ev_it[k] = -1;
    for (int32_t it = 0; it < I; ++it) {
        const int32_t n = counts[it];
        if (n < best) continue;
        best = n; bi = it;
        if (n > min_inliers) { if (ne < max_events) ev_it[ne] = it; ++ne; }
    }
    *n_events = ne; *best_it = bi; *best_n = best;
}

}  // namespace z3
}  // namespace iba

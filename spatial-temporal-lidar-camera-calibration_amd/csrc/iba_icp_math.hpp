// Host side of the ICP driver (include/iba_mi355x.h, iba_icp_*): what happens to the moment block of one pass. Plain C++, no HIP:
//  * Eigen::umeyama (Eigen/src/Geometry/Umeyama.h) restated on the pivoted sums the device returns, the SVD by svd3 (iba_svd3.hpp);
//  * T = update * T, the bookkeeping of Open3D's RegistrationICP (fitness, inlier_rmse, the two convergence criteria);
//  * the conventions of icp_calib.cpp:55-71 (readSim3 form <-> the 4x4 the loop runs on).
// Parity with Open3D / Eigen is unpinned (neither is in the reference tree); tests/icp_ref.py restates the same in numpy.
#pragma once
#include <cmath>
#include <cstring>

#include "../../include/iba_mi355x.h"
#include "iba_svd3.hpp"

// the pieces the pose-graph kernels (iba_pgo_kernels.hpp) share with the host run on the device as well
#if defined(__HIPCC__)
#define IBA_ICP_HD __host__ __device__
#else
#define IBA_ICP_HD
#endif

namespace iba { namespace icp {

// C = A * B, row-major 4x4, each entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3
IBA_ICP_HD inline void mat4_mul(const double* A, const double* B, double* C) {
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c)
        C[r * 4 + c] = ((A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c]) + A[r * 4 + 3] * B[12 + c];
}

// Eigen::umeyama(src = q, dst = p, with_scaling) from the moments of iba_icp_step (sums about the pivot v = m[18..20]) -> row-major 4x4.
// false: fewer than 3 pairs or a source set without spread (Eigen would divide by src_var = 0): no update, U4 untouched.
inline bool umeyama_from_moments(const double* m, bool with_scaling, double* U4) {
    const double n = m[0];
    if (!(n >= 3.0)) return false;
    const double inv = 1.0 / n;
    const double mq[3] = {m[2] * inv, m[3] * inv, m[4] * inv}, mp[3] = {m[5] * inv, m[6] * inv, m[7] * inv};   // means, relative to the pivot
    const double var_q = m[8] * inv - ((mq[0] * mq[0] + mq[1] * mq[1]) + mq[2] * mq[2]);
    if (!(var_q > 0.0) || !std::isfinite(var_q)) return false;
    double sigma[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) sigma[i * 3 + j] = m[9 + 3 * i + j] * inv - mp[i] * mq[j];
    for (int i = 0; i < 9; ++i) if (!std::isfinite(sigma[i])) return false;
    double U[9], V[9];
    la3::svd3(sigma, U, V);   // sigma = U diag(d) V^T, columns
    double d[3];
    for (int c = 0; c < 3; ++c) {   // d_c = u_c^T sigma v_c
        const double v[3] = {V[c], V[3 + c], V[6 + c]};
        double sv[3]; la3::mat3_vec(sigma, v, sv);
        d[c] = (U[c] * sv[0] + U[3 + c] * sv[1]) + U[6 + c] * sv[2];
    }
    const double S2 = la3::det3(U) * la3::det3(V) < 0.0 ? -1.0 : 1.0;
    double R[9];
    for (int i = 0; i < 3; ++i) for (int j = 0; j < 3; ++j) R[i * 3 + j] = (U[i * 3] * V[j * 3] + U[i * 3 + 1] * V[j * 3 + 1]) + S2 * (U[i * 3 + 2] * V[j * 3 + 2]);
    const double c = with_scaling ? ((d[0] + d[1]) + S2 * d[2]) / var_q : 1.0;
    if (!std::isfinite(c) || !(c > 0.0)) return false;
    const double aq[3] = {m[18] + mq[0], m[19] + mq[1], m[20] + mq[2]}, ap[3] = {m[18] + mp[0], m[19] + mp[1], m[20] + mp[2]};   // the means themselves
    double Rq[3]; la3::mat3_vec(R, aq, Rq);
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) U4[i * 4 + j] = c * R[i * 3 + j];
        U4[i * 4 + 3] = ap[i] - c * Rq[i];
    }
    U4[12] = 0.0; U4[13] = 0.0; U4[14] = 0.0; U4[15] = 1.0;
    return true;
}

// ---- scan-to-scan edges (iba_scan_*): the point-to-plane step and the information matrix, from the sums of one pass ----
// A x = b for a symmetric 6x6 A (row-major, both triangles filled) by LDL^T without pivoting (what Eigen's ldlt() does on a positive definite
// matrix up to its pivoting). false: a pivot that is not positive and finite, or a non-finite solution: the system is singular to working precision.
// The factor alone: L (unit lower, row-major 36, entries on and above the diagonal untouched) and d. false at a pivot that is not positive and finite.
IBA_ICP_HD inline bool ldlt6_factor(const double* A, double* L, double* d) {
    for (int j = 0; j < 6; ++j) {
        double s = A[j * 6 + j];
        for (int k = 0; k < j; ++k) s -= L[j * 6 + k] * L[j * 6 + k] * d[k];
        if (!(s > 0.0) || !(s <= 1.7976931348623157e308)) return false;
        d[j] = s;
        for (int i = j + 1; i < 6; ++i) {
            double v = A[i * 6 + j];
            for (int k = 0; k < j; ++k) v -= L[i * 6 + k] * L[j * 6 + k] * d[k];
            L[i * 6 + j] = v / s;
        }
    }
    return true;
}
// x = (L D L^T)^-1 b
IBA_ICP_HD inline void ldlt6_apply(const double* L, const double* d, const double* b, double* x) {
    double y[6];
    for (int i = 0; i < 6; ++i) { double v = b[i]; for (int k = 0; k < i; ++k) v -= L[i * 6 + k] * y[k]; y[i] = v; }
    for (int i = 5; i >= 0; --i) { double v = y[i] / d[i]; for (int k = i + 1; k < 6; ++k) v -= L[k * 6 + i] * x[k]; x[i] = v; }
}
inline bool ldlt6_solve(const double* A, const double* b, double* x) {
    double L[36] = {0.0}, d[6];
    if (!ldlt6_factor(A, L, d)) return false;
    ldlt6_apply(L, d, b, x);
    for (int i = 0; i < 6; ++i) if (!std::isfinite(x[i])) return false;
    // a matrix of rank < 6 passes the pivot test on rounding noise alone: its smallest pivot is then negligible beside the largest of its kind
    // (rotation block 0-2, translation block 3-5 have different units, so each block is compared with itself)
    for (int blk = 0; blk < 2; ++blk) {
        double mx = 0.0, mn = INFINITY;
        for (int i = 3 * blk; i < 3 * blk + 3; ++i) { mx = std::fmax(mx, d[i]); mn = std::fmin(mn, d[i]); }
        if (!(mn > 1e-12 * mx)) return false;
    }
    return true;
}
// Open3D TransformVector6dToMatrix4d: rotation Rz(x2) Ry(x1) Rx(x0), translation x[3..5] -> row-major 4x4
IBA_ICP_HD inline void vec6_to_mat4(const double* x, double* U4) {
    const double ca = cos(x[0]), sa = sin(x[0]), cb = cos(x[1]), sb = sin(x[1]), cg = cos(x[2]), sg = sin(x[2]);
    U4[0] = cg * cb; U4[1] = cg * sb * sa - sg * ca; U4[2] = cg * sb * ca + sg * sa; U4[3] = x[3];
    U4[4] = sg * cb; U4[5] = sg * sb * sa + cg * ca; U4[6] = sg * sb * ca - cg * sa; U4[7] = x[4];
    U4[8] = -sb;     U4[9] = cb * sa;                U4[10] = cb * ca;               U4[11] = x[5];
    U4[12] = 0.0; U4[13] = 0.0; U4[14] = 0.0; U4[15] = 1.0;
}
// TransformationEstimationPointToPlane from the moments of a point-to-plane pass (m[2] pairs with a normal, m[3..23] JtJ upper triangle by rows,
// m[24..29] Jtr): JtJ x = -Jtr, update = vec6_to_mat4(x). false: fewer than 6 pairs with a normal or a singular system: no update, U4 untouched.
inline bool point_to_plane_from_moments(const double* m, double* U4) {
    if (!(m[2] >= 6.0)) return false;
    double A[36], b[6], x[6];
    int o = 3;
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { A[i * 6 + j] = m[o]; A[j * 6 + i] = m[o]; ++o; }
    for (int i = 0; i < 6; ++i) b[i] = -m[24 + i];
    for (int i = 0; i < 36; ++i) if (!std::isfinite(A[i])) return false;
    if (!ldlt6_solve(A, b, x)) return false;
    vec6_to_mat4(x, U4);
    return true;
}
// GetInformationMatrixFromPointClouds from the sums of an information pass (s[0] pairs, s[1..3] sum t, s[4..9] sum t t^T upper triangle by rows):
// sum G^T G with G = [-[t]x | I], row-major 6x6
inline void information_from_sums(const double* s, double* I) {
    const double n = s[0], tx = s[1], ty = s[2], tz = s[3], xx = s[4], xy = s[5], xz = s[6], yy = s[7], yz = s[8], zz = s[9];
    const double M[36] = {yy + zz, -xy, -xz, 0.0, -tz, ty,
                          -xy, xx + zz, -yz, tz, 0.0, -tx,
                          -xz, -yz, xx + yy, -ty, tx, 0.0,
                          0.0, tz, -ty, n, 0.0, 0.0,
                          -tz, 0.0, tx, 0.0, n, 0.0,
                          ty, -tx, 0.0, 0.0, 0.0, n};
    std::memcpy(I, M, sizeof(M));
}

inline double fitness_of(const double* m, int n_src) { return n_src > 0 ? m[0] / (double)n_src : 0.0; }
inline double rmse_of(const double* m) { return m[0] > 0.0 ? std::sqrt(m[1] / m[0]) : 0.0; }
// sqrt((A A^T)_00) of the upper-left block (icp_calib.cpp:67-68)
inline double scale_of(const double* T) { return std::sqrt((T[0] * T[0] + T[1] * T[1]) + T[2] * T[2]); }

// rigid 3x4 inverse (R^T, -R^T t), row-major 12
inline void inv_rigid12(const double* a, double* o) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = a[c * 4 + r];
        o[r * 4 + 3] = -((a[0 * 4 + r] * a[3] + a[1 * 4 + r] * a[7]) + a[2 * 4 + r] * a[11]);
    }
}
// icp_calib.cpp:55-60: readSim3 form -> the init of the loop (R^T, -R^T t, rotation times the scale)
inline void init_from_sim3(const double* rigid12, double scale, double* T16) {
    double inv[12]; inv_rigid12(rigid12, inv);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) T16[r * 4 + c] = inv[r * 4 + c] * scale; T16[r * 4 + 3] = inv[r * 4 + 3]; }
    T16[12] = 0.0; T16[13] = 0.0; T16[14] = 0.0; T16[15] = 1.0;
}
// icp_calib.cpp:67-71: the loop's result -> (rigid 3x4, scale) in writeSim3 form
inline void sim3_from_result(const double* T16, double* rigid12, double* scale) {
    const double s = scale_of(T16);
    double a[12];
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) a[r * 4 + c] = T16[r * 4 + c] / s; a[r * 4 + 3] = T16[r * 4 + 3]; }
    inv_rigid12(a, rigid12);
    *scale = s;
}
// rigid 3x4 (as 4x4 with the row 0 0 0 1) times a 4x4
inline void rigid12_mul_T16(const double* a12, const double* T16, double* out16) {
    double A[16]; std::memcpy(A, a12, 12 * sizeof(double)); A[12] = 0.0; A[13] = 0.0; A[14] = 0.0; A[15] = 1.0;
    mat4_mul(A, T16, out16);
}

} }  // namespace iba::icp

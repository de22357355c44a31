// 3x3 host linear algebra shared by the hand-eye initialiser (iba_handeye.cpp: Kabsch on the rotation vectors) and the ICP driver
// (iba_icp_host.hpp: Eigen's umeyama restated): products, determinant, cyclic-Jacobi eigen-decomposition and the SVD built on it.
// Host only; the expression order is part of what the tests of both callers pin.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

namespace iba { namespace la3 {

inline void mat3_mul(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) C[r * 3 + c] = (A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c]) + A[r * 3 + 2] * B[6 + c];
}
inline void mat3_vec(const double* A, const double* v, double* o) {
    for (int r = 0; r < 3; ++r) o[r] = (A[r * 3] * v[0] + A[r * 3 + 1] * v[1]) + A[r * 3 + 2] * v[2];
}
inline double det3(const double* M) {
    return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// eigen-decomposition of a symmetric 3x3 (cyclic Jacobi); columns of V, eigenvalues sorted descending
inline void sym_eig3(const double* S, double* V, double* lam) {
    double A[9]; std::memcpy(A, S, sizeof(A));
    for (int i = 0; i < 9; ++i) V[i] = (i % 4 == 0) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 60; ++sweep) {
        const double off = A[1] * A[1] + A[2] * A[2] + A[5] * A[5];
        if (off < 1e-300) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p * 3 + q];
                if (std::fabs(apq) < 1e-300) continue;
                const double theta = (A[q * 3 + q] - A[p * 3 + p]) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) { const double akp = A[k * 3 + p], akq = A[k * 3 + q]; A[k * 3 + p] = c * akp - s * akq; A[k * 3 + q] = s * akp + c * akq; }
                for (int k = 0; k < 3; ++k) { const double apk = A[p * 3 + k], aqk = A[q * 3 + k]; A[p * 3 + k] = c * apk - s * aqk; A[q * 3 + k] = s * apk + c * aqk; }
                for (int k = 0; k < 3; ++k) { const double vkp = V[k * 3 + p], vkq = V[k * 3 + q]; V[k * 3 + p] = c * vkp - s * vkq; V[k * 3 + q] = s * vkp + c * vkq; }
            }
    }
    int idx[3] = {0, 1, 2};
    std::sort(idx, idx + 3, [&](int a, int b) { return A[a * 4] > A[b * 4]; });
    double Vs[9];
    for (int c = 0; c < 3; ++c) { lam[c] = A[idx[c] * 4]; for (int r = 0; r < 3; ++r) Vs[r * 3 + c] = V[r * 3 + idx[c]]; }
    std::memcpy(V, Vs, sizeof(Vs));
}

inline void cross(const double* a, const double* b, double* o) { o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0]; }
inline double norm3(const double* a) { return std::sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]); }

// full SVD H = U diag(s) V^T of a 3x3 (columns of U, V)
inline void svd3(const double* H, double* U, double* V) {
    double HtH[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) HtH[r * 3 + c] = H[0 * 3 + r] * H[0 * 3 + c] + H[1 * 3 + r] * H[1 * 3 + c] + H[2 * 3 + r] * H[2 * 3 + c];
    double lam[3];
    sym_eig3(HtH, V, lam);
    double u[3][3];
    const double smax = std::sqrt(std::max(lam[0], 0.0));
    int good = 0;
    for (int c = 0; c < 3; ++c) {
        const double v[3] = {V[0 * 3 + c], V[1 * 3 + c], V[2 * 3 + c]};
        double hv[3]; mat3_vec(H, v, hv);
        const double s = norm3(hv);
        if (s > 1e-12 * std::max(smax, 1e-300) && good == c) { for (int r = 0; r < 3; ++r) u[c][r] = hv[r] / s; ++good; }
        else break;
    }
    if (good == 0) { u[0][0] = 1; u[0][1] = 0; u[0][2] = 0; good = 1; }
    if (good == 1) {   // any unit vector orthogonal to u0
        const double* a = u[0];
        double e[3] = {0, 0, 0}; e[std::fabs(a[0]) < 0.9 ? 0 : 1] = 1.0;
        cross(a, e, u[1]); const double n = norm3(u[1]); for (int r = 0; r < 3; ++r) u[1][r] /= n;
        good = 2;
    }
    if (good == 2) { cross(u[0], u[1], u[2]); const double n = norm3(u[2]); for (int r = 0; r < 3; ++r) u[2][r] /= n; }
    for (int c = 0; c < 3; ++c) for (int r = 0; r < 3; ++r) U[r * 3 + c] = u[c][r];
}

} }  // namespace iba::la3

// The pieces of the pose-graph optimiser's device code that other units build on (iba_smooth_kernels.hpp): the launch constants and the rigid 3x4
// algebra of rules 1-3; the wave reductions both use come with it from iba_wave_sum.hpp. No kernel is defined here; iba_pgo_kernels.hpp holds those
// and is compiled into one unit only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_icp_math.hpp"
#include "iba_wave_sum.hpp"

namespace iba { namespace pgo {

constexpr int kThreads = 256;   // edge / update kernels
constexpr int kNB = 48;         // Cholesky panel width: 8 blocks of 6
constexpr int kTile = 32;       // trailing-update tile
constexpr int kMaxSepDim = 6 * IBA_PGO_MAX_SEPARATORS;
constexpr int kScal = 8;        // scalars the host reads: 0 r, 1 |x|^2, 2 max |b|, 3 max diag H, 4 delta . (lambda delta + b), 5 |delta|^2, 6 r_new, 7 a pivot failed

// ---- the rigid 3x4 algebra of rules 1-3 (rows of 4; works on the first 12 entries of a row-major 4x4 as well) ----
IBA_ICP_HD inline void mul12(const double* A, const double* B, double* C) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) C[r * 4 + c] = (A[r * 4] * B[c] + A[r * 4 + 1] * B[4 + c]) + A[r * 4 + 2] * B[8 + c];
        C[r * 4 + 3] = ((A[r * 4] * B[3] + A[r * 4 + 1] * B[7]) + A[r * 4 + 2] * B[11]) + A[r * 4 + 3];
    }
}
IBA_ICP_HD inline void inv12(const double* a, double* o) {
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) o[r * 4 + c] = a[c * 4 + r];
        o[r * 4 + 3] = -((a[r] * a[3] + a[4 + r] * a[7]) + a[8 + r] * a[11]);
    }
}
IBA_ICP_HD inline void vec6_of(const double* M, double* v) {   // rule 1
    const double sy = sqrt(M[0] * M[0] + M[4] * M[4]);
    if (sy >= 1e-6) { v[0] = atan2(M[9], M[10]); v[1] = atan2(-M[8], sy); v[2] = atan2(M[4], M[0]); }
    else { v[0] = atan2(-M[6], M[5]); v[1] = atan2(-M[8], sy); v[2] = 0.0; }
    v[3] = M[3]; v[4] = M[7]; v[5] = M[11];
}
// zeta and Js (row-major 6x6) of an edge from X^-1, pose_t, pose_s: rules 2 and 3
IBA_ICP_HD inline void edge_zeta_js(const double* Xi, const double* Pt, const double* Ps, double* zeta, double* Js) {
    double Ti[12], B[12], M[12];
    inv12(Pt, Ti);
    mul12(Xi, Ti, B);
    mul12(B, Ps, M);
    vec6_of(M, zeta);
    if (!Js) return;
    for (int k = 0; k < 3; ++k) {
        // Q = e_k x (rows of [R | t] of pose_s): G_k pose_s
        const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
        double Q[12];
        for (int c = 0; c < 4; ++c) { Q[k * 4 + c] = 0.0; Q[k1 * 4 + c] = -Ps[k2 * 4 + c]; Q[k2 * 4 + c] = Ps[k1 * 4 + c]; }
        double W[12];
        for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) W[r * 4 + c] = (B[r * 4] * Q[c] + B[r * 4 + 1] * Q[4 + c]) + B[r * 4 + 2] * Q[8 + c];
        Js[0 * 6 + k] = (W[9] - W[6]) * 0.5; Js[1 * 6 + k] = (W[2] - W[8]) * 0.5; Js[2 * 6 + k] = (W[4] - W[1]) * 0.5;
        Js[3 * 6 + k] = W[3]; Js[4 * 6 + k] = W[7]; Js[5 * 6 + k] = W[11];
    }
    for (int k = 3; k < 6; ++k) {
        Js[0 * 6 + k] = 0.0; Js[1 * 6 + k] = 0.0; Js[2 * 6 + k] = 0.0;
        Js[3 * 6 + k] = B[k - 3]; Js[4 * 6 + k] = B[4 + k - 3]; Js[5 * 6 + k] = B[8 + k - 3];
    }
}
// q = zeta^T L zeta and Lz = L zeta, sums ascending
IBA_ICP_HD inline double quad6(const double* L, const double* z, double* Lz) {
    double q = 0.0;
    for (int i = 0; i < 6; ++i) {
        double s = L[i * 6] * z[0];
        for (int j = 1; j < 6; ++j) s += L[i * 6 + j] * z[j];
        Lz[i] = s;
        q = i == 0 ? z[0] * s : q + z[i] * s;
    }
    return q;
}
IBA_ICP_HD inline double line_weight(double mu, double q) { const double den = mu + q; if (!(den != 0.0)) return 1.0; const double t = mu / den; return t * t; }

} }  // namespace iba::pgo

// Local-map point matching, the float decisions (include/iba_mi355x.h, rules L1, L2 and the acceptance of L4): ONE text for the kernels
// (iba_map_match_kernels.hpp), the host restatement (iba_map_match_host.hpp) and the sanitizer self-test (san/map_match_selftest.cpp, plain g++).
// float32 unless a cast says otherwise, every operation rounded, left to right as written, no contraction, nothing but + - x / sqrt and comparisons.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/iba_mi355x.h"

#if defined(__HIPCC__)
#define IBA_MAPM_HD __host__ __device__ inline
#else
#define IBA_MAPM_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace mapm {

constexpr int kMaxLevels = IBA_MAP_MATCH_MAX_LEVELS;
constexpr int kStatuses = IBA_MAP_MATCH_N_STATUS;

// what a job's points share: the pose, the camera centre formed from it, the intrinsics, the frame's bounds and the scale table
struct Camera {
    float T[12];
    float Ow[3];
    float fx, fy, cx, cy;
    float min_x, max_x, min_y, max_y;
    float th, view_cos_limit;
    int32_t n_levels;
    float sf[kMaxLevels];
};

struct View { int32_t status; float u, v, view_cos; int32_t level; };

IBA_MAPM_HD bool finite_f(float x) { return fabsf(x) <= 3.402823466e38f; }
// the correctly rounded float32 quotient: the double quotient of two floats rounds to it (53 >= 2 * 24 + 2), so it needs no compiler flag
IBA_MAPM_HD float div_f(float a, float b) { return (float)((double)a / (double)b); }

// L1: Ow_i = -((R_0i t_0 + R_1i t_1) + R_2i t_2)
IBA_MAPM_HD void camera_centre(const float* T, float* Ow) {
    for (int i = 0; i < 3; ++i) Ow[i] = -((T[i] * T[3] + T[4 + i] * T[7]) + T[8 + i] * T[11]);
}

// L1 for one point that is not skipped
IBA_MAPM_HD View frustum(const Camera& c, const float* P, const float* nrm, float min_dist, float max_dist) {
    View w{IBA_MAP_MATCH_IN_VIEW, 0.f, 0.f, 0.f, 0};
    const float* T = c.T;
    const float pcx = ((T[0] * P[0] + T[1] * P[1]) + T[2] * P[2]) + T[3];
    const float pcy = ((T[4] * P[0] + T[5] * P[1]) + T[6] * P[2]) + T[7];
    const float pcz = ((T[8] * P[0] + T[9] * P[1]) + T[10] * P[2]) + T[11];
    if (pcz < 0.0f) { w.status = IBA_MAP_MATCH_DEPTH; return w; }
    const float invz = div_f(1.0f, pcz);
    const float u = (c.fx * pcx) * invz + c.cx, v = (c.fy * pcy) * invz + c.cy;
    if (!finite_f(u) || !finite_f(v)) { w.status = IBA_MAP_MATCH_NOT_FINITE; return w; }
    if (u < c.min_x || u > c.max_x || v < c.min_y || v > c.max_y) { w.status = IBA_MAP_MATCH_BOUNDS; return w; }
    const float po0 = P[0] - c.Ow[0], po1 = P[1] - c.Ow[1], po2 = P[2] - c.Ow[2];
    const float dist = (float)sqrt(((double)po0 * (double)po0 + (double)po1 * (double)po1) + (double)po2 * (double)po2);
    if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) { w.status = IBA_MAP_MATCH_DISTANCE; return w; }
    const float view_cos = (float)((((double)po0 * (double)nrm[0] + (double)po1 * (double)nrm[1]) + (double)po2 * (double)nrm[2]) / (double)dist);
    if (!finite_f(view_cos) || view_cos < c.view_cos_limit) { w.status = IBA_MAP_MATCH_ANGLE; return w; }
    const float ratio = div_f(max_dist, dist);
    // the least n with ratio <= sf[n], n_levels - 1 where there is none (the table ascends, so the last n a descending walk meets is the least)
    int level = c.n_levels - 1;
    for (int n = c.n_levels - 2; n >= 0; --n)
        if (ratio <= c.sf[n]) level = n;
    w.u = u; w.v = v; w.view_cos = view_cos; w.level = level;
    return w;
}

// L2: the radius of an in-view point's window
IBA_MAPM_HD float query_radius(float view_cos, float th, float sf_level) {
    float r = ((double)view_cos > 0.998) ? 2.5f : 4.0f;
    if (th != 1.0f) r *= th;
    return r * sf_level;
}

// L4: the acceptance over the two lexicographic minima; a missing slot is (256, -1); `found` = the first slot is not missing
IBA_MAPM_HD bool accept(bool found, int best, int level1, int best2, int level2, int th_high, float nn_ratio) {
    if (!found || best > th_high) return false;
    return !(level1 == level2 && (float)best > nn_ratio * (float)best2);
}

}  // namespace mapm
}  // namespace iba

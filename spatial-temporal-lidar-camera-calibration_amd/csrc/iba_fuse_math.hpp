// Map-point fusion, the float decisions (include/iba_mi355x.h, rules F2-F5): ONE text for the kernels (iba_fuse_kernels.hpp), the host restatement
// (iba_fuse_host.hpp) and the sanitizer self-test (san/fuse_selftest.cpp, plain g++). Where a rule is literally L1's the text is
// iba_map_match_math.hpp's (Pc through the same sums, camera_centre, div_f, finite_f, the level's table walk); where Fuse writes another
// expression (the projection's association, the half-open image test, the angle test without a division, the radius, the chi2 gate) it is
// restated here. float32 unless a cast says otherwise, every operation rounded, left to right as written, no contraction.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_map_match_math.hpp"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace fuse {

constexpr int kMaxLevels = IBA_MAP_MATCH_MAX_LEVELS;
constexpr int kStatuses = IBA_FUSE_N_STATUS;
constexpr uint64_t kNoKey = ~0ull;             // F5: no eligible candidate

// what a job's points share: L1's camera (pose, centre, intrinsics, bounds, th, the angle limit, the scale table) and the gate's table
struct Camera {
    mapm::Camera c;
    float inv_sigma2[kMaxLevels];
};

struct View { int32_t status; float u, v, radius; int32_t level; };       // status IBA_FUSE_PICKED here means "in view": F5 settles it

// F2-F4 for one point that is not skipped
IBA_MAPM_HD View frustum(const Camera& cam, const float* P, const float* nrm, float min_dist, float max_dist) {
    View w{IBA_FUSE_PICKED, 0.f, 0.f, 0.f, 0};
    const mapm::Camera& c = cam.c;
    const float* T = c.T;
    const float pcx = ((T[0] * P[0] + T[1] * P[1]) + T[2] * P[2]) + T[3];
    const float pcy = ((T[4] * P[0] + T[5] * P[1]) + T[6] * P[2]) + T[7];
    const float pcz = ((T[8] * P[0] + T[9] * P[1]) + T[10] * P[2]) + T[11];
    if (pcz < 0.0f) { w.status = IBA_FUSE_DEPTH; return w; }
    const float invz = mapm::div_f(1.0f, pcz);
    const float x = pcx * invz, y = pcy * invz;
    const float u = c.fx * x + c.cx, v = c.fy * y + c.cy;
    if (!mapm::finite_f(u) || !mapm::finite_f(v)) { w.status = IBA_FUSE_NOT_FINITE; return w; }
    if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) { w.status = IBA_FUSE_BOUNDS; return w; }      // KeyFrame::IsInImage, half open
    const float po0 = P[0] - c.Ow[0], po1 = P[1] - c.Ow[1], po2 = P[2] - c.Ow[2];
    const float dist = (float)sqrt(((double)po0 * (double)po0 + (double)po1 * (double)po1) + (double)po2 * (double)po2);
    if (dist < 0.8f * min_dist || dist > 1.2f * max_dist) { w.status = IBA_FUSE_DISTANCE; return w; }
    const double dot = ((double)po0 * (double)nrm[0] + (double)po1 * (double)nrm[1]) + (double)po2 * (double)nrm[2];
    if (dot < (double)c.view_cos_limit * (double)dist) { w.status = IBA_FUSE_ANGLE; return w; }
    const float ratio = mapm::div_f(max_dist, dist);
    int level = c.n_levels - 1;                  // L1's table rule
    for (int n = c.n_levels - 2; n >= 0; --n)
        if (ratio <= c.sf[n]) level = n;
    w.u = u; w.v = v; w.level = level; w.radius = c.th * c.sf[level];
    return w;
}

// F5: the gate of one candidate
IBA_MAPM_HD bool gate_passes(float u, float v, float kp_x, float kp_y, float inv_sigma2, float chi2_mono) {
    const float ex = u - kp_x, ey = v - kp_y;
    const float e2 = ex * ex + ey * ey;
    return !((double)(e2 * inv_sigma2) > (double)chi2_mono);
}

IBA_MAPM_HD uint64_t pick_key(int dist, uint32_t pos) { return ((uint64_t)(uint32_t)dist << 32) | pos; }

}  // namespace fuse
}  // namespace iba

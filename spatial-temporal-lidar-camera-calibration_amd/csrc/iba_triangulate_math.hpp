// New-map-point creation, the float decisions (include/iba_mi355x.h, rules R1, R3-R6 and R8): ONE text for the kernels
// (iba_triangulate_kernels.hpp), the host restatement (iba_triangulate_host.hpp) and the sanitizer self-test (san/triangulate_selftest.cpp, plain
// g++). float32 unless a cast says otherwise, every operation rounded, left to right as written, no contraction, nothing but + - x / sqrt and
// comparisons. The 3 x 3 products and inverses and the Jacobi null vector are those of iba_twoview_math.hpp, Ow and the correctly rounded
// quotient those of iba_map_match_math.hpp.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_map_match_math.hpp"
#include "iba_twoview_math.hpp"

#if defined(__HIPCC__)
#define IBA_TRG_HD __host__ __device__ inline
#else
#define IBA_TRG_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace trg {

constexpr int kMaxLevels = IBA_TRIANGULATE_MAX_LEVELS;
constexpr int kStatuses = IBA_TRIANGULATE_N_STATUS;

using mapm::div_f;
using mapm::finite_f;

// what the slots of a keyframe share: the pose, the camera centre formed from it (L1), the intrinsics and their reciprocals
struct Kf {
    float T[12];
    float Ow[3];
    float fx, fy, cx, cy, invfx, invfy;
    float median_depth;
};

// the thresholds of a call, as the options give them
struct Gates { float min_baseline_ratio, max_cos_parallax, epipole_gate, chi2_line, chi2_mono; int32_t th_low; };

// what the keyframes of a job share
struct Scales {
    int32_t n_levels;
    float scale_factor;
    float sf[kMaxLevels], sigma2[kMaxLevels];
};

// R1: what the slots of a (job, neighbour) pair share
struct PairGeom { float F12[9]; float ex, ey; float baseline; int32_t skipped; };

IBA_TRG_HD void make_kf(const float* Tcw12, float fx, float fy, float cx, float cy, float median_depth, Kf& k) {
    for (int i = 0; i < 12; ++i) k.T[i] = Tcw12[i];
    mapm::camera_centre(k.T, k.Ow);
    k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy;
    k.invfx = div_f(1.0f, fx); k.invfy = div_f(1.0f, fy);
    k.median_depth = median_depth;
}

IBA_TRG_HD void rotation_of(const float* T, float* R) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[i * 3 + j] = T[i * 4 + j];
}

// R1 for the pair (current keyframe k1, neighbour k2)
IBA_TRG_HD void pair_prologue(const Kf& k1, const Kf& k2, float min_baseline_ratio, PairGeom& g) {
    const float b[3] = {k2.Ow[0] - k1.Ow[0], k2.Ow[1] - k1.Ow[1], k2.Ow[2] - k1.Ow[2]};
    g.baseline = (float)tv::norm3(b);
    g.skipped = ((double)div_f(g.baseline, k2.median_depth) < (double)min_baseline_ratio) ? 1 : 0;
    float R1[9], R2[9], R2t[9], R12[9], K1[9], K2[9], K1t[9], K1ti[9], K2i[9], tx[9], m1[9], m2[9], v[3];
    rotation_of(k1.T, R1); rotation_of(k2.T, R2);
    tv::transpose33(R2, R2t);
    tv::mul33(R1, R2t, R12);
    const float t2[3] = {k2.T[3], k2.T[7], k2.T[11]};
    tv::mul331(R12, t2, v);
    const float t12[3] = {-v[0] + k1.T[3], -v[1] + k1.T[7], -v[2] + k1.T[11]};
    tx[0] = 0.f; tx[1] = -t12[2]; tx[2] = t12[1];
    tx[3] = t12[2]; tx[4] = 0.f; tx[5] = -t12[0];
    tx[6] = -t12[1]; tx[7] = t12[0]; tx[8] = 0.f;
    tv::make_K(k1.fx, k1.fy, k1.cx, k1.cy, K1); tv::make_K(k2.fx, k2.fy, k2.cx, k2.cy, K2);
    tv::transpose33(K1, K1t);
    tv::inv33(K1t, K1ti); tv::inv33(K2, K2i);
    tv::mul33(K1ti, tx, m1);
    tv::mul33(m1, R12, m2);
    tv::mul33(m2, K2i, g.F12);
    // the epipole in image 2, literally: a C2z of zero gives an ex, ey that is not finite, and then R3's comparison is false
    float C2[3];
    tv::mul331(R2, k1.Ow, C2);
    C2[0] = C2[0] + t2[0]; C2[1] = C2[1] + t2[1]; C2[2] = C2[2] + t2[2];
    const float invz = div_f(1.0f, C2[2]);
    g.ex = k2.fx * C2[0] * invz + k2.cx;
    g.ey = k2.fy * C2[1] * invz + k2.cy;
}

// R3: the epipolar line of a query in image 2
struct Line { float a, b, c, den; };
IBA_TRG_HD Line epipolar_line(const float* F12, float x1, float y1) {
    Line l;
    l.a = x1 * F12[0] + y1 * F12[3] + F12[6];
    l.b = x1 * F12[1] + y1 * F12[4] + F12[7];
    l.c = x1 * F12[2] + y1 * F12[5] + F12[8];
    l.den = l.a * l.a + l.b * l.b;
    return l;
}

// R3: the two checks of a candidate at (x2, y2) whose octave has scale factor sf2 and sigma2 s2
IBA_TRG_HD bool candidate_passes(const Line& l, float ex, float ey, float x2, float y2, float sf2, float s2, float epipole_gate, float chi2_line) {
    const float dx = ex - x2, dy = ey - y2;
    if (dx * dx + dy * dy < epipole_gate * sf2) return false;
    const float num = l.a * x2 + l.b * y2 + l.c;
    if (l.den == 0.f) return false;
    const float dsqr = div_f(num * num, l.den);
    return (double)dsqr < (double)chi2_line * (double)s2;
}

// R3: the key whose minimum the walk yields: (distance, descending position)
IBA_TRG_HD uint64_t pick_key(int dist, uint32_t pos) { return ((uint64_t)(uint32_t)dist << 32) | (uint32_t)(0xFFFFFFFFu - pos); }
IBA_TRG_HD uint32_t pick_pos(uint64_t key) { return 0xFFFFFFFFu - (uint32_t)key; }

struct Outcome { int32_t status; float x[3]; };

IBA_TRG_HD float row_dot(const float* T, int r, const float* x) {
    return (float)((((double)T[4 * r] * (double)x[0] + (double)T[4 * r + 1] * (double)x[1]) + (double)T[4 * r + 2] * (double)x[2]) + (double)T[4 * r + 3]);
}

IBA_TRG_HD bool reprojection_fails(const Kf& k, const float* x, float z, float u, float v, float s2, float chi2_mono) {
    const float xc = row_dot(k.T, 0, x), yc = row_dot(k.T, 1, x);
    const float invz = (float)(1.0 / (double)z);
    const float pu = k.fx * xc * invz + k.cx, pv = k.fy * yc * invz + k.cy;
    const float ex = pu - u, ey = pv - v;
    return (double)(ex * ex + ey * ey) > (double)chi2_mono * (double)s2;
}

// R4-R6 for one match: (u1, v1, octave o1) of the current keyframe k1 against (u2, v2, o2) of the neighbour k2
IBA_TRG_HD Outcome triangulate(const Kf& k1, const Kf& k2, const Scales& sc, const Gates& gt, float u1, float v1, int o1, float u2, float v2, int o2) {
    Outcome out{IBA_TRIANGULATE_CREATED, {0.f, 0.f, 0.f}};
    // R4
    const float xn1[3] = {(u1 - k1.cx) * k1.invfx, (v1 - k1.cy) * k1.invfy, 1.0f};
    const float xn2[3] = {(u2 - k2.cx) * k2.invfx, (v2 - k2.cy) * k2.invfy, 1.0f};
    float R[9], Rt[9], ray1[3], ray2[3];
    rotation_of(k1.T, R); tv::transpose33(R, Rt); tv::mul331(Rt, xn1, ray1);
    rotation_of(k2.T, R); tv::transpose33(R, Rt); tv::mul331(Rt, xn2, ray2);
    const double dot = ((double)ray1[0] * (double)ray2[0] + (double)ray1[1] * (double)ray2[1]) + (double)ray1[2] * (double)ray2[2];
    const float cosr = (float)(dot / (tv::norm3(ray1) * tv::norm3(ray2)));
    if (!(cosr > 0.f && (double)cosr < (double)gt.max_cos_parallax)) { out.status = IBA_TRIANGULATE_PARALLAX; return out; }
    // R5
    double G[16], V[16];
    for (int j = 0; j < 4; ++j) {
        G[j] = (double)(xn1[0] * k1.T[8 + j] - k1.T[j]);
        G[4 + j] = (double)(xn1[1] * k1.T[8 + j] - k1.T[4 + j]);
        G[8 + j] = (double)(xn2[0] * k2.T[8 + j] - k2.T[j]);
        G[12 + j] = (double)(xn2[1] * k2.T[8 + j] - k2.T[4 + j]);
    }
    float h[4];
    (void)tv::null_vector<4, 4, 1, 1>(G, V, h);
    if (h[3] == 0.f) { out.status = IBA_TRIANGULATE_DEGENERATE; return out; }
    const float x[3] = {div_f(h[0], h[3]), div_f(h[1], h[3]), div_f(h[2], h[3])};
    if (!finite_f(x[0]) || !finite_f(x[1]) || !finite_f(x[2])) { out.status = IBA_TRIANGULATE_DEGENERATE; return out; }
    out.x[0] = x[0]; out.x[1] = x[1]; out.x[2] = x[2];
    // R6
    const float z1 = row_dot(k1.T, 2, x);
    if (z1 <= 0.f) { out.status = IBA_TRIANGULATE_DEPTH1; return out; }
    const float z2 = row_dot(k2.T, 2, x);
    if (z2 <= 0.f) { out.status = IBA_TRIANGULATE_DEPTH2; return out; }
    if (reprojection_fails(k1, x, z1, u1, v1, sc.sigma2[o1], gt.chi2_mono)) { out.status = IBA_TRIANGULATE_REPROJ1; return out; }
    if (reprojection_fails(k2, x, z2, u2, v2, sc.sigma2[o2], gt.chi2_mono)) { out.status = IBA_TRIANGULATE_REPROJ2; return out; }
    const float n1[3] = {x[0] - k1.Ow[0], x[1] - k1.Ow[1], x[2] - k1.Ow[2]}, n2[3] = {x[0] - k2.Ow[0], x[1] - k2.Ow[1], x[2] - k2.Ow[2]};
    const float dist1 = (float)tv::norm3(n1), dist2 = (float)tv::norm3(n2);
    if (dist1 == 0.f || dist2 == 0.f) { out.status = IBA_TRIANGULATE_ZERO_DIST; return out; }
    const float ratioDist = div_f(dist2, dist1), ratioOctave = div_f(sc.sf[o1], sc.sf[o2]), ratioFactor = 1.5f * sc.scale_factor;
    if (ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor) { out.status = IBA_TRIANGULATE_SCALE; return out; }
    return out;
}

// R8: the normal and the two distance bounds of a created point x (the current keyframe first)
IBA_TRG_HD void new_point(const Kf& k1, const Kf& k2, const Scales& sc, const float* x, int o1, float* normal, float* min_dist, float* max_dist) {
    const float d1[3] = {x[0] - k1.Ow[0], x[1] - k1.Ow[1], x[2] - k1.Ow[2]}, d2[3] = {x[0] - k2.Ow[0], x[1] - k2.Ow[1], x[2] - k2.Ow[2]};
    const double l1 = tv::norm3(d1), l2 = tv::norm3(d2);
    for (int i = 0; i < 3; ++i) {
        const float a = (float)((double)d1[i] / l1), b = (float)((double)d2[i] / l2);
        normal[i] = tv::canon((a + b) * 0.5f);
    }
    *max_dist = (float)l1 * sc.sf[o1];
    *min_dist = div_f(*max_dist, sc.sf[sc.n_levels - 1]);
}

}  // namespace trg
}  // namespace iba

// Map-point refresh, the decisions (include/iba_mi355x.h, rules S3-S5): ONE text for the kernels (iba_refresh_kernels.hpp), the host restatement
// (iba_refresh_host.hpp) and the sanitizer self-test (san/refresh_selftest.cpp, plain g++). float32 unless a cast says otherwise, every operation
// rounded, left to right as written, no contraction, nothing but + - x / sqrt and comparisons. Ow and the correctly rounded quotient are those of
// iba_map_match_math.hpp.
#pragma once
#include <cmath>
#include <cstdint>

#include "../../include/iba_mi355x.h"
#include "iba_map_match_math.hpp"

#if defined(__HIPCC__)
#define IBA_RFR_HD __host__ __device__ inline
#else
#define IBA_RFR_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace rfr {

constexpr int kMaxLevels = IBA_REFRESH_MAX_LEVELS;
constexpr int kMaxObs = IBA_REFRESH_MAX_OBS;
constexpr uint64_t kNoKey = ~0ull;

using mapm::div_f;

// what the observations of a keyframe share: the camera centre formed once from the pose (L1) and isBad()
struct KfRec { float Ow[3]; int32_t bad; };
// what S5 reads of the reference keyframe
struct KfScale { int32_t n_levels; float sf[kMaxLevels]; };

// S3: the 256-bit Hamming distance of two descriptors held as four 64-bit words
IBA_RFR_HD int hamming256(const uint64_t* a, const uint64_t* b) {
    return (__builtin_popcountll(a[0] ^ b[0]) + __builtin_popcountll(a[1] ^ b[1])) + (__builtin_popcountll(a[2] ^ b[2]) + __builtin_popcountll(a[3] ^ b[3]));
}

// S3: the rank of the median in a row of N distances, and the key whose minimum over the rows is the pick
IBA_RFR_HD int median_rank(int N) { return (N - 1) / 2; }
IBA_RFR_HD uint64_t pick_key(int median, uint32_t row) { return ((uint64_t)(uint32_t)median << 32) | row; }

// S4: |P - Ow| as L1 forms dist before its narrowing (float32 differences, squares and sums in double)
IBA_RFR_HD double length(const float* P, const float* Ow, float* po) {
    po[0] = P[0] - Ow[0]; po[1] = P[1] - Ow[1]; po[2] = P[2] - Ow[2];
    return sqrt(((double)po[0] * (double)po[0] + (double)po[1] * (double)po[1]) + (double)po[2] * (double)po[2]);
}

// S4: the term of one observation (R8's n_i); false where |PO| == 0 (S6)
IBA_RFR_HD bool term(const float* P, const float* Ow, float* t) {
    float po[3];
    const double l = length(P, Ow, po);
    if (l == 0.0) { t[0] = t[1] = t[2] = 0.f; return false; }
    for (int c = 0; c < 3; ++c) t[c] = (float)((double)po[c] / l);
    return true;
}

// S4: a component of the normal from the float32 sum of the n terms
IBA_RFR_HD float mean_of(float sum, int n) { return (float)((double)sum / (double)n); }

// S5: the two bounds from the reference keyframe's centre and the level of its keypoint
IBA_RFR_HD void distances(const float* P, const KfRec& kf, const KfScale& sc, int level, float* min_dist, float* max_dist) {
    float po[3];
    const float dist = (float)length(P, kf.Ow, po);
    *max_dist = dist * sc.sf[level];
    *min_dist = div_f(*max_dist, sc.sf[sc.n_levels - 1]);
}

}  // namespace rfr
}  // namespace iba

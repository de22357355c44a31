// Windowed ORB matching, the host half (include/iba_mi355x.h, rules M1-M9): the argument checks of iba_orb_match, the two query builders of the
// reference's call sites, the chunk planner, and the three float decisions the kernels share with the host (a keypoint's cell, the first and the last
// cell of a window), marked IBA_ORB_HD. No device code and no HIP type: the sanitizer self-test compiles this file with plain g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"
#include "iba_orb_host.hpp"

namespace iba {
namespace orbm {

constexpr int kCols = IBA_ORB_MATCH_GRID_COLS, kRows = IBA_ORB_MATCH_GRID_ROWS, kCells = kCols * kRows;
constexpr int kHisto = IBA_ORB_MATCH_HISTO;
constexpr float kMaxMagnitude = 1e6f;

// M2 along one axis: the cell of coordinate x, or -1. The range test is made on the rounded float: the same answer as the reference's (int) wherever
// that conversion is defined.
IBA_ORB_HD inline int cell_of(float x, float lo, float inv, int n) {
    const float p = roundf((x - lo) * inv);
    return (p >= 0.f && p < (float)n) ? (int)p : -1;
}
// M3 along one axis: the first cell max(0, floor(..)), n where the list is empty (also for a product that is not a number)
IBA_ORB_HD inline int window_first(float u, float lo, float r, float inv, int n) {
    const float p = floorf((u - lo - r) * inv);
    if (!(p < (float)n)) return n;
    return p < 0.f ? 0 : (int)p;
}
// the last cell min(n - 1, ceil(..)), -1 where the list is empty
IBA_ORB_HD inline int window_last(float u, float lo, float r, float inv, int n) {
    const float p = ceilf((u - lo + r) * inv);
    if (!(p >= 0.f)) return -1;
    return p > (float)(n - 1) ? n - 1 : (int)p;
}

inline std::string check_options(const iba_orb_match_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_orb_match_options)) return "opt->struct_size is not sizeof(iba_orb_match_options)";
    if (o->th_low < 0 || o->th_low > 256 || o->th_high < 0 || o->th_high > 256) return "th_low or th_high outside [0, 256]";
    if (!std::isfinite(o->nn_ratio) || !(o->nn_ratio > 0.f)) return "nn_ratio is not finite or <= 0";
    return "";
}

inline std::string check_frame(const iba_orb_frame& f) {
    if (f.n < 0 || f.n > IBA_ORB_MATCH_MAX_KEYPOINTS) return "n outside [0, " + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS) + "]";
    if (!std::isfinite(f.min_x) || !std::isfinite(f.max_x) || !std::isfinite(f.min_y) || !std::isfinite(f.max_y)) return "a bound is not finite";
    if (!(f.max_x > f.min_x) || !(f.max_y > f.min_y)) return "max <= min";
    if (f.n > 0 && (!f.xy || !f.octave || !f.angle || !f.desc)) return "a NULL array";
    for (int32_t i = 0; i < f.n; ++i) {
        if (!std::isfinite(f.xy[2 * i]) || !std::isfinite(f.xy[2 * i + 1])) return "keypoint " + std::to_string(i) + ": a position that is not finite";
        if (!std::isfinite(f.angle[i]) || f.angle[i] < 0.f || f.angle[i] > 360.f) return "keypoint " + std::to_string(i) + ": an angle that is not finite or outside [0, 360]";
    }
    return "";
}

inline std::string check_frames(const iba_orb_frame* frames, int32_t F) {
    if (!frames) return "frames is NULL";
    if (F < 1) return "F < 1";
    for (int32_t f = 0; f < F; ++f) {
        const std::string why = check_frame(frames[f]);
        if (!why.empty()) return "frame " + std::to_string(f) + ": " + why;
    }
    return "";
}

// the per-query arrays, wherever they come from (a job's, or a builder's outputs)
inline std::string check_queries(int32_t n, const float* centre_xy, const float* radius, const int32_t* level_range, const int32_t* query_index, int32_t n_query_kp) {
    if (n < 0) return "n_queries < 0";
    if (n > 0 && (!centre_xy || !radius || !level_range || !query_index)) return "a NULL array";
    for (int32_t q = 0; q < n; ++q) {
        const float u = centre_xy[2 * q], v = centre_xy[2 * q + 1], r = radius[q];
        if (!std::isfinite(u) || !std::isfinite(v) || !std::isfinite(r)) return "query " + std::to_string(q) + ": a centre or radius that is not finite";
        if (r < 0.f) return "query " + std::to_string(q) + ": r < 0";
        if (std::fabs(u) > kMaxMagnitude || std::fabs(v) > kMaxMagnitude || r > kMaxMagnitude) return "query " + std::to_string(q) + ": a magnitude above 1e6";
        if (query_index[q] < 0 || query_index[q] >= n_query_kp) return "query " + std::to_string(q) + ": query_index outside the query frame";
    }
    return "";
}

inline std::string check_jobs(const iba_orb_frame* frames, int32_t F, const iba_orb_match_job* jobs, int32_t J) {
    if (!jobs) return "jobs is NULL";
    if (J < 1) return "J < 1";
    for (int32_t j = 0; j < J; ++j) {
        const iba_orb_match_job& b = jobs[j];
        const std::string who = "job " + std::to_string(j) + ": ";
        if (b.query_frame < 0 || b.query_frame >= F || b.train_frame < 0 || b.train_frame >= F) return who + "a frame index outside the call's frames";
        if (b.rule != IBA_ORB_MATCH_INIT && b.rule != IBA_ORB_MATCH_CLAIM) return who + "an unknown rule";
        const std::string why = check_queries(b.n_queries, b.centre_xy, b.radius, b.level_range, b.query_index, frames[b.query_frame].n);
        if (!why.empty()) return who + why;
    }
    return "";
}

// SearchForInitialization's queries
inline std::string init_queries(const iba_orb_frame* f, const float* prev_xy, int32_t window_size, float* centre_xy, float* radius, int32_t* level_range, int32_t* query_index, uint8_t* valid) {
    if (!f) return "frame1 is NULL";
    const std::string why = check_frame(*f);
    if (!why.empty()) return "frame1: " + why;
    if (window_size < 0 || (float)window_size > kMaxMagnitude) return "window_size outside [0, 1e6]";
    if (f->n > 0 && (!prev_xy || !centre_xy || !radius || !level_range || !query_index || !valid)) return "a NULL array";
    for (int32_t i = 0; i < f->n; ++i) {
        centre_xy[2 * i] = prev_xy[2 * i]; centre_xy[2 * i + 1] = prev_xy[2 * i + 1];
        radius[i] = (float)window_size;
        level_range[2 * i] = 0; level_range[2 * i + 1] = 0;
        query_index[i] = i;
        valid[i] = f->octave[i] == 0 ? 1 : 0;
    }
    return "";
}

// SearchByProjection(CurrentFrame, LastFrame, th, bMono = true)'s queries
inline std::string motion_queries(const iba_orb_frame* f, const uint8_t* has_point, const uint8_t* outlier, const float* X, const float* T, float fx, float fy, float cx, float cy,
                                  const float* bounds, const float* sf, int32_t n_sf, float th, float* centre_xy, float* radius, int32_t* level_range, int32_t* query_index, uint8_t* valid) {
    if (!f) return "last_frame is NULL";
    const std::string why = check_frame(*f);
    if (!why.empty()) return "last_frame: " + why;
    if (!T || !bounds || !sf) return "a NULL argument";
    if (n_sf < 1) return "n_scale_factors < 1";
    if (f->n > 0 && (!has_point || !outlier || !X || !centre_xy || !radius || !level_range || !query_index || !valid)) return "a NULL array";
    for (int32_t i = 0; i < f->n; ++i)
        if (f->octave[i] < 0 || f->octave[i] >= n_sf) return "keypoint " + std::to_string(i) + ": an octave outside scale_factors";
    const float min_x = bounds[0], max_x = bounds[1], min_y = bounds[2], max_y = bounds[3];
    for (int32_t i = 0; i < f->n; ++i) {
        centre_xy[2 * i] = centre_xy[2 * i + 1] = 0.f; radius[i] = 0.f;
        level_range[2 * i] = level_range[2 * i + 1] = 0;
        query_index[i] = i;
        valid[i] = 0;
        if (!has_point[i] || outlier[i]) continue;
        const float Xw = X[3 * i], Yw = X[3 * i + 1], Zw = X[3 * i + 2];
        const float xc = ((T[0] * Xw + T[1] * Yw) + T[2] * Zw) + T[3];
        const float yc = ((T[4] * Xw + T[5] * Yw) + T[6] * Zw) + T[7];
        const float zc = ((T[8] * Xw + T[9] * Yw) + T[10] * Zw) + T[11];
        const float invzc = (float)(1.0 / (double)zc);
        if (invzc < 0.f) continue;
        const float u = fx * xc * invzc + cx, v = fy * yc * invzc + cy;
        if (!std::isfinite(u) || !std::isfinite(v)) continue;
        if (u < min_x || u > max_x) continue;
        if (v < min_y || v > max_y) continue;
        const int32_t o = f->octave[i];
        centre_xy[2 * i] = u; centre_xy[2 * i + 1] = v;
        radius[i] = th * sf[o];
        level_range[2 * i] = o - 1; level_range[2 * i + 1] = o + 1;
        valid[i] = 1;
    }
    return "";
}

// the jobs' chunks under a byte budget: a chunk of consecutive jobs, at least one each
inline std::vector<int32_t> plan_chunks(const std::vector<int64_t>& candidates, uint64_t budget) {
    std::vector<uint64_t> bytes(candidates.size());
    for (size_t j = 0; j < candidates.size(); ++j) bytes[j] = IBA_ORB_MATCH_BYTES_PER_CANDIDATE * (uint64_t)candidates[j];
    return cut_chunks(bytes, budget);
}

}  // namespace orbm
}  // namespace iba

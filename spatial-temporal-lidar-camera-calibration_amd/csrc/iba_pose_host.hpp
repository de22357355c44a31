// Motion-only pose optimisation, the host half (include/iba_mi355x.h, iba_pose*): the argument checks, the result object, the host restatement of
// the whole call (iba_debug_pose_host: rules P1-P8 over the arithmetic the kernels compile, iba_pose_math.hpp) and iba_pose_edges_from_matches.
// Plain C++, no HIP: the sanitizer self-test (san/pose_selftest.cpp) compiles this file with g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_pose_math.hpp"

namespace iba {
namespace pose {

// what a job's workgroup leaves behind (the kernel writes this struct)
struct JobOut {
    iba_pose_result r;
    double stage[kMaxRounds * 12];   // the pose at the end of every round that ran
    int32_t big_steps, pad;          // P6: steps beyond theta = pi
};

inline float default_delta() { return (float)std::sqrt(5.991); }

inline std::string check_options(const iba_pose_options* o) {
    if (!o) return "options is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_pose_options)) return "options.struct_size is " + std::to_string(o->struct_size) + ", not " + std::to_string(sizeof(iba_pose_options));
    if (o->rounds < 1 || o->rounds > kMaxRounds) return "rounds " + std::to_string(o->rounds) + " is outside 1..8";
    if (o->iterations < 1 || o->iterations > 100) return "iterations " + std::to_string(o->iterations) + " is outside 1..100";
    if (!std::isfinite(o->chi2_threshold) || o->chi2_threshold < 0.f) return "chi2_threshold is not finite or < 0";
    if (!std::isfinite(o->huber_delta) || !(o->huber_delta > 0.f)) return "huber_delta is not finite or <= 0";
    if (o->robust_rounds < 0 || o->robust_rounds > kMaxRounds) return "robust_rounds " + std::to_string(o->robust_rounds) + " is outside 0..8";
    return "";
}

inline std::string check_jobs(const iba_pose_job* jobs, int32_t B) {
    if (!jobs) return "jobs is NULL";
    if (B < 1) return "B = " + std::to_string(B) + " < 1";
    for (int32_t j = 0; j < B; ++j) {
        const iba_pose_job& q = jobs[j];
        const std::string at = "job " + std::to_string(j) + ": ";
        if (q.n < 0 || q.n > IBA_ORB_MATCH_MAX_KEYPOINTS) return at + "n = " + std::to_string(q.n) + " is outside 0.." + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
        if (!q.Tcw12) return at + "Tcw12 is NULL";
        if (q.n && (!q.xyz || !q.obs || !q.inv_sigma2)) return at + "xyz, obs or inv_sigma2 is NULL";
        for (int k = 0; k < 12; ++k) if (!std::isfinite(q.Tcw12[k])) return at + "the pose is not finite";
        if (!std::isfinite(q.fx) || !std::isfinite(q.fy) || !(q.fx > 0.f) || !(q.fy > 0.f)) return at + "fx or fy is not finite or <= 0";
        if (!std::isfinite(q.cx) || !std::isfinite(q.cy)) return at + "cx or cy is not finite";
        for (int32_t i = 0; i < q.n; ++i) {
            const std::string e = at + "edge " + std::to_string(i) + ": ";
            if (!std::isfinite(q.xyz[3 * i]) || !std::isfinite(q.xyz[3 * i + 1]) || !std::isfinite(q.xyz[3 * i + 2])) return e + "the point is not finite";
            if (!std::isfinite(q.obs[2 * i]) || !std::isfinite(q.obs[2 * i + 1])) return e + "the observation is not finite";
            if (!std::isfinite(q.inv_sigma2[i])) return e + "inv_sigma2 is not finite";
            if (q.inv_sigma2[i] < 0.f) return e + "inv_sigma2 < 0";
        }
    }
    return "";
}

// ---- P3 on the host: the lanes' sums in ascending edge order, then the tree. active == nullptr: all. chi2_edges (n, or nullptr) takes every edge's chi2. ----
template <int FULL>
inline void host_sums(const iba_pose_job& q, const double* T, const uint8_t* active, int robust, double delta, double* sums, double* chi2_edges) {
    std::vector<double> acc((size_t)kLanes * kSums, 0.0);
    const Cam K{(double)q.fx, (double)q.fy, (double)q.cx, (double)q.cy};
    for (int32_t i = 0; i < q.n; ++i) {
        const double X = q.xyz[3 * i], Y = q.xyz[3 * i + 1], Z = q.xyz[3 * i + 2], ox = q.obs[2 * i], oy = q.obs[2 * i + 1], w = q.inv_sigma2[i];
        if (chi2_edges) { double ex, ey, c; edge(T, K, X, Y, Z, ox, oy, w, &ex, &ey, &c, nullptr); chi2_edges[i] = c; }
        if (active && !active[i]) continue;
        accumulate<FULL>(&acc[(size_t)(i % kLanes) * kSums], T, K, X, Y, Z, ox, oy, w, robust, delta);
    }
    for (int width = kLanes; width > 1; width /= 2)
        for (int l = 0; l < width / 2; ++l)
            for (int k = 0; k < kSums; ++k) acc[(size_t)l * kSums + k] = acc[(size_t)(2 * l) * kSums + k] + acc[(size_t)(2 * l + 1) * kSums + k];
    for (int k = 0; k < kSums; ++k) sums[k] = acc[k];
}

inline void start_out(const iba_pose_job& q, JobOut& o) {
    std::memset(&o, 0, sizeof(o));
    o.r.n = q.n;
    for (int k = 0; k < 12; ++k) { o.r.Tcw12[k] = q.Tcw12[k]; o.r.Tcw12f[k] = (float)q.Tcw12[k]; }
}

// ---- the whole schedule of one job on the host (P4-P8); outlier and chi2 take n entries ----
inline void host_job(const iba_pose_job& q, const iba_pose_options& opt, JobOut& o, uint8_t* outlier, float* chi2_out) {
    start_out(q, o);
    const int32_t n = q.n;
    for (int32_t i = 0; i < n; ++i) { outlier[i] = 0; chi2_out[i] = 0.f; }
    if (n < 3) return;                                // nInitialCorrespondences < 3
    const double delta = (double)opt.huber_delta;
    std::vector<uint8_t> active((size_t)n, 1);
    std::vector<double> chi2_now((size_t)n);
    double T[12], sums[kSums], trial[kSums] = {0.0};
    Lm s{};
    LmWork w{};
    int nbad = 0;
    for (int round = 0; round < opt.rounds; ++round) {
        const int robust = round < opt.robust_rounds ? 1 : 0;
        std::memcpy(T, q.Tcw12, sizeof(T));           // every round restarts from the start pose
        lm_round_start(&s);
        for (int phase = 0; phase != 2;) {
            if (phase == 0) host_sums<1>(q, T, active.data(), robust, delta, sums, nullptr);
            else host_sums<0>(q, w.Tn, active.data(), robust, delta, trial, nullptr);
            phase = lm_next(&s, &w, sums, trial[27], T, phase, opt.iterations);
        }
        // P7: every edge at the round's final accepted pose
        host_sums<0>(q, T, active.data(), robust, delta, trial, chi2_now.data());
        nbad = 0;
        for (int32_t i = 0; i < n; ++i) {
            const int bad = is_outlier(chi2_now[(size_t)i], opt.chi2_threshold);
            outlier[i] = (uint8_t)bad; active[(size_t)i] = (uint8_t)!bad; nbad += bad;
            chi2_out[i] = canonf((float)chi2_now[(size_t)i]);
        }
        o.r.chi2[round] = canon(s.current);
        o.r.n_bad[round] = nbad; o.r.lm_iterations[round] = s.its; o.r.trials[round] = s.trials;
        std::memcpy(o.stage + 12 * round, T, sizeof(T));
        o.r.rounds_run = round + 1;
        if (n < 10) break;                            // optimizer.edges().size() < 10
    }
    for (int k = 0; k < 12; ++k) { o.r.Tcw12[k] = T[k]; o.r.Tcw12f[k] = (float)T[k]; }
    o.r.n_inliers = n - nbad;
    o.big_steps = s.big;
}

// iba_pose_eval of one job on the host: H (36), b (6), the robust chi2 and, where asked for, every edge's chi2
inline void host_eval(const iba_pose_job& q, const uint8_t* active, int robust, double* H, double* b, double* chi2_robust, double* chi2_edges) {
    double sums[kSums];
    host_sums<1>(q, q.Tcw12, active, robust, (double)default_delta(), sums, chi2_edges);
    for (int r = 0; r < 6; ++r) for (int c = 0; c < 6; ++c) H[r * 6 + c] = canon(sums[r <= c ? hidx(r, c) : hidx(c, r)]);
    for (int k = 0; k < 6; ++k) b[k] = canon(sums[21 + k]);
    *chi2_robust = canon(sums[27]);
    if (chi2_edges) for (int32_t i = 0; i < q.n; ++i) chi2_edges[i] = canon(chi2_edges[i]);
}

// ---- iba_pose_edges_from_matches (P9) ----
inline std::string edges_from_matches(const int32_t* match, const int32_t* query_index, int32_t n_queries, const float* world_xyz, int32_t n_last, const float* cur_xy,
                                      const int32_t* cur_octave, int32_t n_cur, const float* inv_level_sigma2, int32_t n_levels, float* xyz, float* obs, float* inv_sigma2,
                                      int32_t* keypoint_index, int32_t* n_out) {
    if (!n_out) return "n is NULL";
    *n_out = 0;
    if (n_queries < 0 || n_last < 0 || n_cur < 0 || n_levels < 0) return "a negative count";
    if (n_queries > IBA_ORB_MATCH_MAX_KEYPOINTS || n_last > IBA_ORB_MATCH_MAX_KEYPOINTS || n_cur > IBA_ORB_MATCH_MAX_KEYPOINTS) return "a count above " + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
    if ((n_queries && !match) || (n_last && !world_xyz) || (n_cur && (!cur_xy || !cur_octave)) || (n_levels && !inv_level_sigma2)) return "a NULL input";
    if (n_cur && (!xyz || !obs || !inv_sigma2 || !keypoint_index)) return "a NULL output";
    std::vector<int32_t> point((size_t)n_cur, -1);    // mvpMapPoints of the current frame, as the last frame's keypoint
    for (int32_t q = 0; q < n_queries; ++q) {
        const int32_t c = match[q];
        if (c < 0) continue;
        if (c >= n_cur) return "match " + std::to_string(q) + " names keypoint " + std::to_string(c) + " of " + std::to_string(n_cur);
        const int32_t i = query_index ? query_index[q] : q;
        if (i < 0 || i >= n_last) return "query " + std::to_string(q) + " names keypoint " + std::to_string(i) + " of the last frame's " + std::to_string(n_last);
        point[(size_t)c] = i;                         // a later query overwrites, as the assignment does
    }
    int32_t n = 0;
    for (int32_t c = 0; c < n_cur; ++c) {
        const int32_t i = point[(size_t)c];
        if (i < 0) continue;
        const int32_t oct = cur_octave[c];
        if (oct < 0 || oct >= n_levels) return "keypoint " + std::to_string(c) + " has octave " + std::to_string(oct) + " of " + std::to_string(n_levels) + " levels";
        for (int k = 0; k < 3; ++k) xyz[3 * n + k] = world_xyz[3 * i + k];
        obs[2 * n] = cur_xy[2 * c]; obs[2 * n + 1] = cur_xy[2 * c + 1];
        inv_sigma2[n] = inv_level_sigma2[oct];
        keypoint_index[n] = c;
        ++n;
    }
    *n_out = n;
    return "";
}

}  // namespace pose
}  // namespace iba

struct iba_pose_batch {
    iba_pose_options opt{};
    std::vector<iba::pose::JobOut> job;
    std::vector<std::vector<uint8_t>> outlier;
    std::vector<std::vector<float>> chi2;
    float kernel_ms = 0.f;
    int32_t chunks = 0;
};

// Local-map point matching, the host half (include/iba_mi355x.h, rules L1-L6): the argument checks of iba_map_match, the job record the kernels
// read, the result's layout, the whole call restated on the host (iba_debug_map_match_host: L1 / L2 through iba_map_match_math.hpp, M2 / M3 through
// the matcher's cell and window rules, L4 as the two lexicographic minima) and iba_map_match_pose_edges. No device code and no HIP type: the
// sanitizer self-test compiles this file with plain g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"
#include "iba_map_match_math.hpp"
#include "iba_orb_match_host.hpp"

namespace iba {
namespace mapm {

constexpr float kMaxMagnitude = 1e6f;
constexpr uint64_t kNoKey = ~0ull;             // a missing slot of L4: no candidate

// what the kernels read of a job
struct JobRec {
    Camera cam;
    int32_t frame;
    int32_t q0, nq;            // the job's slots in the call's flat table
    int32_t kp_base, n_kp;     // the frame's keypoints in the call's flat table
    int32_t occ_base;          // into the call's flat occupied bytes, or -1: none is occupied
    int32_t kpo_base;          // into the call's flat point_of
    int32_t pad;
};

struct JobRes {
    size_t slot_base = 0, kpo_base = 0, cand_base = 0;
    int32_t n_kp = 0;
    iba_map_match_counts counts{};
};

// what iba_map_matches holds: host memory, one entry per slot (job, list position) or per (job, keypoint)
struct Result {
    iba_map_match_options opt{};
    std::vector<JobRes> job;
    std::vector<uint8_t> status;
    std::vector<float> u, v, view_cos, radius;
    std::vector<int32_t> level, match, dist, point_of;
    int32_t n_chunks = 0;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};       // IBA_MAP_MATCH_TIMING (debug): frustum, grid + list count, scan + list write, resolve
    // keep_stages
    std::vector<int32_t> off, cand;           // per job n_points + 1 offsets; the candidates of all jobs
    std::vector<uint16_t> cand_dist;
    void size_for(uint64_t n_slots, uint64_t n_kpo, int32_t J) {
        status.assign((size_t)n_slots, (uint8_t)IBA_MAP_MATCH_SKIPPED);
        u.assign((size_t)n_slots, 0.f); v.assign((size_t)n_slots, 0.f); view_cos.assign((size_t)n_slots, 0.f); radius.assign((size_t)n_slots, 0.f);
        level.assign((size_t)n_slots, 0); match.assign((size_t)n_slots, -1); dist.assign((size_t)n_slots, -1); point_of.assign((size_t)n_kpo, -1);
        if (opt.keep_stages) off.assign((size_t)n_slots + (size_t)J, 0);
    }
};

inline bool ok_f(float x) { return std::isfinite(x) && std::fabs(x) <= kMaxMagnitude; }
inline const char* why_f(float x) { return std::isfinite(x) ? "a magnitude above 1e6" : "a value that is not finite"; }

inline std::string check_options(const iba_map_match_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_map_match_options)) return "opt->struct_size is not sizeof(iba_map_match_options)";
    if (o->th_high < 0 || o->th_high > 256) return "th_high outside [0, 256]";
    if (!std::isfinite(o->nn_ratio) || !(o->nn_ratio > 0.f)) return "nn_ratio is not finite or <= 0";
    if (!std::isfinite(o->view_cos_limit)) return "view_cos_limit is not finite";
    return "";
}

inline std::string check_points(const iba_map_points* p) {
    if (!p) return "points is NULL";
    if (p->n < 0) return "points: n < 0";
    if (p->n > 0 && (!p->xyz || !p->normal || !p->min_dist || !p->max_dist || !p->desc)) return "points: a NULL array";
    for (int32_t i = 0; i < p->n; ++i) {
        const std::string who = "point " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; ++k) {
            if (!ok_f(p->xyz[3 * i + k])) return who + "xyz: " + why_f(p->xyz[3 * i + k]);
            if (!ok_f(p->normal[3 * i + k])) return who + "normal: " + why_f(p->normal[3 * i + k]);
        }
        if (!ok_f(p->min_dist[i])) return who + "min_dist: " + why_f(p->min_dist[i]);
        if (!ok_f(p->max_dist[i])) return who + "max_dist: " + why_f(p->max_dist[i]);
    }
    return "";
}

inline std::string check_jobs(const iba_orb_frame* frames, int32_t F, int32_t P, const iba_map_match_job* jobs, int32_t J) {
    if (!jobs) return "jobs is NULL";
    if (J < 1) return "J < 1";
    for (int32_t j = 0; j < J; ++j) {
        const iba_map_match_job& b = jobs[j];
        const std::string who = "job " + std::to_string(j) + ": ";
        if (b.frame < 0 || b.frame >= F) return who + "a frame index outside the call's frames";
        if (!b.Tcw12 || !b.scale_factors) return who + "Tcw12 or scale_factors is NULL";
        for (int k = 0; k < 12; ++k)
            if (!ok_f(b.Tcw12[k])) return who + "Tcw12: " + why_f(b.Tcw12[k]);
        const float K[4] = {b.fx, b.fy, b.cx, b.cy};
        for (int k = 0; k < 4; ++k)
            if (!ok_f(K[k])) return who + "an intrinsic: " + why_f(K[k]);
        if (!ok_f(b.th)) return who + "th: " + why_f(b.th);
        if (b.n_levels < 1 || b.n_levels > kMaxLevels) return who + "n_levels outside [1, " + std::to_string(kMaxLevels) + "]";
        for (int32_t n = 0; n < b.n_levels; ++n) {
            if (!ok_f(b.scale_factors[n])) return who + "scale_factors: " + why_f(b.scale_factors[n]);
            if (n == 0 ? b.scale_factors[0] != 1.0f : !(b.scale_factors[n] > b.scale_factors[n - 1])) return who + "scale_factors does not ascend from 1";
        }
        if (b.n_points < 0) return who + "n_points < 0";
        if (!b.points && b.n_points != P) return who + "points is NULL and n_points is not the table's " + std::to_string(P);
        if (b.points)
            for (int32_t k = 0; k < b.n_points; ++k)
                if (b.points[k] < 0 || b.points[k] >= P) return who + "points[" + std::to_string(k) + "] outside the table";
    }
    return "";
}

// the camera of a job: its arguments, the frame's bounds, Ow formed once
inline Camera make_camera(const iba_orb_frame& f, const iba_map_match_job& b, const iba_map_match_options& opt) {
    Camera c{};
    std::memcpy(c.T, b.Tcw12, sizeof(c.T));
    camera_centre(c.T, c.Ow);
    c.fx = b.fx; c.fy = b.fy; c.cx = b.cx; c.cy = b.cy;
    c.min_x = f.min_x; c.max_x = f.max_x; c.min_y = f.min_y; c.max_y = f.max_y;
    c.th = b.th; c.view_cos_limit = opt.view_cos_limit; c.n_levels = b.n_levels;
    for (int32_t n = 0; n < b.n_levels; ++n) c.sf[n] = b.scale_factors[n];
    return c;
}

// the jobs' chunks under a byte budget: a chunk of consecutive jobs, at least one each
inline std::vector<int32_t> plan_chunks(const std::vector<int64_t>& candidates, uint64_t budget) {
    std::vector<uint64_t> bytes(candidates.size());
    for (size_t j = 0; j < candidates.size(); ++j) bytes[j] = IBA_MAP_MATCH_BYTES_PER_CANDIDATE * (uint64_t)candidates[j];
    return cut_chunks(bytes, budget);
}

// ---- M2 / M3 / M4 on the host ----
struct HostGrid { std::vector<int32_t> off, list; float inv_w = 0.f, inv_h = 0.f; };

inline HostGrid host_grid(const iba_orb_frame& f) {
    HostGrid g;
    g.inv_w = 64.0f / (f.max_x - f.min_x); g.inv_h = 48.0f / (f.max_y - f.min_y);
    std::vector<int32_t> cell((size_t)f.n, -1);
    g.off.assign((size_t)orbm::kCells + 1, 0);
    for (int32_t i = 0; i < f.n; ++i) {
        const int px = orbm::cell_of(f.xy[2 * i], f.min_x, g.inv_w, orbm::kCols), py = orbm::cell_of(f.xy[2 * i + 1], f.min_y, g.inv_h, orbm::kRows);
        if (px < 0 || py < 0) continue;
        cell[(size_t)i] = px * orbm::kRows + py;
        ++g.off[(size_t)cell[(size_t)i] + 1];
    }
    for (int c = 0; c < orbm::kCells; ++c) g.off[(size_t)c + 1] += g.off[(size_t)c];
    g.list.resize((size_t)g.off[(size_t)orbm::kCells]);
    std::vector<int32_t> cursor(g.off.begin(), g.off.end() - 1);
    for (int32_t i = 0; i < f.n; ++i)
        if (cell[(size_t)i] >= 0) g.list[(size_t)cursor[(size_t)cell[(size_t)i]]++] = i;
    return g;
}

inline void host_area(const iba_orb_frame& f, const HostGrid& g, float u, float v, float r, int min_level, int max_level, std::vector<int32_t>& out) {
    out.clear();
    const int c0x = orbm::window_first(u, f.min_x, r, g.inv_w, orbm::kCols), c1x = orbm::window_last(u, f.min_x, r, g.inv_w, orbm::kCols);
    const int c0y = orbm::window_first(v, f.min_y, r, g.inv_h, orbm::kRows), c1y = orbm::window_last(v, f.min_y, r, g.inv_h, orbm::kRows);
    if (!(c0x < orbm::kCols && c1x >= 0 && c0y < orbm::kRows && c1y >= 0)) return;
    const bool check = min_level > 0 || max_level >= 0;
    for (int ix = c0x; ix <= c1x; ++ix)
        for (int e = g.off[(size_t)(ix * orbm::kRows + c0y)]; e < g.off[(size_t)(ix * orbm::kRows + c1y + 1)]; ++e) {
            const int32_t i = g.list[(size_t)e];
            if (check) {
                if (f.octave[i] < min_level) continue;
                if (max_level >= 0 && f.octave[i] > max_level) continue;
            }
            if (!(std::fabs(f.xy[2 * i] - u) < r && std::fabs(f.xy[2 * i + 1] - v) < r)) continue;
            out.push_back(i);
        }
}

inline int host_hamming(const uint8_t* a, const uint8_t* b) {
    int n = 0;
    for (int k = 0; k < 32; ++k) n += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return n;
}

// ---- the whole call on the host: the arguments have passed the checks; res->opt is set and res->job sized ----
inline void host_call(Result* res, const iba_orb_frame* frames, int32_t F, const iba_map_points* pts, const iba_map_match_job* jobs, int32_t J) {
    uint64_t n_slots = 0, n_kpo = 0;
    for (int32_t j = 0; j < J; ++j) { n_slots += (uint64_t)jobs[j].n_points; n_kpo += (uint64_t)frames[jobs[j].frame].n; }
    res->size_for(n_slots, n_kpo, J);
    std::vector<HostGrid> grids((size_t)F);
    std::vector<uint8_t> have((size_t)F, 0);
    std::vector<int32_t> cand;
    std::vector<uint8_t> claimed;
    size_t slot = 0, kpo = 0;
    for (int32_t j = 0; j < J; ++j) {
        const iba_map_match_job& b = jobs[j];
        const iba_orb_frame& f = frames[b.frame];
        if (!have[(size_t)b.frame]) { grids[(size_t)b.frame] = host_grid(f); have[(size_t)b.frame] = 1; }
        const HostGrid& g = grids[(size_t)b.frame];
        const Camera cam = make_camera(f, b, res->opt);
        JobRes& jr = res->job[(size_t)j];
        jr.slot_base = slot; jr.kpo_base = kpo; jr.cand_base = res->cand.size(); jr.n_kp = f.n;
        jr.counts = iba_map_match_counts{};
        jr.counts.n_points = b.n_points;
        claimed.assign((size_t)f.n, 0);
        if (b.occupied)
            for (int32_t i = 0; i < f.n; ++i) claimed[(size_t)i] = b.occupied[i] ? 1 : 0;
        int32_t* off = res->opt.keep_stages ? &res->off[slot + (size_t)j] : nullptr;
        int32_t n_cand = 0;
        for (int32_t k = 0; k < b.n_points; ++k, ++slot) {
            if (off) off[k + 1] = off[k];
            if (b.skip && b.skip[k]) { res->status[slot] = (uint8_t)IBA_MAP_MATCH_SKIPPED; ++jr.counts.status[IBA_MAP_MATCH_SKIPPED]; continue; }
            const int32_t p = b.points ? b.points[k] : k;
            const View w = frustum(cam, pts->xyz + 3 * (size_t)p, pts->normal + 3 * (size_t)p, pts->min_dist[p], pts->max_dist[p]);
            res->status[slot] = (uint8_t)w.status;
            ++jr.counts.status[w.status];
            if (w.status != IBA_MAP_MATCH_IN_VIEW) continue;
            const float r = query_radius(w.view_cos, cam.th, cam.sf[w.level]);
            res->u[slot] = w.u; res->v[slot] = w.v; res->view_cos[slot] = w.view_cos; res->level[slot] = w.level; res->radius[slot] = r;
            host_area(f, g, w.u, w.v, r, w.level - 1, w.level, cand);
            n_cand += (int32_t)cand.size();
            if (off) off[k + 1] += (int32_t)cand.size();
            uint64_t k1 = kNoKey, k2 = kNoKey;
            for (size_t e = 0; e < cand.size(); ++e) {
                const int d = host_hamming(pts->desc + 32 * (size_t)p, f.desc + 32 * (size_t)cand[e]);
                if (res->opt.keep_stages) { res->cand.push_back(cand[e]); res->cand_dist.push_back((uint16_t)d); }
                if (d >= 256 || claimed[(size_t)cand[e]]) continue;
                const uint64_t key = ((uint64_t)(uint32_t)d << 32) | (uint32_t)e;
                if (key < k1) { k2 = k1; k1 = key; }
                else if (key < k2) k2 = key;
            }
            const bool found = k1 != kNoKey;
            const int32_t c1 = found ? cand[(size_t)(uint32_t)k1] : -1, c2 = k2 != kNoKey ? cand[(size_t)(uint32_t)k2] : -1;
            const int best = found ? (int)(k1 >> 32) : 256, best2 = c2 >= 0 ? (int)(k2 >> 32) : 256;
            if (!accept(found, best, found ? f.octave[c1] : -1, best2, c2 >= 0 ? f.octave[c2] : -1, res->opt.th_high, res->opt.nn_ratio)) continue;
            claimed[(size_t)c1] = 1;
            res->match[slot] = c1; res->dist[slot] = best; res->point_of[kpo + (size_t)c1] = k;
            ++jr.counts.n_matches;
        }
        jr.counts.n_candidates = n_cand;
        kpo += (size_t)f.n;
    }
}

// ---- iba_map_match_pose_edges (L6) ----
inline std::string pose_edges(const int32_t* prior_point, const int32_t* point_of, const int32_t* points, int32_t n_points, const float* table_xyz, int32_t P, const float* xy,
                              const int32_t* octave, int32_t n_kp, const float* inv_level_sigma2, int32_t n_levels, float* xyz, float* obs, float* inv_sigma2, int32_t* keypoint_index,
                              int32_t* n_out) {
    if (!n_out) return "n is NULL";
    *n_out = 0;
    if (n_points < 0 || P < 0 || n_kp < 0 || n_levels < 0) return "a negative count";
    if (n_kp > IBA_ORB_MATCH_MAX_KEYPOINTS) return "a count above " + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
    if ((P && !table_xyz) || (n_kp && (!xy || !octave)) || (n_levels && !inv_level_sigma2)) return "a NULL input";
    if (!points && n_points != P) return "points is NULL and n_points is not the table's " + std::to_string(P);
    if (n_kp && (!xyz || !obs || !inv_sigma2 || !keypoint_index)) return "a NULL output";
    int32_t n = 0;
    for (int32_t c = 0; c < n_kp; ++c) {
        int32_t p = prior_point ? prior_point[c] : -1;
        if (p >= P) return "keypoint " + std::to_string(c) + " had point " + std::to_string(p) + " of " + std::to_string(P);
        const int32_t k = point_of ? point_of[c] : -1;
        if (k >= n_points) return "keypoint " + std::to_string(c) + " was claimed by list position " + std::to_string(k) + " of " + std::to_string(n_points);
        if (k >= 0) {                                  // the claim overwrites, as the reference's assignment does
            p = points ? points[k] : k;
            if (p < 0 || p >= P) return "points[" + std::to_string(k) + "] outside the table";
        }
        if (p < 0) continue;
        const int32_t oct = octave[c];
        if (oct < 0 || oct >= n_levels) return "keypoint " + std::to_string(c) + " has octave " + std::to_string(oct) + " of " + std::to_string(n_levels) + " levels";
        for (int d = 0; d < 3; ++d) xyz[3 * n + d] = table_xyz[3 * (size_t)p + d];
        obs[2 * n] = xy[2 * c]; obs[2 * n + 1] = xy[2 * c + 1];
        inv_sigma2[n] = inv_level_sigma2[oct];
        keypoint_index[n] = c;
        ++n;
    }
    *n_out = n;
    return "";
}

}  // namespace mapm
}  // namespace iba

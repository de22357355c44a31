// New-map-point creation, the host half (include/iba_mi355x.h, rules R1-R8): the argument checks of iba_triangulate, the records the kernels read,
// the node order of a keyframe (the host sort that goes up with the keyframes), the result's layout, the whole call restated on the host
// (iba_debug_triangulate_host: neighbour after neighbour with a has-point array updated after each, as the reference runs; R3 as the key minimum)
// and iba_triangulate_median_depth. No device code and no HIP type: the sanitizer self-test compiles this file with plain g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"
#include "iba_map_match_host.hpp"      // host_hamming
#include "iba_orb_match_host.hpp"      // check_frames
#include "iba_triangulate_math.hpp"

namespace iba {
namespace trg {

constexpr float kMaxMagnitude = 1e6f;
constexpr uint64_t kNoKey = ~0ull;
constexpr uint8_t kPending = 255;             // a slot the segment kernel hands to the pick kernel (never leaves the device)

// what the kernels read of a keyframe
struct KfRec {
    Kf kf;
    int32_t kp_base, n;        // the frame's keypoints in the call's flat keypoint tables
    int32_t kn_base, n_keys;   // the keyframe's rows in the per-keyframe tables (node, has_point: n rows; sorted keys: the first n_keys of n rows)
};
// a (job, neighbour) pair
struct PairRec { int32_t job, cur, nb, pos, slot_base, n_cur; };
// what the kernels read of a job
struct JobRec {
    Scales sc;
    int32_t cur, n_cur, n_nb;
    int32_t slot_base, pair_base, block_base, n_blocks;      // in the call's flat tables
    int32_t pad;
};
struct BlockRec { int32_t pair, first; };      // a block of slots: its pair and its first keypoint (blocks do not straddle a pair)

struct JobRes {
    size_t slot_base = 0, pair_base = 0, pt_base = 0;
    iba_triangulate_counts counts{};
};

// what iba_triangulation holds: host memory
struct Result {
    iba_triangulate_options opt{};
    std::vector<JobRes> job;
    std::vector<uint8_t> status;
    std::vector<int32_t> match, dist;
    std::vector<float> xyz;
    std::vector<int32_t> pair_matches, pair_created;
    std::vector<int32_t> p_idx1, p_nb, p_idx2;
    std::vector<float> p_xyz, p_normal, p_min, p_max;
    std::vector<uint8_t> p_desc;
    std::vector<int32_t> seg_len;              // keep_stages
    int32_t n_chunks = 0;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};        // IBA_TRIANGULATE_TIMING (debug)
    void size_for(uint64_t n_slots, uint64_t n_pairs) {
        status.assign((size_t)n_slots, 0); match.assign((size_t)n_slots, -1); dist.assign((size_t)n_slots, -1); xyz.assign(3 * (size_t)n_slots, 0.f);
        pair_matches.assign((size_t)n_pairs, 0); pair_created.assign((size_t)n_pairs, 0);
        if (opt.keep_stages) seg_len.assign((size_t)n_slots, 0);
    }
    void grow_points(size_t n) {
        p_idx1.resize(n); p_nb.resize(n); p_idx2.resize(n); p_xyz.resize(3 * n); p_normal.resize(3 * n); p_min.resize(n); p_max.resize(n); p_desc.resize(32 * n);
    }
};

inline bool ok_f(float x) { return std::isfinite(x) && std::fabs(x) <= kMaxMagnitude; }
inline const char* why_f(float x) { return std::isfinite(x) ? "a magnitude above 1e6" : "a value that is not finite"; }

inline std::string check_options(const iba_triangulate_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_triangulate_options)) return "opt->struct_size is not sizeof(iba_triangulate_options)";
    if (o->th_low < 0 || o->th_low > 256) return "th_low outside [0, 256]";
    const float t[5] = {o->min_baseline_ratio, o->max_cos_parallax, o->epipole_gate, o->chi2_line, o->chi2_mono};
    const char* name[5] = {"min_baseline_ratio", "max_cos_parallax", "epipole_gate", "chi2_line", "chi2_mono"};
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(t[k])) return std::string(name[k]) + " is not finite";
    return "";
}

inline std::string check_keyframes(const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* kfs, int32_t K) {
    if (!kfs) return "keyframes is NULL";
    if (K < 1) return "K < 1";
    for (int32_t k = 0; k < K; ++k) {
        const iba_triangulate_keyframe& a = kfs[k];
        const std::string who = "keyframe " + std::to_string(k) + ": ";
        if (a.frame < 0 || a.frame >= F) return who + "a frame index outside the call's frames";
        if (!a.Tcw12) return who + "Tcw12 is NULL";
        if (frames[a.frame].n > 0 && !a.node) return who + "node is NULL";
        for (int i = 0; i < 12; ++i)
            if (!ok_f(a.Tcw12[i])) return who + "Tcw12: " + why_f(a.Tcw12[i]);
        const float in[4] = {a.fx, a.fy, a.cx, a.cy};
        for (int i = 0; i < 4; ++i)
            if (!ok_f(in[i])) return who + "an intrinsic: " + why_f(in[i]);
    }
    return "";
}

inline std::string check_jobs(const iba_orb_frame* frames, const iba_triangulate_keyframe* kfs, int32_t K, const iba_triangulate_job* jobs, int32_t J) {
    if (!jobs) return "jobs is NULL";
    if (J < 1) return "J < 1";
    std::vector<int32_t> seen((size_t)K, -1);
    for (int32_t j = 0; j < J; ++j) {
        const iba_triangulate_job& b = jobs[j];
        const std::string who = "job " + std::to_string(j) + ": ";
        if (b.current < 0 || b.current >= K) return who + "current outside the call's keyframes";
        if (b.n_neighbours < 0) return who + "n_neighbours < 0";
        if (b.n_neighbours > 0 && !b.neighbours) return who + "neighbours is NULL";
        if (!b.scale_factors || !b.level_sigma2) return who + "scale_factors or level_sigma2 is NULL";
        if (b.n_levels < 1 || b.n_levels > kMaxLevels) return who + "n_levels outside [1, " + std::to_string(kMaxLevels) + "]";
        for (int32_t n = 0; n < b.n_levels; ++n) {
            if (!ok_f(b.scale_factors[n])) return who + "scale_factors: " + why_f(b.scale_factors[n]);
            if (n == 0 ? b.scale_factors[0] != 1.0f : !(b.scale_factors[n] > b.scale_factors[n - 1])) return who + "scale_factors does not ascend from 1";
            if (!ok_f(b.level_sigma2[n])) return who + "level_sigma2: " + why_f(b.level_sigma2[n]);
            if (!(b.level_sigma2[n] > 0.f)) return who + "level_sigma2 <= 0";
        }
        if (!ok_f(b.scale_factor)) return who + "scale_factor: " + why_f(b.scale_factor);
        if (!(b.scale_factor > 0.f)) return who + "scale_factor <= 0";
        seen[(size_t)b.current] = j;
        for (int32_t i = 0; i <= b.n_neighbours; ++i) {           // the neighbours, then the current keyframe
            const bool is_cur = i == b.n_neighbours;
            const int32_t k = is_cur ? b.current : b.neighbours[i];
            if (!is_cur) {
                const std::string nb = who + "neighbour " + std::to_string(i);
                if (k < 0 || k >= K) return nb + " outside the call's keyframes";
                if (k == b.current) return nb + " is the current keyframe";
                if (seen[(size_t)k] == j) return nb + " is listed twice";
                seen[(size_t)k] = j;
                if (!std::isfinite(kfs[k].median_depth) || !(kfs[k].median_depth > 0.f)) return nb + ": median_depth is not finite or <= 0";
            }
            const iba_orb_frame& f = frames[kfs[k].frame];
            for (int32_t e = 0; e < f.n; ++e)
                if (f.octave[e] < 0 || f.octave[e] >= b.n_levels)
                    return who + "keyframe " + std::to_string(k) + ": keypoint " + std::to_string(e) + " has octave " + std::to_string(f.octave[e]) + " of " + std::to_string(b.n_levels) + " levels";
        }
    }
    return "";
}

inline KfRec make_kf_rec(const iba_triangulate_keyframe& a, int32_t kp_base, int32_t n, int32_t kn_base) {
    KfRec r{};
    make_kf(a.Tcw12, a.fx, a.fy, a.cx, a.cy, a.median_depth, r.kf);
    r.kp_base = kp_base; r.n = n; r.kn_base = kn_base; r.n_keys = 0;
    return r;
}

inline Scales make_scales(const iba_triangulate_job& b) {
    Scales s{};
    s.n_levels = b.n_levels; s.scale_factor = b.scale_factor;
    for (int32_t n = 0; n < b.n_levels; ++n) { s.sf[n] = b.scale_factors[n]; s.sigma2[n] = b.level_sigma2[n]; }
    return s;
}

inline Gates make_gates(const iba_triangulate_options& o) { return Gates{o.min_baseline_ratio, o.max_cos_parallax, o.epipole_gate, o.chi2_line, o.chi2_mono, o.th_low}; }

// the node order of a keyframe: its keypoints with node >= 0 sorted by (node, index). key[e] = the node, idx[e] = the keypoint, or ~keypoint where
// it has a point (a candidate that is walked past). Writes at most n entries; returns their number.
inline int32_t node_order(const int32_t* node, const uint8_t* has_point, int32_t n, int32_t* key, int32_t* idx) {
    std::vector<uint64_t> k;
    k.reserve((size_t)n);
    for (int32_t i = 0; i < n; ++i)
        if (node[i] >= 0) k.push_back(((uint64_t)(uint32_t)node[i] << 32) | (uint32_t)i);
    std::sort(k.begin(), k.end());
    for (size_t e = 0; e < k.size(); ++e) {
        const int32_t i = (int32_t)(uint32_t)k[e];
        key[e] = (int32_t)(k[e] >> 32);
        idx[e] = (has_point && has_point[i]) ? ~i : i;
    }
    return (int32_t)k.size();
}

// the segment [a, b) of `node` in n sorted keys
inline void segment_of(const int32_t* key, int32_t n, int32_t node, int32_t* a, int32_t* b) {
    *a = (int32_t)(std::lower_bound(key, key + n, node) - key);
    *b = (int32_t)(std::upper_bound(key, key + n, node) - key);
}

// the jobs' chunks under a byte budget: a chunk of consecutive jobs, at least one each
inline std::vector<int32_t> plan_chunks(const std::vector<int64_t>& slots, uint64_t budget) {
    std::vector<uint64_t> bytes(slots.size());
    for (size_t j = 0; j < slots.size(); ++j) bytes[j] = IBA_TRIANGULATE_BYTES_PER_SLOT * (uint64_t)slots[j];
    return cut_chunks(bytes, budget);
}

// KeyFrame::ComputeSceneMedianDepth(q)
inline std::string median_depth(const float* Tcw12, const float* xyz, int32_t n, int32_t q, float* out) {
    if (n < 1) return "n < 1";
    if (q < 1) return "q < 1";
    if (!Tcw12 || !xyz || !out) return "a NULL argument";
    std::vector<float> z((size_t)n);
    for (int32_t i = 0; i < n; ++i) {
        const double dot = ((double)Tcw12[8] * (double)xyz[3 * i] + (double)Tcw12[9] * (double)xyz[3 * i + 1]) + (double)Tcw12[10] * (double)xyz[3 * i + 2];
        z[(size_t)i] = (float)dot + Tcw12[11];
    }
    std::sort(z.begin(), z.end());
    *out = z[(size_t)((n - 1) / q)];
    return "";
}

// ---- the whole call on the host: the arguments have passed the checks; res->opt is set and res->job sized ----
inline void host_call(Result* res, const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* kfs, int32_t K, const iba_triangulate_job* jobs, int32_t J) {
    (void)F;
    const Gates gt = make_gates(res->opt);
    uint64_t n_slots = 0, n_pairs = 0;
    for (int32_t j = 0; j < J; ++j) { n_slots += (uint64_t)jobs[j].n_neighbours * (uint64_t)frames[kfs[jobs[j].current].frame].n; n_pairs += (uint64_t)jobs[j].n_neighbours; }
    res->size_for(n_slots, n_pairs);
    std::vector<KfRec> rec((size_t)K);
    std::vector<std::vector<int32_t>> key((size_t)K), idx((size_t)K);
    for (int32_t k = 0; k < K; ++k) {
        const int32_t n = frames[kfs[k].frame].n;
        rec[(size_t)k] = make_kf_rec(kfs[k], 0, n, 0);
        key[(size_t)k].resize((size_t)n); idx[(size_t)k].resize((size_t)n);
        rec[(size_t)k].n_keys = node_order(kfs[k].node, kfs[k].has_point, n, key[(size_t)k].data(), idx[(size_t)k].data());
    }
    size_t slot = 0, pair = 0;
    std::vector<uint8_t> got;
    for (int32_t j = 0; j < J; ++j) {
        const iba_triangulate_job& b = jobs[j];
        const iba_triangulate_keyframe& c = kfs[b.current];
        const iba_orb_frame& f1 = frames[c.frame];
        const KfRec& k1 = rec[(size_t)b.current];
        const Scales sc = make_scales(b);
        JobRes& jr = res->job[(size_t)j];
        jr.slot_base = slot; jr.pair_base = pair; jr.pt_base = res->p_idx1.size();
        jr.counts = iba_triangulate_counts{};
        jr.counts.n_keypoints = f1.n; jr.counts.n_neighbours = b.n_neighbours;
        got.assign((size_t)f1.n, 0);                               // the keypoints that got a point from an earlier neighbour of this job
        for (int32_t pos = 0; pos < b.n_neighbours; ++pos, ++pair) {
            const int32_t nb = b.neighbours[pos];
            const iba_orb_frame& f2 = frames[kfs[nb].frame];
            const KfRec& k2 = rec[(size_t)nb];
            PairGeom g;
            pair_prologue(k1.kf, k2.kf, gt.min_baseline_ratio, g);
            const size_t first = slot;
            for (int32_t i = 0; i < f1.n; ++i, ++slot) {
                const bool has = c.has_point && c.has_point[i];
                int32_t a = 0, e = 0;
                if (!g.skipped && !has && c.node[i] >= 0) segment_of(key[(size_t)nb].data(), k2.n_keys, c.node[i], &a, &e);
                if (res->opt.keep_stages) res->seg_len[slot] = e - a;
                int st;
                if (got[(size_t)i]) st = IBA_TRIANGULATE_SUPERSEDED;
                else if (g.skipped) st = IBA_TRIANGULATE_PAIR_SKIPPED;
                else if (has) st = IBA_TRIANGULATE_HAS_POINT;
                else if (a == e) st = IBA_TRIANGULATE_NO_NODE;
                else {
                    const float x1 = f1.xy[2 * i], y1 = f1.xy[2 * i + 1];
                    const Line l = epipolar_line(g.F12, x1, y1);
                    uint64_t best = kNoKey;
                    for (int32_t p = a; p < e; ++p) {
                        const int32_t i2 = idx[(size_t)nb][(size_t)p];
                        if (i2 < 0) continue;
                        const int d = mapm::host_hamming(f1.desc + 32 * (size_t)i, f2.desc + 32 * (size_t)i2);
                        if (d > gt.th_low) continue;
                        const uint64_t k = pick_key(d, (uint32_t)(p - a));
                        if (k >= best) continue;
                        const int o2 = f2.octave[i2];
                        if (candidate_passes(l, g.ex, g.ey, f2.xy[2 * i2], f2.xy[2 * i2 + 1], sc.sf[o2], sc.sigma2[o2], gt.epipole_gate, gt.chi2_line)) best = k;
                    }
                    if (best == kNoKey) st = IBA_TRIANGULATE_NO_MATCH;
                    else {
                        const int32_t i2 = idx[(size_t)nb][(size_t)a + (size_t)pick_pos(best)];
                        res->match[slot] = i2; res->dist[slot] = (int32_t)(best >> 32);
                        ++res->pair_matches[pair];
                        const Outcome o = triangulate(k1.kf, k2.kf, sc, gt, x1, y1, f1.octave[i], f2.xy[2 * i2], f2.xy[2 * i2 + 1], f2.octave[i2]);
                        st = o.status;
                        for (int d3 = 0; d3 < 3; ++d3) res->xyz[3 * slot + (size_t)d3] = o.x[d3];
                    }
                }
                res->status[slot] = (uint8_t)st;
                ++jr.counts.status[st];
            }
            // the points of this neighbour, in ascending idx1; from here on their keypoints have a point
            for (int32_t i = 0; i < f1.n; ++i) {
                const size_t s = first + (size_t)i;
                if (res->status[s] != IBA_TRIANGULATE_CREATED) continue;
                got[(size_t)i] = 1;
                const size_t at = res->p_idx1.size();
                res->grow_points(at + 1);
                res->p_idx1[at] = i; res->p_nb[at] = pos; res->p_idx2[at] = res->match[s];
                for (int d3 = 0; d3 < 3; ++d3) res->p_xyz[3 * at + (size_t)d3] = res->xyz[3 * s + (size_t)d3];
                new_point(k1.kf, k2.kf, sc, &res->xyz[3 * s], f1.octave[i], &res->p_normal[3 * at], &res->p_min[at], &res->p_max[at]);
                std::memcpy(&res->p_desc[32 * at], f1.desc + 32 * (size_t)i, 32);
                ++res->pair_created[pair];
            }
        }
        jr.counts.n_created = jr.counts.status[IBA_TRIANGULATE_CREATED];
    }
}

}  // namespace trg
}  // namespace iba

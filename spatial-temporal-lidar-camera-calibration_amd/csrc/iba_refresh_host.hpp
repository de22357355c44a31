// Map-point refresh, the host half (include/iba_mi355x.h, rules S1-S7): the argument checks of iba_refresh, the result's layout, the whole call
// restated on the host (iba_debug_refresh_host: S3 as a histogram of every row, S4 / S5 through iba_refresh_math.hpp) and the two helpers
// (iba_refresh_observations, iba_refresh_store). No device code and no HIP type: the sanitizer self-test compiles this file with plain g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_fuse_host.hpp"
#include "iba_map_match_host.hpp"
#include "iba_refresh_math.hpp"

namespace iba {
namespace rfr {

// the arguments of a call, as the C ABI takes them
struct Args {
    const iba_orb_frame* frames; int32_t F;
    const iba_refresh_keyframe* keyframes; int32_t K;
    const iba_map_points* points;
    const uint8_t* point_bad;
    const int32_t* ref_keyframe;
    const int32_t *obs_off, *obs_keyframe, *obs_keypoint;
    const int32_t* list; int32_t n;
    const iba_refresh_options* opt;
};

// what iba_refreshed holds: host memory, one entry per listed point
struct Result {
    iba_refresh_options opt{};
    iba_refresh_counts counts{};
    std::vector<int32_t> point;               // the copy of the list, for iba_refresh_store
    std::vector<uint8_t> status, desc_state, geo_state;
    std::vector<int32_t> best_obs, best_median, n_desc;
    std::vector<float> normal, min_dist, max_dist;
    std::vector<uint8_t> desc;
    float ms[3] = {0.f, 0.f, 0.f};            // IBA_REFRESH_TIMING (debug): the narrow, the wave and the block kernel
    // keep_stages: per listed point its observations' medians in the order of the FULL list, -1 for an observation of a bad keyframe
    std::vector<int32_t> med_off, median;
    // S1's defaults: every listed point as BAD / EMPTY would leave it, which is also "as given" for what a later rule keeps
    void size_for(const Args& a) {
        const size_t n = (size_t)a.n;
        point.resize(n);
        status.assign(n, (uint8_t)IBA_REFRESH_EMPTY); desc_state.assign(n, (uint8_t)IBA_REFRESH_DESC_NONE); geo_state.assign(n, (uint8_t)IBA_REFRESH_GEO_NONE);
        best_obs.assign(n, -1); best_median.assign(n, -1); n_desc.assign(n, 0);
        normal.resize(3 * n); min_dist.resize(n); max_dist.resize(n); desc.resize(32 * n);
        med_off.assign(n + 1, 0);
        const iba_map_points& t = *a.points;
        for (size_t s = 0; s < n; ++s) {
            const int32_t p = a.list ? a.list[s] : (int32_t)s;
            point[s] = p;
            std::memcpy(&normal[3 * s], t.normal + 3 * (size_t)p, 3 * sizeof(float));
            min_dist[s] = t.min_dist[p]; max_dist[s] = t.max_dist[p];
            std::memcpy(&desc[32 * s], t.desc + 32 * (size_t)p, 32);
            const int32_t len = a.obs_off[p + 1] - a.obs_off[p];
            status[s] = (uint8_t)((a.point_bad && a.point_bad[p]) ? IBA_REFRESH_BAD : len == 0 ? IBA_REFRESH_EMPTY : IBA_REFRESH_REFRESHED);
            med_off[s + 1] = med_off[s] + ((opt.keep_stages && status[s] == IBA_REFRESH_REFRESHED) ? len : 0);
        }
        median.assign((size_t)med_off[n], -1);
        counts = iba_refresh_counts{};
        counts.n_points = a.n;
        counts.n_rows = med_off[n];
    }
    // the counts that follow from the per-point outputs (the host restatement; the device counts them itself)
    void count_states(const iba_map_points& t) {
        for (size_t s = 0; s < point.size(); ++s) {
            ++counts.status[status[s]]; ++counts.desc_state[desc_state[s]]; ++counts.geo_state[geo_state[s]];
            if (desc_state[s] == IBA_REFRESH_DESC_PICKED && std::memcmp(&desc[32 * s], t.desc + 32 * (size_t)point[s], 32) != 0) ++counts.n_desc_changed;
        }
    }
};

using mapm::ok_f;
using mapm::why_f;

// every check of the call; *st is IBA_ERR_INVALID_ARG or, for S7's cap, IBA_ERR_UNSUPPORTED where the answer is not empty
inline std::string check(const Args& a, iba_status* st) {
    *st = IBA_ERR_INVALID_ARG;
    if (!a.opt) return "opt is NULL";
    if (a.opt->struct_size != (int32_t)sizeof(iba_refresh_options)) return "opt->struct_size is not sizeof(iba_refresh_options)";
    std::string why = orbm::check_frames(a.frames, a.F);
    if (!why.empty()) return why;
    if (!a.keyframes) return "keyframes is NULL";
    if (a.K < 1) return "K < 1";
    for (int32_t k = 0; k < a.K; ++k) {
        const iba_refresh_keyframe& b = a.keyframes[k];
        const std::string who = "keyframe " + std::to_string(k) + ": ";
        if (b.frame < 0 || b.frame >= a.F) return who + "a frame index outside the call's frames";
        if (!b.Tcw12 || !b.scale_factors) return who + "Tcw12 or scale_factors is NULL";
        for (int i = 0; i < 12; ++i)
            if (!ok_f(b.Tcw12[i])) return who + "Tcw12: " + why_f(b.Tcw12[i]);
        if (b.n_levels < 1 || b.n_levels > kMaxLevels) return who + "n_levels outside [1, " + std::to_string(kMaxLevels) + "]";
        for (int32_t n = 0; n < b.n_levels; ++n) {
            if (!ok_f(b.scale_factors[n])) return who + "scale_factors: " + why_f(b.scale_factors[n]);
            if (n == 0 ? b.scale_factors[0] != 1.0f : !(b.scale_factors[n] > b.scale_factors[n - 1])) return who + "scale_factors does not ascend from 1";
        }
    }
    why = mapm::check_points(a.points);
    if (!why.empty()) return why;
    const int32_t P = a.points->n;
    if (a.n < 0) return "n < 0";
    if (!a.list && a.n != P) return "list is NULL and n is not the table's " + std::to_string(P);
    if (!a.obs_off) return "obs_off is NULL";
    if (P > 0 && !a.ref_keyframe) return "ref_keyframe is NULL";
    if (a.obs_off[0] != 0) return "obs_off does not start at 0";
    for (int32_t p = 0; p < P; ++p)
        if (a.obs_off[p + 1] < a.obs_off[p]) return "obs_off descends at point " + std::to_string(p);
    if (a.obs_off[P] > 0 && (!a.obs_keyframe || !a.obs_keypoint)) return "obs_keyframe or obs_keypoint is NULL";
    std::vector<int32_t> seen((size_t)a.K, -1);
    for (int32_t p = 0; p < P; ++p)
        for (int32_t e = a.obs_off[p]; e < a.obs_off[p + 1]; ++e) {
            const std::string who = "point " + std::to_string(p) + ", observation " + std::to_string(e - a.obs_off[p]) + ": ";
            const int32_t k = a.obs_keyframe[e], i = a.obs_keypoint[e];
            if (k < 0 || k >= a.K) return who + "a keyframe outside the call's " + std::to_string(a.K);
            const iba_orb_frame& f = a.frames[a.keyframes[k].frame];
            if (i < 0 || i >= f.n) return who + "a keypoint outside its frame's " + std::to_string(f.n);
            if (seen[(size_t)k] == p) return who + "keyframe " + std::to_string(k) + " is listed twice";
            seen[(size_t)k] = p;
            if (f.octave[i] < 0 || f.octave[i] >= a.keyframes[k].n_levels)
                return who + "its keypoint has octave " + std::to_string(f.octave[i]) + " of " + std::to_string(a.keyframes[k].n_levels) + " levels";
        }
    for (int32_t s = 0; s < a.n; ++s) {
        const int32_t p = a.list ? a.list[s] : s;
        if (p < 0 || p >= P) return "list[" + std::to_string(s) + "] outside the table";
        if (a.ref_keyframe[p] < 0 || a.ref_keyframe[p] >= a.K) return "list[" + std::to_string(s) + "]: ref_keyframe outside the call's " + std::to_string(a.K);
    }
    uint64_t listed = 0;
    for (int32_t s = 0; s < a.n; ++s) {
        const int32_t p = a.list ? a.list[s] : s;
        listed += (uint64_t)(a.obs_off[p + 1] - a.obs_off[p]);
        if (a.obs_off[p + 1] - a.obs_off[p] > kMaxObs) {
            *st = IBA_ERR_UNSUPPORTED;
            return "list[" + std::to_string(s) + "] has " + std::to_string(a.obs_off[p + 1] - a.obs_off[p]) + " observations, above IBA_REFRESH_MAX_OBS";
        }
    }
    if (listed >= (1ull << 31)) { *st = IBA_ERR_UNSUPPORTED; return "the listed points hold 2^31 observations or more"; }
    return "";
}

// the tables the rules read of the keyframes: built once per call, by the device call and the host restatement alike
inline void make_keyframes(const Args& a, std::vector<KfRec>& kf, std::vector<KfScale>& sc) {
    kf.resize((size_t)a.K); sc.resize((size_t)a.K);
    for (int32_t k = 0; k < a.K; ++k) {
        const iba_refresh_keyframe& b = a.keyframes[k];
        mapm::camera_centre(b.Tcw12, kf[(size_t)k].Ow);
        kf[(size_t)k].bad = b.bad ? 1 : 0;
        sc[(size_t)k] = KfScale{};
        sc[(size_t)k].n_levels = b.n_levels;
        for (int32_t n = 0; n < b.n_levels; ++n) sc[(size_t)k].sf[n] = b.scale_factors[n];
    }
}

inline void load_words(const uint8_t* d, uint64_t* w) { std::memcpy(w, d, 32); }

// ---- the whole call on the host: the arguments have passed the checks; res->opt is set ----
inline void host_call(Result* res, const Args& a) {
    res->size_for(a);
    std::vector<KfRec> kf; std::vector<KfScale> sc;
    make_keyframes(a, kf, sc);
    const iba_map_points& t = *a.points;
    std::vector<uint64_t> words;
    std::vector<int32_t> pos;
    int32_t hist[257];
    for (size_t s = 0; s < res->point.size(); ++s) {
        if (res->status[s] != IBA_REFRESH_REFRESHED) continue;
        const int32_t p = res->point[s], e0 = a.obs_off[p], len = a.obs_off[p + 1] - e0;
        // S2 / S3
        words.clear(); pos.clear();
        for (int32_t k = 0; k < len; ++k) {
            const int32_t g = a.obs_keyframe[e0 + k];
            if (kf[(size_t)g].bad) continue;
            words.resize(words.size() + 4);
            load_words(a.frames[a.keyframes[g].frame].desc + 32 * (size_t)a.obs_keypoint[e0 + k], &words[words.size() - 4]);
            pos.push_back(k);
        }
        const int32_t N = (int32_t)pos.size();
        res->n_desc[s] = N;
        res->desc_state[s] = (uint8_t)(N ? IBA_REFRESH_DESC_PICKED : IBA_REFRESH_DESC_KEPT);
        if (N) {
            const int need = median_rank(N) + 1;
            uint64_t best = kNoKey;
            for (int32_t i = 0; i < N; ++i) {
                std::memset(hist, 0, sizeof(hist));
                for (int32_t j = 0; j < N; ++j) ++hist[hamming256(&words[4 * (size_t)i], &words[4 * (size_t)j])];
                int v = 0;
                for (int c = hist[0]; c < need; c += hist[v]) ++v;          // the least v with at least m + 1 entries <= v
                if (res->opt.keep_stages) res->median[(size_t)res->med_off[s] + (size_t)pos[(size_t)i]] = v;
                const uint64_t key = pick_key(v, (uint32_t)pos[(size_t)i]);
                if (key < best) best = key;
            }
            res->best_obs[s] = (int32_t)(uint32_t)best; res->best_median[s] = (int32_t)(best >> 32);
            std::memcpy(&res->desc[32 * s], a.frames[a.keyframes[a.obs_keyframe[e0 + res->best_obs[s]]].frame].desc + 32 * (size_t)a.obs_keypoint[e0 + res->best_obs[s]], 32);
        }
        // S4 - S6
        const float* X = t.xyz + 3 * (size_t)p;
        float sum[3] = {0.f, 0.f, 0.f}, tm[3];
        bool degenerate = false;
        int32_t kref = -1;
        for (int32_t k = 0; k < len; ++k) {
            const int32_t g = a.obs_keyframe[e0 + k];
            if (!term(X, kf[(size_t)g].Ow, tm)) degenerate = true;
            sum[0] = sum[0] + tm[0]; sum[1] = sum[1] + tm[1]; sum[2] = sum[2] + tm[2];
            if (kref < 0 && g == a.ref_keyframe[p]) kref = k;
        }
        if (degenerate) { res->geo_state[s] = (uint8_t)IBA_REFRESH_GEO_DEGENERATE; continue; }
        for (int c = 0; c < 3; ++c) res->normal[3 * s + (size_t)c] = mean_of(sum[c], len);
        if (kref < 0) { res->geo_state[s] = (uint8_t)IBA_REFRESH_GEO_NO_REF; continue; }
        const int32_t g = a.obs_keyframe[e0 + kref];
        distances(X, kf[(size_t)g], sc[(size_t)g], a.frames[a.keyframes[g].frame].octave[a.obs_keypoint[e0 + kref]], &res->min_dist[s], &res->max_dist[s]);
        res->geo_state[s] = (uint8_t)IBA_REFRESH_GEO_UPDATED;
    }
    res->count_states(t);
}

// ---- iba_refresh_observations: the CSR lists of every point from a fold's map, keyframes ascending ----
inline std::string observations(const iba_fuse_map* map, int32_t* obs_off, int32_t* obs_keyframe, int32_t* obs_keypoint) {
    const std::string why = fuse::check_map(map);
    if (!why.empty()) return why;
    const iba_fuse_map& m = *map;
    if (!obs_off) return "obs_off is NULL";
    const int32_t total = m.kp_off[m.K];
    if (total > 0 && (!obs_keyframe || !obs_keypoint)) return "obs_keyframe or obs_keypoint is NULL";
    std::vector<int32_t> cnt((size_t)m.P + 1, 0), last((size_t)m.P, -1);
    for (int32_t k = 0; k < m.K; ++k)
        for (int32_t i = m.kp_off[k]; i < m.kp_off[k + 1]; ++i) {
            const int32_t p = m.holder[i];
            if (p < 0) continue;
            if (last[(size_t)p] == k) return "map: point " + std::to_string(p) + " is held twice in keyframe " + std::to_string(k);
            last[(size_t)p] = k;
            ++cnt[(size_t)p + 1];
        }
    obs_off[0] = 0;
    for (int32_t p = 0; p < m.P; ++p) { obs_off[p + 1] = obs_off[p] + cnt[(size_t)p + 1]; cnt[(size_t)p + 1] = obs_off[p]; }
    for (int32_t k = 0; k < m.K; ++k)
        for (int32_t i = m.kp_off[k]; i < m.kp_off[k + 1]; ++i) {
            const int32_t p = m.holder[i];
            if (p < 0) continue;
            const int32_t e = cnt[(size_t)p + 1]++;
            obs_keyframe[e] = k; obs_keypoint[e] = i - m.kp_off[k];
        }
    return "";
}

// ---- iba_refresh_store: a result into the caller's table arrays by listed index ----
inline std::string store(const Result& r, int32_t P, float* normal, float* min_dist, float* max_dist, uint8_t* desc, uint8_t* descriptor_stale) {
    if (P < 0) return "P < 0";
    if (!r.point.empty() && (!normal || !min_dist || !max_dist || !desc)) return "a NULL array";
    for (size_t s = 0; s < r.point.size(); ++s)
        if (r.point[s] >= P) return "listed point " + std::to_string(r.point[s]) + " outside the table's " + std::to_string(P);
    for (size_t s = 0; s < r.point.size(); ++s) {
        if (r.status[s] != IBA_REFRESH_REFRESHED) continue;
        const size_t p = (size_t)r.point[s];
        std::memcpy(normal + 3 * p, &r.normal[3 * s], 3 * sizeof(float));
        min_dist[p] = r.min_dist[s]; max_dist[p] = r.max_dist[s];
        std::memcpy(desc + 32 * p, &r.desc[32 * s], 32);
        if (descriptor_stale) descriptor_stale[p] = 0;
    }
    return "";
}

}  // namespace rfr
}  // namespace iba

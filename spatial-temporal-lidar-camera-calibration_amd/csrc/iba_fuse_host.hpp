// Map-point fusion, the host half (include/iba_mi355x.h, rules F1-F6 and U1-U5): the argument checks of iba_fuse, the job record the kernels read,
// the result's layout, the whole call restated on the host (iba_debug_fuse_host: F2-F5 through iba_fuse_math.hpp, M2 / M3 through the host grid of
// iba_map_match_host.hpp, F5 as the lexicographic minimum) and the fold with its helpers (iba_fuse_apply, iba_fuse_skip, iba_fuse_candidates). No
// device code and no HIP type: the sanitizer self-test compiles this file with plain g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"
#include "iba_fuse_math.hpp"
#include "iba_map_match_host.hpp"

namespace iba {
namespace fuse {

// what the kernels read of a job
struct JobRec {
    Camera cam;
    int32_t frame;
    int32_t q0, nq;            // the job's slots in the call's flat table
    int32_t kp_base, n_kp;     // the frame's keypoints in the call's flat table
    int32_t pad[3];
};

struct JobRes {
    size_t slot_base = 0, cand_base = 0;
    int32_t n_kp = 0;
    iba_fuse_counts counts{};
};

// what iba_fusion holds: host memory, one entry per slot (job, list position)
struct Result {
    iba_fuse_options opt{};
    std::vector<JobRes> job;
    std::vector<int32_t> point;               // the copy of every job's list (a table index, or < 0), for the fold
    std::vector<uint8_t> status;
    std::vector<float> u, v, radius;
    std::vector<int32_t> level, match, dist;
    int32_t n_chunks = 0;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};       // IBA_FUSE_TIMING (debug): frustum, grid + list count, scan + list write, pick
    // keep_stages
    std::vector<int32_t> off, cand;           // per job n_points + 1 offsets; the candidates of all jobs
    std::vector<uint16_t> cand_dist;
    void size_for(uint64_t n_slots, int32_t J) {
        point.assign((size_t)n_slots, -1);
        status.assign((size_t)n_slots, (uint8_t)IBA_FUSE_SKIPPED);
        u.assign((size_t)n_slots, 0.f); v.assign((size_t)n_slots, 0.f); radius.assign((size_t)n_slots, 0.f);
        level.assign((size_t)n_slots, 0); match.assign((size_t)n_slots, -1); dist.assign((size_t)n_slots, -1);
        if (opt.keep_stages) off.assign((size_t)n_slots + (size_t)J, 0);
    }
};

inline std::string check_options(const iba_fuse_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_fuse_options)) return "opt->struct_size is not sizeof(iba_fuse_options)";
    if (o->th_low < 0 || o->th_low > 256) return "th_low outside [0, 256]";
    if (!std::isfinite(o->view_cos_limit)) return "view_cos_limit is not finite";
    if (!std::isfinite(o->chi2_mono)) return "chi2_mono is not finite";
    return "";
}

inline std::string check_jobs(const iba_orb_frame* frames, int32_t F, int32_t P, const iba_fuse_job* jobs, int32_t J) {
    using mapm::ok_f;
    using mapm::why_f;
    if (!jobs) return "jobs is NULL";
    if (J < 1) return "J < 1";
    for (int32_t j = 0; j < J; ++j) {
        const iba_fuse_job& b = jobs[j];
        const std::string who = "job " + std::to_string(j) + ": ";
        if (b.frame < 0 || b.frame >= F) return who + "a frame index outside the call's frames";
        if (!b.Tcw12 || !b.scale_factors || !b.inv_level_sigma2) return who + "Tcw12, scale_factors or inv_level_sigma2 is NULL";
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
            if (!ok_f(b.inv_level_sigma2[n])) return who + "inv_level_sigma2: " + why_f(b.inv_level_sigma2[n]);
            if (!(b.inv_level_sigma2[n] > 0.f)) return who + "inv_level_sigma2: a value <= 0";
        }
        const iba_orb_frame& f = frames[b.frame];
        for (int32_t i = 0; i < f.n; ++i)
            if (f.octave[i] < 0 || f.octave[i] >= b.n_levels)
                return who + "keypoint " + std::to_string(i) + " of its frame has octave " + std::to_string(f.octave[i]) + " of " + std::to_string(b.n_levels) + " levels";
        if (b.n_points < 0) return who + "n_points < 0";
        if (!b.points && b.n_points != P) return who + "points is NULL and n_points is not the table's " + std::to_string(P);
        if (b.points)
            for (int32_t k = 0; k < b.n_points; ++k)
                if (b.points[k] >= P) return who + "points[" + std::to_string(k) + "] outside the table";
    }
    return "";
}

// the camera of a job: its arguments, the frame's bounds, Ow formed once
inline Camera make_camera(const iba_orb_frame& f, const iba_fuse_job& b, const iba_fuse_options& opt) {
    Camera cam{};
    mapm::Camera& c = cam.c;
    std::memcpy(c.T, b.Tcw12, sizeof(c.T));
    mapm::camera_centre(c.T, c.Ow);
    c.fx = b.fx; c.fy = b.fy; c.cx = b.cx; c.cy = b.cy;
    c.min_x = f.min_x; c.max_x = f.max_x; c.min_y = f.min_y; c.max_y = f.max_y;
    c.th = b.th; c.view_cos_limit = opt.view_cos_limit; c.n_levels = b.n_levels;
    for (int32_t n = 0; n < b.n_levels; ++n) { c.sf[n] = b.scale_factors[n]; cam.inv_sigma2[n] = b.inv_level_sigma2[n]; }
    return cam;
}

// the jobs' chunks under a byte budget: a chunk of consecutive jobs, at least one each
inline std::vector<int32_t> plan_chunks(const std::vector<int64_t>& candidates, uint64_t budget) {
    std::vector<uint64_t> bytes(candidates.size());
    for (size_t j = 0; j < candidates.size(); ++j) bytes[j] = IBA_FUSE_BYTES_PER_CANDIDATE * (uint64_t)candidates[j];
    return cut_chunks(bytes, budget);
}

// ---- the whole call on the host: the arguments have passed the checks; res->opt is set and res->job sized ----
inline void host_call(Result* res, const iba_orb_frame* frames, int32_t F, const iba_map_points* pts, const iba_fuse_job* jobs, int32_t J) {
    uint64_t n_slots = 0;
    for (int32_t j = 0; j < J; ++j) n_slots += (uint64_t)jobs[j].n_points;
    res->size_for(n_slots, J);
    std::vector<mapm::HostGrid> grids((size_t)F);
    std::vector<uint8_t> have((size_t)F, 0);
    std::vector<int32_t> cand;
    size_t slot = 0;
    for (int32_t j = 0; j < J; ++j) {
        const iba_fuse_job& b = jobs[j];
        const iba_orb_frame& f = frames[b.frame];
        if (!have[(size_t)b.frame]) { grids[(size_t)b.frame] = mapm::host_grid(f); have[(size_t)b.frame] = 1; }
        const mapm::HostGrid& g = grids[(size_t)b.frame];
        const Camera cam = make_camera(f, b, res->opt);
        JobRes& jr = res->job[(size_t)j];
        jr.slot_base = slot; jr.cand_base = res->cand.size(); jr.n_kp = f.n;
        jr.counts = iba_fuse_counts{};
        jr.counts.n_points = b.n_points;
        int32_t* off = res->opt.keep_stages ? &res->off[slot + (size_t)j] : nullptr;
        int32_t n_cand = 0;
        for (int32_t k = 0; k < b.n_points; ++k, ++slot) {
            if (off) off[k + 1] = off[k];
            const int32_t p = b.points ? b.points[k] : k;
            res->point[slot] = p;
            int st = IBA_FUSE_SKIPPED;
            if (p >= 0 && !(b.skip && b.skip[k])) {
                const View w = frustum(cam, pts->xyz + 3 * (size_t)p, pts->normal + 3 * (size_t)p, pts->min_dist[p], pts->max_dist[p]);
                st = w.status;
                if (st == IBA_FUSE_PICKED) {
                    res->u[slot] = w.u; res->v[slot] = w.v; res->level[slot] = w.level; res->radius[slot] = w.radius;
                    mapm::host_area(f, g, w.u, w.v, w.radius, w.level - 1, w.level, cand);
                    n_cand += (int32_t)cand.size();
                    if (off) off[k + 1] += (int32_t)cand.size();
                    uint64_t best = kNoKey;
                    for (size_t e = 0; e < cand.size(); ++e) {
                        const int32_t c = cand[e];
                        const int d = mapm::host_hamming(pts->desc + 32 * (size_t)p, f.desc + 32 * (size_t)c);
                        if (res->opt.keep_stages) { res->cand.push_back(c); res->cand_dist.push_back((uint16_t)d); }
                        if (d >= 256) continue;
                        if (res->opt.check_reprojection && !gate_passes(w.u, w.v, f.xy[2 * c], f.xy[2 * c + 1], cam.inv_sigma2[f.octave[c]], res->opt.chi2_mono)) continue;
                        const uint64_t key = pick_key(d, (uint32_t)e);
                        if (key < best) best = key;
                    }
                    if (cand.empty()) st = IBA_FUSE_NO_CANDIDATE;
                    else if (best == kNoKey || (int)(best >> 32) > res->opt.th_low) st = IBA_FUSE_NO_MATCH;
                    else { res->match[slot] = cand[(size_t)(uint32_t)best]; res->dist[slot] = (int32_t)(best >> 32); }
                }
            }
            res->status[slot] = (uint8_t)st;
            ++jr.counts.status[st];
        }
        jr.counts.n_candidates = n_cand;
        jr.counts.n_picked = jr.counts.status[IBA_FUSE_PICKED];
    }
}

// ---- the fold (U1-U5) ----
struct Obs { int32_t kf, kp; };

inline std::string check_map(const iba_fuse_map* m) {
    if (!m) return "map is NULL";
    if (m->K < 0 || m->P < 0) return "map: K or P < 0";
    if (!m->kp_off) return "map: kp_off is NULL";
    if (m->kp_off[0] != 0) return "map: kp_off does not start at 0";
    for (int32_t k = 0; k < m->K; ++k)
        if (m->kp_off[k + 1] < m->kp_off[k]) return "map: kp_off descends";
    if (m->kp_off[m->K] > 0 && !m->holder) return "map: holder is NULL";
    if (m->P > 0 && (!m->bad || !m->replaced_by)) return "map: bad or replaced_by is NULL";
    for (int32_t i = 0; i < m->kp_off[m->K]; ++i)
        if (m->holder[i] < -1 || m->holder[i] >= m->P) return "map: holder[" + std::to_string(i) + "] outside [-1, P)";
    return "";
}

// U1: the point -> (keyframe, keypoint) index, built once; refuses a point held twice in one keyframe
inline std::string build_index(const iba_fuse_map& m, std::vector<std::vector<Obs>>& obs) {
    obs.assign((size_t)m.P, {});
    for (int32_t k = 0; k < m.K; ++k)
        for (int32_t i = m.kp_off[k]; i < m.kp_off[k + 1]; ++i) {
            const int32_t p = m.holder[i];
            if (p < 0) continue;
            std::vector<Obs>& o = obs[(size_t)p];
            if (!o.empty() && o.back().kf == k) return "map: point " + std::to_string(p) + " is held twice in keyframe " + std::to_string(k);
            o.push_back(Obs{k, i - m.kp_off[k]});
        }
    return "";
}

inline bool in_keyframe(const std::vector<Obs>& o, int32_t kf) {
    for (const Obs& x : o)
        if (x.kf == kf) return true;
    return false;
}

// U4
inline void replace(iba_fuse_map& m, std::vector<std::vector<Obs>>& obs, int32_t a, int32_t b) {
    std::vector<Obs> oa;
    oa.swap(obs[(size_t)a]);
    m.bad[a] = 1; m.replaced_by[a] = b;
    for (const Obs& x : oa) {
        int32_t& h = m.holder[m.kp_off[x.kf] + x.kp];
        if (in_keyframe(obs[(size_t)b], x.kf)) h = -1;
        else { h = b; obs[(size_t)b].push_back(x); }
    }
    if (m.found) m.found[b] += m.found[a];
    if (m.visible) m.visible[b] += m.visible[a];
    if (m.descriptor_stale) m.descriptor_stale[b] = 1;
}

// U2 / U3 over one job of a result
inline std::string apply(const Result& r, int32_t job, int32_t keyframe, iba_fuse_map* map, int32_t mode, int32_t* op, int32_t* other, int32_t* n_fused) {
    std::string why = check_map(map);
    if (!why.empty()) return why;
    iba_fuse_map& m = *map;
    if (keyframe < 0 || keyframe >= m.K) return "keyframe outside the map's " + std::to_string(m.K);
    if (mode != IBA_FUSE_LOCAL && mode != IBA_FUSE_LOOP) return "mode is neither IBA_FUSE_LOCAL nor IBA_FUSE_LOOP";
    const JobRes& jr = r.job[(size_t)job];
    const int32_t n = jr.counts.n_points, base = m.kp_off[keyframe];
    if (m.kp_off[keyframe + 1] - base != jr.n_kp)
        return "keyframe " + std::to_string(keyframe) + " has " + std::to_string(m.kp_off[keyframe + 1] - base) + " keypoints, the job's frame " + std::to_string(jr.n_kp);
    const int32_t* point = r.point.data() + jr.slot_base;
    for (int32_t k = 0; k < n; ++k)
        if (point[k] >= m.P) return "list position " + std::to_string(k) + " names point " + std::to_string(point[k]) + " of the map's " + std::to_string(m.P);
    std::vector<std::vector<Obs>> obs;
    why = build_index(m, obs);
    if (!why.empty()) return why;
    int32_t fused = 0;
    for (int32_t k = 0; k < n; ++k) {
        int32_t o = IBA_FUSE_OP_NONE, q = -1;
        if (r.status[jr.slot_base + (size_t)k] == IBA_FUSE_PICKED) {
            const int32_t p = point[k], mt = r.match[jr.slot_base + (size_t)k];
            if (m.bad[p]) o = IBA_FUSE_OP_STALE_BAD;
            else if (in_keyframe(obs[(size_t)p], keyframe)) o = IBA_FUSE_OP_STALE_IN_KEYFRAME;
            else {
                q = m.holder[base + mt];
                if (q < 0) { o = IBA_FUSE_OP_ADD; m.holder[base + mt] = p; obs[(size_t)p].push_back(Obs{keyframe, mt}); }
                else if (m.bad[q]) o = IBA_FUSE_OP_HELD_BAD;
                else if (mode == IBA_FUSE_LOOP) o = IBA_FUSE_OP_RECORD;
                else if (obs[(size_t)q].size() > obs[(size_t)p].size()) { o = IBA_FUSE_OP_REPLACED_BY_HELD; replace(m, obs, p, q); }
                else { o = IBA_FUSE_OP_REPLACES_HELD; replace(m, obs, q, p); }
                ++fused;
            }
        }
        if (op) op[k] = o;
        if (other) other[k] = q;
    }
    if (n_fused) *n_fused = fused;
    return "";
}

inline std::string skip_bytes(const iba_fuse_map* map, int32_t keyframe, const int32_t* points, int32_t n, uint8_t* skip) {
    const std::string why = check_map(map);
    if (!why.empty()) return why;
    if (keyframe < 0 || keyframe >= map->K) return "keyframe outside the map's " + std::to_string(map->K);
    if (n < 0 || (n > 0 && (!points || !skip))) return "n < 0 or a NULL array";
    std::vector<uint8_t> held((size_t)map->P, 0);
    for (int32_t i = map->kp_off[keyframe]; i < map->kp_off[keyframe + 1]; ++i)
        if (map->holder[i] >= 0) held[(size_t)map->holder[i]] = 1;
    for (int32_t k = 0; k < n; ++k) {
        const int32_t p = points[k];
        if (p >= map->P) return "points[" + std::to_string(k) + "] outside the map";
        skip[k] = (p < 0 || map->bad[p] || held[(size_t)p]) ? 1 : 0;
    }
    return "";
}

inline std::string candidates(const iba_fuse_map* map, const int32_t* targets, int32_t T, int32_t* points, int32_t* n_out) {
    if (!n_out) return "n is NULL";
    *n_out = 0;
    const std::string why = check_map(map);
    if (!why.empty()) return why;
    if (T < 0 || (T > 0 && !targets) || (map->P > 0 && !points)) return "T < 0 or a NULL array";
    std::vector<uint8_t> listed((size_t)map->P, 0);
    int32_t n = 0;
    for (int32_t t = 0; t < T; ++t) {
        const int32_t k = targets[t];
        if (k < 0 || k >= map->K) return "targets[" + std::to_string(t) + "] outside the map's " + std::to_string(map->K);
        for (int32_t i = map->kp_off[k]; i < map->kp_off[k + 1]; ++i) {
            const int32_t p = map->holder[i];
            if (p < 0 || map->bad[p] || listed[(size_t)p]) continue;
            listed[(size_t)p] = 1;
            points[n++] = p;
        }
    }
    *n_out = n;
    return "";
}

}  // namespace fuse
}  // namespace iba

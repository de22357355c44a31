// Bundle adjustment, the host half (include/iba_mi355x.h, iba_bundle*): the argument checks, the plan of a job (its per-point and per-camera edge
// lists, the blocks of its reduced system and their items), the flat tables of a chunk of jobs, the result object, and the host restatement of the
// whole call (iba_debug_bundle_host: the items of iba_bundle_math.hpp walked in loops, the lanes' sums combined by the trees the kernels use).
// Plain C++, no HIP: the sanitizer self-test (san/bundle_selftest.cpp) compiles this file with g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_bundle_math.hpp"

namespace iba {
namespace bundle {

constexpr int32_t kMaxCount = IBA_BUNDLE_MAX_COUNT;

inline float local_delta() { return (float)std::sqrt(5.991); }
inline float global_delta() { return (float)std::sqrt(5.99); }

inline std::string check_options(const iba_bundle_options* o) {
    if (!o) return "options is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_bundle_options)) return "options.struct_size is " + std::to_string(o->struct_size) + ", not " + std::to_string(sizeof(iba_bundle_options));
    if (o->rounds < 1 || o->rounds > kMaxRounds) return "rounds " + std::to_string(o->rounds) + " is outside 1..4";
    for (int r = 0; r < o->rounds; ++r)
        if (o->iterations[r] < 1 || o->iterations[r] > 100) return "iterations[" + std::to_string(r) + "] = " + std::to_string(o->iterations[r]) + " is outside 1..100";
    if (!std::isfinite(o->chi2_threshold) || o->chi2_threshold < 0.f) return "chi2_threshold is not finite or < 0";
    if (!std::isfinite(o->huber_delta) || !(o->huber_delta > 0.f)) return "huber_delta is not finite or <= 0";
    if (o->robust_rounds < 0 || o->robust_rounds > kMaxRounds) return "robust_rounds " + std::to_string(o->robust_rounds) + " is outside 0..4";
    return "";
}

// ---- the plan of a job: a function of its index arrays alone ----
struct Plan {
    std::vector<int32_t> pt_off, pt_edges, cam_off, cam_edges;   // stable in edge index
    std::vector<int32_t> blk_a, blk_b, blk_off;                 // blocks (a <= b, both free) by a, then b; blk_off has n_blk + 1 entries
    std::vector<int32_t> it_p, it_ea, it_eb;                    // a block's items in ascending point; ea is the edge of camera a
    int32_t n_free = 0;
};
// "" or what is wrong with the job's indices (range, a duplicate pair, too many free cameras, too many items)
inline std::string make_plan(const iba_bundle_job& q, Plan* pl) {
    const int32_t nc = q.n_cameras, np = q.n_points, ne = q.n_edges;
    pl->pt_off.assign((size_t)np + 1, 0); pl->cam_off.assign((size_t)nc + 1, 0);
    pl->pt_edges.assign((size_t)ne, 0); pl->cam_edges.assign((size_t)ne, 0);
    for (int32_t e = 0; e < ne; ++e) {
        const int32_t p = q.edge_point[e], c = q.edge_camera[e];
        if (p < 0 || p >= np) return "edge " + std::to_string(e) + " names point " + std::to_string(p) + " of " + std::to_string(np);
        if (c < 0 || c >= nc) return "edge " + std::to_string(e) + " names camera " + std::to_string(c) + " of " + std::to_string(nc);
        ++pl->pt_off[(size_t)p + 1]; ++pl->cam_off[(size_t)c + 1];
    }
    for (int32_t p = 0; p < np; ++p) pl->pt_off[(size_t)p + 1] += pl->pt_off[(size_t)p];
    for (int32_t c = 0; c < nc; ++c) pl->cam_off[(size_t)c + 1] += pl->cam_off[(size_t)c];
    {
        std::vector<int32_t> pa(pl->pt_off.begin(), pl->pt_off.end() - 1), ca(pl->cam_off.begin(), pl->cam_off.end() - 1);
        for (int32_t e = 0; e < ne; ++e) { pl->pt_edges[(size_t)pa[(size_t)q.edge_point[e]]++] = e; pl->cam_edges[(size_t)ca[(size_t)q.edge_camera[e]]++] = e; }
    }
    std::vector<int32_t> slot((size_t)nc, -1), seen((size_t)nc, -1);
    int32_t nf = 0;
    for (int32_t c = 0; c < nc; ++c) if (!q.fixed[c]) slot[(size_t)c] = nf++;
    pl->n_free = nf;
    if (nf > kMaxFree) return std::to_string(nf) + " free cameras, more than IBA_BUNDLE_MAX_FREE_CAMERAS = " + std::to_string(kMaxFree);
    const int32_t nb = nf * (nf + 1) / 2;
    pl->blk_a.assign((size_t)nb, 0); pl->blk_b.assign((size_t)nb, 0); pl->blk_off.assign((size_t)nb + 1, 0);
    {
        int32_t k = 0;
        for (int32_t a = 0; a < nc; ++a) if (slot[(size_t)a] >= 0) for (int32_t b = a; b < nc; ++b) if (slot[(size_t)b] >= 0) { pl->blk_a[(size_t)k] = a; pl->blk_b[(size_t)k] = b; ++k; }
    }
    auto block_of = [&](int32_t ca, int32_t cb) { const int32_t sa = slot[(size_t)ca], sb = slot[(size_t)cb]; return sa * nf - sa * (sa - 1) / 2 + (sb - sa); };
    uint64_t items = 0;
    for (int pass = 0; pass < 2; ++pass) {
        std::vector<int32_t> at;
        if (pass) {
            if (items >= (1ull << 31)) return "the reduced system has 2^31 pair items or more";
            for (int32_t b = 0; b < nb; ++b) pl->blk_off[(size_t)b + 1] += pl->blk_off[(size_t)b];
            at.assign(pl->blk_off.begin(), pl->blk_off.end() - 1);
            pl->it_p.assign((size_t)items, 0); pl->it_ea.assign((size_t)items, 0); pl->it_eb.assign((size_t)items, 0);
        }
        for (int32_t p = 0; p < np; ++p) {
            const int32_t lo = pl->pt_off[(size_t)p], hi = pl->pt_off[(size_t)p + 1];
            if (!pass)
                for (int32_t i = lo; i < hi; ++i) {
                    const int32_t c = q.edge_camera[pl->pt_edges[(size_t)i]];
                    if (seen[(size_t)c] == p) return "point " + std::to_string(p) + " and camera " + std::to_string(c) + " are joined by two edges";
                    seen[(size_t)c] = p;
                }
            for (int32_t i = lo; i < hi; ++i) {
                const int32_t ei = pl->pt_edges[(size_t)i], ci = q.edge_camera[ei];
                if (slot[(size_t)ci] < 0) continue;
                for (int32_t k = i; k < hi; ++k) {
                    const int32_t ek = pl->pt_edges[(size_t)k], ck = q.edge_camera[ek];
                    if (slot[(size_t)ck] < 0) continue;
                    const int32_t b = ci <= ck ? block_of(ci, ck) : block_of(ck, ci);
                    if (!pass) { ++pl->blk_off[(size_t)b + 1]; ++items; continue; }
                    const size_t w = (size_t)at[(size_t)b]++;
                    pl->it_p[w] = p; pl->it_ea[w] = ci <= ck ? ei : ek; pl->it_eb[w] = ci <= ck ? ek : ei;
                }
            }
        }
    }
    return "";
}

// ---- iba_bundle_local_window: Optimizer.cc:620-669 and the vertex and edge order of :682-779, over the map's observation table ----
struct Window {
    std::vector<int32_t> camera_keyframe, point_id, edge_point, edge_camera, edge_keypoint;
    std::vector<uint8_t> fixed;
    int32_t n_local = 0;
};
inline std::string local_window(const int32_t* obs, int32_t n_obs, const uint8_t* point_bad, int32_t n_mp, const uint8_t* kf_bad, int32_t n_kf, int32_t current,
                                const int32_t* covisible, int32_t n_cov, Window* w) {
    if (n_obs < 0 || n_mp < 0 || n_kf < 1 || n_cov < 0) return "a negative count, or no keyframe";
    if (n_obs > kMaxCount || n_mp > kMaxCount || n_kf > kMaxCount || n_cov > kMaxCount) return "a count above " + std::to_string(kMaxCount);
    if ((n_obs && !obs) || (n_mp && !point_bad) || !kf_bad || (n_cov && !covisible)) return "a NULL input";
    if (current < 0 || current >= n_kf) return "the current keyframe " + std::to_string(current) + " is outside the map's " + std::to_string(n_kf);
    for (int32_t i = 0; i < n_obs; ++i) {
        const int32_t p = obs[3 * (size_t)i], k = obs[3 * (size_t)i + 1], u = obs[3 * (size_t)i + 2];
        if (p < 0 || p >= n_mp || k < 0 || k >= n_kf || u < 0) return "observation " + std::to_string(i) + " names map point " + std::to_string(p) + ", keyframe " + std::to_string(k) + ", keypoint " + std::to_string(u);
    }
    // the rows by (keyframe, keypoint): GetMapPointMatches; and by (map point, keyframe): GetObservations in ascending keyframe id
    std::vector<int32_t> by_kf((size_t)n_obs), by_mp((size_t)n_obs);
    for (int32_t i = 0; i < n_obs; ++i) by_kf[(size_t)i] = by_mp[(size_t)i] = i;
    auto col = [&](int32_t i, int c) { return obs[3 * (size_t)i + c]; };
    std::sort(by_kf.begin(), by_kf.end(), [&](int32_t x, int32_t y) { return col(x, 1) != col(y, 1) ? col(x, 1) < col(y, 1) : (col(x, 2) != col(y, 2) ? col(x, 2) < col(y, 2) : x < y); });
    std::sort(by_mp.begin(), by_mp.end(), [&](int32_t x, int32_t y) { return col(x, 0) != col(y, 0) ? col(x, 0) < col(y, 0) : (col(x, 1) != col(y, 1) ? col(x, 1) < col(y, 1) : x < y); });
    for (int32_t i = 1; i < n_obs; ++i) {
        if (col(by_kf[(size_t)i], 1) == col(by_kf[(size_t)i - 1], 1) && col(by_kf[(size_t)i], 2) == col(by_kf[(size_t)i - 1], 2))
            return "keyframe " + std::to_string(col(by_kf[(size_t)i], 1)) + " holds two map points at keypoint " + std::to_string(col(by_kf[(size_t)i], 2));
        if (col(by_mp[(size_t)i], 0) == col(by_mp[(size_t)i - 1], 0) && col(by_mp[(size_t)i], 1) == col(by_mp[(size_t)i - 1], 1))
            return "map point " + std::to_string(col(by_mp[(size_t)i], 0)) + " is observed twice by keyframe " + std::to_string(col(by_mp[(size_t)i], 1));
    }
    std::vector<int32_t> kf_at((size_t)n_kf + 1, 0), mp_at((size_t)n_mp + 1, 0);
    for (int32_t i = 0; i < n_obs; ++i) { ++kf_at[(size_t)col(i, 1) + 1]; ++mp_at[(size_t)col(i, 0) + 1]; }
    for (int32_t k = 0; k < n_kf; ++k) kf_at[(size_t)k + 1] += kf_at[(size_t)k];
    for (int32_t p = 0; p < n_mp; ++p) mp_at[(size_t)p + 1] += mp_at[(size_t)p];
    std::vector<int32_t> cam_of((size_t)n_kf, -1), pt_of((size_t)n_mp, -1);
    std::vector<uint8_t> marked((size_t)n_kf, 0);      // mnBALocalForKF or mnBAFixedForKF == pKF->mnId
    *w = Window();
    auto add_camera = [&](int32_t k, bool fixed) { cam_of[(size_t)k] = (int32_t)w->camera_keyframe.size(); w->camera_keyframe.push_back(k); w->fixed.push_back((fixed || k == 0) ? 1 : 0); };
    add_camera(current, false); marked[(size_t)current] = 1;
    for (int32_t i = 0; i < n_cov; ++i) {
        const int32_t k = covisible[i];
        if (k < 0 || k >= n_kf) return "covisible " + std::to_string(i) + " names keyframe " + std::to_string(k) + " of " + std::to_string(n_kf);
        if (marked[(size_t)k]) return "covisible " + std::to_string(i) + " is the current keyframe or is listed twice";
        marked[(size_t)k] = 1;
        if (!kf_bad[k]) add_camera(k, false);
    }
    w->n_local = (int32_t)w->camera_keyframe.size();
    for (int32_t c = 0; c < w->n_local; ++c) {
        const int32_t k = w->camera_keyframe[(size_t)c];
        for (int32_t i = kf_at[(size_t)k]; i < kf_at[(size_t)k + 1]; ++i) {
            const int32_t p = col(by_kf[(size_t)i], 0);
            if (point_bad[p] || pt_of[(size_t)p] >= 0) continue;
            pt_of[(size_t)p] = (int32_t)w->point_id.size(); w->point_id.push_back(p);
        }
    }
    for (int32_t p : w->point_id)
        for (int32_t i = mp_at[(size_t)p]; i < mp_at[(size_t)p + 1]; ++i) {
            const int32_t k = col(by_mp[(size_t)i], 1);
            if (marked[(size_t)k]) continue;
            marked[(size_t)k] = 1;
            if (!kf_bad[k]) add_camera(k, true);
        }
    for (size_t x = 0; x < w->point_id.size(); ++x) {
        const int32_t p = w->point_id[x];
        for (int32_t i = mp_at[(size_t)p]; i < mp_at[(size_t)p + 1]; ++i) {
            const int32_t row = by_mp[(size_t)i], k = col(row, 1);
            if (kf_bad[k]) continue;
            w->edge_point.push_back((int32_t)x); w->edge_camera.push_back(cam_of[(size_t)k]); w->edge_keypoint.push_back(col(row, 2));
        }
    }
    return "";
}

inline std::string check_job(const iba_bundle_job& q) {
    if (q.n_cameras < 0 || q.n_cameras > kMaxCount || q.n_points < 0 || q.n_points > kMaxCount || q.n_edges < 0 || q.n_edges > kMaxCount)
        return "n_cameras, n_points or n_edges is outside 0.." + std::to_string(kMaxCount);
    if (q.n_cameras && (!q.Tcw12 || !q.fixed)) return "Tcw12 or fixed is NULL";
    if (q.n_points && !q.xyz) return "xyz is NULL";
    if (q.n_edges && (!q.edge_point || !q.edge_camera || !q.obs || !q.inv_sigma2)) return "edge_point, edge_camera, obs or inv_sigma2 is NULL";
    if (!std::isfinite(q.fx) || !std::isfinite(q.fy) || !(q.fx > 0.f) || !(q.fy > 0.f)) return "fx or fy is not finite or <= 0";
    if (!std::isfinite(q.cx) || !std::isfinite(q.cy)) return "cx or cy is not finite";
    for (int64_t k = 0; k < 12 * (int64_t)q.n_cameras; ++k) if (!std::isfinite(q.Tcw12[k])) return "camera " + std::to_string(k / 12) + ": the pose is not finite";
    for (int64_t k = 0; k < 3 * (int64_t)q.n_points; ++k) if (!std::isfinite(q.xyz[k])) return "point " + std::to_string(k / 3) + " is not finite";
    for (int32_t e = 0; e < q.n_edges; ++e) {
        const std::string at = "edge " + std::to_string(e) + ": ";
        if (!std::isfinite(q.obs[2 * (size_t)e]) || !std::isfinite(q.obs[2 * (size_t)e + 1])) return at + "the observation is not finite";
        if (!std::isfinite(q.inv_sigma2[e])) return at + "inv_sigma2 is not finite";
        if (q.inv_sigma2[e] < 0.f) return at + "inv_sigma2 < 0";
    }
    return "";
}
// the checks of a call and the plans of its jobs
inline std::string check_jobs(const iba_bundle_job* jobs, int32_t B, std::vector<Plan>* plans) {
    if (!jobs) return "jobs is NULL";
    if (B < 1) return "B = " + std::to_string(B) + " < 1";
    plans->resize((size_t)B);
    for (int32_t j = 0; j < B; ++j) {
        std::string why = check_job(jobs[j]);
        if (why.empty()) why = make_plan(jobs[j], &(*plans)[(size_t)j]);
        if (!why.empty()) return "job " + std::to_string(j) + ": " + why;
    }
    return "";
}

// ---- the flat tables of the jobs [a, b): X(type, name, uploaded) ----
#define IBA_BUNDLE_TABLES(X)                                                                                                                        \
    X(JobRec, job, 1) X(Ctl, ctl, 1) X(double, T, 1) X(double, Tn, 0) X(uint8_t, fixed, 1) X(int32_t, cjob, 1) X(int32_t, cam_off, 1)               \
    X(int32_t, cam_edges, 1) X(double, cam_sums, 0) X(int32_t, cam_cnt, 0) X(int32_t, rank, 0) X(double, bs, 0) X(double, dp, 0) X(double, X, 1)      \
    X(double, Xn, 0) X(int32_t, pjob, 1) X(int32_t, pt_off, 1) X(int32_t, pt_edges, 1) X(double, pt_sums, 0) X(double, pt_inv, 0)                    \
    X(double, pt_chi, 0) X(double, dl, 0) X(int32_t, pt_cnt, 0) X(int32_t, ep, 1) X(int32_t, ec, 1) X(int32_t, ejob, 1) X(float, obs, 1)             \
    X(float, w, 1) X(uint8_t, active, 1) X(uint8_t, outlier, 0) X(float, chi2f, 0) X(double, lin, 0) X(double, chi2d, 0) X(int32_t, blk_a, 1)        \
    X(int32_t, blk_b, 1) X(int32_t, blk_job, 1) X(int32_t, blk_off, 1) X(int32_t, it_p, 1) X(int32_t, it_ea, 1) X(int32_t, it_eb, 1) X(double, S, 0) \
    X(double, stT, 0) X(double, stX, 0) X(int32_t, running, 0)

struct Sizes {
#define X(type, name, up) size_t name = 0;
    IBA_BUNDLE_TABLES(X)
#undef X
};
struct HostTables {
#define X(type, name, up) std::vector<type> name;
    IBA_BUNDLE_TABLES(X)
#undef X
    Sizes n;
    int32_t nJ = 0, nC = 0, nP = 0, nE = 0, nB = 0;
    // every table at its size, zeroed where the builder did not fill it (the host restatement's; the device path sizes its buffers from n)
    void whole() {
#define X(type, name, up) name.resize(n.name);
        IBA_BUNDLE_TABLES(X)
#undef X
    }
    Tab tab() {
        Tab t;
#define X(type, name, up) t.name = name.empty() ? nullptr : name.data();
        IBA_BUNDLE_TABLES(X)
#undef X
        return t;
    }
};

inline void start_ctl(Ctl& c) {
    std::memset(&c, 0, sizeof(c));
    c.kind = kLinearise; c.stage = -1;
    pose::lm_round_start(&c.lm);
}

// the device bytes of a job (what cut_chunks adds up)
inline uint64_t job_bytes(const iba_bundle_job& q, const Plan& pl, bool stages, bool eval) {
    const uint64_t nc = (uint64_t)q.n_cameras, np = (uint64_t)q.n_points, ne = (uint64_t)q.n_edges, nr = 6ull * (uint64_t)pl.n_free;
    return sizeof(JobRec) + sizeof(Ctl) + nc * (2 * 96 + 1 + 4 + 4 + 8 * kCamSums + 8 + 96) + np * (2 * 24 + 4 + 4 + 8 * (kPtSums + 6 + 1 + 3) + 4) +
           ne * (4 * 5 + 12 + 1 + 1 + 4 + 8 * kLin + (eval ? 8 : 0)) + 16ull * pl.blk_a.size() + 12ull * pl.it_p.size() + 8 * nr * nr +
           (stages ? (uint64_t)kMaxRounds * 8 * (12 * nc + 3 * np) : 0);
}

// active: NULL, or per job NULL or n_edges bytes (iba_bundle_eval); false: a chunk-wide index would not fit int32
inline bool build_tables(const iba_bundle_job* jobs, const std::vector<Plan>& plans, int32_t a, int32_t b, const uint8_t* const* active, bool stages, bool eval, HostTables* h) {
    uint64_t nC = 0, nP = 0, nE = 0, nB = 0, nI = 0, nS = 0;
    for (int32_t j = a; j < b; ++j) {
        const Plan& pl = plans[(size_t)j];
        nC += (uint64_t)jobs[j].n_cameras; nP += (uint64_t)jobs[j].n_points; nE += (uint64_t)jobs[j].n_edges; nB += pl.blk_a.size(); nI += pl.it_p.size();
        nS += 36ull * (uint64_t)pl.n_free * (uint64_t)pl.n_free;
    }
    if (nC >= (1ull << 27) || nP >= (1ull << 27) || nE >= (1ull << 27) || nB >= (1ull << 31) - 1 || nI >= (1ull << 31) - 1) return false;
    const size_t nJ = (size_t)(b - a);
    h->nJ = (int32_t)nJ; h->nC = (int32_t)nC; h->nP = (int32_t)nP; h->nE = (int32_t)nE; h->nB = (int32_t)nB;
    Sizes& n = h->n;
    n.job = n.ctl = nJ;
    n.T = n.Tn = 12 * nC; n.fixed = n.cjob = n.cam_cnt = n.rank = nC; n.cam_off = nC + 1; n.cam_edges = nE; n.cam_sums = kCamSums * nC; n.bs = n.dp = 6 * nC;
    n.X = n.Xn = n.dl = 3 * nP; n.pjob = n.pt_cnt = n.pt_chi = nP; n.pt_off = nP + 1; n.pt_edges = nE; n.pt_sums = kPtSums * nP; n.pt_inv = 6 * nP;
    n.ep = n.ec = n.ejob = n.w = n.active = n.outlier = n.chi2f = nE; n.obs = 2 * nE; n.lin = (size_t)kLin * nE; n.chi2d = eval ? nE : 0;
    n.blk_a = n.blk_b = n.blk_job = nB; n.blk_off = nB + 1; n.it_p = n.it_ea = n.it_eb = nI; n.S = nS;
    n.stT = stages ? (size_t)kMaxRounds * 12 * nC : 0; n.stX = stages ? (size_t)kMaxRounds * 3 * nP : 0; n.running = 1;
#define X(type, name, up) h->name.clear(); if (up) h->name.resize(n.name);
    IBA_BUNDLE_TABLES(X)
#undef X
    int32_t c0 = 0, p0 = 0, e0 = 0, b0 = 0, i0 = 0;
    int64_t s0 = 0;
    for (size_t k = 0; k < nJ; ++k) {
        const iba_bundle_job& q = jobs[(size_t)a + k];
        const Plan& pl = plans[(size_t)a + k];
        JobRec& r = h->job[k];
        r = JobRec{c0, q.n_cameras, p0, q.n_points, e0, q.n_edges, b0, (int32_t)pl.blk_a.size(), pl.n_free, 0, s0, (double)q.fx, (double)q.fy, (double)q.cx, (double)q.cy};
        start_ctl(h->ctl[k]);
        for (int32_t c = 0; c < q.n_cameras; ++c) {
            std::memcpy(&h->T[12 * (size_t)(c0 + c)], q.Tcw12 + 12 * (size_t)c, 96);
            h->fixed[(size_t)(c0 + c)] = q.fixed[c] ? 1 : 0; h->cjob[(size_t)(c0 + c)] = (int32_t)k;
            h->cam_off[(size_t)(c0 + c)] = e0 + pl.cam_off[(size_t)c];
        }
        for (int32_t p = 0; p < q.n_points; ++p) {
            for (int d = 0; d < 3; ++d) h->X[3 * (size_t)(p0 + p) + d] = (double)q.xyz[3 * (size_t)p + d];
            h->pjob[(size_t)(p0 + p)] = (int32_t)k;
            h->pt_off[(size_t)(p0 + p)] = e0 + pl.pt_off[(size_t)p];
        }
        for (int32_t e = 0; e < q.n_edges; ++e) {
            const size_t g = (size_t)(e0 + e);
            h->ep[g] = p0 + q.edge_point[e]; h->ec[g] = c0 + q.edge_camera[e]; h->ejob[g] = (int32_t)k;
            h->obs[2 * g] = q.obs[2 * (size_t)e]; h->obs[2 * g + 1] = q.obs[2 * (size_t)e + 1]; h->w[g] = q.inv_sigma2[e];
            h->active[g] = (active && active[(size_t)a + k]) ? (active[(size_t)a + k][e] ? 1 : 0) : 1;
            h->cam_edges[g] = e0 + pl.cam_edges[(size_t)e]; h->pt_edges[g] = e0 + pl.pt_edges[(size_t)e];
        }
        for (size_t x = 0; x < pl.blk_a.size(); ++x) {
            h->blk_a[(size_t)b0 + x] = c0 + pl.blk_a[x]; h->blk_b[(size_t)b0 + x] = c0 + pl.blk_b[x]; h->blk_job[(size_t)b0 + x] = (int32_t)k;
            h->blk_off[(size_t)b0 + x] = i0 + pl.blk_off[x];
        }
        for (size_t x = 0; x < pl.it_p.size(); ++x) {
            h->it_p[(size_t)i0 + x] = p0 + pl.it_p[x]; h->it_ea[(size_t)i0 + x] = e0 + pl.it_ea[x]; h->it_eb[(size_t)i0 + x] = e0 + pl.it_eb[x];
        }
        c0 += q.n_cameras; p0 += q.n_points; e0 += q.n_edges; b0 += (int32_t)pl.blk_a.size(); i0 += (int32_t)pl.it_p.size();
        s0 += 36ll * pl.n_free * pl.n_free;
    }
    h->cam_off[(size_t)nC] = e0; h->pt_off[(size_t)nP] = e0; h->blk_off[(size_t)nB] = i0;
    return true;
}

inline DevOpt dev_options(const iba_bundle_options& o) {
    DevOpt d{};
    d.rounds = o.rounds; d.robust_rounds = o.robust_rounds; d.keep_stages = o.keep_stages ? 1 : 0; d.eval = 0;
    for (int r = 0; r < kMaxRounds; ++r) d.iterations[r] = o.iterations[r];
    d.chi2_threshold = o.chi2_threshold; d.delta = (double)o.huber_delta; d.lambda = 0.0;
    return d;
}
inline DevOpt eval_options(int robust, double lambda) {
    DevOpt d{};
    d.rounds = 1; d.iterations[0] = 1; d.robust_rounds = robust ? 1 : 0; d.eval = 1; d.chi2_threshold = 5.991f; d.delta = (double)local_delta(); d.lambda = lambda;
    return d;
}
// the steps a call can take at most: per round its iterations of one linearisation and ten trials each, and the classification
inline int max_steps(const DevOpt& o) {
    if (o.eval) return 1;
    int s = 1;
    for (int r = 0; r < o.rounds; ++r) s += o.iterations[r] * (1 + pose::kMaxTrials) + 1;
    return s;
}

// ---- the host restatement: one step of the chain in three parts, the kernels' order ----
template <int N>
inline void tree(double* v, int width) {    // v[lane * N + k]; the balanced tree v[l] = v[2l] + v[2l + 1]
    for (; width > 1; width /= 2)
        for (int l = 0; l < width / 2; ++l)
            for (int k = 0; k < N; ++k) v[(size_t)l * N + k] = v[(size_t)(2 * l) * N + k] + v[(size_t)(2 * l + 1) * N + k];
}
inline void host_front(const Tab& t, const HostTables& h, const DevOpt& o) {
    for (int e = 0; e < h.nE; ++e) edge_item(t, e, o);
    for (int p = 0; p < h.nP; ++p) point_item(t, p);
    std::vector<double> acc((size_t)kLanes * kBlockSums);
    for (int c = 0; c < h.nC; ++c) {
        if (!camera_runs(t, c)) continue;
        int n = 0;
        for (int l = 0; l < kWave; ++l) n += camera_lane(t, c, l, &acc[(size_t)l * kCamSums]);
        tree<kCamSums>(acc.data(), kWave);
        for (int k = 0; k < kCamSums; ++k) t.cam_sums[(size_t)kCamSums * c + k] = acc[(size_t)k];
        t.cam_cnt[c] = n;
    }
    for (int j = 0; j < h.nJ; ++j) {
        const int kind = t.ctl[j].kind;
        double chi = 0.0, md = 0.0;
        if (kind == kLinearise || kind == kTrial) {
            for (int l = 0; l < kLanes; ++l) acc[(size_t)l] = chi_lane(t, t.job[j], l);
            tree<1>(acc.data(), kLanes);
            chi = acc[0];
        }
        if (kind == kLinearise) for (int l = 0; l < kLanes; ++l) md = larger(md, diag_lane(t, t.job[j], l));
        sequence_front(t, j, o, chi, md);
        copy_item(t, j, 0, 1);
    }
}
inline void host_middle(const Tab& t, const HostTables& h) {
    for (int p = 0; p < h.nP; ++p) inverse_item(t, p);
    std::vector<double> acc((size_t)kWave * kBlockSums);
    for (int b = 0; b < h.nB; ++b) {
        if (!block_runs(t, b)) continue;
        for (int l = 0; l < kWave; ++l) block_lane(t, b, l, &acc[(size_t)l * kBlockSums]);
        tree<kBlockSums>(acc.data(), kWave);
        block_store(t, b, acc.data());
    }
}
inline void host_back(const Tab& t, const HostTables& h, const DevOpt& o) {
    std::vector<double> b((size_t)kMaxReduced), x((size_t)kMaxReduced), y((size_t)kMaxReduced);
    for (int j = 0; j < h.nJ; ++j) {
        Ctl& c = t.ctl[j];
        const JobRec& q = t.job[j];
        if (!c.propose || c.fail) continue;
        const int n = 6 * c.n_part;
        for (int cam = q.cam0; cam < q.cam0 + q.n_cam; ++cam) if (t.rank[cam] >= 0) for (int k = 0; k < 6; ++k) b[(size_t)(6 * t.rank[cam] + k)] = t.bs[6 * (size_t)cam + k];
        if (!reduced_solve(t.S + q.s0, n, b.data(), x.data(), y.data())) { c.fail = 1; continue; }
        for (int cam = q.cam0; cam < q.cam0 + q.n_cam; ++cam) if (t.rank[cam] >= 0) for (int k = 0; k < 6; ++k) t.dp[6 * (size_t)cam + k] = x[(size_t)(6 * t.rank[cam] + k)];
    }
    for (int p = 0; p < h.nP; ++p) backsub_item(t, p);
    for (int c = 0; c < h.nC; ++c) camera_update_item(t, c);
    *t.running = 0;
    for (int j = 0; j < h.nJ; ++j) sequence_back(t, j, o);
}

}  // namespace bundle
}  // namespace iba

// what iba_bundle_eval leaves per job (both paths fill it from the tables)
struct iba_bundle_job_out {
    iba_bundle_result r{};
    std::vector<double> T, X;                       // the final estimates
    std::vector<uint8_t> outlier;
    std::vector<float> chi2;
    std::vector<double> stT, stX;                   // keep_stages: rounds_run x (12 n_cameras), x (3 n_points)
};
struct iba_bundle_batch {
    iba_bundle_options opt{};
    std::vector<iba_bundle_job_out> job;
    float kernel_ms = 0.f;
    int32_t chunks = 0, big_steps = 0;
};

namespace iba {
namespace bundle {

// the results of the jobs [a, a + nJ) out of the tables (host vectors hold what came back)
inline void collect(const HostTables& h, const iba_bundle_options& opt, int32_t a, iba_bundle_batch* res) {
    for (int32_t k = 0; k < h.nJ; ++k) {
        const JobRec& q = h.job[(size_t)k];
        const Ctl& c = h.ctl[(size_t)k];
        iba_bundle_job_out& o = res->job[(size_t)(a + k)];
        o.r.n_cameras = q.n_cam; o.r.n_points = q.n_pt; o.r.n_edges = q.n_e; o.r.n_free = q.n_free; o.r.rounds_run = c.rounds_run;
        o.r.n_outliers = c.rounds_run ? c.r_bad[c.rounds_run - 1] : 0;
        for (int r = 0; r < kMaxRounds; ++r) { o.r.chi2[r] = c.r_chi2[r]; o.r.n_bad[r] = c.r_bad[r]; o.r.lm_iterations[r] = c.r_its[r]; o.r.trials[r] = c.r_trials[r]; }
        o.T.assign(h.T.begin() + 12 * (std::ptrdiff_t)q.cam0, h.T.begin() + 12 * (std::ptrdiff_t)(q.cam0 + q.n_cam));
        o.X.assign(h.X.begin() + 3 * (std::ptrdiff_t)q.pt0, h.X.begin() + 3 * (std::ptrdiff_t)(q.pt0 + q.n_pt));
        for (double& v : o.T) v = pose::canon(v);
        for (double& v : o.X) v = pose::canon(v);
        o.outlier.assign(h.outlier.begin() + q.e0, h.outlier.begin() + q.e0 + q.n_e);
        o.chi2.assign(h.chi2f.begin() + q.e0, h.chi2f.begin() + q.e0 + q.n_e);
        if (opt.keep_stages) {
            const size_t nT = 12 * (size_t)q.n_cam, nX = 3 * (size_t)q.n_pt;
            const double* sT = h.stT.data() + (size_t)kMaxRounds * 12 * (size_t)q.cam0;
            const double* sX = h.stX.data() + (size_t)kMaxRounds * 3 * (size_t)q.pt0;
            o.stT.assign(sT, sT + (size_t)c.rounds_run * nT); o.stX.assign(sX, sX + (size_t)c.rounds_run * nX);
            for (double& v : o.stT) v = pose::canon(v);
            for (double& v : o.stX) v = pose::canon(v);
        }
        res->big_steps += c.big;
    }
}

// iba_bundle_eval's outputs of the jobs [a, a + nJ) out of the tables; S_copy: the reduced matrices before the factorisation
inline void collect_eval(const HostTables& h, const std::vector<double>& S_copy, int32_t a, iba_bundle_eval_out* outs) {
    for (int32_t k = 0; k < h.nJ; ++k) {
        const JobRec& q = h.job[(size_t)k];
        const Ctl& c = h.ctl[(size_t)k];
        iba_bundle_eval_out& o = outs[a + k];
        o.chi2_robust = pose::canon(c.chi); o.lambda = c.lm.lambda; o.n_reduced = 6 * c.n_part; o.solved = c.fail ? 0 : 1;
        for (int32_t i = 0; i < q.n_cam; ++i) {
            const size_t cam = (size_t)(q.cam0 + i);
            const bool has = !h.fixed[cam] && h.cam_cnt[cam] > 0;
            const double* s = &h.cam_sums[(size_t)kCamSums * cam];
            if (o.Hpp) for (int r = 0; r < 6; ++r) for (int cc = 0; cc < 6; ++cc) o.Hpp[36 * (size_t)i + 6 * r + cc] = has ? pose::canon(s[r <= cc ? pose::hidx(r, cc) : pose::hidx(cc, r)]) : 0.0;
            for (int r = 0; r < 6; ++r) {
                if (o.bp) o.bp[6 * (size_t)i + r] = has ? pose::canon(s[21 + r]) : 0.0;
                if (o.bs) o.bs[6 * (size_t)i + r] = (has && !c.fail) ? pose::canon(h.bs[6 * cam + r]) : 0.0;
                if (o.dp) o.dp[6 * (size_t)i + r] = (has && !c.fail) ? pose::canon(h.dp[6 * cam + r]) : 0.0;
            }
        }
        for (int32_t i = 0; i < q.n_pt; ++i) {
            const size_t p = (size_t)(q.pt0 + i);
            const bool has = h.pt_cnt[p] > 0;
            const double* s = &h.pt_sums[(size_t)kPtSums * p];
            if (o.Hll) for (int r = 0; r < 3; ++r) for (int cc = 0; cc < 3; ++cc) o.Hll[9 * (size_t)i + 3 * r + cc] = has ? pose::canon(sym3(s, r, cc)) : 0.0;
            for (int r = 0; r < 3; ++r) {
                if (o.bl) o.bl[3 * (size_t)i + r] = has ? pose::canon(s[6 + r]) : 0.0;
                if (o.dl) o.dl[3 * (size_t)i + r] = (has && !c.fail) ? pose::canon(h.dl[3 * p + r]) : 0.0;
            }
        }
        if (o.chi2_edges) for (int32_t e = 0; e < q.n_e; ++e) o.chi2_edges[e] = h.chi2d[(size_t)(q.e0 + e)];
        if (o.S) {
            const int n = o.n_reduced;
            const double* S = S_copy.data() + q.s0;
            for (int i = 0; i < n; ++i) for (int kk = 0; kk <= i; ++kk) { const double v = c.fail ? 0.0 : pose::canon(S[sidx(n, i, kk)]); o.S[(size_t)i * n + kk] = v; o.S[(size_t)kk * n + i] = v; }
        }
    }
}

// the whole call on the host, job by job (a job's bytes do not depend on its neighbours)
inline void host_call(const iba_bundle_job* jobs, const std::vector<Plan>& plans, int32_t B, const iba_bundle_options& opt, iba_bundle_batch* res) {
    const DevOpt o = dev_options(opt);
    HostTables h;
    for (int32_t j = 0; j < B; ++j) {
        build_tables(jobs, plans, j, j + 1, nullptr, opt.keep_stages != 0, false, &h);
        h.whole();
        const Tab t = h.tab();
        const int bound = max_steps(o);
        for (int s = 0; s < bound; ++s) {
            host_front(t, h, o); host_middle(t, h); host_back(t, h, o);
            if (!h.running[0]) break;
        }
        collect(h, opt, j, res);
    }
}
inline void host_eval(const iba_bundle_job* jobs, const std::vector<Plan>& plans, int32_t B, const uint8_t* const* active, int robust, double lambda, iba_bundle_eval_out* outs) {
    const DevOpt o = eval_options(robust, lambda);
    HostTables h;
    for (int32_t j = 0; j < B; ++j) {
        build_tables(jobs, plans, j, j + 1, active, false, true, &h);
        h.whole();
        const Tab t = h.tab();
        host_front(t, h, o); host_middle(t, h);
        const std::vector<double> S_copy = h.S;
        host_back(t, h, o);
        collect_eval(h, S_copy, j, outs);
    }
}

}  // namespace bundle
}  // namespace iba

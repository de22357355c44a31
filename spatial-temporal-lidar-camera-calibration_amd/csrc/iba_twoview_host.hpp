// Two-view initialisation, the host half (include/iba_mi355x.h, iba_twoview*): the argument checks, T1 (Normalize), the set generator, what a pair
// looks like once prepared for the device (match list, per-match coordinates, the normalising transforms), the result object, the whole call restated
// on the host over iba_twoview_math.hpp (iba_debug_twoview_host), and the last step both paths share (parallax in degrees, status, the chosen
// hypothesis' points). No HIP in this file: the sanitizer self-test compiles it with plain g++.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_twoview_math.hpp"

namespace iba {
namespace tv {

struct PairPrep {
    int32_t n1 = 0, n2 = 0, N = 0;
    float fx = 0.f, fy = 0.f, cx = 0.f, cy = 0.f;
    float T1[9], T2[9], T2inv[9], T2t[9];
    std::vector<int32_t> list;      // N x 2
    std::vector<float> mxy, mn;     // N x 4: u1 v1 u2 v2, as given and normalised
    std::vector<int32_t> sets;      // iterations x 8 (N >= 8)
};

struct PairRes {
    iba_twoview_result r{};
    int32_t n1 = 0, N = 0;
    int32_t cand = -1, fail_before = 0, fail_after = 0;
    std::vector<int32_t> list;
    std::vector<uint8_t> inlier, tri;           // N (of the chosen model), n1
    std::vector<float> points;                  // n1 x 3
    std::vector<float> Hi, H12i, Fi, sH, sF;    // keep_stages: iterations x 9, iterations
    float hyp_R[72] = {}, hyp_t[24] = {};
    std::vector<float> hyp_pts, hyp_cos;        // 8 x N x 3, 8 x N
    std::vector<uint8_t> verdict;               // 8 x N
    std::vector<float> sel_pts, sel_cos;        // the candidate hypothesis' N x 3 and N (where T10 named one): what finish() reads
    std::vector<uint8_t> sel_verdict;
};

// ---- T1 ----
inline void normalize(const float* xy, int32_t n, float* out, float* T) {
    float meanX = 0, meanY = 0;
    for (int32_t i = 0; i < n; ++i) { meanX += xy[2 * i]; meanY += xy[2 * i + 1]; }
    meanX = meanX / n; meanY = meanY / n;
    float meanDevX = 0, meanDevY = 0;
    for (int32_t i = 0; i < n; ++i) {
        out[2 * i] = xy[2 * i] - meanX; out[2 * i + 1] = xy[2 * i + 1] - meanY;
        meanDevX += std::fabs(out[2 * i]); meanDevY += std::fabs(out[2 * i + 1]);
    }
    meanDevX = meanDevX / n; meanDevY = meanDevY / n;
    const float sX = (float)(1.0 / (double)meanDevX), sY = (float)(1.0 / (double)meanDevY);
    for (int32_t i = 0; i < n; ++i) { out[2 * i] = out[2 * i] * sX; out[2 * i + 1] = out[2 * i + 1] * sY; }
    for (int i = 0; i < 9; ++i) T[i] = 0.f;
    T[0] = sX; T[4] = sY; T[8] = 1.f; T[2] = -meanX * sX; T[5] = -meanY * sY;
}

// ---- the sets: the reference's draw loop over splitmix64 ----
inline uint64_t splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline std::string make_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out) {
    if (!out) return "out is NULL";
    if (N < 8 || N > IBA_ORB_MATCH_MAX_KEYPOINTS) return "N = " + std::to_string(N) + " is outside 8.." + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
    if (iterations < 1 || iterations > IBA_TWOVIEW_MAX_ITERATIONS) return "iterations = " + std::to_string(iterations) + " is outside 1.." + std::to_string(IBA_TWOVIEW_MAX_ITERATIONS);
    std::vector<int32_t> all((size_t)N), avail;
    for (int32_t i = 0; i < N; ++i) all[(size_t)i] = i;
    uint64_t s = seed;
    for (int32_t it = 0; it < iterations; ++it) {
        avail = all;
        for (int j = 0; j < 8; ++j) {
            const size_t randi = (size_t)(splitmix64(s) % (uint64_t)avail.size());
            out[8 * it + j] = avail[randi];
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
    return "";
}

// ---- the checks: "" or the reason ----
inline std::string check_options(const iba_twoview_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_twoview_options)) return "opt->struct_size = " + std::to_string(o->struct_size) + ", this library's is " + std::to_string(sizeof(iba_twoview_options));
    if (!std::isfinite(o->sigma) || o->sigma <= 0.f) return "sigma is not finite or <= 0";
    if (o->iterations < 1 || o->iterations > IBA_TWOVIEW_MAX_ITERATIONS) return "iterations = " + std::to_string(o->iterations) + " is outside 1.." + std::to_string(IBA_TWOVIEW_MAX_ITERATIONS);
    if (!std::isfinite(o->min_parallax_deg)) return "min_parallax_deg is not finite";
    if (o->min_triangulated < 0) return "min_triangulated < 0";
    if (!std::isfinite(o->rh_threshold)) return "rh_threshold is not finite";
    return "";
}
inline std::string check_pair(const iba_twoview_pair& p, int32_t iterations) {
    if (p.n1 < 0 || p.n1 > IBA_ORB_MATCH_MAX_KEYPOINTS) return "n1 = " + std::to_string(p.n1) + " is outside 0.." + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
    if (p.n2 < 0 || p.n2 > IBA_ORB_MATCH_MAX_KEYPOINTS) return "n2 = " + std::to_string(p.n2) + " is outside 0.." + std::to_string(IBA_ORB_MATCH_MAX_KEYPOINTS);
    if (p.n1 && (!p.xy1 || !p.matches12)) return "xy1 or matches12 is NULL with n1 > 0";
    if (p.n2 && !p.xy2) return "xy2 is NULL with n2 > 0";
    if (!std::isfinite(p.fx) || p.fx <= 0.f || !std::isfinite(p.fy) || p.fy <= 0.f) return "fx or fy is not finite or <= 0";
    if (!std::isfinite(p.cx) || !std::isfinite(p.cy)) return "cx or cy is not finite";
    for (int32_t i = 0; i < 2 * p.n1; ++i) if (!std::isfinite(p.xy1[i])) return "keypoint " + std::to_string(i / 2) + " of frame 1 has a position that is not finite";
    for (int32_t i = 0; i < 2 * p.n2; ++i) if (!std::isfinite(p.xy2[i])) return "keypoint " + std::to_string(i / 2) + " of frame 2 has a position that is not finite";
    int32_t N = 0;
    for (int32_t i = 0; i < p.n1; ++i) {
        if (p.matches12[i] >= p.n2) return "matches12[" + std::to_string(i) + "] = " + std::to_string(p.matches12[i]) + " with n2 = " + std::to_string(p.n2);
        if (p.matches12[i] >= 0) ++N;
    }
    if (N < 8) return "";
    if (!p.sets) return "sets is NULL with " + std::to_string(N) + " matches";
    for (int32_t it = 0; it < iterations; ++it)
        for (int j = 0; j < 8; ++j) {
            const int32_t v = p.sets[8 * it + j];
            if (v < 0 || v >= N) return "set " + std::to_string(it) + " holds " + std::to_string(v) + " with " + std::to_string(N) + " matches";
            for (int k = 0; k < j; ++k) if (p.sets[8 * it + k] == v) return "set " + std::to_string(it) + " holds " + std::to_string(v) + " twice";
        }
    return "";
}
inline std::string check_call(const iba_twoview_pair* pairs, int32_t B, const iba_twoview_options* opt) {
    std::string why = check_options(opt);
    if (!why.empty()) return why;
    if (!pairs) return "pairs is NULL";
    if (B < 1) return "B < 1";
    for (int32_t b = 0; b < B; ++b) {
        why = check_pair(pairs[b], opt->iterations);
        if (!why.empty()) return "pair " + std::to_string(b) + ": " + why;
    }
    return "";
}

// ---- a checked pair, prepared: the match list, T1 over ALL keypoints of either frame, the per-match coordinates ----
inline void prepare(const iba_twoview_pair& p, int32_t iterations, PairPrep& q) {
    q.n1 = p.n1; q.n2 = p.n2; q.fx = p.fx; q.fy = p.fy; q.cx = p.cx; q.cy = p.cy;
    std::vector<float> pn1(2 * (size_t)p.n1 + 2), pn2(2 * (size_t)p.n2 + 2);
    normalize(p.xy1, p.n1, pn1.data(), q.T1);
    normalize(p.xy2, p.n2, pn2.data(), q.T2);
    inv_affine_diag(q.T2, q.T2inv);
    transpose33(q.T2, q.T2t);
    q.list.clear(); q.mxy.clear(); q.mn.clear();
    for (int32_t i = 0; i < p.n1; ++i) {
        const int32_t j = p.matches12[i];
        if (j < 0) continue;
        q.list.push_back(i); q.list.push_back(j);
        const float raw[4] = {p.xy1[2 * i], p.xy1[2 * i + 1], p.xy2[2 * j], p.xy2[2 * j + 1]};
        const float nrm[4] = {pn1[2 * (size_t)i], pn1[2 * (size_t)i + 1], pn2[2 * (size_t)j], pn2[2 * (size_t)j + 1]};
        q.mxy.insert(q.mxy.end(), raw, raw + 4); q.mn.insert(q.mn.end(), nrm, nrm + 4);
    }
    q.N = (int32_t)(q.list.size() / 2);
    q.sets.clear();
    if (q.N >= 8) q.sets.assign(p.sets, p.sets + 8 * (size_t)iterations);
}

inline void start_result(const PairPrep& q, PairRes& o) {
    o = PairRes();
    o.n1 = q.n1; o.N = q.N; o.list = q.list;
    o.r.n_matches = q.N; o.r.best_it_H = -1; o.r.best_it_F = -1; o.r.chosen = -1;
    o.inlier.assign((size_t)q.N, 0); o.tri.assign((size_t)q.n1, 0); o.points.assign(3 * (size_t)q.n1, 0.f);
    if (q.N < 8) o.r.status = IBA_TWOVIEW_TOO_FEW_MATCHES;
}

// the candidate's slices out of the per-hypothesis arrays
inline void select_from_stages(PairRes& o) {
    if (o.r.status != 0 || o.fail_before != 0) return;
    const size_t N = (size_t)o.N, at = (size_t)o.cand * N;
    o.sel_pts.assign(o.hyp_pts.begin() + (std::ptrdiff_t)(3 * at), o.hyp_pts.begin() + (std::ptrdiff_t)(3 * (at + N)));
    o.sel_cos.assign(o.hyp_cos.begin() + (std::ptrdiff_t)at, o.hyp_cos.begin() + (std::ptrdiff_t)(at + N));
    o.sel_verdict.assign(o.verdict.begin() + (std::ptrdiff_t)at, o.verdict.begin() + (std::ptrdiff_t)(at + N));
}

// ---- the last step of either path: o.r as the kernels (or the host restatement) left it, sel_pts / sel_cos / sel_verdict filled for a pair whose
// T10 named a candidate. parallax_deg calls libm's acos: the one value of the result that is not pinned to the last bit. ----
inline void finish(const iba_twoview_options& opt, bool keep_stages, PairRes& o) {
    iba_twoview_result& r = o.r;
    if (r.status == 0) {
        for (int k = 0; k < r.n_hyp; ++k) r.parallax_deg[k] = (float)(std::acos((double)r.cos_parallax[k]) * 180 / 3.1415926535897932384626433832795);
        if (o.fail_before) r.status = o.fail_before;
        else {
            r.chosen = o.cand;
            const float par = r.parallax_deg[o.cand];
            const bool enough = r.model == 1 ? par >= opt.min_parallax_deg : par > opt.min_parallax_deg;
            r.status = !enough ? IBA_TWOVIEW_LOW_PARALLAX : (o.fail_after ? o.fail_after : IBA_TWOVIEW_OK);
        }
        if (r.status == IBA_TWOVIEW_OK) {
            std::memcpy(r.R21, o.hyp_R + 9 * r.chosen, sizeof(r.R21)); std::memcpy(r.t21, o.hyp_t + 3 * r.chosen, sizeof(r.t21));
            for (size_t i = 0; i < (size_t)o.N; ++i) {
                if (o.sel_verdict[i] != 6) continue;
                const size_t k = (size_t)o.list[2 * i];
                std::memcpy(&o.points[3 * k], &o.sel_pts[3 * i], 3 * sizeof(float));
                if ((double)o.sel_cos[i] < 0.99998) o.tri[k] = 1;
            }
        }
    }
    o.sel_pts = {}; o.sel_cos = {}; o.sel_verdict = {};
    if (!keep_stages) {
        o.Hi = {}; o.H12i = {}; o.Fi = {}; o.sH = {}; o.sF = {}; o.hyp_pts = {}; o.hyp_cos = {}; o.verdict = {};
    }
}

// T6 over the scores of one model: the first iteration strictly above every earlier one, from 0.0f
inline int32_t select_best(const std::vector<float>& s, float* best) {
    int32_t it = -1;
    *best = 0.0f;
    for (size_t k = 0; k < s.size(); ++k) if (s[k] > *best) { *best = s[k]; it = (int32_t)k; }
    return it;
}
inline float score_ratio(float SH, float SF) { return SH + SF > 0.f ? SH / (SH + SF) : 0.f; }

// ---- the whole of one pair on the host: what the launch chain of iba_twoview.hip computes, in its order ----
inline void host_pair(const PairPrep& q, const iba_twoview_options& opt, PairRes& o, int32_t* sweeps30) {
    start_result(q, o);
    iba_twoview_result& r = o.r;
    const size_t N = (size_t)q.N, I = (size_t)opt.iterations;
    if (r.status) { finish(opt, opt.keep_stages != 0, o); return; }
    o.Hi.assign(9 * I, 0.f); o.H12i.assign(9 * I, 0.f); o.Fi.assign(9 * I, 0.f); o.sH.assign(I, 0.f); o.sF.assign(I, 0.f);
    o.hyp_pts.assign(24 * N, 0.f); o.hyp_cos.assign(8 * N, 0.f); o.verdict.assign(8 * N, 0);
    std::vector<double> ws((size_t)kWorkDoubles);
    const float invs = inv_sigma_square(opt.sigma);
    for (size_t it = 0; it < I; ++it) {
        float pn[32];
        for (int j = 0; j < 8; ++j) std::memcpy(pn + 4 * j, &q.mn[4 * (size_t)q.sets[8 * it + (size_t)j]], 4 * sizeof(float));
        if (h_hypothesis<1>(pn, q.T1, q.T2inv, ws.data(), &o.Hi[9 * it], &o.H12i[9 * it]) == kMaxSweeps) ++*sweeps30;
        if (f_hypothesis<1>(pn, q.T1, q.T2t, ws.data(), &o.Fi[9 * it]) == kMaxSweeps) ++*sweeps30;
        for (int k = 0; k < 9; ++k) { o.Hi[9 * it + k] = canon(o.Hi[9 * it + k]); o.H12i[9 * it + k] = canon(o.H12i[9 * it + k]); o.Fi[9 * it + k] = canon(o.Fi[9 * it + k]); }
        float sh = 0.f, sf = 0.f;
        for (size_t i = 0; i < N; ++i) {
            const float* m = &q.mxy[4 * i];
            score_h_match(&o.Hi[9 * it], &o.H12i[9 * it], m[0], m[1], m[2], m[3], invs, sh);
            score_f_match(&o.Fi[9 * it], m[0], m[1], m[2], m[3], invs, sf);
        }
        o.sH[it] = canon(sh); o.sF[it] = canon(sf);
    }
    r.best_it_H = select_best(o.sH, &r.SH);
    r.best_it_F = select_best(o.sF, &r.SF);
    std::vector<uint8_t> inH(N, 0), inF(N, 0);
    if (r.best_it_H >= 0) std::memcpy(r.H21, &o.Hi[9 * (size_t)r.best_it_H], sizeof(r.H21));
    if (r.best_it_F >= 0) std::memcpy(r.F21, &o.Fi[9 * (size_t)r.best_it_F], sizeof(r.F21));
    for (size_t i = 0; i < N; ++i) {
        const float* m = &q.mxy[4 * i];
        float dummy = 0.f;
        if (r.best_it_H >= 0 && score_h_match(r.H21, &o.H12i[9 * (size_t)r.best_it_H], m[0], m[1], m[2], m[3], invs, dummy)) { inH[i] = 1; ++r.n_inliers_H; }
        if (r.best_it_F >= 0 && score_f_match(r.F21, m[0], m[1], m[2], m[3], invs, dummy)) { inF[i] = 1; ++r.n_inliers_F; }
    }
    r.RH = score_ratio(r.SH, r.SF);
    r.model = r.RH > opt.rh_threshold ? 1 : 0;
    o.inlier = r.model ? inH : inF;
    float K[9];
    make_K(q.fx, q.fy, q.cx, q.cy, K);
    if ((r.model ? r.best_it_H : r.best_it_F) < 0) r.status = IBA_TWOVIEW_NO_MODEL;
    else if (r.model == 0) { r.n_hyp = 4; if (motions_from_f(r.F21, K, o.hyp_R, o.hyp_t) == kMaxSweeps) ++*sweeps30; }
    else {
        int sw = 0;
        if (!motions_from_h(r.H21, K, o.hyp_R, o.hyp_t, &sw)) { r.status = IBA_TWOVIEW_H_DEGENERATE; std::memset(o.hyp_R, 0, sizeof(o.hyp_R)); std::memset(o.hyp_t, 0, sizeof(o.hyp_t)); }
        else r.n_hyp = 8;
        if (sw == kMaxSweeps) ++*sweeps30;
    }
    if (r.status) { finish(opt, opt.keep_stages != 0, o); return; }
    const float sigma2 = opt.sigma * opt.sigma, th2 = (float)(4.0 * (double)sigma2);
    const int32_t n_inl = r.model ? r.n_inliers_H : r.n_inliers_F;
    for (int k = 0; k < r.n_hyp; ++k) {
        Cam cam;
        make_cam(K, o.hyp_R + 9 * k, o.hyp_t + 3 * k, cam);
        std::vector<uint32_t> keys;
        for (size_t i = 0; i < N; ++i) {
            if (!o.inlier[i]) continue;
            const float* m = &q.mxy[4 * i];
            float p[3], c;
            int sw = 0;
            const int v = check_rt_match(cam, q.fx, q.fy, q.cx, q.cy, m[0], m[1], m[2], m[3], th2, p, &c, &sw);
            if (sw == kMaxSweeps) ++*sweeps30;
            c = canon(c);
            o.verdict[(size_t)k * N + i] = (uint8_t)v; o.hyp_cos[(size_t)k * N + i] = c;
            std::memcpy(&o.hyp_pts[3 * ((size_t)k * N + i)], p, sizeof(p));
            if (v == 6) keys.push_back(cos_key(c));
        }
        r.n_good[k] = (int32_t)keys.size();
        r.cos_parallax[k] = 1.0f;
        if (!keys.empty()) {
            std::sort(keys.begin(), keys.end());
            r.cos_parallax[k] = canon(cos_unkey(keys[std::min<size_t>(50, keys.size() - 1)]));
        }
    }
    const Accept a = r.model ? accept_h(r.n_good, n_inl, opt.min_triangulated) : accept_f(r.n_good, n_inl, opt.min_triangulated);
    o.cand = a.cand; o.fail_before = a.fail_before; o.fail_after = a.fail_after;
    select_from_stages(o);
    finish(opt, opt.keep_stages != 0, o);
}

}  // namespace tv
}  // namespace iba

// the result object of iba_twoview_init and iba_debug_twoview_host
struct iba_twoview_batch {
    iba_twoview_options opt{};
    std::vector<iba::tv::PairRes> pair;
    int32_t sweeps30 = 0;                       // null-vector solves whose 30th sweep still rotated (debug)
    int32_t chunks = 0;                         // chains the call ran as (debug); 0 on the host
    float ms[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
};

// Sim3 RANSAC, the host half (include/iba_mi355x.h, iba_sim3*): the result object, the argument checks, Z6, the helpers (the constructor's walk, the set
// generator, iterate as a fold, the composition) and the host restatement of the whole call over iba_sim3_math.hpp. Plain C++: the sanitizer self-test
// compiles it with g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_sim3_math.hpp"

namespace iba {
namespace z3 {

// a checked job, prepared: Z6's iterations, the table coordinates of its correspondences gathered, the sets that will be read
struct JobPrep {
    int32_t N = 0, I = 0;                        // I == 0: TOO_FEW, nothing runs
    float K1[4], K2[4], T1[12], T2[12];
    std::vector<float> w1, w2;                   // 4 per correspondence: the world point of point1 / point2, 0
    std::vector<float> th;                       // 2 per correspondence
    std::vector<int32_t> sets;                   // 3 per iteration
};
struct JobRes {
    iba_sim3_result r;
    std::vector<int32_t> counts, ev_it;          // per iteration; per listed event
    std::vector<float> srt;                      // 13 per iteration: s, R, t
    std::vector<uint8_t> flags;                  // (max_events + 1) x N: the listed events, then the best
    std::vector<uint8_t> it_flags;               // keep_stages: iterations x N
};

inline uint64_t splitmix64(uint64_t& s) {
    s += 0x9E3779B97F4A7C15ull;
    uint64_t z = s;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
inline std::string make_sets(int32_t N, int32_t iterations, uint64_t seed, int32_t* out) {
    if (!out) return "out is NULL";
    if (N < 3) return "N = " + std::to_string(N) + " is below 3";
    if (iterations < 1 || iterations > IBA_SIM3_MAX_ITERATIONS) return "iterations = " + std::to_string(iterations) + " is outside 1.." + std::to_string(IBA_SIM3_MAX_ITERATIONS);
    std::vector<int32_t> all((size_t)N), avail;
    for (int32_t i = 0; i < N; ++i) all[(size_t)i] = i;
    uint64_t s = seed;
    for (int32_t it = 0; it < iterations; ++it) {
        avail = all;
        for (int j = 0; j < 3; ++j) {
            const size_t randi = (size_t)(splitmix64(s) % (uint64_t)avail.size());
            out[3 * it + j] = avail[randi];
            avail[randi] = avail.back();
            avail.pop_back();
        }
    }
    return "";
}

// ---- the checks: "" or the reason ----
inline std::string check_options(const iba_sim3_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_sim3_options)) return "opt->struct_size = " + std::to_string(o->struct_size) + ", this library's is " + std::to_string(sizeof(iba_sim3_options));
    if (!(o->probability > 0.0 && o->probability < 1.0)) return "probability is outside (0, 1)";
    if (o->min_inliers < 3) return "min_inliers < 3";
    if (o->max_iterations < 1 || o->max_iterations > IBA_SIM3_MAX_ITERATIONS) return "max_iterations = " + std::to_string(o->max_iterations) + " is outside 1.." + std::to_string(IBA_SIM3_MAX_ITERATIONS);
    if (o->max_events < 1 || o->max_events > IBA_SIM3_MAX_EVENTS) return "max_events = " + std::to_string(o->max_events) + " is outside 1.." + std::to_string(IBA_SIM3_MAX_EVENTS);
    return "";
}

// Z6; N >= 1 and checked options
inline int32_t budget(int32_t N, const iba_sim3_options& o) {
    if (N == o.min_inliers) return 1;
    const float eps = (float)o.min_inliers / (float)N;
    const double q = std::log(1.0 - o.probability) / std::log(1.0 - std::pow((double)eps, 3));
    if (!std::isfinite(q)) return o.max_iterations;
    const double c = std::ceil(q);
    if (c >= (double)o.max_iterations) return o.max_iterations;
    return c < 1.0 ? 1 : (int32_t)c;
}

inline std::string check_job(const iba_map_points& tb, const iba_sim3_job& j, const iba_sim3_options& o) {
    if (j.n < 0) return "n < 0";
    if (!j.Tcw12_1 || !j.Tcw12_2) return "a pose is NULL";
    for (int i = 0; i < 12; ++i) if (!std::isfinite(j.Tcw12_1[i]) || !std::isfinite(j.Tcw12_2[i])) return "a pose entry is not finite";
    const float k[8] = {j.fx1, j.fy1, j.cx1, j.cy1, j.fx2, j.fy2, j.cx2, j.cy2};
    for (int i = 0; i < 8; ++i) if (!std::isfinite(k[i])) return "an intrinsic is not finite";
    if (j.fx1 <= 0.f || j.fy1 <= 0.f || j.fx2 <= 0.f || j.fy2 <= 0.f) return "fx or fy <= 0";
    if (j.n && (!j.point1 || !j.point2 || !j.max_err1 || !j.max_err2)) return "point1, point2, max_err1 or max_err2 is NULL";
    for (int32_t i = 0; i < j.n; ++i) {
        if (j.point1[i] < 0 || j.point1[i] >= tb.n || j.point2[i] < 0 || j.point2[i] >= tb.n)
            return "correspondence " + std::to_string(i) + " names a point outside the table's " + std::to_string(tb.n);
        if (!std::isfinite(j.max_err1[i]) || !std::isfinite(j.max_err2[i])) return "the threshold of correspondence " + std::to_string(i) + " is not finite";
        for (int c = 0; c < 3; ++c)
            if (!std::isfinite(tb.xyz[3 * (size_t)j.point1[i] + c]) || !std::isfinite(tb.xyz[3 * (size_t)j.point2[i] + c])) return "the table point of correspondence " + std::to_string(i) + " is not finite";
    }
    if (j.n < o.min_inliers) return "";
    if (!j.sets) return "sets is NULL";
    const int32_t I = budget(j.n, o);
    for (int32_t it = 0; it < I; ++it) {
        const int32_t* s = j.sets + 3 * (size_t)it;
        for (int c = 0; c < 3; ++c) if (s[c] < 0 || s[c] >= j.n) return "set " + std::to_string(it) + " holds the index " + std::to_string(s[c]) + " outside [0, " + std::to_string(j.n) + ")";
        if (s[0] == s[1] || s[0] == s[2] || s[1] == s[2]) return "set " + std::to_string(it) + " repeats an index";
    }
    return "";
}
inline std::string check_call(const iba_map_points* tb, const iba_sim3_job* jobs, int32_t J, const iba_sim3_options* opt) {
    std::string why = check_options(opt);
    if (!why.empty()) return why;
    if (!tb) return "points is NULL";
    if (tb->n < 0 || (tb->n && !tb->xyz)) return "the table's n < 0 or its xyz is NULL";
    if (!jobs) return "jobs is NULL";
    if (J < 1) return "J < 1";
    for (int32_t b = 0; b < J; ++b) {
        why = check_job(*tb, jobs[b], *opt);
        if (!why.empty()) return "job " + std::to_string(b) + ": " + why;
    }
    return "";
}

inline void prepare(const iba_map_points& tb, const iba_sim3_job& j, const iba_sim3_options& o, JobPrep& q) {
    q.N = j.n; q.I = j.n < o.min_inliers ? 0 : budget(j.n, o);
    const float k1[4] = {j.fx1, j.fy1, j.cx1, j.cy1}, k2[4] = {j.fx2, j.fy2, j.cx2, j.cy2};
    std::memcpy(q.K1, k1, sizeof(k1)); std::memcpy(q.K2, k2, sizeof(k2));
    std::memcpy(q.T1, j.Tcw12_1, sizeof(q.T1)); std::memcpy(q.T2, j.Tcw12_2, sizeof(q.T2));
    q.w1.assign(4 * (size_t)q.N, 0.f); q.w2.assign(4 * (size_t)q.N, 0.f); q.th.resize(2 * (size_t)q.N);
    for (int32_t i = 0; i < q.N; ++i) {
        for (int c = 0; c < 3; ++c) { q.w1[4 * (size_t)i + c] = tb.xyz[3 * (size_t)j.point1[i] + c]; q.w2[4 * (size_t)i + c] = tb.xyz[3 * (size_t)j.point2[i] + c]; }
        q.th[2 * (size_t)i] = j.max_err1[i]; q.th[2 * (size_t)i + 1] = j.max_err2[i];
    }
    q.sets.clear();
    if (q.I) q.sets.assign(j.sets, j.sets + 3 * (size_t)q.I);
}

// the result of a job before anything ran: TOO_FEW stays as this
inline void start_result(const JobPrep& q, const iba_sim3_options& o, JobRes& out) {
    std::memset(&out.r, 0, sizeof(out.r));
    out.r.status = q.I ? IBA_SIM3_NO_MORE : IBA_SIM3_TOO_FEW; out.r.n = q.N; out.r.iterations = q.I; out.r.best_it = -1;
    out.counts.assign((size_t)q.I, 0); out.ev_it.clear(); out.srt.assign(13 * (size_t)q.I, 0.f);
    out.flags.assign((size_t)(o.max_events + 1) * (size_t)q.N, 0);
    out.it_flags.clear();
    if (o.keep_stages) out.it_flags.assign((size_t)q.I * (size_t)q.N, 0);
}
// status and the listed events from the scan's outputs
inline void finish(const iba_sim3_options& o, const int32_t* ev_it, int32_t n_events, int32_t best_it, int32_t best_n, JobRes& out) {
    out.r.n_events = n_events; out.r.n_listed = n_events < o.max_events ? n_events : o.max_events;
    out.r.best_it = best_it; out.r.best_inliers = best_n;
    out.r.status = n_events > 0 ? IBA_SIM3_OK : IBA_SIM3_NO_MORE;
    out.ev_it.assign(ev_it, ev_it + out.r.n_listed);
}

// ---- the whole job on the host: Z2, then per iteration Z3-Z5, then Z7 ----
inline void host_job(const JobPrep& q, const iba_sim3_options& o, JobRes& out) {
    start_result(q, o, out);
    if (!q.I) return;
    const size_t N = (size_t)q.N;
    std::vector<float> c1(3 * N), c2(3 * N), im(4 * N);
    for (size_t i = 0; i < N; ++i) {
        to_camera(q.T1, q.w1[4 * i], q.w1[4 * i + 1], q.w1[4 * i + 2], &c1[3 * i]);
        to_camera(q.T2, q.w2[4 * i], q.w2[4 * i + 1], q.w2[4 * i + 2], &c2[3 * i]);
        to_image(q.K1, c1[3 * i], c1[3 * i + 1], c1[3 * i + 2], &im[4 * i], &im[4 * i + 1]);
        to_image(q.K2, c2[3 * i], c2[3 * i + 1], c2[3 * i + 2], &im[4 * i + 2], &im[4 * i + 3]);
    }
    std::vector<float> T12(12 * (size_t)q.I), T21(12 * (size_t)q.I);
    std::vector<uint8_t> fl(N);
    const auto flags_of = [&](int32_t it, uint8_t* dst) {
        int32_t n = 0;
        for (size_t i = 0; i < N; ++i) {
            dst[i] = is_inlier(&T12[12 * (size_t)it], &T21[12 * (size_t)it], q.K1, q.K2, &c1[3 * i], &c2[3 * i], im[4 * i], im[4 * i + 1], im[4 * i + 2], im[4 * i + 3], q.th[2 * i], q.th[2 * i + 1]) ? 1 : 0;
            n += dst[i];
        }
        return n;
    };
    for (int32_t it = 0; it < q.I; ++it) {
        float P1[9], P2[9];
        for (int j = 0; j < 3; ++j) {
            const size_t idx = (size_t)q.sets[3 * (size_t)it + j];
            for (int r = 0; r < 3; ++r) { P1[3 * r + j] = c1[3 * idx + r]; P2[3 * r + j] = c2[3 * idx + r]; }
        }
        if (horn(P1, P2, o.fix_scale, &out.srt[13 * (size_t)it], &T12[12 * (size_t)it], &T21[12 * (size_t)it]) >= kMaxSweeps) ++out.r.sweep_cap_hits;
        out.counts[(size_t)it] = flags_of(it, o.keep_stages ? &out.it_flags[(size_t)it * N] : fl.data());
    }
    int32_t ev_it[IBA_SIM3_MAX_EVENTS], ne, bi, bn;
    scan(out.counts.data(), q.I, o.min_inliers, o.max_events, ev_it, &ne, &bi, &bn);
    finish(o, ev_it, ne, bi, bn, out);
    for (int32_t k = 0; k < out.r.n_listed; ++k) flags_of(ev_it[k], &out.flags[(size_t)k * N]);
    if (N) flags_of(bi, &out.flags[(size_t)o.max_events * N]);
}

// ---- iterate(n) as a fold over the counts ----
inline void iterate(const JobRes& o, int32_t min_inliers, int32_t from_it, int32_t n, int32_t* next_it, int32_t* event, int32_t* no_more) {
    *next_it = from_it; *event = -1; *no_more = 0;
    if (o.r.status == IBA_SIM3_TOO_FEW) { *no_more = 1; return; }
    int32_t best = 0, ne = 0;
    const int32_t I = o.r.iterations;
    for (int32_t it = 0; it < I && it < from_it + n; ++it) {
        const int32_t c = o.counts[(size_t)it];
        const bool replaces = c >= best, is_event = replaces && c > min_inliers;
        if (replaces) best = c;
        if (it >= from_it) {
            *next_it = it + 1;
            if (is_event) { *event = ne; return; }
        }
        if (is_event) ++ne;
    }
    *no_more = *next_it >= I ? 1 : 0;
}

// ---- the constructor's walk; "" or the reason ----
inline std::string correspondences(const iba_fuse_map* m, int32_t kf1, int32_t kf2, const int32_t* matches12, const int32_t* oct1, const int32_t* oct2, const float* ls1, const float* ls2,
                                   int32_t nl1, int32_t nl2, int32_t* index1, int32_t* point1, int32_t* point2, float* e1, float* e2, int32_t* n) {
    if (!m || !n) return "map or n is NULL";
    if (!m->kp_off || !m->holder || !m->bad) return "the map's kp_off, holder or bad is NULL";
    if (m->K < 1 || m->P < 0) return "the map's K < 1 or P < 0";
    if (kf1 < 0 || kf1 >= m->K || kf2 < 0 || kf2 >= m->K) return "kf1 or kf2 is outside the map's " + std::to_string(m->K) + " keyframes";
    if (!matches12 || !oct1 || !oct2 || !ls1 || !ls2) return "matches12, an octave array or a level table is NULL";
    if (nl1 < 1 || nl2 < 1) return "n_levels < 1";
    for (int32_t l = 0; l < nl1; ++l) if (!std::isfinite(ls1[l]) || ls1[l] < 0.f) return "level_sigma2_1 is not finite or negative";
    for (int32_t l = 0; l < nl2; ++l) if (!std::isfinite(ls2[l]) || ls2[l] < 0.f) return "level_sigma2_2 is not finite or negative";
    const int32_t a1 = m->kp_off[kf1], n1 = m->kp_off[kf1 + 1] - a1, a2 = m->kp_off[kf2], n2 = m->kp_off[kf2 + 1] - a2;
    if (n1 < 0 || n2 < 0) return "kp_off does not ascend";
    const auto index_in = [&](int32_t a, int32_t cnt, int32_t p) { for (int32_t i = 0; i < cnt; ++i) if (m->holder[a + i] == p) return i; return (int32_t)-1; };
    int32_t k = 0;
    for (int32_t i1 = 0; i1 < n1; ++i1) {
        const int32_t p2 = matches12[i1], p1 = m->holder[a1 + i1];
        if (p2 >= m->P || p1 >= m->P) return "keypoint " + std::to_string(i1) + " names a point outside the map's " + std::to_string(m->P);
        if (p2 < 0 || p1 < 0) continue;
        if (m->bad[p1] || m->bad[p2]) continue;
        const int32_t i_kf1 = index_in(a1, n1, p1), i_kf2 = index_in(a2, n2, p2);
        if (i_kf1 < 0 || i_kf2 < 0) continue;
        if (oct1[i_kf1] < 0 || oct1[i_kf1] >= nl1 || oct2[i_kf2] < 0 || oct2[i_kf2] >= nl2) return "an octave is outside its level table";
        if (index1) index1[k] = i1;
        if (point1) point1[k] = p1;
        if (point2) point2[k] = p2;
        if (e1) e1[k] = (float)(uint64_t)(9.210 * (double)ls1[oct1[i_kf1]]);       // Z1: truncated
        if (e2) e2[k] = (float)(uint64_t)(9.210 * (double)ls2[oct2[i_kf2]]);
        ++k;
    }
    *n = k;
    return "";
}

inline void compose(float s, const float* R, const float* t, const float* Tmw, double* s_out, double* R_out, double* t_out) {
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) {
            if (R_out) R_out[3 * i + j] = ((double)R[3 * i] * (double)Tmw[j] + (double)R[3 * i + 1] * (double)Tmw[4 + j]) + (double)R[3 * i + 2] * (double)Tmw[8 + j];
        }
        if (t_out) t_out[i] = (double)s * (((double)R[3 * i] * (double)Tmw[3] + (double)R[3 * i + 1] * (double)Tmw[7]) + (double)R[3 * i + 2] * (double)Tmw[11]) + (double)t[i];
    }
    if (s_out) *s_out = (double)s;
}

}  // namespace z3
}  // namespace iba

struct iba_sim3_batch {
    iba_sim3_options opt;
    std::vector<iba::z3::JobRes> job;
    int32_t chunks = 0, form = 0;
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
};

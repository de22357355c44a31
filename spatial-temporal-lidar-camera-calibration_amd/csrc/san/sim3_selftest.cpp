// Stand-alone sanitizer self-test of the Sim3 RANSAC's host half (csrc/iba_sim3_host.hpp) over the arithmetic the kernels compile
// (csrc/iba_sim3_math.hpp): Horn on a known similarity, the degenerate triple, Z5 at its edges, Z6, Z7, the argument checks, the whole call on the
// host on a seeded scene, and the helpers (the walk, the sets, iterate as a fold, the composition). Plain g++, no HIP:
//   make -C csrc san/sim3_selftest_asan && csrc/san/sim3_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../iba_sim3_host.hpp"

namespace z3 = iba::z3;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)lcg(s) / 16777216.0f; }

int main() {
    // ---- Horn: three points under a known similarity come back ----
    const double a = 0.3, sc = 1.7;
    const float Rt[9] = {(float)std::cos(a), (float)-std::sin(a), 0.f, (float)std::sin(a), (float)std::cos(a), 0.f, 0.f, 0.f, 1.f}, tt[3] = {0.5f, -0.25f, 1.0f};
    {
        const float X2[9] = {1.f, -2.f, 0.5f, 0.f, 1.f, 2.f, 4.f, 5.f, 6.5f};      // rows x, y, z; columns the points
        float X1[9], srt[13], T12[12], T21[12];
        for (int j = 0; j < 3; ++j)
            for (int i = 0; i < 3; ++i) X1[3 * i + j] = (float)(sc * ((double)Rt[3 * i] * X2[j] + (double)Rt[3 * i + 1] * X2[3 + j] + (double)Rt[3 * i + 2] * X2[6 + j]) + tt[i]);
        const int sweeps = z3::horn(X1, X2, 0, srt, T12, T21);
        CHECK(sweeps < z3::kMaxSweeps && std::fabs(srt[0] - (float)sc) < 1e-5f);
        for (int i = 0; i < 9; ++i) CHECK(std::fabs(srt[1 + i] - Rt[i]) < 1e-5f);
        for (int i = 0; i < 3; ++i) CHECK(std::fabs(srt[10 + i] - tt[i]) < 1e-4f);
        // T21 inverts T12 on a point
        const float p[3] = {0.3f, 0.7f, 5.f};
        float q[3], back[3];
        for (int i = 0; i < 3; ++i) q[i] = z3::dot3(T12[4 * i], T12[4 * i + 1], T12[4 * i + 2], p[0], p[1], p[2]) + T12[4 * i + 3];
        for (int i = 0; i < 3; ++i) back[i] = z3::dot3(T21[4 * i], T21[4 * i + 1], T21[4 * i + 2], q[0], q[1], q[2]) + T21[4 * i + 3];
        for (int i = 0; i < 3; ++i) CHECK(std::fabs(back[i] - p[i]) < 1e-4f);
        z3::horn(X1, X2, 1, srt, T12, T21);
        CHECK(srt[0] == 1.0f);
        // Z5 on that hypothesis: the exact image point is an inlier under any positive bound, a NaN bound or a zero bound admits nothing
        const float K[4] = {500.f, 500.f, 320.f, 240.f};
        z3::horn(X1, X2, 0, srt, T12, T21);
        const float c2[3] = {X2[0], X2[3], X2[6]}, c1[3] = {X1[0], X1[3], X1[6]};
        float u1, v1, u2, v2;
        z3::to_image(K, c1[0], c1[1], c1[2], &u1, &v1); z3::to_image(K, c2[0], c2[1], c2[2], &u2, &v2);
        CHECK(z3::is_inlier(T12, T21, K, K, c1, c2, u1, v1, u2, v2, 1.f, 1.f));
        CHECK(!z3::is_inlier(T12, T21, K, K, c1, c2, u1, v1, u2, v2, 0.f, 1.f) && !z3::is_inlier(T12, T21, K, K, c1, c2, u1, v1, u2, v2, 1.f, std::nanf("")));
        float ub, vb;                                               // a point at z == 0: 0 * inf is NaN, 0.1 * inf is inf; neither passes any bound
        z3::to_image(K, 0.f, 0.1f, 0.f, &ub, &vb);
        CHECK(ub != ub && std::isinf(vb) && !z3::is_inlier(T12, T21, K, K, c1, c2, ub, v1, u2, v2, 1e30f, 1e30f) && !z3::is_inlier(T12, T21, K, K, c1, c2, u1, v1, u2, vb, 1e30f, 1e30f));
    }
    {   // the degenerate triple: NaN everywhere, canonical
        const float P[9] = {0.5f, 0.5f, 0.5f, 0.25f, 0.25f, 0.25f, 4.f, 4.f, 4.f};
        float srt[13], T12[12], T21[12];
        z3::horn(P, P, 0, srt, T12, T21);
        uint32_t bits;
        for (int i = 0; i < 13; ++i) { std::memcpy(&bits, &srt[i], 4); CHECK(bits == 0x7FC00000u); }
        for (int i = 0; i < 12; ++i) { CHECK(T12[i] != T12[i] && T21[i] != T21[i]); }
    }
    // ---- Z6, Z7 ----
    iba_sim3_options o{};
    o.struct_size = (int32_t)sizeof(o); o.probability = 0.99; o.min_inliers = 20; o.max_iterations = 300; o.max_events = 1;
    CHECK(z3::check_options(&o).empty());
    CHECK(z3::budget(20, o) == 1 && z3::budget(25, o) == 7 && z3::budget(100, o) == 300 && z3::budget(2000000000, o) == 300);
    {
        const int32_t counts[8] = {0, 25, 21, 25, 3, 30, 30, 29};
        int32_t ev[IBA_SIM3_MAX_EVENTS], ne, bi, bn;
        z3::scan(counts, 8, 20, 2, ev, &ne, &bi, &bn);
        CHECK(ne == 4 && bi == 6 && bn == 30 && ev[0] == 1 && ev[1] == 3);
        z3::scan(counts, 1, 20, 2, ev, &ne, &bi, &bn);
        CHECK(ne == 0 && bi == 0 && bn == 0 && ev[0] == -1);
    }
    // ---- the checks ----
    {
        iba_sim3_options b = o;
        b.probability = 1.0; CHECK(!z3::check_options(&b).empty());
        b = o; b.min_inliers = 2; CHECK(!z3::check_options(&b).empty());
        b = o; b.max_iterations = IBA_SIM3_MAX_ITERATIONS + 1; CHECK(!z3::check_options(&b).empty());
        b = o; b.max_events = 0; CHECK(!z3::check_options(&b).empty());
        b = o; b.struct_size = 4; CHECK(!z3::check_options(&b).empty());
        CHECK(!z3::check_options(nullptr).empty());
    }
    // ---- a seeded scene through the whole call on the host ----
    uint32_t seed = 7;
    const int N = 48, n_out = 12;
    std::vector<float> xyz(6 * N);
    const float T1[12] = {1, 0, 0, 0.1f, 0, 1, 0, -0.2f, 0, 0, 1, 0.05f}, T2[12] = {1, 0, 0, -0.3f, 0, 1, 0, 0.1f, 0, 0, 1, 0.2f};
    for (int i = 0; i < N; ++i) {
        const float c2[3] = {3.f * unit(seed) - 1.5f, 2.f * unit(seed) - 1.f, 2.5f + 5.f * unit(seed)};
        float c1[3];
        for (int r = 0; r < 3; ++r) c1[r] = (float)(sc * ((double)Rt[3 * r] * c2[0] + (double)Rt[3 * r + 1] * c2[1] + (double)Rt[3 * r + 2] * c2[2]) + tt[r]);
        if (i >= N - n_out) { c1[0] = 4.f * unit(seed) - 2.f; c1[1] = 3.f * unit(seed) - 1.5f; c1[2] = 3.f + 7.f * unit(seed); }
        for (int r = 0; r < 3; ++r) { xyz[3 * i + r] = c1[r] - T1[4 * r + 3]; xyz[3 * (N + i) + r] = c2[r] - T2[4 * r + 3]; }
    }
    iba_map_points tb{};
    tb.xyz = xyz.data(); tb.n = 2 * N;
    std::vector<int32_t> p1(N), p2(N), sets(3 * 300);
    std::vector<float> e1(N, 9.f), e2(N, 13.f);
    for (int i = 0; i < N; ++i) { p1[i] = i; p2[i] = N + i; }
    CHECK(z3::make_sets(N, 300, 5, sets.data()).empty() && !z3::make_sets(2, 300, 5, sets.data()).empty() && !z3::make_sets(N, 0, 5, sets.data()).empty());
    for (int it = 0; it < 300; ++it) {
        const int32_t* s = &sets[3 * it];
        CHECK(s[0] >= 0 && s[0] < N && s[1] >= 0 && s[1] < N && s[2] >= 0 && s[2] < N && s[0] != s[1] && s[0] != s[2] && s[1] != s[2]);
    }
    iba_sim3_job job{};
    job.Tcw12_1 = T1; job.Tcw12_2 = T2; job.point1 = p1.data(); job.point2 = p2.data(); job.max_err1 = e1.data(); job.max_err2 = e2.data(); job.sets = sets.data(); job.n = N;
    job.fx1 = job.fy1 = job.fx2 = job.fy2 = 500.f; job.cx1 = job.cx2 = 320.f; job.cy1 = job.cy2 = 240.f;
    o.max_events = 3; o.keep_stages = 1;
    CHECK(z3::check_call(&tb, &job, 1, &o).empty());
    {   // every refusal of a job
        iba_sim3_job b = job;
        b.n = -1; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        b = job; b.Tcw12_1 = nullptr; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        b = job; b.fx2 = 0.f; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        b = job; b.cx1 = INFINITY; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        b = job; b.point2 = nullptr; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        b = job; b.sets = nullptr; CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        std::vector<int32_t> bad_p = p1; bad_p[3] = 2 * N;
        b = job; b.point1 = bad_p.data(); CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        std::vector<float> bad_e = e1; bad_e[2] = std::nanf("");
        b = job; b.max_err1 = bad_e.data(); CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        std::vector<int32_t> bad_s = sets; bad_s[4] = bad_s[3];
        b = job; b.sets = bad_s.data(); CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        bad_s = sets; bad_s[0] = N;
        b = job; b.sets = bad_s.data(); CHECK(!z3::check_call(&tb, &b, 1, &o).empty());
        CHECK(!z3::check_call(&tb, &job, 0, &o).empty() && !z3::check_call(nullptr, &job, 1, &o).empty() && !z3::check_call(&tb, nullptr, 1, &o).empty());
        b = job; b.n = 5; b.sets = nullptr; CHECK(z3::check_call(&tb, &b, 1, &o).empty());                 // too few: legal, no sets needed
    }
    z3::JobPrep prep;
    z3::JobRes res;
    z3::prepare(tb, job, o, prep);
    CHECK(prep.I == z3::budget(N, o) && prep.I > 1 && (int)prep.sets.size() == 3 * prep.I);
    z3::host_job(prep, o, res);
    CHECK(res.r.status == IBA_SIM3_OK && res.r.n_events >= 1 && res.r.best_inliers >= N - n_out - 2 && res.r.iterations == prep.I && (int)res.counts.size() == prep.I);
    CHECK(res.it_flags.size() == (size_t)prep.I * N && res.flags.size() == (size_t)4 * N);
    {   // the best's bytes are its iteration's bytes and count; its scale is the true one
        int n = 0;
        for (int i = 0; i < N; ++i) { CHECK(res.flags[3 * N + i] == res.it_flags[(size_t)res.r.best_it * N + i]); n += res.flags[3 * N + i]; }
        CHECK(n == res.r.best_inliers && std::fabs(res.srt[13 * (size_t)res.r.best_it] - (float)sc) < 1e-3f);
        // iterate as a fold: slices of 5 find event 0 where the scan listed it
        int32_t at = 0, event = -1, no_more = 0, guard = 0;
        while (event < 0 && !no_more && guard++ < 100) z3::iterate(res, o.min_inliers, at, 5, &at, &event, &no_more);
        CHECK(event == 0 && at == res.ev_it[0] + 1 && !no_more);
        z3::iterate(res, o.min_inliers, res.r.iterations, 5, &at, &event, &no_more);
        CHECK(event == -1 && no_more == 1 && at == res.r.iterations);
    }
    {   // too few
        iba_sim3_job b = job; b.n = 5;
        z3::prepare(tb, b, o, prep);
        z3::host_job(prep, o, res);
        int32_t at, event, no_more;
        z3::iterate(res, o.min_inliers, 0, 5, &at, &event, &no_more);
        CHECK(prep.I == 0 && res.r.status == IBA_SIM3_TOO_FEW && res.r.best_it == -1 && res.counts.empty() && event == -1 && no_more == 1 && at == 0);
    }
    // ---- the walk: a point absent from keyframe 2, a bad point, a point held twice, the truncated threshold ----
    {
        const int32_t kp_off[3] = {0, 5, 9};
        int32_t holder[9] = {0, 1, 2, 3, 1, /* keyframe 1 */ 10, 11, 11, 12};
        uint8_t bad[16] = {0};
        bad[3] = 1;
        iba_fuse_map m{};
        m.K = 2; m.kp_off = kp_off; m.holder = holder; m.P = 16; m.bad = bad;
        const int32_t matches[5] = {10, 11, 13, 12, 12}, oct1[5] = {0, 1, 0, 0, 2}, oct2[4] = {0, 2, 1, 0};
        const float ls[3] = {1.0f, 1.44f, 2.0736f};
        int32_t idx[5], q1[5], q2[5], n = -1;
        float m1[5], m2[5];
        CHECK(z3::correspondences(&m, 0, 1, matches, oct1, oct2, ls, ls, 3, 3, idx, q1, q2, m1, m2, &n).empty());
        // keypoint 0: (0, 10); 1: (1, 11), point 11 held twice in keyframe 1: its lowest keypoint (octave 2); 2: point 13 is in no keypoint of keyframe 1;
        // 3: point 3 is bad; 4: point 1 again, held twice in keyframe 0: its lowest keypoint is 1 (octave 1)
        CHECK(n == 3 && idx[0] == 0 && idx[1] == 1 && idx[2] == 4 && q1[2] == 1 && q2[2] == 12);
        CHECK(m1[0] == 9.f && m2[0] == 9.f && m1[1] == 13.f && m2[1] == 19.f && m1[2] == 13.f && m2[2] == 9.f);
        CHECK(!z3::correspondences(&m, 0, 2, matches, oct1, oct2, ls, ls, 3, 3, idx, q1, q2, m1, m2, &n).empty());
        CHECK(!z3::correspondences(&m, 0, 1, matches, oct1, oct2, ls, ls, 3, 2, idx, q1, q2, m1, m2, &n).empty());      // octave 2 outside a table of 2
        CHECK(!z3::correspondences(nullptr, 0, 1, matches, oct1, oct2, ls, ls, 3, 3, idx, q1, q2, m1, m2, &n).empty());
    }
    // ---- the composition ----
    {
        const float I12[12] = {1, 0, 0, 1, 0, 1, 0, 2, 0, 0, 1, 3};
        double so, Ro[9], to[3];
        z3::compose(2.f, Rt, tt, I12, &so, Ro, to);
        CHECK(so == 2.0);
        for (int i = 0; i < 9; ++i) CHECK(Ro[i] == (double)Rt[i]);
        for (int i = 0; i < 3; ++i) CHECK(std::fabs(to[i] - (2.0 * ((double)Rt[3 * i] * 1 + (double)Rt[3 * i + 1] * 2 + (double)Rt[3 * i + 2] * 3) + tt[i])) < 1e-12);
    }
    std::printf("sim3_selftest ok\n");
    return 0;
}

// Stand-alone sanitizer self-test of the two-view initialisation's host half (csrc/iba_twoview_host.hpp) over the arithmetic the kernels compile
// (csrc/iba_twoview_math.hpp): T1, the set generator, the argument checks, T2 on known matrices, and the whole call on the host on a synthetic
// pair that initialises, on a planar one, and on the pairs that end early. Plain g++, no HIP:
//   make -C csrc san/twoview_selftest_asan && csrc/san/twoview_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_twoview_host.hpp"

namespace tv = iba::tv;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static float unit(uint32_t& s) { return (float)(lcg(s) % 100000) / 100000.f; }

struct Scene {
    std::vector<float> xy1, xy2; std::vector<int32_t> m12, sets;
    iba_twoview_pair p{};
    // n points in front of two cameras one metre apart along x; planar: all at depth 8
    Scene(int32_t n, int32_t iterations, bool planar, uint32_t seed, int32_t unmatched_every = 7) : xy1(2 * (size_t)n), xy2(2 * (size_t)n), m12((size_t)n) {
        const float fx = 700.f, fy = 700.f, cx = 620.f, cy = 188.f;
        int32_t N = 0;
        for (int32_t i = 0; i < n; ++i) {
            const float X = -6.f + 12.f * unit(seed), Y = -2.f + 4.f * unit(seed), Z = planar ? 8.f + 0.25f * X : 6.f + 14.f * unit(seed);
            xy1[2 * (size_t)i] = fx * X / Z + cx; xy1[2 * (size_t)i + 1] = fy * Y / Z + cy;
            xy2[2 * (size_t)i] = fx * (X - 1.f) / Z + cx; xy2[2 * (size_t)i + 1] = fy * Y / Z + cy;
            m12[(size_t)i] = (unmatched_every && i % unmatched_every == unmatched_every - 1) ? -1 : i;
            if (m12[(size_t)i] >= 0) ++N;
        }
        if (N >= 8) { sets.resize(8 * (size_t)iterations); if (!tv::make_sets(N, iterations, 1234u + seed, sets.data()).empty()) std::abort(); }
        p.xy1 = xy1.data(); p.xy2 = xy2.data(); p.matches12 = m12.data(); p.sets = sets.empty() ? nullptr : sets.data(); p.n1 = n; p.n2 = n;
        p.fx = fx; p.fy = fy; p.cx = cx; p.cy = cy;
    }
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    iba_twoview_options o{};
    o.struct_size = (int32_t)sizeof(o); o.sigma = 1.f; o.iterations = 40; o.min_parallax_deg = 1.f; o.min_triangulated = 50; o.rh_threshold = 0.40f; o.keep_stages = 1;

    // ---- T1 on four points: means 2 and 3, mean deviations 1 and 2 ----
    {
        const float xy[8] = {1.f, 1.f, 3.f, 5.f, 1.f, 5.f, 3.f, 1.f};
        float out[8], T[9];
        tv::normalize(xy, 4, out, T);
        CHECK(T[0] == 1.f && T[4] == 0.5f && T[2] == -2.f && T[5] == -1.5f && T[8] == 1.f && T[1] == 0.f && T[6] == 0.f);
        CHECK(out[0] == -1.f && out[1] == -1.f && out[2] == 1.f && out[3] == 1.f);
        float Ti[9];
        tv::inv_affine_diag(T, Ti);
        CHECK(Ti[0] == 1.f && Ti[4] == 2.f && Ti[2] == 2.f && Ti[5] == 3.f && Ti[8] == 1.f);
    }
    // ---- the sets ----
    {
        std::vector<int32_t> s(8 * 50);
        CHECK(tv::make_sets(8, 50, 9, s.data()).empty());
        for (int it = 0; it < 50; ++it) { int seen = 0; for (int j = 0; j < 8; ++j) { CHECK(s[8 * it + j] >= 0 && s[8 * it + j] < 8); seen |= 1 << s[8 * it + j]; } CHECK(seen == 255); }
        CHECK(tv::make_sets(11, 50, 9, s.data()).empty());
        for (int it = 0; it < 50; ++it)
            for (int j = 0; j < 8; ++j) { CHECK(s[8 * it + j] >= 0 && s[8 * it + j] < 11); for (int k = 0; k < j; ++k) CHECK(s[8 * it + k] != s[8 * it + j]); }
        CHECK(!tv::make_sets(7, 50, 9, s.data()).empty() && !tv::make_sets(8, 0, 9, s.data()).empty() && !tv::make_sets(8, IBA_TWOVIEW_MAX_ITERATIONS + 1, 9, s.data()).empty());
        CHECK(!tv::make_sets(8, 5, 9, nullptr).empty());
    }
    // ---- T2: a matrix with a known null vector; the 3 x 3 SVD of a diagonal ----
    {
        const float A4[16] = {1.f, 0.f, 0.f, -1.f, 0.f, 2.f, 0.f, -2.f, 0.f, 0.f, 3.f, -3.f, 0.f, 0.f, 0.f, 0.f};   // rows orthogonal to (1, 1, 1, 1)
        float v[4];
        double G[16], V[16];
        for (int i = 0; i < 16; ++i) G[i] = (double)A4[i];
        const int sw = tv::null_vector<4, 4, 1, 1>(G, V, v);
        CHECK(sw < tv::kMaxSweeps);
        for (int i = 0; i < 4; ++i) CHECK(std::fabs(std::fabs(v[i]) - 0.5f) < 1e-6f && (v[i] > 0) == (v[0] > 0));
        const float D[9] = {2.f, 0.f, 0.f, 0.f, 5.f, 0.f, 0.f, 0.f, 3.f};
        float U[9], w[3], Vt[9];
        CHECK(tv::svd33(D, U, w, Vt) == 0 && w[0] == 5.f && w[1] == 3.f && w[2] == 2.f && Vt[1] == 1.f && Vt[5] == 1.f && Vt[6] == 1.f && U[3] == 1.f && U[7] == 1.f && U[2] == 1.f);
    }
    // ---- the checks ----
    Scene a(300, o.iterations, false, 1), pl(300, o.iterations, true, 2), few(9, o.iterations, false, 3, 3), none(0, o.iterations, false, 4);
    CHECK(a.p.sets && few.p.sets == nullptr);
    {
        iba_twoview_pair ps[4] = {a.p, pl.p, few.p, none.p};
        ps[3].xy1 = nullptr; ps[3].xy2 = nullptr; ps[3].matches12 = nullptr;
        CHECK(tv::check_call(ps, 4, &o).empty());
        CHECK(!tv::check_call(nullptr, 4, &o).empty() && !tv::check_call(ps, 0, &o).empty() && !tv::check_call(ps, 4, nullptr).empty());
        { iba_twoview_options b = o; b.struct_size -= 4; CHECK(!tv::check_options(&b).empty()); }
        { iba_twoview_options b = o; b.sigma = 0.f; CHECK(!tv::check_options(&b).empty()); b.sigma = nan; CHECK(!tv::check_options(&b).empty()); b.sigma = inf; CHECK(!tv::check_options(&b).empty()); }
        { iba_twoview_options b = o; b.iterations = 0; CHECK(!tv::check_options(&b).empty()); b.iterations = IBA_TWOVIEW_MAX_ITERATIONS + 1; CHECK(!tv::check_options(&b).empty()); }
        { iba_twoview_options b = o; b.min_triangulated = -1; CHECK(!tv::check_options(&b).empty()); }
        { iba_twoview_options b = o; b.min_parallax_deg = nan; CHECK(!tv::check_options(&b).empty()); b = o; b.rh_threshold = inf; CHECK(!tv::check_options(&b).empty()); }
        { iba_twoview_pair x = a.p; x.n1 = -1; CHECK(!tv::check_pair(x, o.iterations).empty()); x = a.p; x.n2 = IBA_ORB_MATCH_MAX_KEYPOINTS + 1; CHECK(!tv::check_pair(x, o.iterations).empty()); }
        { iba_twoview_pair x = a.p; x.xy2 = nullptr; CHECK(!tv::check_pair(x, o.iterations).empty()); x = a.p; x.matches12 = nullptr; CHECK(!tv::check_pair(x, o.iterations).empty()); }
        { iba_twoview_pair x = a.p; x.sets = nullptr; CHECK(!tv::check_pair(x, o.iterations).empty()); }
        { iba_twoview_pair x = a.p; x.fx = 0.f; CHECK(!tv::check_pair(x, o.iterations).empty()); x = a.p; x.fy = nan; CHECK(!tv::check_pair(x, o.iterations).empty()); x = a.p; x.cx = inf; CHECK(!tv::check_pair(x, o.iterations).empty()); }
        { Scene x(300, o.iterations, false, 1); x.xy1[11] = nan; CHECK(!tv::check_pair(x.p, o.iterations).empty()); x.xy1[11] = 0.f; x.xy2[4] = inf; CHECK(!tv::check_pair(x.p, o.iterations).empty()); }
        { Scene x(300, o.iterations, false, 1); x.m12[5] = 300; CHECK(!tv::check_pair(x.p, o.iterations).empty()); x.m12[5] = 299; CHECK(tv::check_pair(x.p, o.iterations).empty()); }
        { Scene x(300, o.iterations, false, 1); x.sets[13] = -1; CHECK(!tv::check_pair(x.p, o.iterations).empty()); x.sets[13] = x.sets[12]; CHECK(!tv::check_pair(x.p, o.iterations).empty()); }
        { Scene x(300, o.iterations, false, 1); int32_t N = 0; for (int32_t m : x.m12) N += m >= 0; x.sets[8] = N; CHECK(!tv::check_pair(x.p, o.iterations).empty()); }
    }
    // ---- the whole call on the host ----
    int32_t hits = 0;
    {
        tv::PairPrep q; tv::PairRes r;
        tv::prepare(a.p, o.iterations, q);
        tv::host_pair(q, o, r, &hits);
        CHECK(r.r.status == IBA_TWOVIEW_OK && r.r.model == 0 && r.r.n_hyp == 4 && r.r.chosen >= 0 && r.r.n_matches == q.N && r.r.RH < 0.4f);
        CHECK(r.r.n_inliers_F == q.N && r.r.n_good[r.r.chosen] == q.N && r.r.parallax_deg[r.r.chosen] > 1.f);
        CHECK(std::fabs(std::fabs(r.r.t21[0]) - 1.f) < 1e-3f && std::fabs(r.r.R21[0] - 1.f) < 1e-3f && std::fabs(r.r.R21[4] - 1.f) < 1e-3f);
        int32_t n_tri = 0;
        for (int32_t i = 0; i < a.p.n1; ++i) { n_tri += r.tri[(size_t)i]; if (a.m12[(size_t)i] < 0) CHECK(!r.tri[(size_t)i] && r.points[3 * (size_t)i + 2] == 0.f); else CHECK(r.points[3 * (size_t)i + 2] > 0.f); }
        CHECK(n_tri > 200 && r.Hi.size() == 9 * (size_t)o.iterations && r.verdict.size() == 8 * (size_t)q.N);
        iba_twoview_options o2 = o; o2.keep_stages = 0;
        tv::PairRes r2;
        tv::host_pair(q, o2, r2, &hits);
        CHECK(r2.Hi.empty() && r2.verdict.empty() && std::memcmp(&r2.r, &r.r, sizeof(r.r)) == 0 && r2.points == r.points);
        o2 = o; o2.min_parallax_deg = 60.f;
        tv::host_pair(q, o2, r2, &hits);
        CHECK(r2.r.status == IBA_TWOVIEW_LOW_PARALLAX && r2.r.chosen == r.r.chosen && r2.r.R21[0] == 0.f);
    }
    {
        tv::PairPrep q; tv::PairRes r;
        tv::prepare(pl.p, o.iterations, q);
        tv::host_pair(q, o, r, &hits);
        CHECK(r.r.model == 1 && r.r.RH > 0.4f && r.r.n_inliers_H == q.N && (r.r.status == IBA_TWOVIEW_OK || r.r.status == IBA_TWOVIEW_H_DEGENERATE || r.r.status == IBA_TWOVIEW_NO_CLEAR_WINNER));
        if (r.r.status == IBA_TWOVIEW_OK) CHECK(r.r.n_hyp == 8 && std::fabs(std::fabs(r.r.t21[0]) - 1.f) < 1e-2f);
    }
    {
        tv::PairPrep q; tv::PairRes r;
        tv::prepare(few.p, o.iterations, q);
        tv::host_pair(q, o, r, &hits);
        CHECK(q.N == 6 && r.r.status == IBA_TWOVIEW_TOO_FEW_MATCHES && r.r.chosen == -1 && r.r.best_it_H == -1 && r.list.size() == 12 && r.points.size() == 27);
        iba_twoview_pair e = none.p;
        e.xy1 = nullptr; e.xy2 = nullptr; e.matches12 = nullptr;
        tv::prepare(e, o.iterations, q);
        tv::host_pair(q, o, r, &hits);
        CHECK(q.N == 0 && r.r.status == IBA_TWOVIEW_TOO_FEW_MATCHES && r.points.empty());
    }
    {   // every keypoint of frame 1 in one place: T1 is not finite, no hypothesis scores, no model; the sweep cap is reached and counted
        Scene x(40, o.iterations, false, 5, 0);
        for (size_t i = 0; i < x.xy1.size(); i += 2) { x.xy1[i] = 100.f; x.xy1[i + 1] = 50.f; }
        tv::PairPrep q; tv::PairRes r;
        int32_t h2 = 0;
        tv::prepare(x.p, o.iterations, q);
        tv::host_pair(q, o, r, &h2);
        CHECK(r.r.status == IBA_TWOVIEW_NO_MODEL && r.r.best_it_H == -1 && r.r.best_it_F == -1 && r.r.SH == 0.f && r.r.RH == 0.f && h2 > 0);
    }
    CHECK(hits == 0);
    std::printf("twoview_selftest ok\n");
    return 0;
}

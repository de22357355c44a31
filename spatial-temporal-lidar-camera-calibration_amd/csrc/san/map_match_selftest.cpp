// Stand-alone sanitizer self-test of the local-map point matching's host half (csrc/iba_map_match_host.hpp) over the float decisions the kernels
// compile (csrc/iba_map_match_math.hpp): L1 and L2 at their edges, the acceptance of L4, the argument checks, the whole call on the host against a
// literal sequential scan, the edge helper and the chunk planner. Plain g++, no HIP:
//   make -C csrc san/map_match_selftest_asan && csrc/san/map_match_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_map_match_host.hpp"

namespace mapm = iba::mapm;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- L1 / L2 with the identity pose: Pc = P, Ow = 0, a point (0, 0, z) has dist = z and view_cos = n_z ----
    mapm::Camera c{};
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) c.T[k] = I[k];
    mapm::camera_centre(c.T, c.Ow);
    CHECK(c.Ow[0] == 0.f && c.Ow[1] == 0.f && c.Ow[2] == 0.f);
    c.fx = c.fy = 500.f; c.cx = 320.f; c.cy = 240.f; c.min_x = 0.f; c.max_x = 640.f; c.min_y = 0.f; c.max_y = 480.f;
    c.th = 1.f; c.view_cos_limit = 0.5f; c.n_levels = 8;
    c.sf[0] = 1.f;
    for (int n = 1; n < 8; ++n) c.sf[n] = c.sf[n - 1] * 1.2f;
    const float Z[3] = {0.f, 0.f, 1.f};
    auto view = [&](float x, float y, float z, const float* n, float mn, float mx) { const float P[3] = {x, y, z}; return mapm::frustum(c, P, n, mn, mx); };
    CHECK(view(0, 0, -4, Z, 0.1f, 10).status == IBA_MAP_MATCH_DEPTH);
    CHECK(view(1, 1, 0.f, Z, 0.1f, 10).status == IBA_MAP_MATCH_NOT_FINITE && view(1, 1, -0.f, Z, 0.1f, 10).status == IBA_MAP_MATCH_NOT_FINITE);
    CHECK(view(10, 0, 5, Z, 0.1f, 10).status == IBA_MAP_MATCH_BOUNDS);
    { const mapm::View w = view(-3.2f, 0, 5, Z, 0.1f, 10); CHECK(w.status == IBA_MAP_MATCH_IN_VIEW && w.u == 0.f); }
    { const mapm::View w = view(3.2f, 0, 5, Z, 0.1f, 10); CHECK(w.status == IBA_MAP_MATCH_IN_VIEW && w.u == 640.f && w.v == 240.f); }
    const float near = 0.8f * 5.f, far = 1.2f * 5.f;
    CHECK(view(0, 0, near, Z, 5.f, 10).status == IBA_MAP_MATCH_IN_VIEW && view(0, 0, std::nextafter(near, 0.f), Z, 5.f, 10).status == IBA_MAP_MATCH_DISTANCE);
    CHECK(view(0, 0, far, Z, 0.1f, 5.f).status == IBA_MAP_MATCH_IN_VIEW && view(0, 0, std::nextafter(far, inf), Z, 0.1f, 5.f).status == IBA_MAP_MATCH_DISTANCE);
    { const float n[3] = {0, 0, 0.5f}; const mapm::View w = view(0, 0, 4, n, 0.1f, 10); CHECK(w.status == IBA_MAP_MATCH_IN_VIEW && w.view_cos == 0.5f); }
    { const float n[3] = {0, 0, std::nextafter(0.5f, 0.f)}; CHECK(view(0, 0, 4, n, 0.1f, 10).status == IBA_MAP_MATCH_ANGLE); }
    CHECK(view(0, 0, 2, Z, 0.1f, 2.f * c.sf[3]).level == 3 && view(0, 0, 2, Z, 0.1f, 2.f * std::nextafter(c.sf[3], inf)).level == 4);
    CHECK(view(0, 0, 2, Z, 0.1f, 2.f).level == 0 && view(0, 0, 2, Z, 0.1f, 2.f * c.sf[7] * 1.5f).level == 7);
    CHECK(mapm::query_radius(0.998f, 1.f, 1.2f) == 2.5f * 1.2f && mapm::query_radius(std::nextafter(0.998f, 0.f), 1.f, 1.2f) == 4.f * 1.2f);     // (float)0.998 > 0.998
    CHECK(mapm::query_radius(0.5f, 3.f, 1.44f) == (4.f * 3.f) * 1.44f && mapm::query_radius(1.f, 1.f, 1.f) == 2.5f);
    CHECK(mapm::div_f(1.f, 3.f) == 1.f / 3.f && mapm::div_f(1.f, 0.f) == inf && !mapm::finite_f(nan) && !mapm::finite_f(-inf) && mapm::finite_f(3e38f));
    // ---- L4's acceptance ----
    CHECK(mapm::accept(true, 30, 0, 256, -1, 100, 0.8f) && !mapm::accept(false, 256, -1, 256, -1, 256, 2.f));
    CHECK(!mapm::accept(true, 20, 0, 20, 0, 100, 0.8f) && mapm::accept(true, 20, 1, 20, 2, 100, 0.8f) && mapm::accept(true, 0, 0, 0, 0, 100, 0.8f));
    CHECK(mapm::accept(true, 100, 0, 256, -1, 100, 0.8f) && !mapm::accept(true, 101, 0, 256, -1, 100, 0.8f));
    CHECK(mapm::accept(true, 40, 0, 60, 0, 100, 0.8f) && !mapm::accept(true, 50, 0, 60, 0, 100, 0.8f));

    // ---- a seeded call: frames, table, jobs ----
    uint32_t seed = 3;
    const int32_t n_kp = 300, P = 120;
    std::vector<float> xy(2 * n_kp), angle(n_kp, 0.f), xyz(3 * P), normal(3 * P), mn(P), mx(P);
    std::vector<int32_t> octave(n_kp);
    std::vector<uint8_t> kdesc(32 * n_kp), pdesc(32 * P);
    for (int32_t p = 0; p < P; ++p) {
        xyz[3 * p] = (float)(lcg(seed) % 800) * 0.01f - 4.f; xyz[3 * p + 1] = (float)(lcg(seed) % 600) * 0.01f - 3.f; xyz[3 * p + 2] = (float)(lcg(seed) % 1200) * 0.01f - 1.f;
        const float d = std::sqrt(xyz[3 * p] * xyz[3 * p] + xyz[3 * p + 1] * xyz[3 * p + 1] + xyz[3 * p + 2] * xyz[3 * p + 2]) + 1e-3f;
        for (int k = 0; k < 3; ++k) normal[3 * p + k] = xyz[3 * p + k] / d;
        mx[p] = d * (0.7f + (float)(lcg(seed) % 300) * 0.01f); mn[p] = mx[p] / 3.5f;
        for (int b = 0; b < 32; ++b) pdesc[32 * p + b] = (uint8_t)lcg(seed);
    }
    for (int32_t i = 0; i < n_kp; ++i) {                      // keypoints near the projections of the points, descriptors a few bits away
        const int32_t p = i % P;
        const float z = xyz[3 * p + 2] > 0.5f ? xyz[3 * p + 2] : 0.5f;
        xy[2 * i] = 500.f * xyz[3 * p] / z + 320.f + (float)(lcg(seed) % 7) - 3.f; xy[2 * i + 1] = 500.f * xyz[3 * p + 1] / z + 240.f + (float)(lcg(seed) % 7) - 3.f;
        octave[i] = (int32_t)(lcg(seed) % 4);
        for (int b = 0; b < 32; ++b) kdesc[32 * i + b] = pdesc[32 * p + b];
        for (int f = (int)(lcg(seed) % 60); f > 0; --f) kdesc[32 * i + (int)(lcg(seed) % 32)] ^= (uint8_t)(1u << (lcg(seed) % 8));
    }
    iba_orb_frame fr[2] = {};
    fr[0].xy = xy.data(); fr[0].octave = octave.data(); fr[0].angle = angle.data(); fr[0].desc = kdesc.data(); fr[0].n = n_kp;
    fr[0].min_x = 0.f; fr[0].max_x = 640.f; fr[0].min_y = 0.f; fr[0].max_y = 480.f;
    fr[1] = fr[0]; fr[1].n = 0; fr[1].xy = nullptr; fr[1].octave = nullptr; fr[1].angle = nullptr; fr[1].desc = nullptr;
    iba_map_points tb{xyz.data(), normal.data(), mn.data(), mx.data(), pdesc.data(), P};
    std::vector<int32_t> list(77);
    std::vector<uint8_t> skip(77), occ(n_kp);
    for (int32_t k = 0; k < 77; ++k) { list[(size_t)k] = (int32_t)(lcg(seed) % P); skip[(size_t)k] = lcg(seed) % 9 == 0; }
    for (int32_t i = 0; i < n_kp; ++i) occ[(size_t)i] = lcg(seed) % 11 == 0;
    iba_map_match_job jobs[4] = {};
    for (iba_map_match_job& b : jobs) { b.frame = 0; b.n_levels = 8; b.n_points = P; b.th = 1.f; b.fx = b.fy = 500.f; b.cx = 320.f; b.cy = 240.f; b.Tcw12 = I; b.scale_factors = c.sf; }
    jobs[1].n_points = 77; jobs[1].points = list.data(); jobs[1].skip = skip.data(); jobs[1].occupied = occ.data(); jobs[1].th = 3.f;
    jobs[2].n_points = 0; jobs[2].points = list.data();
    jobs[3].frame = 1;
    iba_map_match_options o{};
    o.struct_size = (int32_t)sizeof(o); o.th_high = 100; o.nn_ratio = 0.8f; o.view_cos_limit = 0.5f; o.keep_stages = 1;

    // ---- the checks ----
    CHECK(mapm::check_options(&o).empty() && !mapm::check_options(nullptr).empty());
    { iba_map_match_options b = o; b.struct_size -= 4; CHECK(!mapm::check_options(&b).empty()); }
    { iba_map_match_options b = o; b.th_high = 257; CHECK(!mapm::check_options(&b).empty()); b.th_high = 256; CHECK(mapm::check_options(&b).empty()); }
    { iba_map_match_options b = o; b.nn_ratio = 0.f; CHECK(!mapm::check_options(&b).empty()); b.nn_ratio = nan; CHECK(!mapm::check_options(&b).empty()); }
    { iba_map_match_options b = o; b.view_cos_limit = inf; CHECK(!mapm::check_options(&b).empty()); }
    CHECK(mapm::check_points(&tb).empty() && !mapm::check_points(nullptr).empty());
    { iba_map_points b = tb; b.n = -1; CHECK(!mapm::check_points(&b).empty()); b = tb; b.desc = nullptr; CHECK(!mapm::check_points(&b).empty()); }
    { iba_map_points b{}; CHECK(mapm::check_points(&b).empty()); }
    { std::vector<float> bad(xyz); bad[7] = nan; iba_map_points b = tb; b.xyz = bad.data(); CHECK(!mapm::check_points(&b).empty()); bad[7] = 2e6f; CHECK(!mapm::check_points(&b).empty()); }
    { std::vector<float> bad(mx); bad[5] = inf; iba_map_points b = tb; b.max_dist = bad.data(); CHECK(!mapm::check_points(&b).empty()); }
    CHECK(mapm::check_jobs(fr, 2, P, jobs, 4).empty());
    CHECK(!mapm::check_jobs(fr, 2, P, nullptr, 4).empty() && !mapm::check_jobs(fr, 2, P, jobs, 0).empty());
    { iba_map_match_job b = jobs[0]; b.frame = 2; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_map_match_job b = jobs[0]; b.n_levels = 0; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); b.n_levels = 65; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_map_match_job b = jobs[0]; b.n_points = P - 1; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); b.n_points = -1; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_map_match_job b = jobs[0]; b.th = nan; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); b = jobs[0]; b.fx = 2e6f; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_map_match_job b = jobs[0]; b.Tcw12 = nullptr; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { float T[12]; for (int k = 0; k < 12; ++k) T[k] = I[k]; T[7] = inf; iba_map_match_job b = jobs[0]; b.Tcw12 = T; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { const float sf[3] = {1.f, 1.2f, 1.2f}; iba_map_match_job b = jobs[0]; b.scale_factors = sf; b.n_levels = 3; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); b.n_levels = 2; CHECK(mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { const float sf[2] = {1.1f, 1.2f}; iba_map_match_job b = jobs[0]; b.scale_factors = sf; b.n_levels = 2; CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }
    { std::vector<int32_t> bad(list); bad[9] = P; iba_map_match_job b = jobs[1]; b.points = bad.data(); CHECK(!mapm::check_jobs(fr, 2, P, &b, 1).empty()); }

    // ---- the whole call on the host, against a literal sequential scan over the kept lists ----
    mapm::Result res;
    res.opt = o;
    res.job.resize(4);
    mapm::host_call(&res, fr, 2, &tb, jobs, 4);
    CHECK(res.status.size() == (size_t)(P + 77 + 0 + P) && res.point_of.size() == (size_t)(3 * n_kp));
    int total_matches = 0, refused_by_ratio = 0;
    for (int32_t j = 0; j < 4; ++j) {
        const mapm::JobRes& jr = res.job[(size_t)j];
        const iba_map_match_job& b = jobs[j];
        const iba_orb_frame& f = fr[b.frame];
        const int32_t* off = &res.off[jr.slot_base + (size_t)j];
        std::vector<uint8_t> has((size_t)f.n, 0);
        if (b.occupied) for (int32_t i = 0; i < f.n; ++i) has[(size_t)i] = b.occupied[i];
        int counted[IBA_MAP_MATCH_N_STATUS] = {}, n_matches = 0;
        for (int32_t k = 0; k < b.n_points; ++k) {
            const size_t s = jr.slot_base + (size_t)k;
            ++counted[res.status[s]];
            CHECK((b.skip && b.skip[k]) == (res.status[s] == IBA_MAP_MATCH_SKIPPED));
            if (res.status[s] != IBA_MAP_MATCH_IN_VIEW) { CHECK(off[k + 1] == off[k] && res.match[s] == -1 && res.radius[s] == 0.f); continue; }
            CHECK(res.radius[s] == mapm::query_radius(res.view_cos[s], b.th, b.scale_factors[res.level[s]]));
            int best = 256, lvl = -1, best2 = 256, lvl2 = -1, idx = -1;
            for (int32_t e = off[k]; e < off[k + 1]; ++e) {
                const int32_t i = res.cand[jr.cand_base + (size_t)e];
                const int d = (int)res.cand_dist[jr.cand_base + (size_t)e];
                CHECK(i >= 0 && i < f.n && (f.octave[i] == res.level[s] || f.octave[i] == res.level[s] - 1));
                CHECK(d == mapm::host_hamming(pdesc.data() + 32 * (size_t)(b.points ? b.points[k] : k), f.desc + 32 * (size_t)i));
                if (has[(size_t)i]) continue;
                if (d < best) { best2 = best; best = d; lvl2 = lvl; lvl = f.octave[i]; idx = i; }
                else if (d < best2) { lvl2 = f.octave[i]; best2 = d; }
            }
            int want = -1;
            if (idx >= 0 && best <= o.th_high) {
                if (lvl == lvl2 && (float)best > o.nn_ratio * (float)best2) ++refused_by_ratio;
                else want = idx;
            }
            CHECK(res.match[s] == want && res.dist[s] == (want >= 0 ? best : -1));
            if (want >= 0) { has[(size_t)want] = 1; ++n_matches; CHECK(res.point_of[jr.kpo_base + (size_t)want] == k); }
        }
        for (int st = 0; st < IBA_MAP_MATCH_N_STATUS; ++st) CHECK(counted[st] == jr.counts.status[st]);
        CHECK(jr.counts.n_matches == n_matches && jr.counts.n_candidates == off[b.n_points] && jr.counts.n_points == b.n_points);
        total_matches += n_matches;
    }
    CHECK(total_matches > 20 && res.job[0].counts.status[IBA_MAP_MATCH_IN_VIEW] > 20 && res.job[3].counts.n_candidates == 0 && res.job[2].counts.n_points == 0);
    (void)refused_by_ratio;

    // ---- L6 ----
    {
        const mapm::JobRes& jr = res.job[1];
        std::vector<int32_t> prior((size_t)n_kp, -1);
        prior[3] = 5; prior[10] = 7;
        std::vector<float> exyz(3 * n_kp), eobs(2 * n_kp), ew(n_kp);
        std::vector<int32_t> eidx(n_kp);
        const float lv[4] = {1.f, 0.5f, 0.25f, 0.125f};
        int32_t n = -1;
        CHECK(mapm::pose_edges(prior.data(), &res.point_of[jr.kpo_base], list.data(), 77, xyz.data(), P, xy.data(), octave.data(), n_kp, lv, 4, exyz.data(), eobs.data(), ew.data(), eidx.data(), &n).empty());
        int32_t want = 0;
        for (int32_t i = 0; i < n_kp; ++i) {
            const int32_t k = res.point_of[jr.kpo_base + (size_t)i];
            const int32_t p = k >= 0 ? list[(size_t)k] : prior[(size_t)i];
            if (p < 0) continue;
            CHECK(eidx[(size_t)want] == i && exyz[3 * (size_t)want] == xyz[3 * (size_t)p] && eobs[2 * (size_t)want + 1] == xy[2 * (size_t)i + 1] && ew[(size_t)want] == lv[octave[(size_t)i]]);
            ++want;
        }
        CHECK(n == want && want >= jr.counts.n_matches);
        CHECK(!mapm::pose_edges(prior.data(), nullptr, list.data(), 77, xyz.data(), P, xy.data(), octave.data(), n_kp, lv, 3, exyz.data(), eobs.data(), ew.data(), eidx.data(), &n).empty());
        prior[3] = P;
        CHECK(!mapm::pose_edges(prior.data(), nullptr, list.data(), 77, xyz.data(), P, xy.data(), octave.data(), n_kp, lv, 4, exyz.data(), eobs.data(), ew.data(), eidx.data(), &n).empty());
        CHECK(!mapm::pose_edges(nullptr, nullptr, nullptr, 77, xyz.data(), P, xy.data(), octave.data(), n_kp, lv, 4, exyz.data(), eobs.data(), ew.data(), eidx.data(), &n).empty());
        CHECK(mapm::pose_edges(nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, nullptr, nullptr, &n).empty() && n == 0);
    }

    // ---- the chunk planner ----
    {
        const std::vector<int64_t> cnd = {10, 0, 25, 5, 5, 100, 1};
        std::vector<int32_t> cut = mapm::plan_chunks(cnd, 1ull << 30);
        CHECK(cut.size() == 2 && cut[0] == 0 && cut[1] == 7);
        cut = mapm::plan_chunks(cnd, 1);
        CHECK(cut.size() == 8);
        cut = mapm::plan_chunks(cnd, 35 * IBA_MAP_MATCH_BYTES_PER_CANDIDATE);
        CHECK(cut.size() == 5 && cut[1] == 3 && cut[2] == 5 && cut[3] == 6 && cut[4] == 7);
    }
    std::printf("map_match_selftest ok\n");
    return 0;
}

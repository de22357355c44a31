// Stand-alone sanitizer self-test of the new-map-point creation's host half (csrc/iba_triangulate_host.hpp) over the float decisions the kernels
// compile (csrc/iba_triangulate_math.hpp): R1 at the baseline ratio, R3's gates and key, R4-R6 on exact geometry and at the guards no call
// reaches (DEGENERATE, ZERO_DIST), the node order, the argument checks, the whole call on the host against an independent per-slot evaluation with
// R7 applied afterwards, the median depth and the chunk planner. Plain g++, no HIP:
//   make -C csrc san/triangulate_selftest_asan && csrc/san/triangulate_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_triangulate_host.hpp"

namespace trg = iba::trg;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    const float TX[12] = {1, 0, 0, -0.5f, 0, 1, 0, 0, 0, 0, 1, 0};       // centre (0.5, 0, 0)
    const float TZ[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, -0.5f};       // centre (0, 0, 0.5)
    trg::Kf k0, kx, kz;
    trg::make_kf(I, 512.f, 512.f, 320.f, 240.f, 5.f, k0);
    trg::make_kf(TX, 512.f, 512.f, 320.f, 240.f, 50.f, kx);
    trg::make_kf(TZ, 512.f, 512.f, 320.f, 240.f, 5.f, kz);
    CHECK(kx.Ow[0] == 0.5f && kx.Ow[1] == 0.f && kz.Ow[2] == 0.5f && k0.invfx == 1.f / 512.f);
    trg::Scales sc{};
    sc.n_levels = 8; sc.scale_factor = 1.2f; sc.sf[0] = 1.f;
    for (int n = 1; n < 8; ++n) sc.sf[n] = sc.sf[n - 1] * 1.2f;
    for (int n = 0; n < 8; ++n) sc.sigma2[n] = sc.sf[n] * sc.sf[n];
    const trg::Gates gt{0.01f, 0.9998f, 100.f, 3.84f, 5.991f, 50};

    // ---- R1: exactly at the ratio is kept, one ulp of median depth further is skipped; the epipoles ----
    trg::PairGeom g;
    trg::pair_prologue(k0, kx, gt.min_baseline_ratio, g);
    CHECK(g.baseline == 0.5f && trg::div_f(0.5f, 50.f) == 0.01f && !g.skipped && !trg::finite_f(g.ex));
    { trg::Kf far = kx; far.median_depth = std::nextafter(50.f, inf); trg::PairGeom h; trg::pair_prologue(k0, far, gt.min_baseline_ratio, h); CHECK(h.skipped); }
    CHECK(g.F12[0] == 0.f && g.F12[3] == 0.f && g.F12[6] == 0.f);       // horizontal lines: a == 0 for every query
    trg::PairGeom gz;
    trg::pair_prologue(k0, kz, gt.min_baseline_ratio, gz);
    CHECK(gz.ex == 320.f && gz.ey == 240.f && !gz.skipped);
    // ---- R3: den == 0 at the epipole of image 1; the gate; the line test at its edge; the key ----
    { const trg::Line l = trg::epipolar_line(gz.F12, 320.f, 240.f); CHECK(l.den == 0.f && !trg::candidate_passes(l, gz.ex, gz.ey, 400.f, 300.f, 1.f, 1.f, 100.f, 3.84f)); }
    {
        const trg::Line l = trg::epipolar_line(gz.F12, 420.f, 240.f);    // the line y = 240
        CHECK(l.den > 0.f && trg::candidate_passes(l, gz.ex, gz.ey, 440.f, 240.f, 1.f, 1.f, 100.f, 3.84f));
        CHECK(!trg::candidate_passes(l, gz.ex, gz.ey, 329.f, 240.f, 1.f, 1.f, 100.f, 3.84f) && trg::candidate_passes(l, gz.ex, gz.ey, 330.f, 240.f, 1.f, 1.f, 100.f, 3.84f));   // 81 < 100, 100 < 100 is false
        CHECK(trg::candidate_passes(l, gz.ex, gz.ey, 440.f, 241.9f, 1.f, 1.f, 100.f, 3.84f) && !trg::candidate_passes(l, gz.ex, gz.ey, 440.f, 242.f, 1.f, 1.f, 100.f, 3.84f));
        CHECK(trg::candidate_passes(l, nan, nan, 329.f, 240.f, 1.f, 1.f, 100.f, 3.84f));        // an epipole that is not finite gates nothing
    }
    CHECK(trg::pick_key(30, 5) < trg::pick_key(30, 4) && trg::pick_key(29, 0) < trg::pick_key(30, 9) && trg::pick_pos(trg::pick_key(7, 123)) == 123u && trg::pick_key(256, 0) < trg::kNoKey);
    // ---- R4-R6 on exact geometry ----
    auto proj = [](const trg::Kf& k, float X, float Y, float Z, float* u, float* v) {
        const double x = k.T[0] * X + k.T[1] * Y + k.T[2] * Z + k.T[3], y = k.T[4] * X + k.T[5] * Y + k.T[6] * Z + k.T[7], z = k.T[8] * X + k.T[9] * Y + k.T[10] * Z + k.T[11];
        *u = (float)(512.0 * x / z + 320.0); *v = (float)(512.0 * y / z + 240.0);
    };
    float u1, v1, u2, v2;
    proj(k0, 1.f, -0.5f, 6.f, &u1, &v1); proj(kx, 1.f, -0.5f, 6.f, &u2, &v2);
    trg::Outcome o = trg::triangulate(k0, kx, sc, gt, u1, v1, 0, u2, v2, 0);
    CHECK(o.status == IBA_TRIANGULATE_CREATED && std::fabs(o.x[0] - 1.f) < 1e-3f && std::fabs(o.x[1] + 0.5f) < 1e-3f && std::fabs(o.x[2] - 6.f) < 6e-3f);
    float nrm[3], mn, mx;
    trg::new_point(k0, kx, sc, o.x, 2, nrm, &mn, &mx);
    CHECK(std::fabs(mx - std::sqrt(o.x[0] * o.x[0] + o.x[1] * o.x[1] + o.x[2] * o.x[2]) * sc.sf[2]) < 1e-4f && mn == trg::div_f(mx, sc.sf[7]) && nrm[2] > 0.9f);
    CHECK(trg::triangulate(k0, kx, sc, gt, u1, v1, 0, u2, v2, 5).status == IBA_TRIANGULATE_SCALE);
    CHECK(trg::triangulate(k0, kx, sc, gt, u1, v1, 0, u1 + 20.f, v1, 0).status == IBA_TRIANGULATE_DEPTH1);
    proj(k0, 3.f, 2.f, 100.f, &u1, &v1); proj(kx, 3.f, 2.f, 100.f, &u2, &v2);
    CHECK(trg::triangulate(k0, kx, sc, gt, u1, v1, 0, u2, v2, 0).status == IBA_TRIANGULATE_PARALLAX);
    proj(k0, 0.05f, 0.02f, 0.3f, &u1, &v1); proj(kz, 0.05f, 0.02f, 0.3f, &u2, &v2);
    CHECK(trg::triangulate(k0, kz, sc, gt, u1, v1, 0, u2, v2, 0).status == IBA_TRIANGULATE_DEPTH2);
    // the guards: parallel rays from two centres give x[3] == 0 exactly once the parallax gate is open; a centre that IS the triangulated point
    { trg::Gates open = gt; open.max_cos_parallax = 2.f; o = trg::triangulate(k0, kx, sc, open, 320.f, 240.f, 0, 320.f, 240.f, 0); CHECK(o.status == IBA_TRIANGULATE_DEGENERATE && o.x[0] == 0.f && o.x[2] == 0.f); }
    CHECK(trg::triangulate(k0, kx, sc, gt, 320.f, 240.f, 0, 320.f, 240.f, 0).status == IBA_TRIANGULATE_PARALLAX);
    {
        proj(k0, 1.f, -0.5f, 6.f, &u1, &v1); proj(kx, 1.f, -0.5f, 6.f, &u2, &v2);
        o = trg::triangulate(k0, kx, sc, gt, u1, v1, 0, u2, v2, 0);
        trg::Kf odd = kx;                                   // (no pose has this centre: Ow is formed from T everywhere else)
        for (int i = 0; i < 3; ++i) odd.Ow[i] = o.x[i];
        CHECK(trg::triangulate(k0, odd, sc, gt, u1, v1, 0, u2, v2, 0).status == IBA_TRIANGULATE_ZERO_DIST);
    }

    // ---- the node order ----
    {
        const int32_t node[8] = {5, -1, 3, 5, 3, 9, -2, 3};
        const uint8_t has[8] = {0, 0, 1, 0, 0, 0, 0, 0};
        int32_t key[8], idx[8], a, b;
        CHECK(trg::node_order(node, has, 8, key, idx) == 6);
        const int32_t want_key[6] = {3, 3, 3, 5, 5, 9}, want_idx[6] = {~2, 4, 7, 0, 3, 5};
        for (int e = 0; e < 6; ++e) CHECK(key[e] == want_key[e] && idx[e] == want_idx[e]);
        trg::segment_of(key, 6, 3, &a, &b); CHECK(a == 0 && b == 3);
        trg::segment_of(key, 6, 5, &a, &b); CHECK(a == 3 && b == 5);
        trg::segment_of(key, 6, 4, &a, &b); CHECK(a == b);
        trg::segment_of(key, 6, 10, &a, &b); CHECK(a == 6 && b == 6);
        CHECK(trg::node_order(node, nullptr, 0, key, idx) == 0);
    }

    // ---- a seeded call: five keyframes along x over one cloud, nodes shared by families of points ----
    uint32_t seed = 11;
    const int32_t KF = 5, NP = 240;
    std::vector<float> X(3 * NP);
    std::vector<uint8_t> base(32 * NP);
    for (int32_t p = 0; p < NP; ++p) {
        X[3 * p] = (float)(lcg(seed) % 800) * 0.01f - 4.f; X[3 * p + 1] = (float)(lcg(seed) % 500) * 0.01f - 2.5f; X[3 * p + 2] = 5.f + (float)(lcg(seed) % 700) * 0.01f;
        for (int b = 0; b < 32; ++b) base[32 * p + b] = (uint8_t)lcg(seed);
    }
    std::vector<std::vector<float>> xy(KF), angle(KF), T(KF);
    std::vector<std::vector<int32_t>> octave(KF), node(KF);
    std::vector<std::vector<uint8_t>> desc(KF), has(KF);
    iba_orb_frame fr[6] = {};
    iba_triangulate_keyframe kf[6] = {};
    for (int32_t k = 0; k < KF; ++k) {
        T[k].assign(I, I + 12); T[k][3] = -0.3f * (float)k; T[k][11] = 0.02f * (float)k;
        trg::Kf cam; trg::make_kf(T[k].data(), 512.f, 512.f, 320.f, 240.f, 8.f, cam);
        for (int32_t p = 0; p < NP; ++p) {
            if (lcg(seed) % 4 == 0) continue;
            float u, v; proj(cam, X[3 * p], X[3 * p + 1], X[3 * p + 2], &u, &v);
            if (!(u > 0.f && u < 640.f && v > 0.f && v < 480.f)) continue;
            xy[k].push_back(u + ((float)(lcg(seed) % 100) - 50.f) * 0.01f); xy[k].push_back(v + ((float)(lcg(seed) % 100) - 50.f) * 0.01f);
            octave[k].push_back((int32_t)(lcg(seed) % 3)); angle[k].push_back(0.f);
            node[k].push_back(lcg(seed) % 25 == 0 ? -1 : p % 20); has[k].push_back(lcg(seed) % 4 == 0);
            for (int b = 0; b < 32; ++b) desc[k].push_back(base[32 * p + b]);
            for (int f = (int)(lcg(seed) % 30); f > 0; --f) desc[k][desc[k].size() - 32 + lcg(seed) % 32] ^= (uint8_t)(1u << (lcg(seed) % 8));
        }
        fr[k].xy = xy[k].data(); fr[k].octave = octave[k].data(); fr[k].angle = angle[k].data(); fr[k].desc = desc[k].data(); fr[k].n = (int32_t)octave[k].size();
        fr[k].min_x = 0.f; fr[k].max_x = 640.f; fr[k].min_y = 0.f; fr[k].max_y = 480.f;
        kf[k] = iba_triangulate_keyframe{k, 512.f, 512.f, 320.f, 240.f, k == 3 ? 1000.f : 8.f, T[k].data(), node[k].data(), k == 2 ? nullptr : has[k].data()};
    }
    fr[5] = fr[0]; fr[5].n = 0; fr[5].xy = nullptr; fr[5].octave = nullptr; fr[5].angle = nullptr; fr[5].desc = nullptr;
    kf[5] = iba_triangulate_keyframe{5, 512.f, 512.f, 320.f, 240.f, 8.f, I, nullptr, nullptr};
    const int32_t nb0[4] = {1, 2, 3, 4}, nb2[3] = {0, 5, 4}, nb3[2] = {0, 1};
    iba_triangulate_job jobs[4] = {};
    for (iba_triangulate_job& b : jobs) { b.n_levels = 8; b.scale_factor = 1.2f; b.scale_factors = sc.sf; b.level_sigma2 = sc.sigma2; }
    jobs[0].current = 0; jobs[0].n_neighbours = 4; jobs[0].neighbours = nb0;
    jobs[1].current = 1; jobs[1].n_neighbours = 0; jobs[1].neighbours = nullptr;
    jobs[2].current = 2; jobs[2].n_neighbours = 3; jobs[2].neighbours = nb2;
    jobs[3].current = 5; jobs[3].n_neighbours = 2; jobs[3].neighbours = nb3;
    iba_triangulate_options opt{};
    opt.struct_size = (int32_t)sizeof(opt); opt.th_low = 50; opt.min_baseline_ratio = 0.01f; opt.max_cos_parallax = 0.9998f; opt.epipole_gate = 100.f; opt.chi2_line = 3.84f;
    opt.chi2_mono = 5.991f; opt.keep_stages = 1;

    // ---- the checks ----
    CHECK(trg::check_options(&opt).empty() && !trg::check_options(nullptr).empty());
    { iba_triangulate_options b = opt; b.struct_size -= 4; CHECK(!trg::check_options(&b).empty()); }
    { iba_triangulate_options b = opt; b.th_low = 257; CHECK(!trg::check_options(&b).empty()); b.th_low = 256; CHECK(trg::check_options(&b).empty()); b.th_low = -1; CHECK(!trg::check_options(&b).empty()); }
    { iba_triangulate_options b = opt; b.chi2_line = nan; CHECK(!trg::check_options(&b).empty()); b = opt; b.epipole_gate = inf; CHECK(!trg::check_options(&b).empty()); }
    CHECK(iba::orbm::check_frames(fr, 6).empty() && trg::check_keyframes(fr, 6, kf, 6).empty() && trg::check_jobs(fr, kf, 6, jobs, 4).empty());
    CHECK(!trg::check_keyframes(fr, 6, nullptr, 6).empty() && !trg::check_keyframes(fr, 6, kf, 0).empty());
    { iba_triangulate_keyframe b = kf[0]; b.frame = 6; CHECK(!trg::check_keyframes(fr, 6, &b, 1).empty()); b = kf[0]; b.node = nullptr; CHECK(!trg::check_keyframes(fr, 6, &b, 1).empty()); }
    { iba_triangulate_keyframe b = kf[0]; b.Tcw12 = nullptr; CHECK(!trg::check_keyframes(fr, 6, &b, 1).empty()); b = kf[0]; b.fx = 2e6f; CHECK(!trg::check_keyframes(fr, 6, &b, 1).empty()); }
    { std::vector<float> bad(T[0]); bad[7] = nan; iba_triangulate_keyframe b = kf[0]; b.Tcw12 = bad.data(); CHECK(!trg::check_keyframes(fr, 6, &b, 1).empty()); }
    CHECK(!trg::check_jobs(fr, kf, 6, nullptr, 4).empty() && !trg::check_jobs(fr, kf, 6, jobs, 0).empty());
    { iba_triangulate_job b = jobs[0]; b.current = 6; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); b = jobs[0]; b.n_neighbours = -1; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { const int32_t nb[2] = {1, 0}; iba_triangulate_job b = jobs[0]; b.n_neighbours = 2; b.neighbours = nb; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { const int32_t nb[3] = {1, 2, 1}; iba_triangulate_job b = jobs[0]; b.n_neighbours = 3; b.neighbours = nb; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { const int32_t nb[1] = {6}; iba_triangulate_job b = jobs[0]; b.n_neighbours = 1; b.neighbours = nb; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { iba_triangulate_job b = jobs[0]; b.neighbours = nullptr; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); b = jobs[0]; b.level_sigma2 = nullptr; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { iba_triangulate_job b = jobs[0]; b.n_levels = 2; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); b.n_levels = 65; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { iba_triangulate_job b = jobs[0]; b.scale_factor = 0.f; CHECK(!trg::check_jobs(fr, kf, 6, &b, 1).empty()); }
    { iba_triangulate_keyframe k2[6]; for (int i = 0; i < 6; ++i) k2[i] = kf[i]; k2[2].median_depth = 0.f; CHECK(!trg::check_jobs(fr, k2, 6, jobs, 1).empty() && trg::check_jobs(fr, k2, 6, jobs + 2, 1).empty()); }

    // ---- the whole call on the host, against every slot on its own with R7 applied afterwards ----
    trg::Result res;
    res.opt = opt;
    res.job.resize(4);
    trg::host_call(&res, fr, 6, kf, 6, jobs, 4);
    const trg::Gates g2 = trg::make_gates(opt);
    int total_created = 0, total_superseded = 0;
    for (int32_t j = 0; j < 4; ++j) {
        const trg::JobRes& jr = res.job[(size_t)j];
        const iba_triangulate_job& b = jobs[j];
        const iba_orb_frame& f1 = fr[kf[b.current].frame];
        trg::Kf c1; trg::make_kf(kf[b.current].Tcw12, 512.f, 512.f, 320.f, 240.f, kf[b.current].median_depth, c1);
        std::vector<uint8_t> got((size_t)f1.n, 0);
        int counted[IBA_TRIANGULATE_N_STATUS] = {};
        size_t pt = jr.pt_base;
        for (int32_t pos = 0; pos < b.n_neighbours; ++pos) {
            const int32_t nb = b.neighbours[pos];
            const iba_orb_frame& f2 = fr[kf[nb].frame];
            trg::Kf c2; trg::make_kf(kf[nb].Tcw12, 512.f, 512.f, 320.f, 240.f, kf[nb].median_depth, c2);
            trg::PairGeom pg; trg::pair_prologue(c1, c2, g2.min_baseline_ratio, pg);
            CHECK(j == 3 || (nb == 3) == (pg.skipped != 0));        // keyframe 3's median depth is 1000; (job 3's keyframe 5 shares keyframe 0's centre)
            int n_matches = 0, n_created = 0;
            for (int32_t i = 0; i < f1.n; ++i) {
                const size_t s = jr.slot_base + (size_t)pos * (size_t)f1.n + (size_t)i;
                // the slot's own outcome: the literal walk
                int own = -1, m = -1, bestDist = g2.th_low, seg = 0;
                const bool hp = kf[b.current].has_point && kf[b.current].has_point[i];
                if (pg.skipped) own = IBA_TRIANGULATE_PAIR_SKIPPED;
                else if (hp) own = IBA_TRIANGULATE_HAS_POINT;
                else {
                    const trg::Line l = trg::epipolar_line(pg.F12, f1.xy[2 * i], f1.xy[2 * i + 1]);
                    for (int32_t i2 = 0; i2 < f2.n; ++i2) {
                        if (kf[b.current].node[i] < 0 || kf[nb].node[i2] != kf[b.current].node[i]) continue;
                        ++seg;
                        if (kf[nb].has_point && kf[nb].has_point[i2]) continue;
                        const int d = iba::mapm::host_hamming(f1.desc + 32 * (size_t)i, f2.desc + 32 * (size_t)i2);
                        if (d > g2.th_low || d > bestDist) continue;
                        if (!trg::candidate_passes(l, pg.ex, pg.ey, f2.xy[2 * i2], f2.xy[2 * i2 + 1], sc.sf[f2.octave[i2]], sc.sigma2[f2.octave[i2]], g2.epipole_gate, g2.chi2_line)) continue;
                        m = i2; bestDist = d;
                    }
                    if (!seg) own = IBA_TRIANGULATE_NO_NODE;
                    else if (m < 0) own = IBA_TRIANGULATE_NO_MATCH;
                    else own = trg::triangulate(c1, c2, sc, g2, f1.xy[2 * i], f1.xy[2 * i + 1], f1.octave[i], f2.xy[2 * m], f2.xy[2 * m + 1], f2.octave[m]).status;
                }
                CHECK(res.seg_len[s] == seg);
                const int want = got[(size_t)i] ? (int)IBA_TRIANGULATE_SUPERSEDED : own;
                CHECK(res.status[s] == want);
                ++counted[want];
                if (got[(size_t)i]) { CHECK(res.match[s] == -1 && res.dist[s] == -1 && res.xyz[3 * s] == 0.f); continue; }
                CHECK(res.match[s] == m && res.dist[s] == (m >= 0 ? bestDist : -1));
                n_matches += m >= 0;
                if (own == IBA_TRIANGULATE_CREATED) {
                    ++n_created;
                    CHECK(res.p_idx1[pt] == i && res.p_nb[pt] == pos && res.p_idx2[pt] == m && res.p_xyz[3 * pt + 2] == res.xyz[3 * s + 2] && res.p_desc[32 * pt + 31] == f1.desc[32 * (size_t)i + 31]);
                    CHECK(res.p_max[pt] > res.p_min[pt] && res.p_min[pt] > 0.f);
                    ++pt;
                }
            }
            for (int32_t i = 0; i < f1.n; ++i)
                if (res.status[jr.slot_base + (size_t)pos * (size_t)f1.n + (size_t)i] == IBA_TRIANGULATE_CREATED) got[(size_t)i] = 1;
            CHECK(res.pair_matches[jr.pair_base + (size_t)pos] == n_matches && res.pair_created[jr.pair_base + (size_t)pos] == n_created);
        }
        for (int st = 0; st < IBA_TRIANGULATE_N_STATUS; ++st) CHECK(counted[st] == jr.counts.status[st]);
        CHECK(jr.counts.n_created == (int32_t)(pt - jr.pt_base) && jr.counts.n_keypoints == f1.n && jr.counts.n_neighbours == b.n_neighbours);
        total_created += jr.counts.n_created; total_superseded += jr.counts.status[IBA_TRIANGULATE_SUPERSEDED];
    }
    CHECK(total_created > 20 && total_superseded > 20 && res.job[1].counts.n_created == 0 && res.job[3].counts.n_keypoints == 0 && res.p_idx1.size() == (size_t)total_created);

    // ---- the median depth ----
    {
        float out = 0.f;
        const float pts[12] = {0, 0, 5, 0, 0, 1, 0, 0, 9, 0, 0, 3};
        CHECK(trg::median_depth(I, pts, 4, 2, &out).empty() && out == 3.f);          // sorted 1 3 5 9, element (4 - 1) / 2 = 1
        CHECK(trg::median_depth(TZ, pts, 3, 1, &out).empty() && out == 8.5f);        // element 2 of 0.5 4.5 8.5
        CHECK(!trg::median_depth(I, pts, 0, 2, &out).empty() && !trg::median_depth(I, pts, 4, 0, &out).empty() && !trg::median_depth(I, nullptr, 4, 2, &out).empty());
    }
    // ---- the chunk planner ----
    {
        const std::vector<int64_t> slots = {10, 0, 25, 5, 5, 100, 1};
        std::vector<int32_t> cut = trg::plan_chunks(slots, 1ull << 30);
        CHECK(cut.size() == 2 && cut[0] == 0 && cut[1] == 7);
        cut = trg::plan_chunks(slots, 1);
        CHECK(cut.size() == 8);
        cut = trg::plan_chunks(slots, 35 * IBA_TRIANGULATE_BYTES_PER_SLOT);
        CHECK(cut.size() == 5 && cut[1] == 3 && cut[2] == 5 && cut[3] == 6 && cut[4] == 7);
    }
    std::printf("triangulate_selftest ok\n");
    return 0;
}

// Stand-alone sanitizer self-test of the map-point fusion's host half (csrc/iba_fuse_host.hpp) over the float decisions the kernels compile
// (csrc/iba_fuse_math.hpp): F2-F4 at their edges, the gate of F5, the argument checks, the whole call on the host against a literal walk, the fold
// on a hand-made map that reaches every op, its helpers, its entry checks and the chunk planner. Plain g++, no HIP:
//   make -C csrc san/fuse_selftest_asan && csrc/san/fuse_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_fuse_host.hpp"

namespace fuse = iba::fuse;
namespace mapm = iba::mapm;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- F2-F4 with the identity pose ----
    fuse::Camera cam{};
    mapm::Camera& c = cam.c;
    const float I[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    for (int k = 0; k < 12; ++k) c.T[k] = I[k];
    mapm::camera_centre(c.T, c.Ow);
    c.fx = c.fy = 500.f; c.cx = 320.f; c.cy = 240.f; c.min_x = 0.f; c.max_x = 640.f; c.min_y = 0.f; c.max_y = 480.f;
    c.th = 3.f; c.view_cos_limit = 0.5f; c.n_levels = 8;
    c.sf[0] = 1.f;
    for (int n = 1; n < 8; ++n) c.sf[n] = c.sf[n - 1] * 1.2f;
    for (int n = 0; n < 8; ++n) cam.inv_sigma2[n] = 1.f / (c.sf[n] * c.sf[n]);
    const float Z[3] = {0.f, 0.f, 1.f};
    auto view = [&](float x, float y, float z, const float* n, float mn, float mx) { const float P[3] = {x, y, z}; return fuse::frustum(cam, P, n, mn, mx); };
    CHECK(view(0, 0, -4, Z, 0.1f, 10).status == IBA_FUSE_DEPTH && view(1, 1, 0.f, Z, 0.1f, 10).status == IBA_FUSE_NOT_FINITE && view(10, 0, 5, Z, 0.1f, 10).status == IBA_FUSE_BOUNDS);
    { const float n[3] = {-0.64f, 0, 1}; const fuse::View w = view(-0.64f, 0, 1, n, 0.1f, 10); CHECK(w.status == IBA_FUSE_PICKED && w.u == 0.f && w.v == 240.f); }
    { const float n[3] = {0.64f, 0, 1}; CHECK(500.f * 0.64f + 320.f == 640.f && view(0.64f, 0, 1, n, 0.1f, 10).status == IBA_FUSE_BOUNDS); }      // half open: L1 keeps this one
    { const float n[3] = {0.64f, 0, 1}; const float P[3] = {0.64f, 0, 1}; CHECK(mapm::frustum(c, P, n, 0.1f, 10).status == IBA_MAP_MATCH_IN_VIEW); }
    const float near = 0.8f * 5.f, far = 1.2f * 5.f;
    CHECK(view(0, 0, near, Z, 5.f, 10).status == IBA_FUSE_PICKED && view(0, 0, std::nextafter(near, 0.f), Z, 5.f, 10).status == IBA_FUSE_DISTANCE);
    CHECK(view(0, 0, far, Z, 0.1f, 5.f).status == IBA_FUSE_PICKED && view(0, 0, std::nextafter(far, inf), Z, 0.1f, 5.f).status == IBA_FUSE_DISTANCE);
    { const float n[3] = {0, 0, 0.5f}; CHECK(view(0, 0, 4, n, 0.1f, 10).status == IBA_FUSE_PICKED); }
    { const float n[3] = {0, 0, std::nextafter(0.5f, 0.f)}; CHECK(view(0, 0, 4, n, 0.1f, 10).status == IBA_FUSE_ANGLE); }
    { const fuse::View w = view(0, 0, 2, Z, 0.1f, 2.f * c.sf[3]); CHECK(w.level == 3 && w.radius == 3.f * c.sf[3]); }
    CHECK(view(0, 0, 2, Z, 0.1f, 2.f).level == 0 && view(0, 0, 2, Z, 0.1f, 2.f * c.sf[7] * 1.5f).level == 7);
    // ---- F5's gate: 5.99f widened lies below the double 5.99... whichever side, the comparison is the rule's ----
    CHECK(fuse::gate_passes(10.f, 10.f, 10.f, 10.f, 1.f, 5.99f) && fuse::gate_passes(10.f, 10.f, 12.f, 11.f, 1.f, 5.99f) && !fuse::gate_passes(10.f, 10.f, 12.75f, 10.f, 1.f, 5.99f));
    CHECK(fuse::gate_passes(10.f, 10.f, 12.75f, 10.f, 0.25f, 5.99f) && fuse::gate_passes(0.f, 0.f, std::sqrt(5.99f), 0.f, 1.f, 5.99f) == !((double)(std::sqrt(5.99f) * std::sqrt(5.99f)) > (double)5.99f));
    CHECK(fuse::pick_key(3, 7) < fuse::pick_key(3, 8) && fuse::pick_key(3, 900) < fuse::pick_key(4, 0) && fuse::pick_key(255, 0xFFFFFFFFu) < fuse::kNoKey);

    // ---- a seeded call ----
    uint32_t seed = 5;
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
        xy[2 * i] = 500.f * xyz[3 * p] / z + 320.f + (float)(lcg(seed) % 5) - 2.f; xy[2 * i + 1] = 500.f * xyz[3 * p + 1] / z + 240.f + (float)(lcg(seed) % 5) - 2.f;
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
    std::vector<uint8_t> skip(77);
    for (int32_t k = 0; k < 77; ++k) { list[(size_t)k] = lcg(seed) % 13 == 0 ? -1 : (int32_t)(lcg(seed) % P); skip[(size_t)k] = lcg(seed) % 9 == 0; }
    iba_fuse_job jobs[4] = {};
    for (iba_fuse_job& b : jobs) { b.frame = 0; b.n_levels = 8; b.n_points = P; b.th = 3.f; b.fx = b.fy = 500.f; b.cx = 320.f; b.cy = 240.f; b.Tcw12 = I; b.scale_factors = c.sf; b.inv_level_sigma2 = cam.inv_sigma2; }
    jobs[1].n_points = 77; jobs[1].points = list.data(); jobs[1].skip = skip.data(); jobs[1].th = 5.f;
    jobs[2].n_points = 0; jobs[2].points = list.data();
    jobs[3].frame = 1;
    iba_fuse_options o{};
    o.struct_size = (int32_t)sizeof(o); o.th_low = 50; o.view_cos_limit = 0.5f; o.chi2_mono = 5.99f; o.check_reprojection = 1; o.keep_stages = 1;

    // ---- the checks ----
    CHECK(fuse::check_options(&o).empty() && !fuse::check_options(nullptr).empty());
    { iba_fuse_options b = o; b.struct_size -= 4; CHECK(!fuse::check_options(&b).empty()); }
    { iba_fuse_options b = o; b.th_low = 257; CHECK(!fuse::check_options(&b).empty()); b.th_low = -1; CHECK(!fuse::check_options(&b).empty()); b.th_low = 256; CHECK(fuse::check_options(&b).empty()); }
    { iba_fuse_options b = o; b.view_cos_limit = inf; CHECK(!fuse::check_options(&b).empty()); b = o; b.chi2_mono = nan; CHECK(!fuse::check_options(&b).empty()); }
    CHECK(fuse::check_jobs(fr, 2, P, jobs, 4).empty());
    CHECK(!fuse::check_jobs(fr, 2, P, nullptr, 4).empty() && !fuse::check_jobs(fr, 2, P, jobs, 0).empty());
    { iba_fuse_job b = jobs[0]; b.frame = 2; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_fuse_job b = jobs[0]; b.n_levels = 0; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); b.n_levels = 65; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_fuse_job b = jobs[0]; b.n_levels = 3; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); b.frame = 1; CHECK(fuse::check_jobs(fr, 2, P, &b, 1).empty()); }      // an octave of 3 in the frame
    { iba_fuse_job b = jobs[0]; b.n_points = P - 1; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); b.n_points = -1; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_fuse_job b = jobs[0]; b.th = nan; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); b = jobs[0]; b.fx = 2e6f; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { iba_fuse_job b = jobs[0]; b.Tcw12 = nullptr; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); b = jobs[0]; b.inv_level_sigma2 = nullptr; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { float lv[8]; for (int n = 0; n < 8; ++n) lv[n] = cam.inv_sigma2[n]; iba_fuse_job b = jobs[0]; b.inv_level_sigma2 = lv; lv[2] = 0.f; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty());
      lv[2] = inf; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); lv[2] = -1.f; CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); }
    { std::vector<int32_t> bad(list); bad[9] = P; iba_fuse_job b = jobs[1]; b.points = bad.data(); CHECK(!fuse::check_jobs(fr, 2, P, &b, 1).empty()); bad[9] = -5; CHECK(fuse::check_jobs(fr, 2, P, &b, 1).empty()); }

    // ---- the whole call on the host, against a literal walk over the kept lists ----
    for (int gate = 1; gate >= 0; --gate) {
        fuse::Result res;
        res.opt = o; res.opt.check_reprojection = gate;
        res.job.resize(4);
        fuse::host_call(&res, fr, 2, &tb, jobs, 4);
        CHECK(res.status.size() == (size_t)(P + 77 + 0 + P));
        int total = 0, gated = 0;
        for (int32_t j = 0; j < 4; ++j) {
            const fuse::JobRes& jr = res.job[(size_t)j];
            const iba_fuse_job& b = jobs[j];
            const iba_orb_frame& f = fr[b.frame];
            const int32_t* off = &res.off[jr.slot_base + (size_t)j];
            int counted[IBA_FUSE_N_STATUS] = {};
            for (int32_t k = 0; k < b.n_points; ++k) {
                const size_t s = jr.slot_base + (size_t)k;
                const int32_t p = b.points ? b.points[k] : k;
                ++counted[res.status[s]];
                CHECK(res.point[s] == p && ((p < 0 || (b.skip && b.skip[k])) == (res.status[s] == IBA_FUSE_SKIPPED)));
                const bool reached = res.status[s] == IBA_FUSE_PICKED || res.status[s] >= IBA_FUSE_NO_CANDIDATE;
                if (!reached) { CHECK(off[k + 1] == off[k] && res.match[s] == -1 && res.dist[s] == -1 && res.radius[s] == 0.f); continue; }
                CHECK(res.radius[s] == b.th * b.scale_factors[res.level[s]]);
                int best = 256, idx = -1;
                for (int32_t e = off[k]; e < off[k + 1]; ++e) {
                    const int32_t i = res.cand[jr.cand_base + (size_t)e];
                    const int d = (int)res.cand_dist[jr.cand_base + (size_t)e];
                    CHECK(i >= 0 && i < f.n && (f.octave[i] == res.level[s] || f.octave[i] == res.level[s] - 1));
                    CHECK(d == mapm::host_hamming(pdesc.data() + 32 * (size_t)p, f.desc + 32 * (size_t)i));
                    if (gate) {
                        const float ex = res.u[s] - f.xy[2 * i], ey = res.v[s] - f.xy[2 * i + 1];
                        const float e2 = ex * ex + ey * ey;
                        if (e2 * b.inv_level_sigma2[f.octave[i]] > 5.99) { ++gated; continue; }
                    }
                    if (d < best) { best = d; idx = i; }
                }
                const int want = off[k + 1] == off[k] ? IBA_FUSE_NO_CANDIDATE : best <= o.th_low ? IBA_FUSE_PICKED : IBA_FUSE_NO_MATCH;
                CHECK(res.status[s] == want && res.match[s] == (want == IBA_FUSE_PICKED ? idx : -1) && res.dist[s] == (want == IBA_FUSE_PICKED ? best : -1));
                total += want == IBA_FUSE_PICKED;
            }
            for (int st = 0; st < IBA_FUSE_N_STATUS; ++st) CHECK(counted[st] == jr.counts.status[st]);
            CHECK(jr.counts.n_picked == counted[IBA_FUSE_PICKED] && jr.counts.n_candidates == off[b.n_points] && jr.counts.n_points == b.n_points && jr.n_kp == f.n);
        }
        CHECK(total > 20 && (gate ? gated > 0 : gated == 0) && res.job[3].counts.n_candidates == 0 && res.job[2].counts.n_points == 0 && res.job[3].counts.status[IBA_FUSE_NO_CANDIDATE] > 0);
    }

    // ---- the fold on a hand-made map: 3 keyframes of 4 keypoints, 8 points; the job is written by hand into a Result ----
    {
        const int32_t kp_off[4] = {0, 4, 8, 12};
        //                     keyframe 0        keyframe 1        keyframe 2
        int32_t holder[12] = {0, 1, -1, 7,      1, 2, -1, -1,     1, 3, 4, -1};
        uint8_t bad[8] = {0, 0, 0, 0, 0, 0, 0, 1}, stale[8] = {};
        int32_t rep[8], found[8], visible[8];
        for (int p = 0; p < 8; ++p) { rep[p] = -1; found[p] = p; visible[p] = 10 * p; }
        iba_fuse_map m{3, kp_off, holder, 8, bad, rep, found, visible, stale};
        fuse::Result r;
        r.job.resize(1);
        r.job[0].n_kp = 4; r.job[0].counts.n_points = 8;
        //             ADD    REPLACED_BY_HELD (1 has 3)   REPLACES_HELD (0 has 1, 4 has 1)   HELD_BAD   STALE_BAD (2 died)  STALE_IN_KEYFRAME (5 was added)  NONE   the -1 branch
        r.point  = {   5,     2,                            4,                                 6,         2,                  5,                               3,     3};
        r.match  = {   2,     1,                            0,                                 3,         0,                  1,                               -1,    1};
        r.status = {0, 0, 0, 0, 0, 0, (uint8_t)IBA_FUSE_NO_MATCH, 0};
        int32_t op[8], other[8], nf = -1;
        CHECK(fuse::apply(r, 0, 0, &m, IBA_FUSE_LOCAL, op, other, &nf).empty());
        const int32_t want_op[8] = {IBA_FUSE_OP_ADD, IBA_FUSE_OP_REPLACED_BY_HELD, IBA_FUSE_OP_REPLACES_HELD, IBA_FUSE_OP_HELD_BAD, IBA_FUSE_OP_STALE_BAD, IBA_FUSE_OP_STALE_IN_KEYFRAME,
                                    IBA_FUSE_OP_NONE, IBA_FUSE_OP_REPLACED_BY_HELD};
        const int32_t want_other[8] = {-1, 1, 0, 7, -1, -1, -1, 1};
        for (int k = 0; k < 8; ++k) CHECK(op[k] == want_op[k] && other[k] == want_other[k]);
        // 2 died into 1: keyframe 1 held both, so 2's keypoint there is erased. 0 died into 4. 3 died into 1: keyframe 2 held both.
        const int32_t want_holder[12] = {4, 1, 5, 7, 1, -1, -1, -1, 1, -1, 4, -1};
        for (int i = 0; i < 12; ++i) CHECK(holder[i] == want_holder[i]);
        CHECK(nf == 5 && bad[2] && bad[0] && bad[3] && !bad[1] && !bad[4] && rep[2] == 1 && rep[0] == 4 && rep[3] == 1 && rep[1] == -1);
        CHECK(found[1] == 1 + 2 + 3 && visible[1] == 10 + 20 + 30 && found[4] == 4 + 0 && stale[1] && stale[4] && !stale[5] && !stale[2]);
        // LOOP: records, changes nothing but the ADD
        int32_t holder2[12] = {0, 1, -1, 7, 1, 2, -1, -1, 1, 3, 4, -1};
        uint8_t bad2[8] = {0, 0, 0, 0, 0, 0, 0, 1};
        for (int p = 0; p < 8; ++p) rep[p] = -1;
        iba_fuse_map m2{3, kp_off, holder2, 8, bad2, rep, nullptr, nullptr, nullptr};
        CHECK(fuse::apply(r, 0, 0, &m2, IBA_FUSE_LOOP, op, other, &nf).empty());
        CHECK(op[0] == IBA_FUSE_OP_ADD && op[1] == IBA_FUSE_OP_RECORD && other[1] == 1 && op[2] == IBA_FUSE_OP_RECORD && other[2] == 0 && op[3] == IBA_FUSE_OP_HELD_BAD && op[4] == IBA_FUSE_OP_RECORD &&
              op[5] == IBA_FUSE_OP_STALE_IN_KEYFRAME && op[7] == IBA_FUSE_OP_RECORD && nf == 6 && holder2[2] == 5 && holder2[0] == 0 && !bad2[2]);
        // U5
        const int32_t pl[6] = {-1, 0, 7, 4, 5, 2};
        uint8_t sk[6];
        CHECK(fuse::skip_bytes(&m2, 0, pl, 6, sk).empty() && sk[0] == 1 && sk[1] == 1 && sk[2] == 1 && sk[3] == 0 && sk[4] == 1 && sk[5] == 0);
        const int32_t tg[3] = {2, 0, 2};
        int32_t cd[8], n = -1;
        CHECK(fuse::candidates(&m2, tg, 3, cd, &n).empty() && n == 5 && cd[0] == 1 && cd[1] == 3 && cd[2] == 4 && cd[3] == 0 && cd[4] == 5);
        // U1's refusals
        CHECK(!fuse::apply(r, 0, 3, &m2, IBA_FUSE_LOCAL, op, other, &nf).empty() && !fuse::apply(r, 0, 0, &m2, 2, op, other, &nf).empty() && !fuse::apply(r, 0, 0, nullptr, 0, op, other, &nf).empty());
        holder2[5] = 1;                                       // point 1 twice in keyframe 1
        CHECK(fuse::apply(r, 0, 0, &m2, IBA_FUSE_LOCAL, op, other, &nf).find("held twice") != std::string::npos);
        holder2[5] = 8;
        CHECK(fuse::apply(r, 0, 0, &m2, IBA_FUSE_LOCAL, op, other, &nf).find("outside [-1, P)") != std::string::npos);
        holder2[5] = -2;
        CHECK(!fuse::skip_bytes(&m2, 0, pl, 6, sk).empty() && !fuse::candidates(&m2, tg, 3, cd, &n).empty());
        holder2[5] = 2;
        r.job[0].n_kp = 5;
        CHECK(fuse::apply(r, 0, 0, &m2, IBA_FUSE_LOCAL, op, other, &nf).find("keypoints") != std::string::npos);
        r.job[0].n_kp = 4; r.point[0] = 8;
        CHECK(fuse::apply(r, 0, 0, &m2, IBA_FUSE_LOCAL, op, other, &nf).find("names point") != std::string::npos);
    }

    // ---- the chunk planner ----
    {
        const std::vector<int64_t> cnd = {10, 0, 25, 5, 5, 100, 1};
        std::vector<int32_t> cut = fuse::plan_chunks(cnd, 1ull << 30);
        CHECK(cut.size() == 2 && cut[0] == 0 && cut[1] == 7);
        cut = fuse::plan_chunks(cnd, 1);
        CHECK(cut.size() == 8);
        cut = fuse::plan_chunks(cnd, 35 * IBA_FUSE_BYTES_PER_CANDIDATE);
        CHECK(cut.size() == 5 && cut[1] == 3 && cut[2] == 5 && cut[3] == 6 && cut[4] == 7);
    }
    std::printf("fuse_selftest ok\n");
    return 0;
}

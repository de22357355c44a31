// Stand-alone sanitizer self-test of the windowed matching's host half (csrc/iba_orb_match_host.hpp): the cell and window rules at their edges, the
// argument checks, the two query builders and the chunk planner. Plain g++, no HIP:
//   make -C csrc san/orb_match_selftest_asan && csrc/san/orb_match_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_orb_match_host.hpp"

namespace orbm = iba::orbm;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

struct Frame {
    std::vector<float> xy, angle; std::vector<int32_t> octave; std::vector<uint8_t> desc;
    iba_orb_frame f{};
    explicit Frame(int32_t n, uint32_t seed = 1) : xy(2 * (size_t)n), angle((size_t)n), octave((size_t)n), desc(32 * (size_t)n) {
        for (int32_t i = 0; i < n; ++i) {
            xy[2 * i] = (float)(lcg(seed) % 640); xy[2 * i + 1] = (float)(lcg(seed) % 480);
            angle[(size_t)i] = (float)(lcg(seed) % 360); octave[(size_t)i] = (int32_t)(lcg(seed) % 3);
            for (int b = 0; b < 32; ++b) desc[32 * (size_t)i + (size_t)b] = (uint8_t)lcg(seed);
        }
        f.xy = xy.data(); f.octave = octave.data(); f.angle = angle.data(); f.desc = desc.data(); f.n = n;
        f.min_x = 0.f; f.max_x = 640.f; f.min_y = 0.f; f.max_y = 480.f;
    }
};

struct Queries {
    std::vector<float> centre, radius; std::vector<int32_t> levels, index; std::vector<uint8_t> valid;
    explicit Queries(int32_t n) : centre(2 * (size_t)n + 2), radius((size_t)n + 1), levels(2 * (size_t)n + 2), index((size_t)n + 1), valid((size_t)n + 1) {}
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // ---- M2 / M3 along one axis (inv = 0.1: ten pixels per cell) ----
    CHECK(orbm::cell_of(25.f, 0.f, 0.1f, 64) == 3);         // 2.5 rounds away from zero
    CHECK(orbm::cell_of(-5.f, 0.f, 0.1f, 64) == -1);        // -0.5 rounds to -1
    CHECK(orbm::cell_of(-4.f, 0.f, 0.1f, 64) == 0);
    CHECK(orbm::cell_of(635.f, 0.f, 0.1f, 64) == -1);       // 63.5 rounds to 64
    CHECK(orbm::cell_of(1e30f, 0.f, 1e30f, 64) == -1 && orbm::cell_of(nan, 0.f, 0.1f, 64) == -1);
    CHECK(orbm::window_first(100.f, 0.f, 15.f, 0.1f, 64) == 8 && orbm::window_last(100.f, 0.f, 15.f, 0.1f, 64) == 12);
    CHECK(orbm::window_first(-100.f, 0.f, 15.f, 0.1f, 64) == 0 && orbm::window_last(-100.f, 0.f, 15.f, 0.1f, 64) == -1);
    CHECK(orbm::window_first(700.f, 0.f, 15.f, 0.1f, 64) == 64 && orbm::window_last(700.f, 0.f, 15.f, 0.1f, 64) == 63);
    CHECK(orbm::window_first(nan, 0.f, 15.f, 0.1f, 64) == 64 && orbm::window_last(nan, 0.f, 15.f, 0.1f, 64) == -1);
    CHECK(orbm::window_first(-inf, 0.f, 15.f, 0.1f, 64) == 0 && orbm::window_last(inf, 0.f, 15.f, 0.1f, 64) == 63);

    // ---- options ----
    iba_orb_match_options o{};
    o.struct_size = (int32_t)sizeof(o); o.th_low = 50; o.th_high = 100; o.nn_ratio = 0.9f; o.check_orientation = 1;
    CHECK(orbm::check_options(&o).empty() && !orbm::check_options(nullptr).empty());
    { iba_orb_match_options b = o; b.struct_size -= 4; CHECK(!orbm::check_options(&b).empty()); }
    { iba_orb_match_options b = o; b.th_low = 257; CHECK(!orbm::check_options(&b).empty()); b.th_low = 256; CHECK(orbm::check_options(&b).empty()); }
    { iba_orb_match_options b = o; b.th_high = -1; CHECK(!orbm::check_options(&b).empty()); }
    { iba_orb_match_options b = o; b.nn_ratio = 0.f; CHECK(!orbm::check_options(&b).empty()); b.nn_ratio = nan; CHECK(!orbm::check_options(&b).empty()); b.nn_ratio = inf; CHECK(!orbm::check_options(&b).empty()); }

    // ---- frames ----
    Frame a(100, 7), b(37, 9), empty(0);
    iba_orb_frame fr[3] = {a.f, b.f, empty.f};
    fr[2].xy = nullptr; fr[2].octave = nullptr; fr[2].angle = nullptr; fr[2].desc = nullptr;
    CHECK(orbm::check_frames(fr, 3).empty());
    CHECK(!orbm::check_frames(nullptr, 3).empty() && !orbm::check_frames(fr, 0).empty());
    { iba_orb_frame x = a.f; x.n = IBA_ORB_MATCH_MAX_KEYPOINTS + 1; CHECK(!orbm::check_frame(x).empty()); x.n = -1; CHECK(!orbm::check_frame(x).empty()); }
    { iba_orb_frame x = a.f; x.max_x = x.min_x; CHECK(!orbm::check_frame(x).empty()); x.max_x = inf; CHECK(!orbm::check_frame(x).empty()); }
    { iba_orb_frame x = a.f; x.min_y = nan; CHECK(!orbm::check_frame(x).empty()); }
    { iba_orb_frame x = a.f; x.desc = nullptr; CHECK(!orbm::check_frame(x).empty()); }
    { Frame x(5); x.xy[3] = nan; CHECK(!orbm::check_frame(x.f).empty()); }
    { Frame x(5); x.angle[4] = 360.5f; CHECK(!orbm::check_frame(x.f).empty()); x.angle[4] = 360.f; CHECK(orbm::check_frame(x.f).empty()); x.angle[4] = -1.f; CHECK(!orbm::check_frame(x.f).empty()); }

    // ---- the first builder, and its outputs as a job ----
    Queries qi(a.f.n);
    std::vector<float> prev(a.xy);
    CHECK(orbm::init_queries(&a.f, prev.data(), 100, qi.centre.data(), qi.radius.data(), qi.levels.data(), qi.index.data(), qi.valid.data()).empty());
    for (int32_t i = 0; i < a.f.n; ++i) {
        CHECK(qi.valid[(size_t)i] == (a.octave[(size_t)i] == 0 ? 1 : 0) && qi.index[(size_t)i] == i && qi.radius[(size_t)i] == 100.f);
        CHECK(qi.centre[2 * (size_t)i] == a.xy[2 * (size_t)i] && qi.levels[2 * (size_t)i] == 0 && qi.levels[2 * (size_t)i + 1] == 0);
    }
    CHECK(!orbm::init_queries(nullptr, prev.data(), 100, qi.centre.data(), qi.radius.data(), qi.levels.data(), qi.index.data(), qi.valid.data()).empty());
    CHECK(!orbm::init_queries(&a.f, nullptr, 100, qi.centre.data(), qi.radius.data(), qi.levels.data(), qi.index.data(), qi.valid.data()).empty());
    CHECK(!orbm::init_queries(&a.f, prev.data(), -1, qi.centre.data(), qi.radius.data(), qi.levels.data(), qi.index.data(), qi.valid.data()).empty());
    CHECK(orbm::init_queries(&fr[2], nullptr, 10, nullptr, nullptr, nullptr, nullptr, nullptr).empty());       // n == 0: nothing is read or written
    iba_orb_match_job job{};
    job.query_frame = 0; job.train_frame = 1; job.rule = IBA_ORB_MATCH_INIT; job.n_queries = a.f.n;
    job.centre_xy = qi.centre.data(); job.radius = qi.radius.data(); job.level_range = qi.levels.data(); job.query_index = qi.index.data(); job.valid = qi.valid.data();
    iba_orb_match_job none{};
    none.query_frame = 2; none.train_frame = 2; none.rule = IBA_ORB_MATCH_CLAIM;
    iba_orb_match_job jobs[2] = {job, none};
    CHECK(orbm::check_jobs(fr, 3, jobs, 2).empty());
    CHECK(!orbm::check_jobs(fr, 3, nullptr, 2).empty() && !orbm::check_jobs(fr, 3, jobs, 0).empty());
    { iba_orb_match_job x = job; x.train_frame = 3; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); x.train_frame = -1; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { iba_orb_match_job x = job; x.rule = 2; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { iba_orb_match_job x = job; x.n_queries = -1; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { iba_orb_match_job x = job; x.radius = nullptr; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); x = job; x.valid = nullptr; CHECK(orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { iba_orb_match_job x = job; x.query_frame = 1; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }       // query_index 37 .. 99 outside frame 1
    { Queries q2 = qi; q2.radius[5] = -1.f; iba_orb_match_job x = job; x.radius = q2.radius.data(); CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { Queries q2 = qi; q2.radius[5] = nan; iba_orb_match_job x = job; x.radius = q2.radius.data(); CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { Queries q2 = qi; q2.centre[11] = 1.5e6f; iba_orb_match_job x = job; x.centre_xy = q2.centre.data(); CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); q2.centre[11] = -inf; CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }
    { Queries q2 = qi; q2.index[0] = -1; iba_orb_match_job x = job; x.query_index = q2.index.data(); CHECK(!orbm::check_jobs(fr, 3, &x, 1).empty()); }

    // ---- the second builder ----
    const int32_t n = 6;
    Frame last(n, 3);
    const int32_t oct[n] = {0, 1, 2, 0, 1, 2};
    for (int32_t i = 0; i < n; ++i) last.octave[(size_t)i] = oct[i];
    //                     in front      behind       has no point   outlier      on min_x       zc == 0
    const float X[3 * n] = {1.f, 2.f, 10.f, 1.f, 2.f, -10.f, 1.f, 2.f, 10.f, 1.f, 2.f, 10.f, -32.f, 0.f, 10.f, 1.f, 2.f, 0.f};
    const uint8_t has[n] = {1, 1, 0, 1, 1, 1}, outl[n] = {0, 0, 0, 1, 0, 0};
    const float T[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}, bounds[4] = {0.f, 640.f, 0.f, 480.f}, sf[3] = {1.f, 1.2f, 1.44f};
    Queries qm(n);
    CHECK(orbm::motion_queries(&last.f, has, outl, X, T, 100.f, 100.f, 320.f, 240.f, bounds, sf, 3, 15.f, qm.centre.data(), qm.radius.data(), qm.levels.data(), qm.index.data(), qm.valid.data()).empty());
    CHECK(qm.valid[0] == 1 && qm.centre[0] == 100.f * 1.f * (float)(1.0 / 10.0) + 320.f && qm.radius[0] == 15.f && qm.levels[0] == -1 && qm.levels[1] == 1);
    CHECK(qm.valid[1] == 0 && qm.valid[2] == 0 && qm.valid[3] == 0 && qm.radius[1] == 0.f && qm.centre[2] == 0.f);
    CHECK(qm.valid[4] == 1 && qm.centre[8] == 0.f && qm.radius[4] == 15.f * 1.2f && qm.levels[8] == 0 && qm.levels[9] == 2);     // u == min_x is kept
    CHECK(qm.valid[5] == 0);                                                                                                      // u is not finite
    CHECK(!orbm::motion_queries(&last.f, has, outl, X, T, 100.f, 100.f, 320.f, 240.f, bounds, sf, 2, 15.f, qm.centre.data(), qm.radius.data(), qm.levels.data(), qm.index.data(), qm.valid.data()).empty());
    CHECK(!orbm::motion_queries(&last.f, has, outl, X, nullptr, 100.f, 100.f, 320.f, 240.f, bounds, sf, 3, 15.f, qm.centre.data(), qm.radius.data(), qm.levels.data(), qm.index.data(), qm.valid.data()).empty());
    CHECK(!orbm::motion_queries(&last.f, nullptr, outl, X, T, 100.f, 100.f, 320.f, 240.f, bounds, sf, 3, 15.f, qm.centre.data(), qm.radius.data(), qm.levels.data(), qm.index.data(), qm.valid.data()).empty());
    CHECK(orbm::check_queries(n, qm.centre.data(), qm.radius.data(), qm.levels.data(), qm.index.data(), n).empty());

    // ---- the chunk planner ----
    {
        const std::vector<int64_t> c = {10, 0, 25, 5, 5, 100, 1};
        std::vector<int32_t> cut = orbm::plan_chunks(c, 1ull << 30);
        CHECK(cut.size() == 2 && cut[0] == 0 && cut[1] == 7);
        cut = orbm::plan_chunks(c, 1);                       // every job alone: a chunk holds at least one
        CHECK(cut.size() == 8);
        for (int32_t k = 0; k < 8; ++k) CHECK(cut[(size_t)k] == k);
        cut = orbm::plan_chunks(c, 35 * IBA_ORB_MATCH_BYTES_PER_CANDIDATE);
        CHECK(cut.size() == 5 && cut[1] == 3 && cut[2] == 5 && cut[3] == 6 && cut[4] == 7);      // 10 0 25 | 5 5 | 100 | 1
        uint32_t seed = 5;
        for (int trial = 0; trial < 50; ++trial) {
            std::vector<int64_t> r((size_t)(1 + lcg(seed) % 20));
            for (int64_t& v : r) v = (int64_t)(lcg(seed) % 1000);
            const uint64_t budget = (uint64_t)(lcg(seed) % 6000);
            const std::vector<int32_t> k = orbm::plan_chunks(r, budget);
            CHECK(k.front() == 0 && k.back() == (int32_t)r.size());
            for (size_t i = 0; i + 1 < k.size(); ++i) {
                CHECK(k[i] < k[i + 1]);
                uint64_t bytes = 0;
                for (int32_t j = k[i]; j < k[i + 1]; ++j) bytes += IBA_ORB_MATCH_BYTES_PER_CANDIDATE * (uint64_t)r[(size_t)j];
                CHECK(bytes <= budget || k[i + 1] - k[i] == 1);
            }
        }
    }
    std::printf("orb_match_selftest ok\n");
    return 0;
}

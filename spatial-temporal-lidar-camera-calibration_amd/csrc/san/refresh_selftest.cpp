// Stand-alone sanitizer self-test of the map-point refresh's host half (csrc/iba_refresh_host.hpp) over the decisions the kernels compile
// (csrc/iba_refresh_math.hpp): S3's key and rank, S4 / S5 at their edges, the argument checks, the whole call on the host against a literal sort
// and walk at every observation count from 0 to 70 and at the cap, the guards, and the two helpers. Plain g++, no HIP:
//   make -C csrc san/refresh_selftest_asan && csrc/san/refresh_selftest_asan
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_refresh_host.hpp"

namespace rfr = iba::rfr;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

int main() {
    // ---- the decisions ----
    CHECK(rfr::median_rank(1) == 0 && rfr::median_rank(2) == 0 && rfr::median_rank(3) == 1 && rfr::median_rank(4) == 1 && rfr::median_rank(1024) == 511);
    CHECK(rfr::pick_key(3, 7) < rfr::pick_key(3, 8) && rfr::pick_key(3, 1023) < rfr::pick_key(4, 0) && rfr::pick_key(256, 1023) < rfr::kNoKey);
    {
        uint64_t a[4] = {0, 0, 0, 0}, b[4] = {~0ull, ~0ull, ~0ull, ~0ull}, c[4] = {1, 0, 0x8000000000000000ull, 0};
        CHECK(rfr::hamming256(a, a) == 0 && rfr::hamming256(a, b) == 256 && rfr::hamming256(a, c) == 2 && rfr::hamming256(b, c) == 254);
    }
    {
        const float O[3] = {1.f, 2.f, 3.f}, P[3] = {1.f, 2.f, 7.f};
        float t[3];
        CHECK(rfr::term(P, O, t) && t[0] == 0.f && t[1] == 0.f && t[2] == 1.f && !rfr::term(O, O, t) && t[2] == 0.f);
        CHECK(rfr::mean_of(1.5f, 2) == 0.75f && rfr::mean_of(1.f, 3) == (float)(1.0 / 3.0));
        rfr::KfRec kf{{1.f, 2.f, 3.f}, 0};
        rfr::KfScale sc{};
        sc.n_levels = 3; sc.sf[0] = 1.f; sc.sf[1] = 1.2f; sc.sf[2] = 1.2f * 1.2f;
        float mn = 0.f, mx = 0.f;
        rfr::distances(P, kf, sc, 1, &mn, &mx);
        CHECK(mx == 4.f * 1.2f && mn == (float)((double)mx / (double)sc.sf[2]));
    }

    // ---- a seeded call: K keyframes of one keypoint frame each, point p has p observations (0..70), and one point at the cap ----
    uint32_t seed = 11;
    const int32_t K = rfr::kMaxObs + 1, n_small = 71, P = n_small + 3;
    std::vector<std::vector<uint8_t>> kdesc((size_t)K, std::vector<uint8_t>(3 * 32));
    std::vector<std::vector<int32_t>> koct((size_t)K, std::vector<int32_t>(3));
    std::vector<std::vector<float>> kxy((size_t)K, std::vector<float>(6, 10.f)), kang((size_t)K, std::vector<float>(3, 0.f));
    std::vector<iba_orb_frame> frames((size_t)K);
    std::vector<std::vector<float>> T((size_t)K, std::vector<float>(12, 0.f));
    std::vector<iba_refresh_keyframe> kfs((size_t)K);
    float sf[8];
    sf[0] = 1.f;
    for (int n = 1; n < 8; ++n) sf[n] = sf[n - 1] * 1.2f;
    for (int32_t k = 0; k < K; ++k) {
        for (auto& b : kdesc[(size_t)k]) b = (uint8_t)((lcg(seed) & 7) ? 0x5A : lcg(seed));     // mostly alike, so that medians tie
        for (auto& o : koct[(size_t)k]) o = (int32_t)(lcg(seed) % 8);
        frames[(size_t)k] = iba_orb_frame{kxy[(size_t)k].data(), koct[(size_t)k].data(), kang[(size_t)k].data(), kdesc[(size_t)k].data(), 3, 0.f, 640.f, 0.f, 480.f};
        T[(size_t)k][0] = T[(size_t)k][5] = T[(size_t)k][10] = 1.f;
        T[(size_t)k][3] = 0.01f * (float)(lcg(seed) % 400) - 2.f; T[(size_t)k][7] = 0.01f * (float)(lcg(seed) % 200) - 1.f; T[(size_t)k][11] = 0.5f;
        kfs[(size_t)k] = iba_refresh_keyframe{k, 8, T[(size_t)k].data(), sf, (k % 13 == 5) ? 1 : 0, 0};
    }
    std::vector<float> xyz(3 * (size_t)P), normal(3 * (size_t)P, 0.5f), mn((size_t)P, 1.f), mx((size_t)P, 9.f);
    std::vector<uint8_t> pdesc(32 * (size_t)P), pbad((size_t)P, 0);
    for (auto& b : pdesc) b = (uint8_t)lcg(seed);
    for (int32_t p = 0; p < P; ++p) { xyz[3 * (size_t)p] = 0.01f * (float)(lcg(seed) % 300); xyz[3 * (size_t)p + 1] = 0.01f * (float)(lcg(seed) % 300); xyz[3 * (size_t)p + 2] = 5.f + 0.01f * (float)(lcg(seed) % 300); }
    std::vector<int32_t> off(1, 0), okf, okp, ref((size_t)P, 0);
    auto add_point = [&](int32_t p, int32_t n, int32_t first) {
        for (int32_t j = 0; j < n; ++j) { okf.push_back((first + 7 * j) % K); okp.push_back((int32_t)(lcg(seed) % 3)); }      // 7 and K = 1025 are coprime: distinct keyframes
        ref[(size_t)p] = n ? okf[(size_t)off.back() + (size_t)(n / 2)] : 0;
        off.push_back(off.back() + n);
    };
    for (int32_t p = 0; p < n_small; ++p) add_point(p, p, 3 * p);
    add_point(n_small, rfr::kMaxObs, 1);                                  // the cap
    add_point(n_small + 1, 4, 9); ref[(size_t)n_small + 1] = 8;           // NO_REF: 9, 16, 23, 30 are listed
    add_point(n_small + 2, 3, 100);                                       // DEGENERATE: the point on the centre of keyframe 107
    { float Ow[3]; iba::mapm::camera_centre(T[107].data(), Ow); for (int c = 0; c < 3; ++c) xyz[3 * ((size_t)n_small + 2) + (size_t)c] = Ow[c]; }
    pbad[5] = 1;
    const iba_map_points table{xyz.data(), normal.data(), mn.data(), mx.data(), pdesc.data(), P};
    iba_refresh_options opt{(int32_t)sizeof(iba_refresh_options), 1};
    rfr::Args a{frames.data(), K, kfs.data(), K, &table, pbad.data(), ref.data(), off.data(), okf.data(), okp.data(), nullptr, P, &opt};
    iba_status st = IBA_OK;
    CHECK(rfr::check(a, &st).empty());
    rfr::Result res;
    res.opt = opt;
    rfr::host_call(&res, a);
    CHECK(res.counts.status[IBA_REFRESH_BAD] == 1 && res.counts.status[IBA_REFRESH_EMPTY] == 1 && res.counts.status[IBA_REFRESH_REFRESHED] == P - 2);
    CHECK(res.counts.geo_state[IBA_REFRESH_GEO_NO_REF] == 1 && res.counts.geo_state[IBA_REFRESH_GEO_DEGENERATE] == 1 && res.status[5] == IBA_REFRESH_BAD && res.status[0] == IBA_REFRESH_EMPTY);
    CHECK(res.geo_state[(size_t)n_small + 1] == IBA_REFRESH_GEO_NO_REF && res.min_dist[(size_t)n_small + 1] == 1.f && res.normal[3 * ((size_t)n_small + 1)] != 0.5f);
    CHECK(res.geo_state[(size_t)n_small + 2] == IBA_REFRESH_GEO_DEGENERATE && res.normal[3 * ((size_t)n_small + 2)] == 0.5f && res.max_dist[(size_t)n_small + 2] == 9.f);
    // the literal walk: the full matrix, a sort of every row, element (N - 1) / 2, `<` from INT_MAX
    int n_ties = 0;
    for (int32_t p = 0; p < P; ++p) {
        if (res.status[(size_t)p] != IBA_REFRESH_REFRESHED) continue;
        std::vector<const uint8_t*> d; std::vector<int32_t> pos;
        for (int32_t e = off[(size_t)p]; e < off[(size_t)p + 1]; ++e)
            if (!kfs[(size_t)okf[(size_t)e]].bad) { d.push_back(kdesc[(size_t)okf[(size_t)e]].data() + 32 * okp[(size_t)e]); pos.push_back(e - off[(size_t)p]); }
        const int N = (int)d.size();
        CHECK(res.n_desc[(size_t)p] == N);
        if (!N) { CHECK(res.desc_state[(size_t)p] == IBA_REFRESH_DESC_KEPT && std::memcmp(&res.desc[32 * (size_t)p], &pdesc[32 * (size_t)p], 32) == 0); continue; }
        int best_median = INT_MAX, best_idx = 0, n_at_best = 0;
        for (int i = 0; i < N; ++i) {
            std::vector<int> row((size_t)N);
            for (int j = 0; j < N; ++j) row[(size_t)j] = iba::mapm::host_hamming(d[(size_t)i], d[(size_t)j]);
            std::sort(row.begin(), row.end());
            const int median = row[(size_t)(0.5 * (N - 1))];
            CHECK(res.median[(size_t)res.med_off[(size_t)p] + (size_t)pos[(size_t)i]] == median);
            if (median == best_median) ++n_at_best;
            if (median < best_median) { best_median = median; best_idx = i; n_at_best = 1; }
        }
        n_ties += n_at_best > 1;
        CHECK(res.best_obs[(size_t)p] == pos[(size_t)best_idx] && res.best_median[(size_t)p] == best_median && std::memcmp(&res.desc[32 * (size_t)p], d[(size_t)best_idx], 32) == 0);
    }
    CHECK(n_ties > 5 && res.n_desc[(size_t)n_small] > 900 && res.n_desc[(size_t)n_small] < rfr::kMaxObs);
    // ---- the checks ----
    {
        rfr::Args b = a;
        std::vector<int32_t> big(off);
        const int32_t l2[2] = {1, P};
        b.list = l2; b.n = 2;
        CHECK(rfr::check(b, &st).find("list[1] outside the table") != std::string::npos && st == IBA_ERR_INVALID_ARG);
        b = a; b.n = P - 1;
        CHECK(rfr::check(b, &st).find("list is NULL and n is not") != std::string::npos);
        std::vector<int32_t> twice(okf); twice[(size_t)off[3] + 1] = twice[(size_t)off[3]];
        b = a; b.obs_keyframe = twice.data();
        CHECK(rfr::check(b, &st).find("is listed twice") != std::string::npos);
        std::vector<int32_t> out_kp(okp); out_kp[2] = 3;
        b = a; b.obs_keypoint = out_kp.data();
        CHECK(rfr::check(b, &st).find("a keypoint outside its frame's 3") != std::string::npos);
        const float nan = std::numeric_limits<float>::quiet_NaN();
        const float keep = T[4][7];
        T[4][7] = nan;
        CHECK(rfr::check(a, &st).find("keyframe 4: Tcw12: a value that is not finite") != std::string::npos);
        T[4][7] = keep;
        // one observation above the cap
        std::vector<int32_t> off2(off), okf2(okf), okp2(okp);
        okf2.insert(okf2.begin() + off[(size_t)n_small + 1], 1 + 7 * rfr::kMaxObs % K); okp2.insert(okp2.begin() + off[(size_t)n_small + 1], 0);
        for (size_t p = (size_t)n_small + 1; p < off2.size(); ++p) ++off2[p];
        b = a; b.obs_off = off2.data(); b.obs_keyframe = okf2.data(); b.obs_keypoint = okp2.data();
        CHECK(rfr::check(b, &st).find("above IBA_REFRESH_MAX_OBS") != std::string::npos && st == IBA_ERR_UNSUPPORTED);
        const int32_t l1[1] = {3};
        b.list = l1; b.n = 1;
        CHECK(rfr::check(b, &st).empty());                                // the long point is not listed
    }
    // ---- the helpers ----
    {
        const int32_t kp_off[4] = {0, 3, 5, 8};
        int32_t holder[8] = {2, -1, 0, 0, 1, 2, 1, -1};
        uint8_t bad[3] = {0, 0, 0}, stale[3] = {1, 1, 1};
        int32_t replaced[3] = {-1, -1, -1};
        iba_fuse_map m{3, kp_off, holder, 3, bad, replaced, nullptr, nullptr, stale};
        int32_t o[4], ok[8], oi[8];
        CHECK(rfr::observations(&m, o, ok, oi).empty());
        const int32_t want_o[4] = {0, 2, 4, 6}, want_k[6] = {0, 1, 1, 2, 0, 2}, want_i[6] = {2, 0, 1, 1, 0, 0};
        CHECK(std::equal(o, o + 4, want_o) && std::equal(ok, ok + 6, want_k) && std::equal(oi, oi + 6, want_i));
        holder[7] = 2;
        CHECK(rfr::observations(&m, o, ok, oi).find("point 2 is held twice in keyframe 2") != std::string::npos);
        std::vector<float> n2(normal), mn2(mn), mx2(mx);
        std::vector<uint8_t> d2(pdesc), st2((size_t)P, 1);
        CHECK(rfr::store(res, P, n2.data(), mn2.data(), mx2.data(), d2.data(), st2.data()).empty());
        CHECK(st2[0] == 1 && st2[5] == 1 && st2[7] == 0 && n2[3 * 7] == res.normal[3 * 7] && mx2[7] == res.max_dist[7] && std::memcmp(&d2[32 * 7], &res.desc[32 * 7], 32) == 0 && mx2[5] == 9.f);
        CHECK(rfr::store(res, P - 1, n2.data(), mn2.data(), mx2.data(), d2.data(), nullptr).find("outside the table's") != std::string::npos);
    }
    std::printf("refresh_selftest ok\n");
    return 0;
}

// Stand-alone sanitizer self-test of the ORB extraction's host half (csrc/iba_orb_host.hpp): the plan of several image sizes, the cells' tiling, the
// resize tables, the quadtree distribution on seeded and hand-built candidate sets, the arctangent and the sine / cosine pair. Plain g++, no HIP:
//   make -C csrc san/orb_selftest_asan && csrc/san/orb_selftest_asan
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../iba_orb_host.hpp"

namespace orb = iba::orb;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }

static int check_distribute(const std::vector<int32_t>& xy, const std::vector<int32_t>& score, int32_t width, int32_t height, int32_t N) {
    std::vector<int32_t> chosen;
    orb::DistributeStats st;
    orb::distribute(xy.data(), score.data(), (int32_t)score.size(), width, height, N, chosen, &st);
    std::set<int32_t> seen(chosen.begin(), chosen.end());
    CHECK(seen.size() == chosen.size());
    CHECK(chosen.size() <= score.size());
    for (const int32_t c : chosen) CHECK(c >= 0 && (size_t)c < score.size());
    if (!score.empty()) CHECK(!chosen.empty());
    return 0;
}

int main() {
    iba_orb_options o;
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int32_t)sizeof(o); o.n_features = 2000; o.scale_factor = 1.2f; o.n_levels = 8; o.ini_th_fast = 20; o.min_th_fast = 7;
    CHECK(orb::check_options(&o, false).empty());
    CHECK(!orb::check_options(&o, true).empty());       // no pattern
    orb::Plan p;
    CHECK(orb::make_plan(1241, 376, o, p).empty());
    const int32_t feats[8] = {434, 362, 302, 251, 209, 175, 145, 122}, um[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    for (int l = 0; l < 8; ++l) CHECK(p.lv[l].n_features == feats[l]);
    for (int v = 0; v < 16; ++v) CHECK(p.umax[v] == um[v]);
    CHECK(p.lv[7].W == 346 && p.lv[7].H == 105);
    CHECK(!orb::make_plan(100, 260, o, p).empty());     // cells but no start node
    const int32_t sizes[6][2] = {{1241, 376}, {200, 150}, {97, 83}, {320, 120}, {700, 937}, {40, 3}};
    for (const auto& wh : sizes) {
        CHECK(orb::make_plan(wh[0], wh[1], o, p).empty());
        for (int l = 0; l < p.L; ++l) {
            const orb::LevelPlan& v = p.lv[l];
            if (l > 0 && v.W > 0) {
                std::vector<int32_t> tab(2 * (size_t)v.W);
                orb::resize_table(p.lv[l - 1].W, v.W, tab.data());
                for (int32_t d = 0; d < v.W; ++d) CHECK(tab[2 * d] >= 0 && tab[2 * d] < p.lv[l - 1].W && tab[2 * d + 1] >= 0 && tab[2 * d + 1] <= 2048);
            }
            if (v.nCols < 1) continue;
            std::vector<int> cover((size_t)v.W * (size_t)v.H, 0);
            for (int i = 0; i < v.nRows; ++i)
                for (int j = 0; j < v.nCols; ++j) {
                    int32_t r[4];
                    if (!orb::cell_region(v, i, j, r)) continue;
                    CHECK(r[1] - r[0] <= 59 && r[3] - r[2] <= 59);
                    for (int y = r[2]; y < r[3]; ++y) for (int x = r[0]; x < r[1]; ++x) ++cover[(size_t)y * (size_t)v.W + (size_t)x];
                }
            for (int y = 0; y < v.H; ++y)
                for (int x = 0; x < v.W; ++x) CHECK(cover[(size_t)y * (size_t)v.W + (size_t)x] == (x >= 19 && x < v.W - 19 && y >= 19 && y < v.H - 19 ? 1 : 0));
        }
    }
    // seeded candidate sets at several sizes and N, distinct pixels
    uint32_t s = 12345u;
    for (int round = 0; round < 40; ++round) {
        const int32_t width = 30 + (int32_t)(lcg(s) % 400u), height = std::max<int32_t>(30, width / (1 + (int32_t)(lcg(s) % 4u)));
        const int32_t n = (int32_t)(lcg(s) % 600u);
        std::set<std::pair<int32_t, int32_t>> pts;
        while ((int32_t)pts.size() < std::min(n, width * height / 4)) pts.insert({(int32_t)(lcg(s) % (uint32_t)width), (int32_t)(lcg(s) % (uint32_t)height)});
        std::vector<int32_t> xy, score;
        for (const auto& q : pts) { xy.push_back(q.first); xy.push_back(q.second); score.push_back(7 + (int32_t)(lcg(s) % 40u)); }
        for (const int32_t N : {0, 1, 7, 60, 300, 5000})
            if (check_distribute(xy, score, width, height, N)) return 1;
    }
    if (check_distribute({5, 7}, {9}, 60, 40, 10)) return 1;
    if (check_distribute({}, {}, 60, 40, 10)) return 1;
    if (check_distribute({41, 3, 50, 30, 60, 10, 79, 39, 45, 20}, {10, 30, 20, 30, 5}, 120, 40, 3)) return 1;
    // the arctangent and the sine / cosine pair over their ranges
    for (int k = 0; k < 100000; ++k) {
        const float y = (float)((int32_t)(lcg(s) % 6000001u) - 3000000), x = (float)((int32_t)(lcg(s) % 6000001u) - 3000000);
        const float a = orb::orb_atan2_deg(y, x);
        CHECK(a >= 0.f && a <= 360.f);
        double c, sn;
        orb::orb_sincos((double)(a * (float)(3.14159265358979323846 / 180.0)), &c, &sn);
        CHECK(std::fabs(c * c + sn * sn - 1.0) < 1e-14);
        CHECK(std::fabs(c - std::cos((double)(a * (float)(3.14159265358979323846 / 180.0)))) < 1e-15);
    }
    std::printf("orb_selftest ok\n");
    return 0;
}

// Stand-alone sanitizer self-test of the pose optimisation's host half (csrc/iba_pose_host.hpp) over the arithmetic the kernels compile
// (csrc/iba_pose_math.hpp): the argument checks, the series of P6 at known angles, Exp, the Jacobian against differences, the whole call on the host
// on a synthetic job with outliers, on the small jobs that end early, and the edge builder. Plain g++, no HIP:
//   make -C csrc san/pose_selftest_asan && csrc/san/pose_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_pose_host.hpp"

namespace ps = iba::pose;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static double unit(uint32_t& s) { return (double)(lcg(s) % 100000) / 100000.0; }

struct Scene {
    std::vector<float> xyz, obs, w;
    double T_true[12], T_start[12];
    iba_pose_job q{};
    // n points 4..30 m in front of a camera at a small rotation; every `bad_every`-th observation is moved by 60 pixels
    Scene(int32_t n, uint32_t seed, int32_t bad_every) : xyz(3 * (size_t)n), obs(2 * (size_t)n), w((size_t)n) {
        const float fx = 700.f, fy = 700.f, cx = 620.f, cy = 188.f;
        const double id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        const double d_true[6] = {0.05, -0.1, 0.02, 0.3, -0.2, 0.5}, d_start[6] = {0.01, 0.008, -0.012, 0.05, -0.04, 0.08};
        ps::exp_update(d_true, id, T_true);
        ps::exp_update(d_start, T_true, T_start);
        for (int32_t i = 0; i < n; ++i) {
            const double X = -8.0 + 16.0 * unit(seed), Y = -2.0 + 4.0 * unit(seed), Z = 4.0 + 26.0 * unit(seed);
            xyz[3 * (size_t)i] = (float)X; xyz[3 * (size_t)i + 1] = (float)Y; xyz[3 * (size_t)i + 2] = (float)Z;
            const double Xf = xyz[3 * (size_t)i], Yf = xyz[3 * (size_t)i + 1], Zf = xyz[3 * (size_t)i + 2];
            const double px = T_true[0] * Xf + T_true[1] * Yf + T_true[2] * Zf + T_true[3], py = T_true[4] * Xf + T_true[5] * Yf + T_true[6] * Zf + T_true[7],
                         pz = T_true[8] * Xf + T_true[9] * Yf + T_true[10] * Zf + T_true[11];
            const bool bad = bad_every && i % bad_every == bad_every - 1;
            obs[2 * (size_t)i] = (float)(fx * px / pz + cx + (bad ? 60.0 : 0.0)); obs[2 * (size_t)i + 1] = (float)(fy * py / pz + cy);
            w[(size_t)i] = (float)std::pow(1.2, -2.0 * (double)(i % 8));
        }
        q.Tcw12 = T_start; q.xyz = xyz.data(); q.obs = obs.data(); q.inv_sigma2 = w.data(); q.n = n; q.fx = fx; q.fy = fy; q.cx = cx; q.cy = cy;
    }
};

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    iba_pose_options o{};
    o.struct_size = (int32_t)sizeof(o); o.rounds = 4; o.iterations = 10; o.chi2_threshold = 5.991f; o.huber_delta = ps::default_delta(); o.robust_rounds = 3; o.keep_stages = 1;

    // ---- P6: the series at 0, at a small and a large angle, against libm's value of the same quantity ----
    {
        CHECK(ps::series(0.0, 1) == 1.0 && ps::series(0.0, 2) == 0.5 && ps::series(0.0, 3) == 1.0 / 6.0);
        for (double th : {1e-4, 0.3, 1.0, 2.0, 3.0, 3.14159}) {
            const double s = th * th, t = std::sqrt(s);
            CHECK(std::fabs(ps::series(s, 1) - std::sin(t) / t) <= 4e-16);
            CHECK(std::fabs(ps::series(s, 2) - (1.0 - std::cos(t)) / s) <= 4e-16 + 2.3e-16 / s);      // libm's form cancels: an ulp of 1, divided by s
            if (t > 0.2) CHECK(std::fabs(ps::series(s, 3) - (t - std::sin(t)) / (s * t)) <= 1e-14);
        }
    }
    // ---- Exp: a rotation about z by pi / 2 and a pure translation; beyond pi the libm branch reports itself ----
    {
        const double id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        double T[12];
        const double dz[6] = {0, 0, 1.5707963267948966, 0, 0, 0};
        CHECK(ps::exp_update(dz, id, T) == 0);
        CHECK(std::fabs(T[0]) < 1e-15 && std::fabs(T[1] + 1.0) < 1e-15 && std::fabs(T[4] - 1.0) < 1e-15 && T[10] == 1.0 && T[3] == 0.0);
        const double dt[6] = {0, 0, 0, 1, 2, 3};
        CHECK(ps::exp_update(dt, id, T) == 0 && T[3] == 1.0 && T[7] == 2.0 && T[11] == 3.0 && T[0] == 1.0);
        const double db[6] = {0, 4.0, 0, 0, 0, 0};
        CHECK(ps::exp_update(db, id, T) == 1 && std::fabs(T[0] - std::cos(4.0)) < 1e-15);
    }
    // ---- P1: the Jacobian against central differences through Exp ----
    {
        Scene sc(8, 5u, 0);
        const ps::Cam K{700.0, 700.0, 620.0, 188.0};
        for (int i = 0; i < 8; ++i) {
            double ex, ey, c, J[12];
            ps::edge(sc.T_start, K, sc.xyz[3 * i], sc.xyz[3 * i + 1], sc.xyz[3 * i + 2], sc.obs[2 * i], sc.obs[2 * i + 1], sc.w[i], &ex, &ey, &c, J);
            for (int k = 0; k < 6; ++k) {
                double dp[6] = {0}, dm[6] = {0}, Tp[12], Tm[12], exp_, eyp, exm, eym, cc;
                dp[k] = 1e-6; dm[k] = -1e-6;
                ps::exp_update(dp, sc.T_start, Tp); ps::exp_update(dm, sc.T_start, Tm);
                ps::edge(Tp, K, sc.xyz[3 * i], sc.xyz[3 * i + 1], sc.xyz[3 * i + 2], sc.obs[2 * i], sc.obs[2 * i + 1], sc.w[i], &exp_, &eyp, &cc, nullptr);
                ps::edge(Tm, K, sc.xyz[3 * i], sc.xyz[3 * i + 1], sc.xyz[3 * i + 2], sc.obs[2 * i], sc.obs[2 * i + 1], sc.w[i], &exm, &eym, &cc, nullptr);
                CHECK(std::fabs((exp_ - exm) / 2e-6 - J[k]) <= 1e-4 * (1.0 + std::fabs(J[k])));
                CHECK(std::fabs((eyp - eym) / 2e-6 - J[6 + k]) <= 1e-4 * (1.0 + std::fabs(J[6 + k])));
            }
        }
    }
    // ---- the checks ----
    {
        Scene sc(20, 7u, 0);
        CHECK(ps::check_options(&o).empty() && ps::check_jobs(&sc.q, 1).empty());
        CHECK(!ps::check_options(nullptr).empty() && !ps::check_jobs(nullptr, 1).empty() && !ps::check_jobs(&sc.q, 0).empty());
        iba_pose_options b = o;
        b.struct_size = 4; CHECK(!ps::check_options(&b).empty()); b = o;
        b.rounds = 0; CHECK(!ps::check_options(&b).empty()); b.rounds = 9; CHECK(!ps::check_options(&b).empty()); b = o;
        b.iterations = 0; CHECK(!ps::check_options(&b).empty()); b.iterations = 101; CHECK(!ps::check_options(&b).empty()); b = o;
        b.chi2_threshold = nan; CHECK(!ps::check_options(&b).empty()); b = o;
        b.huber_delta = 0.f; CHECK(!ps::check_options(&b).empty()); b = o;
        b.robust_rounds = -1; CHECK(!ps::check_options(&b).empty());
        iba_pose_job q = sc.q;
        q.n = -1; CHECK(!ps::check_jobs(&q, 1).empty()); q.n = IBA_ORB_MATCH_MAX_KEYPOINTS + 1; CHECK(!ps::check_jobs(&q, 1).empty()); q = sc.q;
        q.fx = 0.f; CHECK(!ps::check_jobs(&q, 1).empty()); q = sc.q;
        q.cy = inf; CHECK(!ps::check_jobs(&q, 1).empty()); q = sc.q;
        q.xyz = nullptr; CHECK(!ps::check_jobs(&q, 1).empty()); q = sc.q;
        sc.w[3] = -1.f; CHECK(!ps::check_jobs(&q, 1).empty()); sc.w[3] = nan; CHECK(!ps::check_jobs(&q, 1).empty()); sc.w[3] = 1.f;
        sc.obs[5] = inf; CHECK(!ps::check_jobs(&q, 1).empty()); sc.obs[5] = 0.f;
        sc.xyz[7] = nan; CHECK(!ps::check_jobs(&q, 1).empty()); sc.xyz[7] = 1.f;
        sc.T_start[4] = nan; CHECK(!ps::check_jobs(&q, 1).empty());
        q.n = 0; q.xyz = nullptr; q.obs = nullptr; q.inv_sigma2 = nullptr; sc.T_start[4] = 0.0; CHECK(ps::check_jobs(&q, 1).empty());
    }
    // ---- the whole call on the host: exact observations but every 5th one gross: those and only those are flagged, the pose comes back ----
    for (int32_t n : {300, 257, 1500}) {
        Scene sc(n, 11u + (uint32_t)n, 5);
        ps::JobOut out;
        std::vector<uint8_t> flag((size_t)n);
        std::vector<float> chi2((size_t)n);
        ps::host_job(sc.q, o, out, flag.data(), chi2.data());
        CHECK(out.r.n == n && out.r.rounds_run == 4 && out.r.n_inliers == n - n / 5 && out.big_steps == 0);
        for (int32_t i = 0; i < n; ++i) CHECK(flag[(size_t)i] == (i % 5 == 4 ? 1 : 0));
        for (int k = 0; k < 12; ++k) CHECK(std::fabs(out.r.Tcw12[k] - sc.T_true[k]) < 1e-3);       // float32 observations: a few 1e-5 pixels
        for (int r = 0; r < 4; ++r) CHECK(out.r.lm_iterations[r] >= 1 && out.r.trials[r] >= out.r.lm_iterations[r] && out.r.n_bad[r] >= n / 5);
        CHECK(out.r.n_bad[3] == n / 5);
        // one linearisation: symmetric H, and the chi2 sum equals the per-edge chi2 summed the same way
        double H[36], b[6], c;
        std::vector<double> ce((size_t)n);
        ps::host_eval(sc.q, nullptr, 0, H, b, &c, ce.data());
        for (int r = 0; r < 6; ++r) for (int cc = 0; cc < 6; ++cc) CHECK(H[r * 6 + cc] == H[cc * 6 + r]);
        CHECK(c > 0.0 && std::isfinite(c));
    }
    // ---- the small jobs: n < 3 does nothing, n < 10 runs one round ----
    for (int32_t n : {0, 1, 2, 3, 9, 10}) {
        Scene sc(n, 3u, 0);
        ps::JobOut out;
        std::vector<uint8_t> flag((size_t)n + 1);
        std::vector<float> chi2((size_t)n + 1);
        ps::host_job(sc.q, o, out, flag.data(), chi2.data());
        CHECK(out.r.rounds_run == (n < 3 ? 0 : (n < 10 ? 1 : 4)));
        CHECK(out.r.n_inliers == (n < 3 ? 0 : n));
        if (n < 3) for (int k = 0; k < 12; ++k) CHECK(out.r.Tcw12[k] == sc.T_start[k]);
    }
    // ---- a point behind the camera: the chi2 is what IEEE gives and nothing traps ----
    {
        Scene sc(40, 9u, 0);
        sc.xyz[2] = -50.f; sc.xyz[5] = (float)(-sc.T_start[11] / sc.T_start[10]);
        ps::JobOut out;
        std::vector<uint8_t> flag(40);
        std::vector<float> chi2(40);
        ps::host_job(sc.q, o, out, flag.data(), chi2.data());
        CHECK(out.r.rounds_run == 4);
    }
    // ---- P9 ----
    {
        const int32_t match[6] = {2, -1, 0, 2, -1, 3}, qidx[6] = {5, 4, 3, 2, 1, 0}, oct[4] = {0, 1, 2, 7};
        const float world[18] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5}, xy[8] = {10, 11, 20, 21, 30, 31, 40, 41}, lv[8] = {1.f, .5f, .25f, .125f, .1f, .05f, .02f, .01f};
        float xyz[12], obs[8], w[4];
        int32_t idx[4], n = -1;
        CHECK(ps::edges_from_matches(match, qidx, 6, world, 6, xy, oct, 4, lv, 8, xyz, obs, w, idx, &n).empty());
        CHECK(n == 3 && idx[0] == 0 && idx[1] == 2 && idx[2] == 3);
        CHECK(xyz[0] == 3.f && xyz[3] == 2.f && xyz[6] == 0.f);         // keypoint 2 was named by queries 0 and 3: the later one (last keypoint 2) holds
        CHECK(obs[0] == 10.f && obs[2] == 30.f && obs[5] == 41.f && w[0] == 1.f && w[1] == .25f && w[2] == .01f);
        const int32_t bad_match[1] = {4};
        CHECK(!ps::edges_from_matches(bad_match, nullptr, 1, world, 6, xy, oct, 4, lv, 8, xyz, obs, w, idx, &n).empty());
        CHECK(!ps::edges_from_matches(match, qidx, 6, world, 5, xy, oct, 4, lv, 8, xyz, obs, w, idx, &n).empty());
        CHECK(!ps::edges_from_matches(match, qidx, 6, world, 6, xy, oct, 4, lv, 7, xyz, obs, w, idx, &n).empty());
    }
    std::printf("pose selftest: 0 failure(s)\n");
    return 0;
}

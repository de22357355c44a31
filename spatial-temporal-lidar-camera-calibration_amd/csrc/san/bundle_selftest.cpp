// Stand-alone sanitizer self-test of the bundle adjustment's host half (csrc/iba_bundle_host.hpp) over the arithmetic the kernels compile
// (csrc/iba_bundle_math.hpp): the argument checks, the plan of a job, the local-window helper, the point Jacobian against differences, the reduced
// solve against a residual, and the whole call and the single evaluation on the host on synthetic jobs (outliers, no free camera, no edge, a point
// behind a camera). Plain g++, no HIP:
//   make -C csrc san/bundle_selftest_asan && csrc/san/bundle_selftest_asan
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../iba_bundle_host.hpp"

namespace bd = iba::bundle;
namespace ps = iba::pose;

#define CHECK(c)                                                                  \
    do {                                                                          \
        if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } \
    } while (0)

static uint32_t lcg(uint32_t& s) { s = s * 1664525u + 1013904223u; return s >> 8; }
static double unit(uint32_t& s) { return (double)(lcg(s) % 100000) / 100000.0; }

// nc cameras side by side looking down z at np points 6..14 m away; every camera sees every point; the first n_fixed cameras are fixed and start at
// the truth, the others start a little off; every `bad_every`-th observation is moved by 60 pixels
struct Scene {
    std::vector<double> T_true, T_start;
    std::vector<uint8_t> fixed;
    std::vector<float> xyz, obs, w;
    std::vector<int32_t> ep, ec;
    iba_bundle_job q{};
    Scene(int32_t nc, int32_t np, int32_t n_fixed, uint32_t seed, int32_t bad_every) : T_true(12 * (size_t)nc), T_start(12 * (size_t)nc), fixed((size_t)nc), xyz(3 * (size_t)np) {
        const float fx = 700.f, fy = 700.f, cx = 620.f, cy = 188.f;
        const double id[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
        for (int32_t c = 0; c < nc; ++c) {
            const double d_true[6] = {0.01 * c, -0.02 * c, 0.005, 0.5 * c, 0.05 * c, 0.1}, d_start[6] = {0.002, -0.001, 0.0015, 0.01, -0.008, 0.012};
            ps::exp_update(d_true, id, &T_true[12 * (size_t)c]);
            fixed[(size_t)c] = c < n_fixed ? 1 : 0;
            if (c < n_fixed) for (int k = 0; k < 12; ++k) T_start[12 * (size_t)c + k] = T_true[12 * (size_t)c + k];
            else ps::exp_update(d_start, &T_true[12 * (size_t)c], &T_start[12 * (size_t)c]);
        }
        for (int32_t p = 0; p < np; ++p) { xyz[3 * (size_t)p] = (float)(-3.0 + 6.0 * unit(seed)); xyz[3 * (size_t)p + 1] = (float)(-1.0 + 2.0 * unit(seed)); xyz[3 * (size_t)p + 2] = (float)(6.0 + 8.0 * unit(seed)); }
        int32_t e = 0;
        for (int32_t p = 0; p < np; ++p)
            for (int32_t c = nc - 1; c >= 0; --c, ++e) {      // cameras descending: the lists are not in edge order by construction alone
                double P[3];
                bd::camera_point(&T_true[12 * (size_t)c], xyz[3 * (size_t)p], xyz[3 * (size_t)p + 1], xyz[3 * (size_t)p + 2], P);
                const bool bad = bad_every && e % bad_every == bad_every - 1;
                ep.push_back(p); ec.push_back(c);
                obs.push_back((float)(fx * P[0] / P[2] + cx + (bad ? 60.0 : 0.0))); obs.push_back((float)(fy * P[1] / P[2] + cy));
                w.push_back((float)std::pow(1.2, -2.0 * (double)(e % 8)));
            }
        q.Tcw12 = T_start.data(); q.fixed = fixed.data(); q.xyz = xyz.data(); q.edge_point = ep.data(); q.edge_camera = ec.data(); q.obs = obs.data(); q.inv_sigma2 = w.data();
        q.n_cameras = nc; q.n_points = np; q.n_edges = e; q.fx = fx; q.fy = fy; q.cx = cx; q.cy = cy;
    }
};

static iba_bundle_options local_options() {
    iba_bundle_options o{};
    o.struct_size = (int32_t)sizeof(o); o.rounds = 2; o.iterations[0] = 5; o.iterations[1] = 10; o.robust_rounds = 1; o.chi2_threshold = 5.991f; o.huber_delta = bd::local_delta(); o.keep_stages = 1;
    return o;
}

int main() {
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const iba_bundle_options o = local_options();

    // ---- the checks ----
    {
        Scene sc(3, 10, 1, 7u, 0);
        std::vector<bd::Plan> plans;
        CHECK(bd::check_options(&o).empty() && bd::check_jobs(&sc.q, 1, &plans).empty());
        CHECK(!bd::check_options(nullptr).empty() && !bd::check_jobs(nullptr, 1, &plans).empty() && !bd::check_jobs(&sc.q, 0, &plans).empty());
        iba_bundle_options b = o;
        b.struct_size = 4; CHECK(!bd::check_options(&b).empty()); b = o;
        b.rounds = 0; CHECK(!bd::check_options(&b).empty()); b.rounds = 5; CHECK(!bd::check_options(&b).empty()); b = o;
        b.iterations[1] = 0; CHECK(!bd::check_options(&b).empty()); b.iterations[1] = 101; CHECK(!bd::check_options(&b).empty()); b = o;
        b.iterations[3] = -7; CHECK(bd::check_options(&b).empty()); b = o;          // beyond `rounds`: not read
        b.chi2_threshold = nan; CHECK(!bd::check_options(&b).empty()); b = o;
        b.huber_delta = 0.f; CHECK(!bd::check_options(&b).empty()); b = o;
        b.robust_rounds = -1; CHECK(!bd::check_options(&b).empty());
        iba_bundle_job q = sc.q;
        q.n_edges = -1; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); q = sc.q;
        q.n_points = IBA_BUNDLE_MAX_COUNT + 1; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); q = sc.q;
        q.fx = 0.f; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); q = sc.q;
        q.cy = inf; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); q = sc.q;
        q.fixed = nullptr; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); q = sc.q;
        sc.w[3] = -1.f; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.w[3] = nan; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.w[3] = 1.f;
        sc.obs[5] = inf; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.obs[5] = 0.f;
        sc.xyz[7] = nan; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.xyz[7] = 1.f;
        sc.T_start[16] = nan; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.T_start[16] = 0.0;
        sc.ep[2] = 10; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.ep[2] = 0;
        sc.ec[4] = -1; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.ec[4] = 1;
        sc.ec[0] = sc.ec[1]; CHECK(!bd::check_jobs(&q, 1, &plans).empty()); sc.ec[0] = 2;       // a duplicate (point 0, camera)
        CHECK(bd::check_jobs(&q, 1, &plans).empty());
        Scene many(66, 2, 1, 3u, 0);
        CHECK(!bd::check_jobs(&many.q, 1, &plans).empty());                                    // 65 free cameras
        iba_bundle_job none{};
        none.fx = none.fy = 500.f;
        CHECK(bd::check_jobs(&none, 1, &plans).empty());                                       // nothing at all is legal
    }
    // ---- the plan: stable lists, the blocks by (a, b), the items by point ----
    {
        Scene sc(4, 6, 1, 9u, 0);
        bd::Plan pl;
        CHECK(bd::make_plan(sc.q, &pl).empty());
        CHECK(pl.n_free == 3 && pl.blk_a.size() == 6 && pl.it_p.size() == 6 * 6);
        for (int32_t p = 0; p < 6; ++p) for (int32_t k = pl.pt_off[(size_t)p]; k + 1 < pl.pt_off[(size_t)p + 1]; ++k) CHECK(pl.pt_edges[(size_t)k] < pl.pt_edges[(size_t)k + 1]);
        for (int32_t c = 0; c < 4; ++c) for (int32_t k = pl.cam_off[(size_t)c]; k + 1 < pl.cam_off[(size_t)c + 1]; ++k) CHECK(pl.cam_edges[(size_t)k] < pl.cam_edges[(size_t)k + 1]);
        for (size_t b = 0; b < pl.blk_a.size(); ++b) {
            CHECK(pl.blk_a[b] <= pl.blk_b[b] && pl.blk_a[b] >= 1);
            for (int32_t k = pl.blk_off[b]; k < pl.blk_off[b + 1]; ++k) {
                CHECK(sc.ec[(size_t)pl.it_ea[(size_t)k]] == pl.blk_a[b] && sc.ec[(size_t)pl.it_eb[(size_t)k]] == pl.blk_b[b]);
                CHECK(sc.ep[(size_t)pl.it_ea[(size_t)k]] == pl.it_p[(size_t)k] && sc.ep[(size_t)pl.it_eb[(size_t)k]] == pl.it_p[(size_t)k]);
                if (k > pl.blk_off[b]) CHECK(pl.it_p[(size_t)k - 1] < pl.it_p[(size_t)k]);
            }
        }
    }
    // ---- the window helper on a map of four keyframes ----
    {
        //                 point, keyframe, keypoint
        const int32_t obs[] = {0, 1, 5,  0, 0, 2,  1, 1, 3,  1, 3, 0,  2, 2, 1,  2, 1, 9,  3, 3, 4,  4, 1, 1,  4, 2, 7};
        const uint8_t pbad[5] = {0, 0, 0, 0, 1}, kbad[4] = {0, 0, 0, 0};
        const int32_t cov[1] = {2};
        bd::Window w;
        CHECK(bd::local_window(obs, 9, pbad, 5, kbad, 4, 1, cov, 1, &w).empty());
        // local: keyframes 1, 2. Points by keyframe 1's keypoints 1 (point 4, bad), 3 (point 1), 5 (point 0), 9 (point 2). Fixed: 3 (from point 1), 0 (from point 0)
        CHECK(w.n_local == 2 && w.camera_keyframe == (std::vector<int32_t>{1, 2, 3, 0}) && w.fixed == (std::vector<uint8_t>{0, 0, 1, 1}));
        CHECK(w.point_id == (std::vector<int32_t>{1, 0, 2}));
        CHECK(w.edge_point == (std::vector<int32_t>{0, 0, 1, 1, 2, 2}) && w.edge_camera == (std::vector<int32_t>{0, 2, 3, 0, 0, 1}) && w.edge_keypoint == (std::vector<int32_t>{3, 0, 2, 5, 9, 1}));
        const uint8_t kbad3[4] = {0, 0, 0, 1};
        CHECK(bd::local_window(obs, 9, pbad, 5, kbad3, 4, 1, cov, 1, &w).empty());
        CHECK(w.camera_keyframe == (std::vector<int32_t>{1, 2, 0}) && w.edge_point.size() == 5);
        const int32_t twice[2] = {2, 2}, self[1] = {1};
        CHECK(!bd::local_window(obs, 9, pbad, 5, kbad, 4, 1, twice, 2, &w).empty() && !bd::local_window(obs, 9, pbad, 5, kbad, 4, 1, self, 1, &w).empty());
        CHECK(!bd::local_window(obs, 9, pbad, 5, kbad, 4, 4, cov, 1, &w).empty() && !bd::local_window(obs, 9, pbad, 3, kbad, 4, 1, cov, 1, &w).empty());
        const int32_t dup[] = {0, 1, 5, 0, 1, 6};
        CHECK(!bd::local_window(dup, 2, pbad, 5, kbad, 4, 1, cov, 1, &w).empty());
    }
    // ---- B1: the point Jacobian against central differences ----
    {
        Scene sc(2, 8, 1, 5u, 0);
        const ps::Cam K{700.0, 700.0, 620.0, 188.0};
        for (int i = 0; i < 8; ++i) {
            const double* T = &sc.T_start[12];
            double X[3] = {sc.xyz[3 * i], sc.xyz[3 * i + 1], sc.xyz[3 * i + 2]}, P[3], Jl[6];
            bd::camera_point(T, X[0], X[1], X[2], P);
            bd::point_jacobian(T, K, P, Jl);
            for (int k = 0; k < 3; ++k) {
                double Xp[3] = {X[0], X[1], X[2]}, Xm[3] = {X[0], X[1], X[2]}, exp_, eyp, exm, eym, cc;
                Xp[k] += 1e-6; Xm[k] -= 1e-6;
                ps::edge(T, K, Xp[0], Xp[1], Xp[2], 0.0, 0.0, 1.0, &exp_, &eyp, &cc, nullptr);
                ps::edge(T, K, Xm[0], Xm[1], Xm[2], 0.0, 0.0, 1.0, &exm, &eym, &cc, nullptr);
                CHECK(std::fabs((exp_ - exm) / 2e-6 - Jl[k]) <= 1e-4 * (1.0 + std::fabs(Jl[k])));
                CHECK(std::fabs((eyp - eym) / 2e-6 - Jl[3 + k]) <= 1e-4 * (1.0 + std::fabs(Jl[3 + k])));
            }
        }
    }
    // ---- B7: the reduced solve leaves a small residual, and refuses a matrix that is not positive definite ----
    {
        const int n = 7;
        std::vector<double> A((size_t)n * n), S((size_t)n * n), b((size_t)n), x((size_t)n), y((size_t)n);
        uint32_t s = 3u;
        for (int i = 0; i < n; ++i) for (int k = 0; k <= i; ++k) A[(size_t)i * n + k] = A[(size_t)k * n + i] = (i == k ? 10.0 : 0.0) + unit(s);
        for (int i = 0; i < n; ++i) { b[(size_t)i] = unit(s); for (int k = 0; k <= i; ++k) S[bd::sidx(n, i, k)] = A[(size_t)i * n + k]; }
        CHECK(bd::reduced_solve(S.data(), n, b.data(), x.data(), y.data()));
        for (int i = 0; i < n; ++i) { double r = -b[(size_t)i]; for (int k = 0; k < n; ++k) r += A[(size_t)i * n + k] * x[(size_t)k]; CHECK(std::fabs(r) < 1e-13); }
        S[bd::sidx(2, 0, 0)] = 1.0; S[bd::sidx(2, 1, 0)] = 2.0; S[bd::sidx(2, 1, 1)] = 1.0;
        CHECK(!bd::reduced_solve(S.data(), 2, b.data(), x.data(), y.data()));
        CHECK(bd::reduced_solve(S.data(), 0, b.data(), x.data(), y.data()));
    }
    // ---- the whole call on the host: exact observations but every 7th one gross: those are flagged, the cameras come back ----
    for (int32_t nc : {2, 5}) {
        Scene sc(nc, 70, nc == 2 ? 1 : 2, 11u + (uint32_t)nc, 7);
        std::vector<bd::Plan> plans;
        CHECK(bd::check_jobs(&sc.q, 1, &plans).empty());
        iba_bundle_batch res;
        res.opt = o; res.job.resize(1);
        bd::host_call(&sc.q, plans, 1, o, &res);
        const iba_bundle_job_out& out = res.job[0];
        CHECK(out.r.rounds_run == 2 && out.r.n_free == nc - (nc == 2 ? 1 : 2) && res.big_steps == 0);
        CHECK(out.stT.size() == 2 * 12 * (size_t)nc && out.stX.size() == 2 * 3 * 70);
        for (int32_t e = 0; e < sc.q.n_edges; ++e) if (e % 7 == 6) CHECK(out.outlier[(size_t)e] == 1);
        CHECK(out.r.n_outliers >= sc.q.n_edges / 7 && out.r.n_bad[0] >= sc.q.n_edges / 7);
        for (int r = 0; r < 2; ++r) CHECK(out.r.lm_iterations[r] >= 1 && out.r.trials[r] >= out.r.lm_iterations[r]);
        for (size_t k = 0; k < 12 * (size_t)(nc == 2 ? 1 : 2); ++k) CHECK(out.T[k] == sc.T_start[k]);     // the fixed cameras are untouched
        if (nc == 5) for (size_t k = 0; k < out.T.size(); ++k) CHECK(std::fabs(out.T[k] - sc.T_true[k]) < 5e-2);
        // one evaluation: the reduced matrix is symmetric, its size follows the free cameras, the step is finite
        std::vector<double> S((size_t)(36 * nc * nc)), dp(6 * (size_t)nc), dl(3 * 70);
        iba_bundle_eval_out ev{};
        ev.S = S.data(); ev.dp = dp.data(); ev.dl = dl.data();
        bd::host_eval(&sc.q, plans, 1, nullptr, 1, 1e-3, &ev);
        CHECK(ev.solved == 1 && ev.n_reduced == 6 * out.r.n_free && ev.chi2_robust > 0.0 && ev.lambda == 1e-3);
        for (int i = 0; i < ev.n_reduced; ++i) for (int k = 0; k < ev.n_reduced; ++k) CHECK(S[(size_t)i * ev.n_reduced + k] == S[(size_t)k * ev.n_reduced + i]);
        for (double v : dp) CHECK(std::isfinite(v));
        for (double v : dl) CHECK(std::isfinite(v));
    }
    // ---- no free camera, no edge, no point, and a point behind a camera: nothing traps, the estimates stay finite where the inputs allow ----
    {
        Scene fixed_only(3, 20, 3, 2u, 0), behind(2, 20, 1, 4u, 0);
        behind.xyz[2] = -50.f;
        iba_bundle_job none{};
        none.fx = none.fy = 500.f;
        iba_bundle_job no_edges = fixed_only.q;
        no_edges.n_edges = 0;
        for (const iba_bundle_job* q : {&fixed_only.q, &behind.q, &none, &no_edges}) {
            std::vector<bd::Plan> plans;
            CHECK(bd::check_jobs(q, 1, &plans).empty());
            iba_bundle_batch res;
            res.opt = o; res.job.resize(1);
            bd::host_call(q, plans, 1, o, &res);
            CHECK(res.job[0].r.rounds_run == 2 && (int32_t)res.job[0].outlier.size() == q->n_edges);
        }
    }
    std::printf("bundle selftest: 0 failure(s)\n");
    return 0;
}

// The LiDAR back end's loop-closure run (include/iba_mi355x.h, iba_backend_*): the defaults of backend.yml, the plan (iba_backend_host.hpp, host only)
// and iba_backend_run, which composes the library's own entry points — iba_submap_handle, iba_sc_*, iba_scan_register, iba_smooth_* — and launches no
// kernel of its own. Clouds stay on the device from the raw scans to the registration; the host sees poses, plans and results.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_backend_host.hpp"
#include "iba_pgo_math.hpp"

struct iba_backend_result {
    std::vector<double> poses12;
    std::vector<int32_t> keyframes;
    std::vector<iba_backend_detection> detections;
    std::vector<iba_smooth_result> updates;
    std::vector<std::vector<double>> update_poses12;   // with keep_update_poses: the estimates after every update, 12 per node
};

namespace {
thread_local std::string t_err;
iba_status fail(iba_status s, const std::string& m) { t_err = m; return s; }
}  // namespace

extern "C" {

const char* iba_backend_last_error(void) { return t_err.c_str(); }

iba_status iba_default_backend_options(iba_backend_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->voxel = 0.2; o->keyframe_meter_gap = 1.5; o->keyframe_rad_gap = 0.15;
    o->lc_keyframe_meter_gap = 3.0; o->lc_keyframe_rad_gap = 1.0; o->lc_submap_size = 25;
    o->loop_overlap_thre = 0.5; o->loop_inlier_rmse_thre = 0.2;
    o->cloud_lag = 1;
    iba_status st = iba_default_sc_options(&o->sc);
    if (st == IBA_OK) st = iba_default_scan_options(&o->scan);
    if (st == IBA_OK) st = iba_default_smooth_options(&o->smooth);
    if (st != IBA_OK) return st;
    o->sc.dist_thres = 0.2; o->sc.max_radius = 80.0;          // BackEndOption scDistThres, scMaximumRadius
    // Registration(src, tgt, init, icp_corase_dist, icp_refine_dist) as written: the distances stand where the iteration counts are taken
    o->scan.estimation = IBA_SCAN_POINT_TO_POINT;
    o->scan.coarse_dist = 1.0; o->scan.coarse_max_iter = 1; o->scan.coarse_rel_fitness = 1e-4; o->scan.coarse_rel_rmse = 1e-4;
    o->scan.refine_dist = 0.3; o->scan.refine_max_iter = 0; o->scan.refine_rel_fitness = 1e-6; o->scan.refine_rel_rmse = 1e-6;
    o->scan.info_dist = 0.0;
    for (int k = 0; k < 6; ++k) { o->prior_var[k] = 1e-12; o->odom_var[k] = k < 3 ? 1e-6 : 1e-4; o->loop_var[k] = 0.5; }
    return IBA_OK;
}

iba_status iba_backend_plan(const double* poses12, int32_t N, const iba_backend_options* opt, int32_t* keyframes, int32_t* described, uint8_t* detects, int32_t* n_keyframes,
                            int32_t* sizes_at_call, int32_t* n_calls) {
    std::string why = iba::backend::validate_options(opt);
    if (why.empty()) why = iba::backend::validate_poses(poses12, N);
    if (!why.empty()) return fail(IBA_ERR_INVALID_ARG, "iba_backend_plan: " + why);
    const iba::backend::Plan p = iba::backend::make_plan(poses12, N, *opt);
    for (size_t k = 0; k < p.keyframes.size(); ++k) {
        if (keyframes) keyframes[k] = p.keyframes[k];
        if (described) described[k] = p.described[k];
        if (detects) detects[k] = p.detects[k];
    }
    if (n_keyframes) *n_keyframes = (int32_t)p.keyframes.size();
    if (sizes_at_call) for (size_t k = 0; k < p.sizes_at_call.size(); ++k) sizes_at_call[k] = p.sizes_at_call[k];
    if (n_calls) *n_calls = (int32_t)p.sizes_at_call.size();
    return IBA_OK;
}

iba_status iba_backend_run(iba_handle* h, const double* poses12, int32_t N, const iba_backend_options* opt, iba_backend_result** out) {
    using namespace iba::backend;
    if (out) *out = nullptr;
    if (!h) return fail(IBA_ERR_INVALID_ARG, "iba_backend_run: h is NULL");
    if (!out) return fail(IBA_ERR_INVALID_ARG, "iba_backend_run: out is NULL");
    std::string why = validate_options(opt);
    if (why.empty()) why = validate_poses(poses12, N);
    if (!why.empty()) return fail(IBA_ERR_INVALID_ARG, "iba_backend_run: " + why);
    const Plan plan = make_plan(poses12, N, *opt);                                                  // step 1
    const int32_t K = (int32_t)plan.keyframes.size(), n_calls = (int32_t)plan.sizes_at_call.size();
    iba_params params;
    if (iba_default_params(&params) != IBA_OK) return fail(IBA_ERR_INVALID_ARG, "iba_backend_run: iba_default_params");
    const double eye12[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    iba_handle* clouds = nullptr;
    iba_sc_db* db = nullptr;
    iba_smooth* sm = nullptr;
    iba_handle* lc = nullptr;
    auto bail = [&](iba_status st, const std::string& m) {
        if (lc) iba_destroy(lc);
        if (sm) iba_smooth_destroy(sm);
        if (db) iba_sc_db_free(db);
        if (clouds) iba_destroy(clouds);
        return fail(st, "iba_backend_run: " + m);
    };
    // step 2: the voxel clouds of all described frames as one batch; frame k of `clouds` is keyframe k's cloud
    std::vector<iba_submap_desc> subs(K);
    for (int32_t k = 0; k < K; ++k) subs[k] = iba_submap_desc{(int32_t)sizeof(iba_submap_desc), 1, &plan.described[k], eye12, nullptr, opt->voxel};
    iba_status st = iba_submap_handle(h, subs.data(), K, &params, &clouds);
    if (st != IBA_OK) return bail(st, std::string("iba_submap_handle (described frames): ") + iba_last_error(h));
    const int device = iba_handle_device(h);
    // steps 3 and 4: one describe, the whole detection sequence in one detect
    std::vector<int32_t> nodes(K);
    for (int32_t k = 0; k < K; ++k) nodes[k] = k;
    st = iba_sc_describe(clouds, nodes.data(), K, &opt->sc, &db);
    if (st != IBA_OK) return bail(st, std::string("iba_sc_describe: ") + iba_last_error(clouds));
    std::vector<iba_sc_result> hits(std::max(n_calls, 1));
    if (n_calls > 0) {
        std::vector<int32_t> db_end(n_calls);
        st = iba_sc_replay_plan(plan.sizes_at_call.data(), n_calls, &opt->sc, db_end.data());
        if (st != IBA_OK) return bail(st, std::string("iba_sc_replay_plan: ") + iba_sc_last_error(nullptr));
        std::vector<iba_sc_query> q(n_calls);
        for (int32_t c = 0; c < n_calls; ++c) q[c] = iba_sc_query{(int32_t)sizeof(iba_sc_query), plan.sizes_at_call[c] - 1, db_end[c], 0};
        st = iba_sc_detect(db, q.data(), n_calls, &opt->sc, hits.data());
        if (st != IBA_OK) return bail(st, std::string("iba_sc_detect: ") + iba_sc_last_error(db));
    }
    iba_sc_db_free(db); db = nullptr;
    // steps 5-10
    st = iba_smooth_create(&opt->smooth, device, &sm);
    if (st != IBA_OK) return bail(st, std::string("iba_smooth_create: ") + iba_smooth_last_error(nullptr));
    iba_backend_result* res = new iba_backend_result();
    res->keyframes = plan.keyframes;
    std::vector<double>& cur = res->poses12;                                                        // the CURRENT poses: estimates where optimised, raw elsewhere
    cur.assign(poses12, poses12 + 12 * (size_t)N);
    auto fail_run = [&](iba_status s2, const std::string& m) { delete res; return bail(s2, m); };
    auto to16 = [](const double* p12, double* p16) { std::memcpy(p16, p12, 12 * sizeof(double)); p16[12] = 0.0; p16[13] = 0.0; p16[14] = 0.0; p16[15] = 1.0; };
    auto pull = [&](int32_t count) -> iba_status {                                                  // estimates of nodes 0 .. count - 1 into cur
        std::vector<double> n16(16 * (size_t)count);
        const iba_status s2 = iba_smooth_read(sm, 0, count, n16.data(), nullptr);
        if (s2 == IBA_OK) for (int32_t i = 0; i < count; ++i) std::memcpy(&cur[12 * (size_t)i], &n16[16 * (size_t)i], 12 * sizeof(double));
        if (s2 == IBA_OK && opt->keep_update_poses) res->update_poses12.emplace_back(cur.begin(), cur.begin() + 12 * (size_t)count);
        return s2;
    };
    double p16[16], z16[16];
    to16(poses12, p16);
    st = iba_smooth_add_node(sm, p16);
    if (st == IBA_OK) st = iba_smooth_add_prior(sm, 0, p16, opt->prior_var);
    if (st != IBA_OK) return fail_run(st, std::string("node 0: ") + iba_smooth_last_error(sm));
    int32_t k = 1, call = 0;
    for (int32_t j = 1; j < N; ++j) {
        // step 6: between(raw_(j-1), raw_j) = raw_(j-1)^-1 raw_j, node j at its raw pose
        double inv[12], rel[12];
        iba::pgo::inv12(poses12 + 12 * (size_t)(j - 1), inv);
        iba::pgo::mul12(inv, poses12 + 12 * (size_t)j, rel);
        to16(poses12 + 12 * (size_t)j, p16); to16(rel, z16);
        st = iba_smooth_add_node(sm, p16);
        if (st == IBA_OK) st = iba_smooth_add_between(sm, j - 1, j, z16, opt->odom_var, 0);
        if (st != IBA_OK) return fail_run(st, "frame " + std::to_string(j) + ": " + iba_smooth_last_error(sm));
        if (k >= K || plan.keyframes[k] != j) continue;
        const int32_t kq = k++;
        if (!plan.detects[kq]) continue;
        const iba_sc_result& hit = hits[call++];
        if (hit.loop_node < 0) continue;
        // step 7: the sub-map around the history frame at the current poses, in the history frame; the query's voxel cloud; registration from the identity
        const int32_t history = plan.keyframes[hit.loop_node];
        const int32_t lo = std::max(0, history - opt->lc_submap_size), hi = std::min(history + opt->lc_submap_size, N);
        std::vector<int32_t> members;
        for (int32_t f = lo; f < hi; ++f) members.push_back(f);
        double out12[12];
        iba::pgo::inv12(&cur[12 * (size_t)history], out12);
        iba_submap_desc pair[2];
        pair[0] = iba_submap_desc{(int32_t)sizeof(iba_submap_desc), 1, &plan.described[kq], eye12, nullptr, opt->voxel};
        pair[1] = iba_submap_desc{(int32_t)sizeof(iba_submap_desc), (int32_t)members.size(), members.data(), &cur[12 * (size_t)lo], out12, opt->voxel};
        st = iba_submap_handle(h, pair, 2, &params, &lc);
        if (st != IBA_OK) return fail_run(st, "iba_submap_handle (loop " + std::to_string(history) + ", " + std::to_string(j) + "): " + iba_last_error(h));
        iba_scan_edge edge{};
        edge.src_frame = 0; edge.tgt_frame = 1;
        edge.T[0] = edge.T[5] = edge.T[10] = edge.T[15] = 1.0;
        iba_scan_result reg;
        st = iba_scan_register(lc, &edge, 1, &opt->scan, &reg);
        if (st != IBA_OK) return fail_run(st, std::string("iba_scan_register: ") + iba_last_error(lc));
        iba_destroy(lc); lc = nullptr;
        iba_backend_detection d{};
        d.query_frame = j; d.history_frame = history; d.sc_dist = hit.min_dist; d.fitness = reg.reg.fitness; d.rmse = reg.reg.inlier_rmse;
        std::memcpy(d.T, reg.reg.T, sizeof(d.T));
        d.accepted = (reg.reg.fitness > opt->loop_overlap_thre && reg.reg.inlier_rmse < opt->loop_inlier_rmse_thre) ? 1 : 0;   // step 8: both strict
        res->detections.push_back(d);
        if (!d.accepted) continue;
        // step 9
        d.T[12] = 0.0; d.T[13] = 0.0; d.T[14] = 0.0; d.T[15] = 1.0;
        st = iba_smooth_add_between(sm, history, j, d.T, opt->loop_var, 1);
        iba_smooth_result ur;
        if (st == IBA_OK) st = iba_smooth_update(sm, &ur);
        if (st == IBA_OK) { res->updates.push_back(ur); st = pull(j + 1); }
        if (st != IBA_OK) return fail_run(st, "loop (" + std::to_string(history) + ", " + std::to_string(j) + "): " + iba_smooth_last_error(sm));
    }
    iba_smooth_result ur;                                                                           // step 10
    st = iba_smooth_update(sm, &ur);
    if (st == IBA_OK) { res->updates.push_back(ur); st = pull(N); }
    if (st != IBA_OK) return fail_run(st, std::string("the final update: ") + iba_smooth_last_error(sm));
    iba_smooth_destroy(sm);
    iba_destroy(clouds);
    *out = res;
    return IBA_OK;
}

void iba_backend_result_free(iba_backend_result* r) { delete r; }
int32_t iba_backend_result_n_frames(const iba_backend_result* r) { return r ? (int32_t)(r->poses12.size() / 12) : 0; }
const double* iba_backend_result_poses12(const iba_backend_result* r) { return r ? r->poses12.data() : nullptr; }
int32_t iba_backend_result_n_keyframes(const iba_backend_result* r) { return r ? (int32_t)r->keyframes.size() : 0; }
const int32_t* iba_backend_result_keyframes(const iba_backend_result* r) { return r ? r->keyframes.data() : nullptr; }
int32_t iba_backend_result_n_detections(const iba_backend_result* r) { return r ? (int32_t)r->detections.size() : 0; }
const iba_backend_detection* iba_backend_result_detections(const iba_backend_result* r) { return r ? r->detections.data() : nullptr; }
int32_t iba_backend_result_n_updates(const iba_backend_result* r) { return r ? (int32_t)r->updates.size() : 0; }
const iba_smooth_result* iba_backend_result_updates(const iba_backend_result* r) { return r ? r->updates.data() : nullptr; }
const double* iba_backend_result_update_poses12(const iba_backend_result* r, int32_t u) {
    return (r && u >= 0 && (size_t)u < r->update_poses12.size()) ? r->update_poses12[u].data() : nullptr;
}

}  // extern "C"

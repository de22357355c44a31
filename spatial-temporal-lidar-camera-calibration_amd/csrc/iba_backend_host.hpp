// Host side of the LiDAR back end's loop-closure run (include/iba_mi355x.h, iba_backend_*). Plain C++, no HIP: the argument checks and the plan —
// SCManage's keyframe and loop-closure gates (backend_opt.cpp:338-370) as a pure function of the raw poses. tests/backend_ref.py restates it.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"

namespace iba { namespace backend {

struct Plan {
    std::vector<int32_t> keyframes;       // KeyFrameQuery: frame 0 first
    std::vector<int32_t> described;       // per keyframe, the frame whose cloud is described
    std::vector<uint8_t> detects;         // per keyframe, 1: detectLoopClosureID is called with it as the query
    std::vector<int32_t> sizes_at_call;   // per call, the descriptors held (iba_sc_replay_plan)
};

inline std::string validate_options(const iba_backend_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_backend_options)) return "opt->struct_size is " + std::to_string(o->struct_size) + ", this library's iba_backend_options has " + std::to_string(sizeof(iba_backend_options));
    const double v[] = {o->voxel, o->keyframe_meter_gap, o->keyframe_rad_gap, o->lc_keyframe_meter_gap, o->lc_keyframe_rad_gap, o->loop_overlap_thre, o->loop_inlier_rmse_thre};
    for (double x : v) if (!std::isfinite(x)) return "an option is not finite";
    for (int k = 0; k < 6; ++k)
        for (double x : {o->prior_var[k], o->odom_var[k], o->loop_var[k]}) if (!std::isfinite(x) || !(x > 0.0)) return "a variance is not finite or not > 0";
    if (!(o->voxel > 0.0)) return "voxel is not > 0";
    if (o->lc_submap_size < 0) return "lc_submap_size " + std::to_string(o->lc_submap_size) + " < 0";
    if (o->keep_update_poses != 0 && o->keep_update_poses != 1) return "keep_update_poses " + std::to_string(o->keep_update_poses) + " is neither 0 nor 1";
    if (o->cloud_lag != 0 && o->cloud_lag != 1) return "cloud_lag " + std::to_string(o->cloud_lag) + " is neither 0 nor 1";
    return "";
}

inline std::string validate_poses(const double* poses12, int32_t N) {
    if (N < 1) return "N = " + std::to_string(N) + " < 1";
    if (!poses12) return "poses12 is NULL";
    for (size_t k = 0; k < 12 * (size_t)N; ++k) if (!std::isfinite(poses12[k])) return "pose " + std::to_string(k / 12) + " is not finite";
    return "";
}

// PoseDif (backend_opt.cpp:19-24) of two row-major 3x4: |t_b - t_a| and the angle of R_b R_a^T as atan2(s, c), c = (trace - 1) / 2, s = half the
// norm of (R21 - R12, R02 - R20, R10 - R01); every sum in ascending index
inline void pose_dif(const double* a, const double* b, double* translation, double* rotation) {
    const double dx = b[3] - a[3], dy = b[7] - a[7], dz = b[11] - a[11];
    *translation = std::sqrt((dx * dx + dy * dy) + dz * dz);
    double R[9];
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r * 3 + c] = (b[r * 4] * a[c * 4] + b[r * 4 + 1] * a[c * 4 + 1]) + b[r * 4 + 2] * a[c * 4 + 2];
    const double cs = (((R[0] + R[4]) + R[8]) - 1.0) / 2.0;
    const double vx = R[7] - R[5], vy = R[2] - R[6], vz = R[3] - R[1];
    const double sn = std::sqrt((vx * vx + vy * vy) + vz * vz) / 2.0;
    *rotation = std::atan2(sn, cs);
}

inline Plan make_plan(const double* poses12, int32_t N, const iba_backend_options& o) {
    Plan p;
    p.keyframes.push_back(0); p.described.push_back(0); p.detects.push_back(0);   // SCManage(0): described, never a query
    double t_acc = 0.0, r_acc = 0.0, lc_t_acc = 0.0, lc_r_acc = 0.0;
    for (int32_t j = 1; j < N; ++j) {
        double td, rd;
        pose_dif(poses12 + 12 * (size_t)(j - 1), poses12 + 12 * (size_t)j, &td, &rd);
        t_acc += td; r_acc += rd; lc_t_acc += td; lc_r_acc += rd;
        if (t_acc > o.keyframe_meter_gap || r_acc > o.keyframe_rad_gap) {
            t_acc = 0.0; r_acc = 0.0;
            p.keyframes.push_back(j); p.described.push_back(j - o.cloud_lag);
            const bool detect = lc_t_acc > o.lc_keyframe_meter_gap || lc_r_acc > o.lc_keyframe_rad_gap;
            if (detect) { lc_t_acc = 0.0; lc_r_acc = 0.0; p.sizes_at_call.push_back((int32_t)p.described.size()); }
            p.detects.push_back(detect ? 1 : 0);
        }
    }
    return p;
}

} }  // namespace iba::backend

// Map-point refresh (include/iba_mi355x.h, iba_refresh*): the C ABI, the result object and the launches of a call. The kernel is
// iba_refresh_kernels.hpp, the decisions iba_refresh_math.hpp, the host rules (argument checks, the restatement, the two helpers)
// iba_refresh_host.hpp. A per-call unit (iba_call.hpp) without chunks: the call allocates its inputs and outputs only - no N x N table leaves the
// LDS - so there is no budget. Frames, keyframe tables, the point table and the observation lists go up once as flat tables; the host, which holds
// obs_off, settles BAD and EMPTY (S1) and bins the other listed points by the length of their list into three work lists, one launch each; the
// results come down by slot. The result is host memory.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_call.hpp"
#include "iba_device_buf.hpp"
#include "iba_refresh_host.hpp"
#include "iba_refresh_kernels.hpp"

using iba::DevBuf;
namespace rfr = iba::rfr;

struct iba_refreshed : rfr::Result {};

namespace {
thread_local iba::CallError t_err;

constexpr int kShippedNarrowLanes = 16;   // profiles/refresh_bench.md
constexpr int kShippedRowForm = 1;        // one pass that keeps the row: profiles/refresh_bench.md

template <int G>
void launch(bool row, uint32_t n_work, hipStream_t st, const rfr::Tables& t, const rfr::Outputs& o, const int32_t* work) {
    const uint32_t per_block = (uint32_t)(rfr::kThreads / G), blocks = (n_work + per_block - 1) / per_block;
    if (row) hipLaunchKernelGGL((rfr::refresh_kernel<G, true>), dim3(blocks), dim3(rfr::kThreads), 0, st, t, o, work, (int)n_work);
    else hipLaunchKernelGGL((rfr::refresh_kernel<G, false>), dim3(blocks), dim3(rfr::kThreads), 0, st, t, o, work, (int)n_work);
}

iba_status run_call(iba_refreshed* res, const rfr::Args& a, int device) {
    const iba_map_points& pts = *a.points;
    const size_t P = (size_t)pts.n, n = (size_t)a.n, n_obs = (size_t)a.obs_off[P];
    // ---- the flat tables ----
    uint64_t n_kp = 0;
    std::vector<int32_t> kp_base((size_t)a.F);
    for (int32_t f = 0; f < a.F; ++f) { kp_base[(size_t)f] = (int32_t)n_kp; n_kp += (uint64_t)a.frames[f].n; }
    if (n_kp >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "2^31 keypoints or more in one call");
    std::vector<uint8_t> h_desc(32 * (size_t)n_kp);
    std::vector<int32_t> h_octave((size_t)n_kp), h_obs_kp(n_obs);
    for (int32_t f = 0; f < a.F; ++f) {
        const iba_orb_frame& fr = a.frames[f];
        if (!fr.n) continue;
        std::memcpy(&h_desc[32 * (size_t)kp_base[(size_t)f]], fr.desc, 32 * (size_t)fr.n);
        std::memcpy(&h_octave[(size_t)kp_base[(size_t)f]], fr.octave, sizeof(int32_t) * (size_t)fr.n);
    }
    for (size_t e = 0; e < n_obs; ++e) h_obs_kp[e] = kp_base[(size_t)a.keyframes[a.obs_keyframe[e]].frame] + a.obs_keypoint[e];
    std::vector<rfr::KfRec> kf; std::vector<rfr::KfScale> sc;
    rfr::make_keyframes(a, kf, sc);
    res->size_for(a);                         // S1 on the host: BAD and EMPTY are settled, every output holds the table's values
    // ---- the device from here on ----
    int narrow = kShippedNarrowLanes, row = kShippedRowForm, min_path = IBA_REFRESH_PATH_NARROW;
    if (const char* e = iba::debug_env("IBA_REFRESH_NARROW_LANES")) {
        const int w = std::atoi(e);
        if (w == 4 || w == 8 || w == 16 || w == 32) narrow = w;
    }
    if (const char* e = iba::debug_env("IBA_REFRESH_MEDIAN")) row = std::atoi(e) == 1 ? 1 : 0;
    if (const char* e = iba::debug_env("IBA_REFRESH_MIN_PATH")) {
        const int m = std::atoi(e);
        if (m == IBA_REFRESH_PATH_WAVE || m == IBA_REFRESH_PATH_BLOCK) min_path = m;
    }
    const bool timing = iba::debug_env("IBA_REFRESH_TIMING") != nullptr;
    // the work lists: a point goes to the least shape at or above min_path that holds its FULL list
    std::vector<int32_t> work[3];
    for (size_t s = 0; s < n; ++s) {
        if (res->status[s] != IBA_REFRESH_REFRESHED) continue;
        const int32_t len = a.obs_off[res->point[s] + 1] - a.obs_off[res->point[s]];
        int path = len <= narrow ? IBA_REFRESH_PATH_NARROW : len <= 64 ? IBA_REFRESH_PATH_WAVE : IBA_REFRESH_PATH_BLOCK;
        if (path < min_path) path = min_path;
        work[path].push_back((int32_t)s);
    }
    std::vector<int32_t> h_work;
    size_t work_at[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; ++k) { h_work.insert(h_work.end(), work[k].begin(), work[k].end()); work_at[k + 1] = h_work.size(); res->counts.path[k] = (int32_t)work[k].size(); }
    int32_t h_counts[rfr::kCounters] = {0};
    hipStream_t st = nullptr;
    IBA_CALL_TRY(hipSetDevice(device));
    DevBuf<uint64_t> d_desc, d_pdesc, d_odesc; DevBuf<int32_t> d_octave, d_ref, d_off, d_obs_kf, d_obs_kp, d_slot_point, d_med_off, d_work, d_best_obs, d_best_median, d_n_desc, d_median, d_counts;
    DevBuf<rfr::KfRec> d_kf; DevBuf<rfr::KfScale> d_sc; DevBuf<float> d_xyz, d_normal, d_min, d_max, d_onormal, d_omin, d_omax; DevBuf<uint8_t> d_ds, d_gs;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after the host tables, the result's arrays and the buffers
    IBA_CALL_TRY(d_desc.alloc(4 * (size_t)n_kp)); IBA_CALL_TRY(d_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(d_kf.alloc(kf.size())); IBA_CALL_TRY(d_sc.alloc(sc.size()));
    IBA_CALL_TRY(d_xyz.alloc(3 * P)); IBA_CALL_TRY(d_normal.alloc(3 * P)); IBA_CALL_TRY(d_min.alloc(P)); IBA_CALL_TRY(d_max.alloc(P)); IBA_CALL_TRY(d_pdesc.alloc(4 * P));
    IBA_CALL_TRY(d_ref.alloc(P)); IBA_CALL_TRY(d_off.alloc(P + 1)); IBA_CALL_TRY(d_obs_kf.alloc(n_obs)); IBA_CALL_TRY(d_obs_kp.alloc(n_obs));
    IBA_CALL_TRY(d_slot_point.alloc(n)); IBA_CALL_TRY(d_med_off.alloc(n + 1)); IBA_CALL_TRY(d_work.alloc(h_work.size()));
    IBA_CALL_TRY(d_ds.alloc(n)); IBA_CALL_TRY(d_gs.alloc(n)); IBA_CALL_TRY(d_best_obs.alloc(n)); IBA_CALL_TRY(d_best_median.alloc(n)); IBA_CALL_TRY(d_n_desc.alloc(n));
    IBA_CALL_TRY(d_onormal.alloc(3 * n)); IBA_CALL_TRY(d_omin.alloc(n)); IBA_CALL_TRY(d_omax.alloc(n)); IBA_CALL_TRY(d_odesc.alloc(4 * n));
    IBA_CALL_TRY(d_median.alloc(res->median.size())); IBA_CALL_TRY(d_counts.alloc(rfr::kCounters));
#define IBA_RFR_UP(dst, src, count) \
    if (count) IBA_CALL_TRY(hipMemcpyAsync((dst).p, (src), sizeof(*(dst).p) * (size_t)(count), hipMemcpyHostToDevice, st))
#define IBA_RFR_DOWN(dst, src, count) \
    if (count) IBA_CALL_TRY(hipMemcpyAsync((dst), (src).p, sizeof(*(src).p) * (size_t)(count), hipMemcpyDeviceToHost, st))
    IBA_RFR_UP(d_desc, (const uint64_t*)(const void*)h_desc.data(), 4 * (size_t)n_kp); IBA_RFR_UP(d_octave, h_octave.data(), n_kp);
    IBA_RFR_UP(d_kf, kf.data(), kf.size()); IBA_RFR_UP(d_sc, sc.data(), sc.size());
    IBA_RFR_UP(d_xyz, pts.xyz, 3 * P); IBA_RFR_UP(d_normal, pts.normal, 3 * P); IBA_RFR_UP(d_min, pts.min_dist, P); IBA_RFR_UP(d_max, pts.max_dist, P);
    IBA_RFR_UP(d_pdesc, (const uint64_t*)(const void*)pts.desc, 4 * P);
    IBA_RFR_UP(d_ref, a.ref_keyframe, P); IBA_RFR_UP(d_off, a.obs_off, P + 1); IBA_RFR_UP(d_obs_kf, a.obs_keyframe, n_obs); IBA_RFR_UP(d_obs_kp, h_obs_kp.data(), n_obs);
    IBA_RFR_UP(d_slot_point, res->point.data(), n); IBA_RFR_UP(d_med_off, res->med_off.data(), n + 1); IBA_RFR_UP(d_work, h_work.data(), h_work.size());
    // the outputs start as S1 left them: the kernel writes the slots of its work lists only
    IBA_RFR_UP(d_ds, res->desc_state.data(), n); IBA_RFR_UP(d_gs, res->geo_state.data(), n); IBA_RFR_UP(d_best_obs, res->best_obs.data(), n);
    IBA_RFR_UP(d_best_median, res->best_median.data(), n); IBA_RFR_UP(d_n_desc, res->n_desc.data(), n); IBA_RFR_UP(d_onormal, res->normal.data(), 3 * n);
    IBA_RFR_UP(d_omin, res->min_dist.data(), n); IBA_RFR_UP(d_omax, res->max_dist.data(), n); IBA_RFR_UP(d_odesc, (const uint64_t*)(const void*)res->desc.data(), 4 * n);
    IBA_CALL_TRY(hipMemsetAsync(d_counts.p, 0, sizeof(int32_t) * rfr::kCounters, st));
    const rfr::Tables tb{d_desc.p, d_octave.p, d_kf.p, d_sc.p, d_xyz.p, d_normal.p, d_min.p, d_max.p, d_pdesc.p, d_ref.p, d_off.p, d_obs_kf.p, d_obs_kp.p, d_slot_point.p, d_med_off.p};
    const rfr::Outputs out{d_ds.p, d_gs.p, d_best_obs.p, d_best_median.p, d_n_desc.p, d_onormal.p, d_omin.p, d_omax.p, d_odesc.p, res->opt.keep_stages ? d_median.p : nullptr, d_counts.p};
    if (timing) IBA_CALL_TRY(ev.create(4));
    for (int k = 0; k < 3; ++k) {
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[(size_t)k], st));
        const uint32_t nw = (uint32_t)work[k].size();
        if (!nw) continue;
        const int32_t* wl = d_work.p + work_at[k];
        if (k == IBA_REFRESH_PATH_BLOCK) launch<256>(row != 0, nw, st, tb, out, wl);
        else if (k == IBA_REFRESH_PATH_WAVE) launch<64>(row != 0, nw, st, tb, out, wl);
        else if (narrow == 4) launch<4>(row != 0, nw, st, tb, out, wl);
        else if (narrow == 8) launch<8>(row != 0, nw, st, tb, out, wl);
        else if (narrow == 16) launch<16>(row != 0, nw, st, tb, out, wl);
        else launch<32>(row != 0, nw, st, tb, out, wl);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[3], st));
    IBA_RFR_DOWN(res->desc_state.data(), d_ds, n); IBA_RFR_DOWN(res->geo_state.data(), d_gs, n); IBA_RFR_DOWN(res->best_obs.data(), d_best_obs, n);
    IBA_RFR_DOWN(res->best_median.data(), d_best_median, n); IBA_RFR_DOWN(res->n_desc.data(), d_n_desc, n); IBA_RFR_DOWN(res->normal.data(), d_onormal, 3 * n);
    IBA_RFR_DOWN(res->min_dist.data(), d_omin, n); IBA_RFR_DOWN(res->max_dist.data(), d_omax, n); IBA_RFR_DOWN((uint64_t*)(void*)res->desc.data(), d_odesc, 4 * n);
    if (res->opt.keep_stages) IBA_RFR_DOWN(res->median.data(), d_median, res->median.size());
    IBA_RFR_DOWN(h_counts, d_counts, rfr::kCounters);
#undef IBA_RFR_UP
#undef IBA_RFR_DOWN
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (timing)
        for (int k = 0; k < 3; ++k) IBA_CALL_TRY(hipEventElapsedTime(&res->ms[k], ev.e[(size_t)k], ev.e[(size_t)k + 1]));
    // the counts: the statuses are the host's (S1), the states of the refreshed points the device's
    iba_refresh_counts& c = res->counts;
    for (size_t s = 0; s < n; ++s) ++c.status[res->status[s]];
    const int32_t settled = c.status[IBA_REFRESH_BAD] + c.status[IBA_REFRESH_EMPTY];
    for (int k = 0; k < 3; ++k) c.desc_state[k] = h_counts[k];
    for (int k = 0; k < 4; ++k) c.geo_state[k] = h_counts[3 + k];
    c.desc_state[IBA_REFRESH_DESC_NONE] += settled; c.geo_state[IBA_REFRESH_GEO_NONE] += settled;
    c.n_desc_changed = h_counts[7];
    return IBA_OK;
}

iba_status run(const char* name, const rfr::Args& a, int device, bool host, iba_refreshed** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    iba_status st = IBA_ERR_INVALID_ARG;
    const std::string why = rfr::check(a, &st);
    if (!why.empty()) return t_err.fail(st, who + why);
    iba_refreshed* res = new iba_refreshed();
    res->opt = *a.opt;
    if (host) rfr::host_call(res, a);
    else if (const iba_status s = run_call(res, a, device)) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

template <class T>
void copy_out(T* dst, const std::vector<T>& src) {
    if (dst && !src.empty()) std::memcpy(dst, src.data(), sizeof(T) * src.size());
}

}  // namespace

extern "C" {

const char* iba_refresh_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_refresh_options(iba_refresh_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_refresh_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_refresh(const iba_orb_frame* frames, int32_t F, const iba_refresh_keyframe* keyframes, int32_t K, const iba_map_points* points, const uint8_t* point_bad,
                       const int32_t* ref_keyframe, const int32_t* obs_off, const int32_t* obs_keyframe, const int32_t* obs_keypoint, const int32_t* list, int32_t n,
                       const iba_refresh_options* opt, int device, iba_refreshed** out) {
    return run("iba_refresh", rfr::Args{frames, F, keyframes, K, points, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, list, n, opt}, device, false, out);
}

void iba_refreshed_free(iba_refreshed* r) { delete r; }

int32_t iba_refreshed_n(const iba_refreshed* r) { return r ? (int32_t)r->point.size() : 0; }

iba_status iba_refreshed_counts(const iba_refreshed* r, iba_refresh_counts* counts) {
    if (!r || !counts) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_refreshed_counts: a NULL argument");
    *counts = r->counts;
    return IBA_OK;
}

iba_status iba_refreshed_read(const iba_refreshed* r, uint8_t* status, uint8_t* desc_state, uint8_t* geo_state, int32_t* best_obs, int32_t* best_median, int32_t* n_desc, float* normal,
                              float* min_dist, float* max_dist, uint8_t* desc) {
    if (!r) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_refreshed_read: the result is NULL");
    copy_out(status, r->status); copy_out(desc_state, r->desc_state); copy_out(geo_state, r->geo_state); copy_out(best_obs, r->best_obs); copy_out(best_median, r->best_median);
    copy_out(n_desc, r->n_desc); copy_out(normal, r->normal); copy_out(min_dist, r->min_dist); copy_out(max_dist, r->max_dist); copy_out(desc, r->desc);
    return IBA_OK;
}

iba_status iba_refreshed_medians(const iba_refreshed* r, int32_t* off, int32_t* median) {
    if (!r) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_refreshed_medians: the result is NULL");
    if (!r->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_refreshed_medians: the call did not ask for keep_stages");
    copy_out(off, r->med_off); copy_out(median, r->median);
    return IBA_OK;
}

iba_status iba_refresh_observations(const iba_fuse_map* map, int32_t* obs_off, int32_t* obs_keyframe, int32_t* obs_keypoint) {
    const std::string why = rfr::observations(map, obs_off, obs_keyframe, obs_keypoint);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_refresh_observations: " + why);
}

iba_status iba_refresh_store(const iba_refreshed* r, int32_t P, float* normal, float* min_dist, float* max_dist, uint8_t* desc, uint8_t* descriptor_stale) {
    if (!r) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_refresh_store: the result is NULL");
    const std::string why = rfr::store(*r, P, normal, min_dist, max_dist, desc, descriptor_stale);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_refresh_store: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_refresh_host(const iba_orb_frame* frames, int32_t F, const iba_refresh_keyframe* keyframes, int32_t K, const iba_map_points* points, const uint8_t* point_bad,
                                  const int32_t* ref_keyframe, const int32_t* obs_off, const int32_t* obs_keyframe, const int32_t* obs_keypoint, const int32_t* list, int32_t n,
                                  const iba_refresh_options* opt, iba_refreshed** out) {
    return run("iba_debug_refresh_host", rfr::Args{frames, F, keyframes, K, points, point_bad, ref_keyframe, obs_off, obs_keyframe, obs_keypoint, list, n, opt}, 0, true, out);
}

iba_status iba_debug_refresh_stage_ms(const iba_refreshed* r, float ms[3]) {
    if (!r || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_refresh_stage_ms: a NULL argument");
    std::memcpy(ms, r->ms, sizeof(r->ms));
    return IBA_OK;
}

}  // extern "C"

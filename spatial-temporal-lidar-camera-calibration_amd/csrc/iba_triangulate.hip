// New-map-point creation (include/iba_mi355x.h, iba_triangulate*): the C ABI, the result object and the launch chain of a call. The kernels are
// iba_triangulate_kernels.hpp, the float decisions iba_triangulate_math.hpp, the host rules (argument checks, the node order, the restatement, the
// median depth) iba_triangulate_host.hpp. A per-call unit (iba_call.hpp): frames, keyframes with their node order, pairs, jobs and blocks go up
// once as flat tables; the jobs are cut into chunks by their slots; the chain of a chunk: prologue, segments, pick, compaction, triangulation,
// resolve, counts, scan, gather, the results down. The host does nothing between a chunk's upload and its download. The result is host memory.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_call.hpp"
#include "iba_device_buf.hpp"
#include "iba_triangulate_host.hpp"
#include "iba_triangulate_kernels.hpp"

using iba::DevBuf;
using iba::PinnedBuf;
namespace trg = iba::trg;
namespace orbm = iba::orbm;
using trg::BlockRec;
using trg::JobRec;
using trg::JobRes;
using trg::KfRec;
using trg::PairRec;

struct iba_triangulation : trg::Result {};

namespace {
thread_local iba::CallError t_err;

constexpr int kShippedPickLanes = 8;       // the fastest of 8, 16 and 64 on the bench scene: profiles/triangulate_bench.md

uint32_t blocks_of(size_t n) { return (uint32_t)((n + trg::kThreads - 1) / trg::kThreads); }

// the tables and buffers of the whole call
struct CallState {
    std::vector<KfRec> kfs;
    std::vector<PairRec> pairs;
    std::vector<JobRec> jobs;
    std::vector<BlockRec> blocks;
    DevBuf<KfRec> d_kfs; DevBuf<PairRec> d_pairs; DevBuf<JobRec> d_jobs; DevBuf<BlockRec> d_blocks;
    DevBuf<float2> d_xy; DevBuf<int32_t> d_octave, d_kf_node, d_skey, d_sidx; DevBuf<uint64_t> d_desc; DevBuf<uint8_t> d_kf_has;
    int pick_lanes = kShippedPickLanes;
};

void launch_pick(int lanes, uint32_t grid, hipStream_t st, const trg::ChunkView& v, const trg::PairGeom* geom, const int32_t* seg_a, const int32_t* seg_b, uint8_t* status, int32_t* match,
                 int32_t* dist) {
    if (lanes == 16) hipLaunchKernelGGL(trg::trg_pick_kernel<16>, dim3(grid), dim3(trg::kThreads), 0, st, v, geom, seg_a, seg_b, status, match, dist);
    else if (lanes == 64) hipLaunchKernelGGL(trg::trg_pick_kernel<64>, dim3(grid), dim3(trg::kThreads), 0, st, v, geom, seg_a, seg_b, status, match, dist);
    else hipLaunchKernelGGL(trg::trg_pick_kernel<8>, dim3(grid), dim3(trg::kThreads), 0, st, v, geom, seg_a, seg_b, status, match, dist);
}

iba_status run_chunk(iba_triangulation* res, CallState& cs, int32_t ja, int32_t jb, bool timing) {
    hipStream_t st = nullptr;
    const JobRec& first = cs.jobs[(size_t)ja];
    const JobRec& last = cs.jobs[(size_t)jb - 1];
    trg::ChunkView v{};
    v.kfs = cs.d_kfs.p; v.pairs = cs.d_pairs.p; v.jobs = cs.d_jobs.p; v.blocks = cs.d_blocks.p;
    v.xy = cs.d_xy.p; v.octave = cs.d_octave.p; v.desc = cs.d_desc.p; v.kf_node = cs.d_kf_node.p; v.kf_has = cs.d_kf_has.p; v.skey = cs.d_skey.p; v.sidx = cs.d_sidx.p;
    v.slot0 = first.slot_base; v.pair0 = first.pair_base; v.block0 = first.block_base; v.job0 = ja;
    v.n_slots = last.slot_base + last.n_nb * last.n_cur - first.slot_base; v.n_pairs = last.pair_base + last.n_nb - first.pair_base;
    v.n_blocks = last.block_base + last.n_blocks - first.block_base; v.n_jobs = jb - ja;
    v.gt = trg::make_gates(res->opt);
    const size_t nS = (size_t)v.n_slots, nP = (size_t)v.n_pairs, nB = (size_t)v.n_blocks, nJ = (size_t)v.n_jobs;
    size_t max_pts = 0;                       // a keypoint of a job is created at most once
    for (int32_t j = ja; j < jb; ++j)
        if (cs.jobs[(size_t)j].n_nb > 0) max_pts += (size_t)cs.jobs[(size_t)j].n_cur;
    std::vector<int32_t> job_counts(nJ * trg::kStatuses, 0), pair_counts(2 * nP, 0), seg_a, seg_b;
    DevBuf<trg::PairGeom> d_geom; DevBuf<uint8_t> d_status; DevBuf<int32_t> d_match, d_dist, d_seg_a, d_seg_b, d_n_list, d_list_slot, d_list_pair, d_job_counts, d_pair_counts, d_blk_cnt, d_blk_off;
    DevBuf<float> d_xyz, d_p_xyz, d_p_normal, d_p_min, d_p_max; DevBuf<int32_t> d_p_idx1, d_p_nb, d_p_idx2; DevBuf<uint64_t> d_p_desc;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after the host arrays (the counts, the result's) and the buffers
    IBA_CALL_TRY(d_geom.alloc(nP)); IBA_CALL_TRY(d_status.alloc(nS)); IBA_CALL_TRY(d_match.alloc(nS)); IBA_CALL_TRY(d_dist.alloc(nS)); IBA_CALL_TRY(d_xyz.alloc(3 * nS));
    IBA_CALL_TRY(d_seg_a.alloc(nS)); IBA_CALL_TRY(d_seg_b.alloc(nS)); IBA_CALL_TRY(d_n_list.alloc(1)); IBA_CALL_TRY(d_list_slot.alloc(nS)); IBA_CALL_TRY(d_list_pair.alloc(nS));
    IBA_CALL_TRY(d_job_counts.alloc(job_counts.size())); IBA_CALL_TRY(d_pair_counts.alloc(pair_counts.size())); IBA_CALL_TRY(d_blk_cnt.alloc(nB)); IBA_CALL_TRY(d_blk_off.alloc(nB + 1));
    IBA_CALL_TRY(d_p_idx1.alloc(max_pts)); IBA_CALL_TRY(d_p_nb.alloc(max_pts)); IBA_CALL_TRY(d_p_idx2.alloc(max_pts)); IBA_CALL_TRY(d_p_xyz.alloc(3 * max_pts));
    IBA_CALL_TRY(d_p_normal.alloc(3 * max_pts)); IBA_CALL_TRY(d_p_min.alloc(max_pts)); IBA_CALL_TRY(d_p_max.alloc(max_pts)); IBA_CALL_TRY(d_p_desc.alloc(4 * max_pts));
    IBA_CALL_TRY(hipMemsetAsync(d_n_list.p, 0, sizeof(int32_t), st));
    IBA_CALL_TRY(hipMemsetAsync(d_job_counts.p, 0, sizeof(int32_t) * std::max<size_t>(job_counts.size(), 1), st));
    IBA_CALL_TRY(hipMemsetAsync(d_pair_counts.p, 0, sizeof(int32_t) * std::max<size_t>(pair_counts.size(), 1), st));
    if (timing) IBA_CALL_TRY(ev.create(5));
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    const uint32_t gB = (uint32_t)nB;
    if (nP) {
        hipLaunchKernelGGL(trg::trg_prologue_kernel, dim3(blocks_of(nP)), dim3(trg::kThreads), 0, st, v, d_geom.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (nB) {
        hipLaunchKernelGGL(trg::trg_segment_kernel, dim3(gB), dim3(trg::kThreads), 0, st, v, d_geom.p, d_status.p, d_match.p, d_dist.p, d_xyz.p, d_seg_a.p, d_seg_b.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    if (nB) {
        launch_pick(cs.pick_lanes, gB, st, v, d_geom.p, d_seg_a.p, d_seg_b.p, d_status.p, d_match.p, d_dist.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    if (nB) {
        hipLaunchKernelGGL(trg::trg_compact_kernel, dim3(gB), dim3(trg::kThreads), 0, st, v, d_status.p, d_n_list.p, d_list_slot.p, d_list_pair.p);
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(trg::trg_triangulate_kernel, dim3(blocks_of(nS)), dim3(trg::kThreads), 0, st, v, d_n_list.p, d_list_slot.p, d_list_pair.p, d_match.p, d_status.p, d_xyz.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[3], st));
    if (nB) {
        hipLaunchKernelGGL(trg::trg_resolve_kernel, dim3(gB), dim3(trg::kThreads), 0, st, v, d_status.p, d_match.p, d_dist.p, d_xyz.p);
        IBA_CALL_TRY(hipGetLastError());
        hipLaunchKernelGGL(trg::trg_count_kernel, dim3(gB), dim3(trg::kThreads), 0, st, v, d_status.p, d_match.p, d_job_counts.p, d_pair_counts.p, d_blk_cnt.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(trg::orbk::orbm_scan_kernel, dim3(1), dim3(1024), 0, st, d_blk_cnt.p, d_blk_off.p, (int)nB);
    IBA_CALL_TRY(hipGetLastError());
    if (nB) {
        hipLaunchKernelGGL(trg::trg_gather_kernel, dim3(gB), dim3(trg::kThreads), 0, st, v, d_status.p, d_match.p, d_xyz.p, d_blk_off.p, d_p_idx1.p, d_p_nb.p, d_p_idx2.p, d_p_xyz.p, d_p_normal.p,
                           d_p_min.p, d_p_max.p, d_p_desc.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4], st));
    // ---- the results down: the slots and the counts, then the points, whose number the counts give ----
    const size_t s0 = (size_t)v.slot0, p0 = (size_t)v.pair0;
    if (nS) {
        IBA_CALL_TRY(hipMemcpyAsync(res->status.data() + s0, d_status.p, nS, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->match.data() + s0, d_match.p, sizeof(int32_t) * nS, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->dist.data() + s0, d_dist.p, sizeof(int32_t) * nS, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->xyz.data() + 3 * s0, d_xyz.p, sizeof(float) * 3 * nS, hipMemcpyDeviceToHost, st));
        if (res->opt.keep_stages) {
            seg_a.resize(nS); seg_b.resize(nS);
            IBA_CALL_TRY(hipMemcpyAsync(seg_a.data(), d_seg_a.p, sizeof(int32_t) * nS, hipMemcpyDeviceToHost, st));
            IBA_CALL_TRY(hipMemcpyAsync(seg_b.data(), d_seg_b.p, sizeof(int32_t) * nS, hipMemcpyDeviceToHost, st));
        }
    }
    if (nP) IBA_CALL_TRY(hipMemcpyAsync(pair_counts.data(), d_pair_counts.p, sizeof(int32_t) * pair_counts.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipMemcpyAsync(job_counts.data(), d_job_counts.p, sizeof(int32_t) * job_counts.size(), hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipStreamSynchronize(st));
    size_t n_pts = 0;
    for (size_t j = 0; j < nJ; ++j) {
        const int32_t created = job_counts[j * trg::kStatuses + IBA_TRIANGULATE_CREATED];
        if (created < 0 || created > cs.jobs[(size_t)ja + j].n_cur) return t_err.fail(IBA_ERR_STATE, "more created points than keypoints");
        n_pts += (size_t)created;
    }
    if (n_pts > max_pts) return t_err.fail(IBA_ERR_STATE, "more created points than keypoints");
    const size_t at = res->p_idx1.size();
    res->grow_points(at + n_pts);
    if (n_pts) {
        IBA_CALL_TRY(hipMemcpyAsync(res->p_idx1.data() + at, d_p_idx1.p, sizeof(int32_t) * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_nb.data() + at, d_p_nb.p, sizeof(int32_t) * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_idx2.data() + at, d_p_idx2.p, sizeof(int32_t) * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_xyz.data() + 3 * at, d_p_xyz.p, sizeof(float) * 3 * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_normal.data() + 3 * at, d_p_normal.p, sizeof(float) * 3 * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_min.data() + at, d_p_min.p, sizeof(float) * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_max.data() + at, d_p_max.p, sizeof(float) * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->p_desc.data() + 32 * at, d_p_desc.p, 32 * n_pts, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipStreamSynchronize(st));
    }
    sync.disarm();
    if (timing) {
        for (int k = 0; k < 4; ++k) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[(size_t)k], ev.e[(size_t)k + 1])); res->ms[k] += ms; }
    }
    if (res->opt.keep_stages)
        for (size_t s = 0; s < nS; ++s) res->seg_len[s0 + s] = seg_b[s] - seg_a[s];
    size_t pt = at;
    for (size_t j = 0; j < nJ; ++j) {
        JobRes& jr = res->job[(size_t)ja + j];
        std::memcpy(jr.counts.status, &job_counts[j * trg::kStatuses], sizeof(int32_t) * trg::kStatuses);
        jr.counts.n_created = jr.counts.status[IBA_TRIANGULATE_CREATED];
        jr.pt_base = pt; pt += (size_t)jr.counts.n_created;
    }
    for (size_t p = 0; p < nP; ++p) { res->pair_matches[p0 + p] = pair_counts[2 * p]; res->pair_created[p0 + p] = pair_counts[2 * p + 1]; }
    return IBA_OK;
}

iba_status run_call(iba_triangulation* res, const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* kfs, int32_t K, const iba_triangulate_job* jobs, int32_t J, int device) {
    CallState cs;
    // ---- the flat tables ----
    uint64_t n_kp = 0, n_kn = 0, n_slots = 0, n_pairs = 0, n_blocks = 0;
    for (int32_t f = 0; f < F; ++f) n_kp += (uint64_t)frames[f].n;
    for (int32_t k = 0; k < K; ++k) n_kn += (uint64_t)frames[kfs[k].frame].n;
    for (int32_t j = 0; j < J; ++j) {
        const uint64_t n_cur = (uint64_t)frames[kfs[jobs[j].current].frame].n;
        n_slots += (uint64_t)jobs[j].n_neighbours * n_cur; n_pairs += (uint64_t)jobs[j].n_neighbours; n_blocks += (uint64_t)jobs[j].n_neighbours * blocks_of((size_t)n_cur);
    }
    if (n_kp >= (1ull << 31) || n_kn >= (1ull << 31) || n_slots >= (1ull << 31) || n_pairs >= (1ull << 31) || n_blocks >= (1ull << 31))
        return t_err.fail(IBA_ERR_UNSUPPORTED, "2^31 keypoints, slots, pairs or blocks or more in one call");
    std::vector<int32_t> frame_base((size_t)F);
    PinnedBuf<float> h_xy; PinnedBuf<int32_t> h_octave, h_kf_node, h_skey, h_sidx; PinnedBuf<uint8_t> h_desc, h_kf_has;
    // ---- the device from here on ----
    hipStream_t st = nullptr;
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, IBA_TRIANGULATE_BUDGET_BYTES, "IBA_TRIANGULATE_BUDGET", &budget));
    if (const char* e = iba::debug_env("IBA_TRIANGULATE_PICK_LANES")) {
        const int w = std::atoi(e);
        if (w == 8 || w == 16 || w == 64) cs.pick_lanes = w;
    }
    iba::SyncOnExit sync(st);                // after cs, the host tables and the pinned staging
    IBA_CALL_TRY(h_xy.alloc(2 * (size_t)n_kp)); IBA_CALL_TRY(h_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(h_desc.alloc(32 * (size_t)n_kp));
    IBA_CALL_TRY(h_kf_node.alloc((size_t)n_kn)); IBA_CALL_TRY(h_kf_has.alloc((size_t)n_kn)); IBA_CALL_TRY(h_skey.alloc((size_t)n_kn)); IBA_CALL_TRY(h_sidx.alloc((size_t)n_kn));
    size_t base = 0;
    for (int32_t f = 0; f < F; ++f) {
        const iba_orb_frame& fr = frames[f];
        frame_base[(size_t)f] = (int32_t)base;
        const size_t n = (size_t)fr.n;
        if (!n) continue;
        std::memcpy(h_xy.p + 2 * base, fr.xy, sizeof(float) * 2 * n); std::memcpy(h_octave.p + base, fr.octave, sizeof(int32_t) * n); std::memcpy(h_desc.p + 32 * base, fr.desc, 32 * n);
        base += n;
    }
    cs.kfs.resize((size_t)K);
    base = 0;
    for (int32_t k = 0; k < K; ++k) {
        const iba_triangulate_keyframe& a = kfs[k];
        const int32_t n = frames[a.frame].n;
        KfRec& r = cs.kfs[(size_t)k];
        r = trg::make_kf_rec(a, frame_base[(size_t)a.frame], n, (int32_t)base);
        for (int32_t i = 0; i < n; ++i) { h_kf_node.p[base + (size_t)i] = a.node[i]; h_kf_has.p[base + (size_t)i] = (a.has_point && a.has_point[i]) ? 1 : 0; }
        r.n_keys = trg::node_order(a.node, a.has_point, n, h_skey.p + base, h_sidx.p + base);
        for (int32_t e = r.n_keys; e < n; ++e) { h_skey.p[base + (size_t)e] = INT32_MAX; h_sidx.p[base + (size_t)e] = -1; }
        base += (size_t)n;
    }
    cs.jobs.resize((size_t)J); cs.pairs.reserve((size_t)n_pairs); cs.blocks.reserve((size_t)n_blocks);
    std::vector<int64_t> per_job((size_t)J, 0);
    size_t slot = 0;
    for (int32_t j = 0; j < J; ++j) {
        const iba_triangulate_job& b = jobs[j];
        const int32_t n_cur = cs.kfs[(size_t)b.current].n;
        JobRec& rec = cs.jobs[(size_t)j];
        rec.sc = trg::make_scales(b);
        rec.cur = b.current; rec.n_cur = n_cur; rec.n_nb = b.n_neighbours;
        rec.slot_base = (int32_t)slot; rec.pair_base = (int32_t)cs.pairs.size(); rec.block_base = (int32_t)cs.blocks.size(); rec.pad = 0;
        JobRes& jr = res->job[(size_t)j];
        jr.slot_base = slot; jr.pair_base = cs.pairs.size(); jr.pt_base = 0;
        jr.counts = iba_triangulate_counts{};
        jr.counts.n_keypoints = n_cur; jr.counts.n_neighbours = b.n_neighbours;
        for (int32_t pos = 0; pos < b.n_neighbours; ++pos) {
            const int32_t pair = (int32_t)cs.pairs.size();
            cs.pairs.push_back(PairRec{j, b.current, b.neighbours[pos], pos, (int32_t)slot, n_cur});
            for (int32_t i = 0; i < n_cur; i += trg::kThreads) cs.blocks.push_back(BlockRec{pair, i});
            slot += (size_t)n_cur;
        }
        rec.n_blocks = (int32_t)cs.blocks.size() - rec.block_base;
        per_job[(size_t)j] = (int64_t)b.n_neighbours * (int64_t)n_cur;
    }
    res->size_for(n_slots, n_pairs);
    const bool timing = iba::debug_env("IBA_TRIANGULATE_TIMING") != nullptr;
    IBA_CALL_TRY(cs.d_kfs.alloc((size_t)K)); IBA_CALL_TRY(cs.d_pairs.alloc(cs.pairs.size())); IBA_CALL_TRY(cs.d_jobs.alloc((size_t)J)); IBA_CALL_TRY(cs.d_blocks.alloc(cs.blocks.size()));
    IBA_CALL_TRY(cs.d_xy.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_desc.alloc(4 * (size_t)n_kp));
    IBA_CALL_TRY(cs.d_kf_node.alloc((size_t)n_kn)); IBA_CALL_TRY(cs.d_kf_has.alloc((size_t)n_kn)); IBA_CALL_TRY(cs.d_skey.alloc((size_t)n_kn)); IBA_CALL_TRY(cs.d_sidx.alloc((size_t)n_kn));
    IBA_CALL_TRY(hipMemcpyAsync(cs.d_kfs.p, cs.kfs.data(), sizeof(KfRec) * (size_t)K, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(cs.d_jobs.p, cs.jobs.data(), sizeof(JobRec) * (size_t)J, hipMemcpyHostToDevice, st));
    if (!cs.pairs.empty()) IBA_CALL_TRY(hipMemcpyAsync(cs.d_pairs.p, cs.pairs.data(), sizeof(PairRec) * cs.pairs.size(), hipMemcpyHostToDevice, st));
    if (!cs.blocks.empty()) IBA_CALL_TRY(hipMemcpyAsync(cs.d_blocks.p, cs.blocks.data(), sizeof(BlockRec) * cs.blocks.size(), hipMemcpyHostToDevice, st));
    if (n_kp) {
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_xy.p, h_xy.p, sizeof(float) * 2 * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_octave.p, h_octave.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_desc.p, h_desc.p, 32 * (size_t)n_kp, hipMemcpyHostToDevice, st));
    }
    if (n_kn) {
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_kf_node.p, h_kf_node.p, sizeof(int32_t) * (size_t)n_kn, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_kf_has.p, h_kf_has.p, (size_t)n_kn, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_skey.p, h_skey.p, sizeof(int32_t) * (size_t)n_kn, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_sidx.p, h_sidx.p, sizeof(int32_t) * (size_t)n_kn, hipMemcpyHostToDevice, st));
    }
    const std::vector<int32_t> cut = trg::plan_chunks(per_job, budget);
    res->n_chunks = (int32_t)cut.size() - 1;
    for (int32_t c = 0; c < res->n_chunks; ++c)
        if (const iba_status s = run_chunk(res, cs, cut[(size_t)c], cut[(size_t)c + 1], timing)) return s;      // (every chunk waits for its own copies, and so for the uploads)
    sync.disarm();
    return IBA_OK;
}

iba_status check_job_index(const iba_triangulation* t, int32_t job, const char* who) {
    return t_err.check_index(!t, job, t ? t->job.size() : 0, std::string(who) + ": ", "job");
}

iba_status run(const char* name, const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* kfs, int32_t K, const iba_triangulate_job* jobs, int32_t J,
               const iba_triangulate_options* opt, int device, bool host, iba_triangulation** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    std::string why = trg::check_options(opt);
    if (why.empty()) why = orbm::check_frames(frames, F);
    if (why.empty()) why = trg::check_keyframes(frames, F, kfs, K);
    if (why.empty()) why = trg::check_jobs(frames, kfs, K, jobs, J);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_triangulation* res = new iba_triangulation();
    res->opt = *opt;
    res->job.resize((size_t)J);
    if (host) trg::host_call(res, frames, F, kfs, K, jobs, J);
    else if (const iba_status s = run_call(res, frames, F, kfs, K, jobs, J, device)) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

template <class T>
void copy_out(T* dst, const std::vector<T>& src, size_t base, size_t n) {
    if (dst && n) std::memcpy(dst, &src[base], sizeof(T) * n);
}

}  // namespace

extern "C" {

const char* iba_triangulate_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_triangulate_options(iba_triangulate_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_triangulate_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->th_low = 50; opt->min_baseline_ratio = 0.01f; opt->max_cos_parallax = 0.9998f; opt->epipole_gate = 100.f; opt->chi2_line = 3.84f; opt->chi2_mono = 5.991f; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_triangulate(const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* keyframes, int32_t K, const iba_triangulate_job* jobs, int32_t J,
                           const iba_triangulate_options* opt, int device, iba_triangulation** out) {
    return run("iba_triangulate", frames, F, keyframes, K, jobs, J, opt, device, false, out);
}

void iba_triangulation_free(iba_triangulation* t) { delete t; }

int32_t iba_triangulation_n_jobs(const iba_triangulation* t) { return t ? (int32_t)t->job.size() : 0; }

iba_status iba_triangulation_job(const iba_triangulation* t, int32_t job, iba_triangulate_counts* counts, int32_t* n_matches, int32_t* n_created) {
    if (const iba_status s = check_job_index(t, job, "iba_triangulation_job")) return s;
    if (!counts) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_triangulation_job: counts is NULL");
    const JobRes& jr = t->job[(size_t)job];
    *counts = jr.counts;
    copy_out(n_matches, t->pair_matches, jr.pair_base, (size_t)jr.counts.n_neighbours); copy_out(n_created, t->pair_created, jr.pair_base, (size_t)jr.counts.n_neighbours);
    return IBA_OK;
}

iba_status iba_triangulation_read(const iba_triangulation* t, int32_t job, uint8_t* status, int32_t* match, int32_t* dist, float* xyz) {
    if (const iba_status s = check_job_index(t, job, "iba_triangulation_read")) return s;
    const JobRes& jr = t->job[(size_t)job];
    const size_t n = (size_t)jr.counts.n_neighbours * (size_t)jr.counts.n_keypoints, b = jr.slot_base;
    copy_out(status, t->status, b, n); copy_out(match, t->match, b, n); copy_out(dist, t->dist, b, n); copy_out(xyz, t->xyz, 3 * b, 3 * n);
    return IBA_OK;
}

iba_status iba_triangulation_points(const iba_triangulation* t, int32_t job, int32_t* idx1, int32_t* neighbour, int32_t* idx2, float* xyz, float* normal, float* min_dist, float* max_dist,
                                    uint8_t* desc) {
    if (const iba_status s = check_job_index(t, job, "iba_triangulation_points")) return s;
    const JobRes& jr = t->job[(size_t)job];
    const size_t n = (size_t)jr.counts.n_created, b = jr.pt_base;
    copy_out(idx1, t->p_idx1, b, n); copy_out(neighbour, t->p_nb, b, n); copy_out(idx2, t->p_idx2, b, n); copy_out(xyz, t->p_xyz, 3 * b, 3 * n);
    copy_out(normal, t->p_normal, 3 * b, 3 * n); copy_out(min_dist, t->p_min, b, n); copy_out(max_dist, t->p_max, b, n); copy_out(desc, t->p_desc, 32 * b, 32 * n);
    return IBA_OK;
}

iba_status iba_triangulation_segments(const iba_triangulation* t, int32_t job, int32_t* seg_len) {
    if (const iba_status s = check_job_index(t, job, "iba_triangulation_segments")) return s;
    if (!t->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_triangulation_segments: the call did not ask for keep_stages");
    const JobRes& jr = t->job[(size_t)job];
    copy_out(seg_len, t->seg_len, jr.slot_base, (size_t)jr.counts.n_neighbours * (size_t)jr.counts.n_keypoints);
    return IBA_OK;
}

iba_status iba_triangulate_median_depth(const float* Tcw12, const float* xyz, int32_t n, int32_t q, float* out) {
    const std::string why = trg::median_depth(Tcw12, xyz, n, q, out);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_triangulate_median_depth: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_triangulate_host(const iba_orb_frame* frames, int32_t F, const iba_triangulate_keyframe* keyframes, int32_t K, const iba_triangulate_job* jobs, int32_t J,
                                      const iba_triangulate_options* opt, iba_triangulation** out) {
    return run("iba_debug_triangulate_host", frames, F, keyframes, K, jobs, J, opt, 0, true, out);
}

int32_t iba_debug_triangulate_chunks(const iba_triangulation* t) { return t ? t->n_chunks : 0; }

iba_status iba_debug_triangulate_stage_ms(const iba_triangulation* t, float ms[4]) {
    if (!t || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_triangulate_stage_ms: a NULL argument");
    std::memcpy(ms, t->ms, sizeof(t->ms));
    return IBA_OK;
}

}  // extern "C"

// Map-point fusion (include/iba_mi355x.h, iba_fuse*): the C ABI, the result object and the launch chain of a call. The two kernels of its own are
// iba_fuse_kernels.hpp, the grid and list kernels the matcher's (iba_orb_match_kernels.hpp, included and not edited), the float decisions
// iba_fuse_math.hpp, the host rules (argument checks, the restatement, the fold and its helpers) iba_fuse_host.hpp. A per-call unit (iba_call.hpp)
// with a chain before the chunks: frames, the point table and the slots go up once as flat tables, the frustum kernel writes every slot's status
// and query, the grid of every frame is built and every slot's list counted; the chunks are sized from those counts. The chain of a chunk of
// jobs: scan, list write with the distances, pick, the results down. The result is host memory.
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
#include "iba_fuse_host.hpp"
#include "iba_fuse_kernels.hpp"

using iba::DevBuf;
using iba::PinnedBuf;
namespace fuse = iba::fuse;
namespace mapm = iba::mapm;
namespace orbm = iba::orbm;           // the matcher's host half
namespace orbk = iba::fuse::orbk;     // the matcher's kernels as this unit compiles them (iba_fuse_kernels.hpp)
using fuse::JobRec;
using fuse::JobRes;
using orbk::FrameRec;
using orbk::QueryRec;

struct iba_fusion : fuse::Result {};

namespace {
thread_local iba::CallError t_err;

constexpr int kShippedPickLanes = 8;      // profiles/fuse_bench.md

uint32_t blocks_of(size_t n) { return (uint32_t)((n + orbk::kThreads - 1) / orbk::kThreads); }

// the tables and buffers of the whole call
struct CallState {
    std::vector<FrameRec> frames;
    std::vector<JobRec> jobs;
    std::vector<int32_t> block0;              // per job its first block, and one past the last job's
    std::vector<int32_t> cnt;                 // per slot, from the count pass
    std::vector<int32_t> job_counts;
    int pick_lanes = kShippedPickLanes;
    DevBuf<FrameRec> d_frames; DevBuf<QueryRec> d_queries; DevBuf<JobRec> d_jobs; DevBuf<fuse::BlockRec> d_blocks;
    DevBuf<float2> d_xy; DevBuf<int32_t> d_octave, d_kp_frame, d_kp_cell, d_cell_cnt, d_cell_off, d_list, d_cnt, d_match, d_dist, d_job_counts; DevBuf<uint64_t> d_desc; DevBuf<uint8_t> d_status;
};

template <int W>
void launch_pick(CallState& cs, const iba_fuse_options& opt, hipStream_t st, int32_t b0, int32_t nb, int32_t q0, const int32_t* off, const int32_t* cand, const uint16_t* cdist) {
    hipLaunchKernelGGL(fuse::fuse_pick_kernel<W>, dim3((uint32_t)nb), dim3(orbk::kThreads), 0, st, cs.d_blocks.p + b0, cs.d_jobs.p, (int)q0, cs.d_queries.p, cs.d_xy.p, cs.d_octave.p, off, cand,
                       cdist, (int)opt.th_low, opt.chi2_mono, (int)opt.check_reprojection, cs.d_status.p, cs.d_match.p, cs.d_dist.p, cs.d_job_counts.p);
}

iba_status run_chunk(iba_fusion* res, CallState& cs, int32_t ja, int32_t jb, bool timing) {
    const iba_fuse_options& opt = res->opt;
    hipStream_t st = nullptr;
    const int32_t nJ = jb - ja;
    const JobRec& first = cs.jobs[(size_t)ja];
    const JobRec& last = cs.jobs[(size_t)jb - 1];
    const int32_t q0 = first.q0, nq = last.q0 + last.nq - q0;
    const int32_t b0 = cs.block0[(size_t)ja], nb = cs.block0[(size_t)jb] - b0;
    uint64_t n_cand = 0;
    for (int32_t q = q0; q < q0 + nq; ++q) n_cand += (uint64_t)cs.cnt[(size_t)q];
    if (n_cand >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "the candidate lists of one chunk hold 2^31 entries or more");
    DevBuf<int32_t> d_off, d_cand; DevBuf<uint16_t> d_cdist;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after the host arrays (the result's, cs.job_counts) and the buffers
    IBA_CALL_TRY(d_off.alloc((size_t)nq + 1)); IBA_CALL_TRY(d_cand.alloc((size_t)n_cand)); IBA_CALL_TRY(d_cdist.alloc((size_t)n_cand));
    if (timing) IBA_CALL_TRY(ev.create(3));
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(orbk::orbm_scan_kernel, dim3(1), dim3(1024), 0, st, cs.d_cnt.p + q0, d_off.p, (int)nq);
    IBA_CALL_TRY(hipGetLastError());
    if (nq) {
        hipLaunchKernelGGL(orbk::orbm_list_kernel<true>, dim3(blocks_of((size_t)nq)), dim3(orbk::kThreads), 0, st, cs.d_frames.p, cs.d_queries.p, (int)q0, (int)nq, cs.d_xy.p, cs.d_octave.p,
                           cs.d_desc.p, cs.d_cell_off.p, cs.d_list.p, (int32_t*)nullptr, d_off.p, d_cand.p, d_cdist.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    if (nb) {
        if (cs.pick_lanes == 8) launch_pick<8>(cs, opt, st, b0, nb, q0, d_off.p, d_cand.p, d_cdist.p);
        else if (cs.pick_lanes == 16) launch_pick<16>(cs, opt, st, b0, nb, q0, d_off.p, d_cand.p, d_cdist.p);
        else launch_pick<64>(cs, opt, st, b0, nb, q0, d_off.p, d_cand.p, d_cdist.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    IBA_CALL_TRY(hipMemcpyAsync(cs.job_counts.data() + (size_t)ja * fuse::kStatuses, cs.d_job_counts.p + (size_t)ja * fuse::kStatuses, sizeof(int32_t) * (size_t)nJ * fuse::kStatuses,
                                hipMemcpyDeviceToHost, st));
    if (nq) {
        IBA_CALL_TRY(hipMemcpyAsync(res->status.data() + q0, cs.d_status.p + q0, (size_t)nq, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->match.data() + q0, cs.d_match.p + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->dist.data() + q0, cs.d_dist.p + q0, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
    }
    const size_t cand_base = res->cand.size();
    if (opt.keep_stages && n_cand) {
        res->cand.resize(cand_base + (size_t)n_cand); res->cand_dist.resize(cand_base + (size_t)n_cand);
        IBA_CALL_TRY(hipMemcpyAsync(res->cand.data() + cand_base, d_cand.p, sizeof(int32_t) * (size_t)n_cand, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->cand_dist.data() + cand_base, d_cdist.p, sizeof(uint16_t) * (size_t)n_cand, hipMemcpyDeviceToHost, st));
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    if (timing) {
        float ms = 0.f;
        IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[0], ev.e[1])); res->ms[2] += ms;
        IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[1], ev.e[2])); res->ms[3] += ms;
    }
    size_t at = cand_base;
    for (int32_t j = 0; j < nJ; ++j) {
        JobRes& jr = res->job[(size_t)(ja + j)];
        const JobRec& rec = cs.jobs[(size_t)(ja + j)];
        int64_t nc = 0;
        for (int32_t k = 0; k < rec.nq; ++k) nc += cs.cnt[(size_t)rec.q0 + (size_t)k];
        jr.cand_base = at; at += (size_t)nc;
        std::memcpy(jr.counts.status, &cs.job_counts[(size_t)(ja + j) * fuse::kStatuses], sizeof(int32_t) * fuse::kStatuses);
        jr.counts.n_candidates = (int32_t)nc; jr.counts.n_picked = jr.counts.status[IBA_FUSE_PICKED];
        if (opt.keep_stages) {                 // the job's own offsets, from 0
            int32_t* off = &res->off[(size_t)rec.q0 + (size_t)(ja + j)];
            off[0] = 0;
            for (int32_t k = 0; k < rec.nq; ++k) off[k + 1] = off[k] + cs.cnt[(size_t)rec.q0 + (size_t)k];
        }
    }
    return IBA_OK;
}

iba_status run_call(iba_fusion* res, const iba_orb_frame* frames, int32_t F, const iba_map_points* pts, const iba_fuse_job* jobs, int32_t J, int device) {
    const iba_fuse_options& opt = res->opt;
    CallState cs;
    // ---- the flat tables ----
    const uint64_t P = (uint64_t)pts->n;
    uint64_t n_kp = 0, n_q = 0, n_blocks = 0;
    for (int32_t f = 0; f < F; ++f) n_kp += (uint64_t)frames[f].n;
    for (int32_t j = 0; j < J; ++j) { n_q += (uint64_t)jobs[j].n_points; n_blocks += blocks_of((size_t)jobs[j].n_points); }
    if (n_kp + P >= (1ull << 31) || n_q + (uint64_t)J >= (1ull << 31) || (uint64_t)F * orbm::kCells >= (1ull << 31) || (uint64_t)J * fuse::kStatuses >= (1ull << 31))
        return t_err.fail(IBA_ERR_UNSUPPORTED, "2^31 keypoints and points, slots or cells or more in one call");
    cs.frames.resize((size_t)F);
    std::vector<fuse::BlockRec> blocks; blocks.reserve((size_t)n_blocks);
    cs.job_counts.assign((size_t)J * fuse::kStatuses, 0);
    std::vector<QueryRec> queries((size_t)n_q);
    PinnedBuf<float> h_xy; PinnedBuf<int32_t> h_octave, h_kp_frame; PinnedBuf<uint8_t> h_desc, h_slot_skip;
    // ---- the device from here on ----
    hipStream_t st = nullptr;
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, IBA_FUSE_BUDGET_BYTES, "IBA_FUSE_BUDGET", &budget));
    if (const char* e = iba::debug_env("IBA_FUSE_PICK_LANES")) {
        const int w = std::atoi(e);
        if (w == 8 || w == 16 || w == 64) cs.pick_lanes = w;
    }
    DevBuf<int32_t> d_slot_point, d_level; DevBuf<uint8_t> d_slot_skip; DevBuf<float> d_pxyz, d_pnormal, d_pmin, d_pmax;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after cs, the host tables, the pinned staging and the buffers
    IBA_CALL_TRY(h_xy.alloc(2 * (size_t)n_kp)); IBA_CALL_TRY(h_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(h_kp_frame.alloc((size_t)n_kp)); IBA_CALL_TRY(h_desc.alloc(32 * (size_t)(n_kp + P)));
    IBA_CALL_TRY(h_slot_skip.alloc((size_t)n_q));
    size_t base = 0;
    for (int32_t f = 0; f < F; ++f) {
        const iba_orb_frame& fr = frames[f];
        cs.frames[(size_t)f] = FrameRec{(int32_t)base, fr.n, fr.min_x, fr.min_y, 64.0f / (fr.max_x - fr.min_x), 48.0f / (fr.max_y - fr.min_y)};
        const size_t n = (size_t)fr.n;
        if (!n) continue;
        std::memcpy(h_xy.p + 2 * base, fr.xy, sizeof(float) * 2 * n); std::memcpy(h_octave.p + base, fr.octave, sizeof(int32_t) * n); std::memcpy(h_desc.p + 32 * base, fr.desc, 32 * n);
        std::fill(h_kp_frame.p + base, h_kp_frame.p + base + n, f);
        base += n;
    }
    if (P) std::memcpy(h_desc.p + 32 * (size_t)n_kp, pts->desc, 32 * (size_t)P);      // the point descriptors behind the keypoints'
    cs.jobs.resize((size_t)J);
    cs.block0.resize((size_t)J + 1);
    res->size_for(n_q, J);                   // (with the copy of the lists, which is also what goes up)
    size_t slot = 0;
    for (int32_t j = 0; j < J; ++j) {
        const iba_fuse_job& b = jobs[j];
        const FrameRec& fr = cs.frames[(size_t)b.frame];
        JobRec& rec = cs.jobs[(size_t)j];
        rec = JobRec{};
        rec.cam = fuse::make_camera(frames[b.frame], b, opt);
        rec.frame = b.frame; rec.q0 = (int32_t)slot; rec.nq = b.n_points; rec.kp_base = fr.kp_base; rec.n_kp = fr.n;
        for (int32_t k = 0; k < b.n_points; ++k) {
            res->point[slot + (size_t)k] = b.points ? b.points[k] : k;
            h_slot_skip.p[slot + (size_t)k] = (b.skip && b.skip[k]) ? 1 : 0;
        }
        cs.block0[(size_t)j] = (int32_t)blocks.size();
        for (int32_t k = 0; k < b.n_points; k += orbk::kThreads) blocks.push_back(fuse::BlockRec{j, k});
        JobRes& jr = res->job[(size_t)j];
        jr.slot_base = slot; jr.n_kp = fr.n;
        jr.counts = iba_fuse_counts{};
        jr.counts.n_points = b.n_points;
        slot += (size_t)b.n_points;
    }
    cs.block0[(size_t)J] = (int32_t)blocks.size();
    const bool timing = iba::debug_env("IBA_FUSE_TIMING") != nullptr;
    const size_t n_cells = (size_t)F * orbm::kCells;
    IBA_CALL_TRY(cs.d_frames.alloc((size_t)F)); IBA_CALL_TRY(cs.d_queries.alloc((size_t)n_q)); IBA_CALL_TRY(cs.d_jobs.alloc((size_t)J)); IBA_CALL_TRY(cs.d_blocks.alloc(blocks.size()));
    IBA_CALL_TRY(cs.d_xy.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_desc.alloc(4 * (size_t)(n_kp + P)));
    IBA_CALL_TRY(cs.d_kp_frame.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_kp_cell.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_list.alloc((size_t)n_kp));
    IBA_CALL_TRY(cs.d_cell_cnt.alloc(n_cells)); IBA_CALL_TRY(cs.d_cell_off.alloc(n_cells + 1)); IBA_CALL_TRY(cs.d_cnt.alloc((size_t)n_q));
    IBA_CALL_TRY(cs.d_status.alloc((size_t)n_q)); IBA_CALL_TRY(cs.d_match.alloc((size_t)n_q)); IBA_CALL_TRY(cs.d_dist.alloc((size_t)n_q)); IBA_CALL_TRY(cs.d_job_counts.alloc(cs.job_counts.size()));
    IBA_CALL_TRY(d_slot_point.alloc((size_t)n_q)); IBA_CALL_TRY(d_slot_skip.alloc((size_t)n_q)); IBA_CALL_TRY(d_level.alloc((size_t)n_q));
    IBA_CALL_TRY(d_pxyz.alloc(3 * (size_t)P)); IBA_CALL_TRY(d_pnormal.alloc(3 * (size_t)P)); IBA_CALL_TRY(d_pmin.alloc((size_t)P)); IBA_CALL_TRY(d_pmax.alloc((size_t)P));
    IBA_CALL_TRY(hipMemcpyAsync(cs.d_frames.p, cs.frames.data(), sizeof(FrameRec) * (size_t)F, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemcpyAsync(cs.d_jobs.p, cs.jobs.data(), sizeof(JobRec) * (size_t)J, hipMemcpyHostToDevice, st));
    if (n_kp) {
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_xy.p, h_xy.p, sizeof(float) * 2 * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_octave.p, h_octave.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_kp_frame.p, h_kp_frame.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyHostToDevice, st));
    }
    if (n_kp + P) IBA_CALL_TRY(hipMemcpyAsync(cs.d_desc.p, h_desc.p, 32 * (size_t)(n_kp + P), hipMemcpyHostToDevice, st));
    if (P) {       // (straight from the caller's arrays, which outlive the call)
        IBA_CALL_TRY(hipMemcpyAsync(d_pxyz.p, pts->xyz, sizeof(float) * 3 * (size_t)P, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(d_pnormal.p, pts->normal, sizeof(float) * 3 * (size_t)P, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(d_pmin.p, pts->min_dist, sizeof(float) * (size_t)P, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(d_pmax.p, pts->max_dist, sizeof(float) * (size_t)P, hipMemcpyHostToDevice, st));
    }
    if (n_q) {
        IBA_CALL_TRY(hipMemcpyAsync(d_slot_point.p, res->point.data(), sizeof(int32_t) * (size_t)n_q, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(d_slot_skip.p, h_slot_skip.p, (size_t)n_q, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_blocks.p, blocks.data(), sizeof(fuse::BlockRec) * blocks.size(), hipMemcpyHostToDevice, st));
    }
    IBA_CALL_TRY(hipMemsetAsync(cs.d_cell_cnt.p, 0, sizeof(int32_t) * n_cells, st));
    IBA_CALL_TRY(hipMemsetAsync(cs.d_job_counts.p, 0, sizeof(int32_t) * cs.job_counts.size(), st));
    if (timing) IBA_CALL_TRY(ev.create(3));
    // ---- the frustum of every slot ----
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    if (n_q) {
        hipLaunchKernelGGL(fuse::fuse_frustum_kernel, dim3((uint32_t)blocks.size()), dim3(orbk::kThreads), 0, st, cs.d_blocks.p, cs.d_jobs.p, d_slot_point.p, d_slot_skip.p, d_pxyz.p, d_pnormal.p,
                           d_pmin.p, d_pmax.p, (int)n_kp, cs.d_status.p, d_level.p, cs.d_match.p, cs.d_dist.p, cs.d_queries.p, cs.d_job_counts.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    // ---- the grid of every frame, and the count pass over every slot of the call; the chunks are sized from it ----
    if (n_kp) {
        hipLaunchKernelGGL(orbk::orbm_cell_kernel, dim3(blocks_of((size_t)n_kp)), dim3(orbk::kThreads), 0, st, cs.d_frames.p, cs.d_kp_frame.p, cs.d_xy.p, (int)n_kp, cs.d_kp_cell.p, cs.d_cell_cnt.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(orbk::orbm_scan_kernel, dim3(1), dim3(1024), 0, st, cs.d_cell_cnt.p, cs.d_cell_off.p, (int)n_cells);
    IBA_CALL_TRY(hipGetLastError());
    if (n_kp) {
        hipLaunchKernelGGL(orbk::orbm_fill_kernel, dim3((uint32_t)F), dim3(64), 0, st, cs.d_frames.p, cs.d_kp_cell.p, cs.d_cell_off.p, cs.d_list.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    cs.cnt.assign((size_t)n_q, 0);
    if (n_q) {
        hipLaunchKernelGGL(orbk::orbm_list_kernel<false>, dim3(blocks_of((size_t)n_q)), dim3(orbk::kThreads), 0, st, cs.d_frames.p, cs.d_queries.p, 0, (int)n_q, cs.d_xy.p, cs.d_octave.p, cs.d_desc.p,
                           cs.d_cell_off.p, cs.d_list.p, cs.d_cnt.p, (const int32_t*)nullptr, (int32_t*)nullptr, (uint16_t*)nullptr);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    if (n_q) {
        IBA_CALL_TRY(hipMemcpyAsync(cs.cnt.data(), cs.d_cnt.p, sizeof(int32_t) * (size_t)n_q, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(queries.data(), cs.d_queries.p, sizeof(QueryRec) * (size_t)n_q, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->level.data(), d_level.p, sizeof(int32_t) * (size_t)n_q, hipMemcpyDeviceToHost, st));
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();                           // (every chunk below waits for its own copies)
    if (timing) {
        IBA_CALL_TRY(hipEventElapsedTime(&res->ms[0], ev.e[0], ev.e[1]));
        IBA_CALL_TRY(hipEventElapsedTime(&res->ms[1], ev.e[1], ev.e[2]));
    }
    for (size_t q = 0; q < (size_t)n_q; ++q) { res->u[q] = queries[q].u; res->v[q] = queries[q].v; res->radius[q] = queries[q].r; }
    std::vector<int64_t> per_job((size_t)J, 0);
    for (int32_t j = 0; j < J; ++j)
        for (int32_t k = 0; k < cs.jobs[(size_t)j].nq; ++k) {
            const int32_t c = cs.cnt[(size_t)cs.jobs[(size_t)j].q0 + (size_t)k];
            if (c < 0 || c > cs.jobs[(size_t)j].n_kp) return t_err.fail(IBA_ERR_STATE, "a list longer than its frame");
            per_job[(size_t)j] += c;
        }
    const std::vector<int32_t> cut = fuse::plan_chunks(per_job, budget);
    res->n_chunks = (int32_t)cut.size() - 1;
    for (int32_t c = 0; c < res->n_chunks; ++c)
        if (const iba_status s = run_chunk(res, cs, cut[(size_t)c], cut[(size_t)c + 1], timing)) return s;
    return IBA_OK;
}

iba_status check_job_index(const iba_fusion* f, int32_t job, const char* who) {
    return t_err.check_index(!f, job, f ? f->job.size() : 0, std::string(who) + ": ", "job");
}

iba_status run(const char* name, const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_fuse_job* jobs, int32_t J, const iba_fuse_options* opt, int device, bool host,
               iba_fusion** out) {
    const std::string who = std::string(name) + ": ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    std::string why = fuse::check_options(opt);
    if (why.empty()) why = orbm::check_frames(frames, F);
    if (why.empty()) why = mapm::check_points(points);
    if (why.empty()) why = fuse::check_jobs(frames, F, points->n, jobs, J);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_fusion* res = new iba_fusion();
    res->opt = *opt;
    res->job.resize((size_t)J);
    if (host) fuse::host_call(res, frames, F, points, jobs, J);
    else if (const iba_status s = run_call(res, frames, F, points, jobs, J, device)) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

template <class T>
void copy_out(T* dst, const std::vector<T>& src, size_t base, size_t n) {
    if (dst && n) std::memcpy(dst, &src[base], sizeof(T) * n);
}

}  // namespace

extern "C" {

const char* iba_fuse_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_fuse_options(iba_fuse_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_fuse_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->th_low = 50; opt->view_cos_limit = 0.5f; opt->chi2_mono = 5.99f; opt->check_reprojection = 1; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_fuse(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_fuse_job* jobs, int32_t J, const iba_fuse_options* opt, int device, iba_fusion** out) {
    return run("iba_fuse", frames, F, points, jobs, J, opt, device, false, out);
}

void iba_fusion_free(iba_fusion* f) { delete f; }

int32_t iba_fusion_n_jobs(const iba_fusion* f) { return f ? (int32_t)f->job.size() : 0; }

iba_status iba_fusion_job(const iba_fusion* f, int32_t job, iba_fuse_counts* counts) {
    if (const iba_status s = check_job_index(f, job, "iba_fusion_job")) return s;
    if (!counts) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_fusion_job: counts is NULL");
    *counts = f->job[(size_t)job].counts;
    return IBA_OK;
}

iba_status iba_fusion_read(const iba_fusion* f, int32_t job, uint8_t* status, float* u, float* v, int32_t* level, float* radius, int32_t* match, int32_t* dist) {
    if (const iba_status s = check_job_index(f, job, "iba_fusion_read")) return s;
    const JobRes& jr = f->job[(size_t)job];
    const size_t n = (size_t)jr.counts.n_points, b = jr.slot_base;
    copy_out(status, f->status, b, n); copy_out(u, f->u, b, n); copy_out(v, f->v, b, n); copy_out(level, f->level, b, n);
    copy_out(radius, f->radius, b, n); copy_out(match, f->match, b, n); copy_out(dist, f->dist, b, n);
    return IBA_OK;
}

iba_status iba_fusion_lists(const iba_fusion* f, int32_t job, int32_t* off, int32_t* index, uint16_t* dist) {
    if (const iba_status s = check_job_index(f, job, "iba_fusion_lists")) return s;
    if (!f->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_fusion_lists: the call did not ask for keep_stages");
    const JobRes& jr = f->job[(size_t)job];
    const size_t nq = (size_t)jr.counts.n_points, nc = (size_t)jr.counts.n_candidates;
    copy_out(off, f->off, jr.slot_base + (size_t)job, nq + 1);
    copy_out(index, f->cand, jr.cand_base, nc); copy_out(dist, f->cand_dist, jr.cand_base, nc);
    return IBA_OK;
}

iba_status iba_fuse_apply(const iba_fusion* f, int32_t job, int32_t keyframe, iba_fuse_map* map, int32_t mode, int32_t* op, int32_t* other, int32_t* n_fused) {
    if (n_fused) *n_fused = 0;
    if (const iba_status s = check_job_index(f, job, "iba_fuse_apply")) return s;
    const std::string why = fuse::apply(*f, job, keyframe, map, mode, op, other, n_fused);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_fuse_apply: " + why);
}

iba_status iba_fuse_skip(const iba_fuse_map* map, int32_t keyframe, const int32_t* points, int32_t n, uint8_t* skip) {
    const std::string why = fuse::skip_bytes(map, keyframe, points, n, skip);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_fuse_skip: " + why);
}

iba_status iba_fuse_candidates(const iba_fuse_map* map, const int32_t* targets, int32_t T, int32_t* points, int32_t* n) {
    const std::string why = fuse::candidates(map, targets, T, points, n);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_fuse_candidates: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_fuse_host(const iba_orb_frame* frames, int32_t F, const iba_map_points* points, const iba_fuse_job* jobs, int32_t J, const iba_fuse_options* opt, iba_fusion** out) {
    return run("iba_debug_fuse_host", frames, F, points, jobs, J, opt, 0, true, out);
}

int32_t iba_debug_fuse_chunks(const iba_fusion* f) { return f ? f->n_chunks : 0; }

iba_status iba_debug_fuse_stage_ms(const iba_fusion* f, float ms[4]) {
    if (!f || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_fuse_stage_ms: a NULL argument");
    std::memcpy(ms, f->ms, sizeof(f->ms));
    return IBA_OK;
}

}  // extern "C"

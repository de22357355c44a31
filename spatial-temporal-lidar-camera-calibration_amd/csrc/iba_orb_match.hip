// Windowed ORB matching (include/iba_mi355x.h, iba_orb_match*): the C ABI, the result object and the launch chain of a call. The kernels are
// iba_orb_match_kernels.hpp, the host rules (argument checks, the two query builders, the chunk planner) iba_orb_match_host.hpp. A per-call unit
// (iba_call.hpp) with a chain of its own before the chunks: the frames and queries go up once as flat tables, the grid of every frame is built
// (cell, scan, ordered fill) and every query's list counted; the chunks are sized from those counts. The chain of a chunk of jobs: scan, list write
// with the distances, resolve, the results down. The result is host memory; with keep_stages it also keeps the grid and the candidate lists.
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
#include "iba_orb_match_host.hpp"
#include "iba_orb_match_kernels.hpp"

using iba::DevBuf;
using iba::PinnedBuf;
namespace orbm = iba::orbm;
using orbm::FrameRec;
using orbm::JobOut;
using orbm::JobRec;
using orbm::QueryRec;

namespace {
struct JobRes {
    size_t q_base = 0;         // into match / dist; the job's offsets start at q_base + job
    size_t cand_base = 0;      // into cand / cand_dist (keep_stages)
    iba_orb_match_counts counts{};
};
}  // namespace

struct iba_orb_matches {
    iba_orb_match_options opt{};
    std::vector<JobRes> job;
    std::vector<int32_t> match, dist;
    int32_t n_chunks = 0;
    float ms[4] = {0.f, 0.f, 0.f, 0.f};       // IBA_ORB_MATCH_TIMING (debug): grid, list count, scan + list write, resolve
    // keep_stages
    std::vector<FrameRec> frame;
    std::vector<int32_t> cell_off, list;      // the call's (frame, cell) table scanned, and the lists it points into
    std::vector<int32_t> off, cand;           // per job n_queries + 1 offsets; the candidates of all jobs
    std::vector<uint16_t> cand_dist;
};

namespace {
thread_local iba::CallError t_err;

uint32_t blocks_of(size_t n) { return (uint32_t)((n + orbm::kThreads - 1) / orbm::kThreads); }

// the tables and buffers of the whole call
struct CallState {
    std::vector<FrameRec> frames;
    std::vector<QueryRec> queries;
    std::vector<JobRec> jobs;
    std::vector<int32_t> cnt;                 // per query, from the count pass
    DevBuf<FrameRec> d_frames; DevBuf<QueryRec> d_queries;
    DevBuf<float2> d_xy; DevBuf<int32_t> d_octave, d_kp_frame, d_kp_cell, d_cell_cnt, d_cell_off, d_list, d_cnt; DevBuf<float> d_angle; DevBuf<uint64_t> d_desc;
};

iba_status run_chunk(iba_orb_matches* res, CallState& cs, int32_t ja, int32_t jb, bool timing) {
    const iba_orb_match_options& opt = res->opt;
    hipStream_t st = nullptr;
    const int32_t nJ = jb - ja;
    const int32_t q0 = cs.jobs[(size_t)ja].q0, q1 = cs.jobs[(size_t)jb - 1].q0 + cs.jobs[(size_t)jb - 1].nq, nq = q1 - q0;
    uint64_t n_cand = 0, n_state = 0;
    for (int32_t q = q0; q < q1; ++q) n_cand += (uint64_t)cs.cnt[(size_t)q];
    if (n_cand >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "the candidate lists of one chunk hold 2^31 entries or more");
    std::vector<JobRec> jobs(cs.jobs.begin() + ja, cs.jobs.begin() + jb);
    std::vector<JobOut> out((size_t)nJ);
    for (JobRec& j : jobs) {
        j.state_base = -1;
        if (j.n_train > IBA_ORB_MATCH_LDS_TRAIN) { j.state_base = (int32_t)n_state; n_state += (uint64_t)j.n_train; }
    }
    if (n_state >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "the train frames of one chunk hold 2^31 keypoints or more");
    DevBuf<JobRec> d_jobs; DevBuf<int32_t> d_off, d_cand, d_holder, d_match, d_dist; DevBuf<uint16_t> d_cdist, d_held; DevBuf<int8_t> d_qbin; DevBuf<JobOut> d_out;
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after the host arrays (jobs, out, the result's) and the buffers
    IBA_CALL_TRY(d_jobs.alloc((size_t)nJ)); IBA_CALL_TRY(d_off.alloc((size_t)nq + 1)); IBA_CALL_TRY(d_cand.alloc((size_t)n_cand)); IBA_CALL_TRY(d_cdist.alloc((size_t)n_cand));
    IBA_CALL_TRY(d_held.alloc((size_t)n_state)); IBA_CALL_TRY(d_holder.alloc((size_t)n_state));
    IBA_CALL_TRY(d_match.alloc((size_t)nq)); IBA_CALL_TRY(d_dist.alloc((size_t)nq)); IBA_CALL_TRY(d_qbin.alloc((size_t)nq)); IBA_CALL_TRY(d_out.alloc((size_t)nJ));
    if (timing) IBA_CALL_TRY(ev.create(3));
    IBA_CALL_TRY(hipMemcpyAsync(d_jobs.p, jobs.data(), sizeof(JobRec) * jobs.size(), hipMemcpyHostToDevice, st));
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    hipLaunchKernelGGL(orbm::orbm_scan_kernel, dim3(1), dim3(1024), 0, st, cs.d_cnt.p + q0, d_off.p, (int)nq);
    IBA_CALL_TRY(hipGetLastError());
    if (nq) {
        hipLaunchKernelGGL(orbm::orbm_list_kernel<true>, dim3(blocks_of((size_t)nq)), dim3(orbm::kThreads), 0, st, cs.d_frames.p, cs.d_queries.p, (int)q0, (int)nq, cs.d_xy.p, cs.d_octave.p,
                           cs.d_desc.p, cs.d_cell_off.p, cs.d_list.p, (int32_t*)nullptr, d_off.p, d_cand.p, d_cdist.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    hipLaunchKernelGGL(orbm::orbm_resolve_kernel, dim3((uint32_t)nJ), dim3(64), 0, st, d_jobs.p, cs.d_queries.p, cs.d_angle.p, (int)q0, d_off.p, d_cand.p, d_cdist.p, d_held.p, d_holder.p,
                       (int)opt.th_low, (int)opt.th_high, opt.nn_ratio, (int)opt.check_orientation, d_match.p, d_dist.p, d_qbin.p, d_out.p);
    IBA_CALL_TRY(hipGetLastError());
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    IBA_CALL_TRY(hipMemcpyAsync(out.data(), d_out.p, sizeof(JobOut) * out.size(), hipMemcpyDeviceToHost, st));
    if (nq) {
        IBA_CALL_TRY(hipMemcpyAsync(res->match.data() + q0, d_match.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
        IBA_CALL_TRY(hipMemcpyAsync(res->dist.data() + q0, d_dist.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, st));
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
        const JobRec& rec = jobs[(size_t)j];
        const JobOut& o = out[(size_t)j];
        int64_t nc = 0;
        for (int32_t k = 0; k < rec.nq; ++k) nc += cs.cnt[(size_t)rec.q0 + (size_t)k];
        jr.q_base = (size_t)rec.q0; jr.cand_base = at; at += (size_t)nc;
        jr.counts.n_queries = rec.nq; jr.counts.n_matches = o.n_matches; jr.counts.n_candidates = (int32_t)nc; jr.counts.n_displaced = o.n_displaced; jr.counts.n_rot_removed = o.n_rot_removed;
        std::memcpy(jr.counts.hist, o.hist, sizeof(o.hist)); std::memcpy(jr.counts.ind, o.ind, sizeof(o.ind));
        if (opt.keep_stages) {                 // the job's own offsets, from 0
            int32_t* off = &res->off[(size_t)rec.q0 + (size_t)(ja + j)];
            off[0] = 0;
            for (int32_t k = 0; k < rec.nq; ++k) off[k + 1] = off[k] + cs.cnt[(size_t)rec.q0 + (size_t)k];
        }
    }
    return IBA_OK;
}

iba_status run_call(iba_orb_matches* res, const iba_orb_frame* frames, int32_t F, const iba_orb_match_job* jobs, int32_t J, int device) {
    const iba_orb_match_options& opt = res->opt;
    CallState cs;
    // ---- the flat tables ----
    uint64_t n_kp = 0, n_q = 0;
    for (int32_t f = 0; f < F; ++f) n_kp += (uint64_t)frames[f].n;
    for (int32_t j = 0; j < J; ++j) n_q += (uint64_t)jobs[j].n_queries;
    if (n_kp >= (1ull << 31) || n_q + (uint64_t)J >= (1ull << 31) || (uint64_t)F * orbm::kCells >= (1ull << 31)) return t_err.fail(IBA_ERR_UNSUPPORTED, "2^31 keypoints, queries or cells or more in one call");
    cs.frames.resize((size_t)F);
    PinnedBuf<float> h_xy, h_angle; PinnedBuf<int32_t> h_octave, h_kp_frame; PinnedBuf<uint8_t> h_desc;
    // ---- the device from here on ----
    hipStream_t st = nullptr;
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(device, IBA_ORB_MATCH_BUDGET_BYTES, "IBA_ORB_MATCH_BUDGET", &budget));
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after cs and the pinned staging
    IBA_CALL_TRY(h_xy.alloc(2 * (size_t)n_kp)); IBA_CALL_TRY(h_angle.alloc((size_t)n_kp)); IBA_CALL_TRY(h_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(h_kp_frame.alloc((size_t)n_kp)); IBA_CALL_TRY(h_desc.alloc(32 * (size_t)n_kp));
    size_t base = 0;
    for (int32_t f = 0; f < F; ++f) {
        const iba_orb_frame& fr = frames[f];
        cs.frames[(size_t)f] = FrameRec{(int32_t)base, fr.n, fr.min_x, fr.min_y, 64.0f / (fr.max_x - fr.min_x), 48.0f / (fr.max_y - fr.min_y)};
        const size_t n = (size_t)fr.n;
        if (!n) continue;
        std::memcpy(h_xy.p + 2 * base, fr.xy, sizeof(float) * 2 * n); std::memcpy(h_angle.p + base, fr.angle, sizeof(float) * n);
        std::memcpy(h_octave.p + base, fr.octave, sizeof(int32_t) * n); std::memcpy(h_desc.p + 32 * base, fr.desc, 32 * n);
        std::fill(h_kp_frame.p + base, h_kp_frame.p + base + n, f);
        base += n;
    }
    cs.queries.reserve((size_t)n_q); cs.jobs.resize((size_t)J);
    for (int32_t j = 0; j < J; ++j) {
        const iba_orb_match_job& b = jobs[j];
        const FrameRec& tf = cs.frames[(size_t)b.train_frame];
        cs.jobs[(size_t)j] = JobRec{(int32_t)cs.queries.size(), b.n_queries, b.rule, tf.kp_base, tf.n, -1};
        for (int32_t q = 0; q < b.n_queries; ++q)
            cs.queries.push_back(QueryRec{b.centre_xy[2 * q], b.centre_xy[2 * q + 1], b.radius[q], b.level_range[2 * q], b.level_range[2 * q + 1],
                                          cs.frames[(size_t)b.query_frame].kp_base + b.query_index[q], b.train_frame, (b.valid && !b.valid[q]) ? 0 : 1});
    }
    const bool timing = iba::debug_env("IBA_ORB_MATCH_TIMING") != nullptr;
    const size_t n_cells = (size_t)F * orbm::kCells;
    IBA_CALL_TRY(cs.d_frames.alloc((size_t)F)); IBA_CALL_TRY(cs.d_queries.alloc((size_t)n_q));
    IBA_CALL_TRY(cs.d_xy.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_octave.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_angle.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_desc.alloc(4 * (size_t)n_kp));
    IBA_CALL_TRY(cs.d_kp_frame.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_kp_cell.alloc((size_t)n_kp)); IBA_CALL_TRY(cs.d_list.alloc((size_t)n_kp));
    IBA_CALL_TRY(cs.d_cell_cnt.alloc(n_cells)); IBA_CALL_TRY(cs.d_cell_off.alloc(n_cells + 1)); IBA_CALL_TRY(cs.d_cnt.alloc((size_t)n_q));
    IBA_CALL_TRY(hipMemcpyAsync(cs.d_frames.p, cs.frames.data(), sizeof(FrameRec) * (size_t)F, hipMemcpyHostToDevice, st));
    if (n_q) IBA_CALL_TRY(hipMemcpyAsync(cs.d_queries.p, cs.queries.data(), sizeof(QueryRec) * (size_t)n_q, hipMemcpyHostToDevice, st));
    if (n_kp) {
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_xy.p, h_xy.p, sizeof(float) * 2 * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_octave.p, h_octave.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_angle.p, h_angle.p, sizeof(float) * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_desc.p, h_desc.p, 32 * (size_t)n_kp, hipMemcpyHostToDevice, st));
        IBA_CALL_TRY(hipMemcpyAsync(cs.d_kp_frame.p, h_kp_frame.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyHostToDevice, st));
    }
    IBA_CALL_TRY(hipMemsetAsync(cs.d_cell_cnt.p, 0, sizeof(int32_t) * n_cells, st));
    if (timing) IBA_CALL_TRY(ev.create(3));
    // ---- the grid of every frame ----
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[0], st));
    if (n_kp) {
        hipLaunchKernelGGL(orbm::orbm_cell_kernel, dim3(blocks_of((size_t)n_kp)), dim3(orbm::kThreads), 0, st, cs.d_frames.p, cs.d_kp_frame.p, cs.d_xy.p, (int)n_kp, cs.d_kp_cell.p, cs.d_cell_cnt.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(orbm::orbm_scan_kernel, dim3(1), dim3(1024), 0, st, cs.d_cell_cnt.p, cs.d_cell_off.p, (int)n_cells);
    IBA_CALL_TRY(hipGetLastError());
    if (n_kp) {
        hipLaunchKernelGGL(orbm::orbm_fill_kernel, dim3((uint32_t)F), dim3(64), 0, st, cs.d_frames.p, cs.d_kp_cell.p, cs.d_cell_off.p, cs.d_list.p);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[1], st));
    // ---- the count pass over every query of the call; the chunks are sized from it ----
    cs.cnt.assign((size_t)n_q, 0);
    if (n_q) {
        hipLaunchKernelGGL(orbm::orbm_list_kernel<false>, dim3(blocks_of((size_t)n_q)), dim3(orbm::kThreads), 0, st, cs.d_frames.p, cs.d_queries.p, 0, (int)n_q, cs.d_xy.p, cs.d_octave.p, cs.d_desc.p,
                           cs.d_cell_off.p, cs.d_list.p, cs.d_cnt.p, (const int32_t*)nullptr, (int32_t*)nullptr, (uint16_t*)nullptr);
        IBA_CALL_TRY(hipGetLastError());
    }
    if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[2], st));
    if (n_q) IBA_CALL_TRY(hipMemcpyAsync(cs.cnt.data(), cs.d_cnt.p, sizeof(int32_t) * (size_t)n_q, hipMemcpyDeviceToHost, st));
    if (opt.keep_stages) {
        res->frame = cs.frames;
        res->cell_off.resize(n_cells + 1); res->list.resize((size_t)n_kp);
        IBA_CALL_TRY(hipMemcpyAsync(res->cell_off.data(), cs.d_cell_off.p, sizeof(int32_t) * (n_cells + 1), hipMemcpyDeviceToHost, st));
        if (n_kp) IBA_CALL_TRY(hipMemcpyAsync(res->list.data(), cs.d_list.p, sizeof(int32_t) * (size_t)n_kp, hipMemcpyDeviceToHost, st));
        res->off.assign((size_t)n_q + (size_t)J, 0);
    }
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();                           // (every chunk below waits for its own copies)
    if (timing) {
        IBA_CALL_TRY(hipEventElapsedTime(&res->ms[0], ev.e[0], ev.e[1]));
        IBA_CALL_TRY(hipEventElapsedTime(&res->ms[1], ev.e[1], ev.e[2]));
    }
    std::vector<int64_t> per_job((size_t)J, 0);
    for (int32_t j = 0; j < J; ++j)
        for (int32_t k = 0; k < cs.jobs[(size_t)j].nq; ++k) {
            const int32_t c = cs.cnt[(size_t)cs.jobs[(size_t)j].q0 + (size_t)k];
            if (c < 0 || c > cs.jobs[(size_t)j].n_train) return t_err.fail(IBA_ERR_STATE, "a list longer than its train frame");
            per_job[(size_t)j] += c;
        }
    const std::vector<int32_t> cut = orbm::plan_chunks(per_job, budget);
    res->n_chunks = (int32_t)cut.size() - 1;
    res->match.assign((size_t)n_q, -1); res->dist.assign((size_t)n_q, -1);
    for (int32_t c = 0; c < res->n_chunks; ++c)
        if (const iba_status s = run_chunk(res, cs, cut[(size_t)c], cut[(size_t)c + 1], timing)) return s;
    return IBA_OK;
}

iba_status check_job_index(const iba_orb_matches* m, int32_t job, const char* who) {
    return t_err.check_index(!m, job, m ? m->job.size() : 0, std::string(who) + ": ", "job");
}

}  // namespace

extern "C" {

const char* iba_orb_match_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_orb_match_options(iba_orb_match_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_orb_match_options: opt is NULL");
    std::memset(opt, 0, sizeof(*opt));
    opt->struct_size = (int32_t)sizeof(*opt);
    opt->th_low = 50; opt->th_high = 100; opt->nn_ratio = 0.9f; opt->check_orientation = 1; opt->keep_stages = 0;
    return IBA_OK;
}

iba_status iba_orb_match(const iba_orb_frame* frames, int32_t F, const iba_orb_match_job* jobs, int32_t J, const iba_orb_match_options* opt, int device, iba_orb_matches** out) {
    const std::string who = "iba_orb_match: ";
    if (out) *out = nullptr;
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    std::string why = orbm::check_options(opt);
    if (why.empty()) why = orbm::check_frames(frames, F);
    if (why.empty()) why = orbm::check_jobs(frames, F, jobs, J);
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    iba_orb_matches* res = new iba_orb_matches();
    res->opt = *opt;
    res->job.resize((size_t)J);
    const iba_status s = run_call(res, frames, F, jobs, J, device);
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

void iba_orb_matches_free(iba_orb_matches* m) { delete m; }

int32_t iba_orb_matches_n_jobs(const iba_orb_matches* m) { return m ? (int32_t)m->job.size() : 0; }

iba_status iba_orb_matches_job(const iba_orb_matches* m, int32_t job, iba_orb_match_counts* counts) {
    if (const iba_status s = check_job_index(m, job, "iba_orb_matches_job")) return s;
    if (!counts) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_matches_job: counts is NULL");
    *counts = m->job[(size_t)job].counts;
    return IBA_OK;
}

iba_status iba_orb_matches_read(const iba_orb_matches* m, int32_t job, int32_t* match, int32_t* dist) {
    if (const iba_status s = check_job_index(m, job, "iba_orb_matches_read")) return s;
    const JobRes& jr = m->job[(size_t)job];
    const size_t n = (size_t)jr.counts.n_queries;
    if (!n) return IBA_OK;
    if (match) std::memcpy(match, &m->match[jr.q_base], sizeof(int32_t) * n);
    if (dist) std::memcpy(dist, &m->dist[jr.q_base], sizeof(int32_t) * n);
    return IBA_OK;
}

iba_status iba_orb_matches_grid(const iba_orb_matches* m, int32_t frame, int32_t* cell_off, int32_t* list, int32_t* n_listed) {
    const std::string who = "iba_orb_matches_grid: ";
    if (!m) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the result is NULL");
    if (!m->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, who + "the call did not ask for keep_stages");
    if (frame < 0 || (size_t)frame >= m->frame.size()) return t_err.fail(IBA_ERR_INVALID_ARG, who + "frame " + std::to_string(frame) + " is outside the result's " + std::to_string(m->frame.size()) + " frames");
    const int32_t* off = &m->cell_off[(size_t)frame * orbm::kCells];
    const int32_t n = off[orbm::kCells] - off[0];
    if (cell_off) for (int c = 0; c <= orbm::kCells; ++c) cell_off[c] = off[c] - off[0];
    if (list && n) std::memcpy(list, &m->list[(size_t)off[0]], sizeof(int32_t) * (size_t)n);
    if (n_listed) *n_listed = n;
    return IBA_OK;
}

iba_status iba_orb_matches_lists(const iba_orb_matches* m, int32_t job, int32_t* off, int32_t* index, uint16_t* dist) {
    if (const iba_status s = check_job_index(m, job, "iba_orb_matches_lists")) return s;
    if (!m->opt.keep_stages) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_matches_lists: the call did not ask for keep_stages");
    const JobRes& jr = m->job[(size_t)job];
    const size_t nq = (size_t)jr.counts.n_queries, nc = (size_t)jr.counts.n_candidates;
    if (off) std::memcpy(off, &m->off[jr.q_base + (size_t)job], sizeof(int32_t) * (nq + 1));
    if (index && nc) std::memcpy(index, &m->cand[jr.cand_base], sizeof(int32_t) * nc);
    if (dist && nc) std::memcpy(dist, &m->cand_dist[jr.cand_base], sizeof(uint16_t) * nc);
    return IBA_OK;
}

iba_status iba_orb_match_init_queries(const iba_orb_frame* frame1, const float* prev_matched_xy, int32_t window_size, float* centre_xy, float* radius, int32_t* level_range, int32_t* query_index,
                                      uint8_t* valid) {
    const std::string why = orbm::init_queries(frame1, prev_matched_xy, window_size, centre_xy, radius, level_range, query_index, valid);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_match_init_queries: " + why);
}

iba_status iba_orb_match_motion_queries(const iba_orb_frame* last_frame, const uint8_t* has_point, const uint8_t* outlier, const float* world_xyz, const float Tcw12[12], float fx, float fy, float cx,
                                        float cy, const float bounds[4], const float* scale_factors, int32_t n_scale_factors, float th, float* centre_xy, float* radius, int32_t* level_range,
                                        int32_t* query_index, uint8_t* valid) {
    const std::string why = orbm::motion_queries(last_frame, has_point, outlier, world_xyz, Tcw12, fx, fy, cx, cy, bounds, scale_factors, n_scale_factors, th, centre_xy, radius, level_range, query_index, valid);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_orb_match_motion_queries: " + why);
}

// ---- debug (include/iba_mi355x_debug.h) ----

iba_status iba_debug_orb_match_stub(int32_t n_jobs, int32_t n_frames, int32_t keep_stages, iba_orb_matches** out) {
    if (!out || n_jobs < 0 || n_frames < 0) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_match_stub: out is NULL, n_jobs < 0 or n_frames < 0");
    iba_orb_matches* res = new iba_orb_matches();
    (void)iba_default_orb_match_options(&res->opt);
    res->opt.keep_stages = keep_stages ? 1 : 0;
    res->job.resize((size_t)n_jobs);
    res->off.assign((size_t)n_jobs, 0);
    res->frame.assign((size_t)n_frames, FrameRec{0, 0, 0.f, 0.f, 0.f, 0.f});
    res->cell_off.assign((size_t)n_frames * orbm::kCells + 1, 0);
    *out = res;
    return IBA_OK;
}

int32_t iba_debug_orb_match_chunks(const iba_orb_matches* m) { return m ? m->n_chunks : 0; }

iba_status iba_debug_orb_match_stage_ms(const iba_orb_matches* m, float ms[4]) {
    if (!m || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_match_stage_ms: a NULL argument");
    std::memcpy(ms, m->ms, sizeof(m->ms));
    return IBA_OK;
}

iba_status iba_debug_orb_match_plan(const int64_t* candidates, int32_t n_jobs, uint64_t budget, int32_t* cut, int32_t* n_cut) {
    if (!candidates || !cut || !n_cut || n_jobs < 1) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_match_plan: a NULL argument or n_jobs < 1");
    for (int32_t j = 0; j < n_jobs; ++j)
        if (candidates[j] < 0) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_orb_match_plan: a negative count");
    const std::vector<int32_t> c = orbm::plan_chunks(std::vector<int64_t>(candidates, candidates + n_jobs), budget);
    for (size_t k = 0; k < c.size(); ++k) cut[k] = c[k];
    *n_cut = (int32_t)c.size();
    return IBA_OK;
}

}  // extern "C"

// Scan-to-image projection (include/iba_mi355x.h, iba_project_* / iba_projection_*): the C ABI, the result object and the launch chain of a call.
// The kernels and their launches are iba_project_kernels.hpp (compiled beside the evaluation kernels, whose quotient helper they share); the
// validation, the palette and the bytes of a job are iba_project_host.hpp. A per-call unit (iba_call.hpp) on the handle's stream, ONE chain for all
// chunks: poses on the host (P1), the job table up, then per chunk of jobs a fill of the key image and the splat, resolve and visible kernels; the
// counters come down. The result owns its device buffers (DevBuf) and reads nothing of the handle afterwards: its accessors copy on the null stream.
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
#include "iba_host_math.hpp"
#include "iba_project_host.hpp"

using iba::DevBuf;
using iba::project::ProjJob;
using iba::project::ProjRec;
namespace prj = iba::project;

struct iba_projection {
    int device = -1;                         // -1: a result without device buffers (iba_debug_project_stub)
    iba_project_options opt{};
    std::vector<ProjJob> jobs;
    std::vector<uint32_t> counts;            // kCounters per job, as the device left them
    int32_t n_chunks = 0;
    float ms[5] = {0.f, 0.f, 0.f, 0.f, 0.f};   // IBA_PROJECT_TIMING (debug): splat, resolve, visible summed over the chunks; the last colourise; the last overlay
    DevBuf<ProjJob> d_jobs;
    DevBuf<float> d_depth; DevBuf<uint32_t> d_index;   // the images of all jobs, job after job
    DevBuf<ProjRec> d_rec;                   // the records of all jobs, job after job, original point order inside a job
    DevBuf<uint32_t> d_cnt;
};

namespace {
thread_local iba::CallError t_err;

// one launch on the null stream between two events (debug): its time into *ms
template <class F>
hipError_t timed(bool timing, float* ms, F launch) {
    if (!timing) return launch();
    iba::EventSet ev;
    hipError_t err = ev.create(2);
    if (err == hipSuccess) err = hipEventRecord(ev.e[0], nullptr);
    if (err == hipSuccess) err = launch();
    if (err == hipSuccess) err = hipEventRecord(ev.e[1], nullptr);
    if (err == hipSuccess) err = hipEventSynchronize(ev.e[1]);
    if (err == hipSuccess) err = hipEventElapsedTime(ms, ev.e[0], ev.e[1]);
    return err;
}

uint64_t job_pixels(const ProjJob& j) { return (uint64_t)j.Wi * (uint64_t)j.Hi; }

// the job index of an accessor: "" or the refusal
iba_status check_job(const iba_projection* p, int32_t job, const char* who) {
    return t_err.check_index(!p, job, p ? p->jobs.size() : 0, std::string(who) + ": ", "job");
}

// the launch chain of a call on a result whose job table is complete; on failure the caller deletes the result
iba_status run_chain(const iba::ProjectView& v, iba_projection* res) {
    const std::vector<ProjJob>& jobs = res->jobs;
    const int32_t J = (int32_t)jobs.size();
    const ProjJob& last = jobs[(size_t)J - 1];
    const uint64_t n_rec = last.rec_base + last.P, n_pix = last.img_base + job_pixels(last);
    uint64_t budget = 0;
    IBA_CALL_TRY(iba::call_budget(v.device, IBA_PROJECT_BUDGET_BYTES, "IBA_PROJECT_BUDGET", &budget));
    std::vector<uint64_t> pixels((size_t)J);
    for (int32_t j = 0; j < J; ++j) pixels[(size_t)j] = job_pixels(jobs[(size_t)j]);
    const std::vector<int32_t> cut = prj::cut_chunks(pixels, budget);
    res->n_chunks = (int32_t)cut.size() - 1;
    uint64_t key_cap = 0;
    for (int32_t c = 0; c < res->n_chunks; ++c) {
        uint64_t at = 0;
        for (int32_t j = cut[(size_t)c]; j < cut[(size_t)c + 1]; ++j) { res->jobs[(size_t)j].key_base = at; at += pixels[(size_t)j]; }
        key_cap = std::max(key_cap, at);
    }
    hipStream_t st = v.stream;
    DevBuf<unsigned long long> d_keys;       // the z-buffer of one chunk: lives for this call only
    iba::EventSet ev;
    iba::SyncOnExit sync(st);                // after d_keys; the host arrays of the chain are the result's (jobs, counts), which outlive this function
    IBA_CALL_TRY(d_keys.alloc((size_t)key_cap));
    IBA_CALL_TRY(res->d_jobs.alloc((size_t)J));
    IBA_CALL_TRY(res->d_depth.alloc((size_t)n_pix));
    IBA_CALL_TRY(res->d_index.alloc((size_t)n_pix));
    IBA_CALL_TRY(res->d_rec.alloc((size_t)n_rec));
    IBA_CALL_TRY(res->d_cnt.alloc((size_t)J * prj::kCounters));
    const bool timing = iba::debug_env("IBA_PROJECT_TIMING") != nullptr;   // (debug: four events per chunk, read after the synchronise)
    if (timing) IBA_CALL_TRY(ev.create(4 * (size_t)res->n_chunks));
    IBA_CALL_TRY(hipMemcpyAsync(res->d_jobs.p, jobs.data(), sizeof(ProjJob) * (size_t)J, hipMemcpyHostToDevice, st));
    IBA_CALL_TRY(hipMemsetAsync(res->d_cnt.p, 0, sizeof(uint32_t) * (size_t)J * prj::kCounters, st));
    for (int32_t c = 0; c < res->n_chunks; ++c) {
        const int32_t a = cut[(size_t)c], b = cut[(size_t)c + 1], nj = b - a;
        const ProjJob& ja = jobs[(size_t)a]; const ProjJob& jz = jobs[(size_t)b - 1];
        const uint64_t chunk_pix = jz.key_base + job_pixels(jz);
        const uint32_t pt_blocks = jz.first_block + (jz.P + (uint32_t)prj::kSlice - 1u) / (uint32_t)prj::kSlice - ja.first_block;
        const uint32_t px_blocks = jz.first_pblock + (uint32_t)((job_pixels(jz) + (uint64_t)prj::kThreads - 1u) / (uint64_t)prj::kThreads) - ja.first_pblock;
        uint32_t* cnt = res->d_cnt.p + (size_t)a * prj::kCounters;
        IBA_CALL_TRY(hipMemsetAsync(d_keys.p, 0xFF, sizeof(unsigned long long) * (size_t)chunk_pix, st));
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4 * (size_t)c], st));
        IBA_CALL_TRY(iba::project_splat(st, v.pts4, res->d_jobs.p + a, nj, ja.first_block, pt_blocks, res->opt.splat, res->opt.z_min, res->opt.z_max, d_keys.p, res->d_rec.p, cnt));
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4 * (size_t)c + 1], st));
        IBA_CALL_TRY(iba::project_resolve(st, res->d_jobs.p + a, nj, ja.first_pblock, px_blocks, d_keys.p, res->d_depth.p, res->d_index.p, cnt));
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4 * (size_t)c + 2], st));
        IBA_CALL_TRY(iba::project_visible(st, res->d_jobs.p + a, nj, ja.first_block, pt_blocks, res->opt.occlusion_tol, res->d_rec.p, res->d_depth.p, cnt, nullptr, nullptr));
        if (timing) IBA_CALL_TRY(hipEventRecord(ev.e[4 * (size_t)c + 3], st));
    }
    res->counts.assign((size_t)J * prj::kCounters, 0u);
    IBA_CALL_TRY(hipMemcpyAsync(res->counts.data(), res->d_cnt.p, sizeof(uint32_t) * (size_t)J * prj::kCounters, hipMemcpyDeviceToHost, st));
    IBA_CALL_TRY(hipStreamSynchronize(st));
    sync.disarm();
    for (size_t c = 0; timing && c < (size_t)res->n_chunks; ++c)
        for (int k = 0; k < 3; ++k) { float ms = 0.f; IBA_CALL_TRY(hipEventElapsedTime(&ms, ev.e[4 * c + k], ev.e[4 * c + k + 1])); res->ms[k] += ms; }
    return IBA_OK;
}

#define PRJ_ACCESS(p, job, who)                                         \
    do {                                                                \
        if (const iba_status _s = check_job(p, job, who)) return _s;    \
    } while (0)

}  // namespace

extern "C" {

const char* iba_project_last_error(void) { return t_err.msg.c_str(); }

iba_status iba_default_project_options(iba_project_options* opt) {
    if (!opt) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_default_project_options: opt is NULL");
    prj::default_options(*opt);
    return IBA_OK;
}

iba_status iba_project_gradient(double zn, uint8_t rgb[3]) {
    if (!rgb) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_project_gradient: rgb is NULL");
    prj::gradient(zn, rgb);
    return IBA_OK;
}

iba_status iba_project_run(iba_handle* h, const double* x7, const int32_t* frames, int32_t J, const iba_project_options* opt, iba_projection** out) {
    const std::string who = "iba_project_run: ";
    if (out) *out = nullptr;
    if (!h) return t_err.fail(IBA_ERR_INVALID_ARG, who + "h is NULL");
    if (!out) return t_err.fail(IBA_ERR_INVALID_ARG, who + "out is NULL");
    const iba::ProjectView v = iba::project_view(h);
    std::vector<double> intr;
    if (!v.scans_only) {
        intr.resize(6 * (size_t)std::max(v.n_frames, 0));
        for (int f = 0; f < v.n_frames; ++f) {
            const iba::FrameHdr& x = v.frames[f];
            const double c[6] = {x.fx, x.fy, x.cx, x.cy, x.W, x.H};
            std::memcpy(&intr[6 * (size_t)f], c, sizeof(c));
        }
    }
    const std::string why = prj::validate(opt, x7, frames, J, v.n_frames, v.scans_only ? nullptr : intr.data());
    if (!why.empty()) return t_err.fail(IBA_ERR_INVALID_ARG, who + why);
    // the job table: P1 on the host, the camera, the places of the job's records, pixels and blocks
    iba_projection* res = new iba_projection();
    res->device = v.device; res->opt = *opt;
    res->jobs.resize((size_t)J);
    const bool own_camera = !prj::camera_all_zero(opt->camera);
    uint64_t rec = 0, pix = 0, blocks = 0, pblocks = 0;
    for (int32_t j = 0; j < J; ++j) {
        ProjJob& jb = res->jobs[(size_t)j];
        std::memset(&jb, 0, sizeof(jb));
        const iba::FrameHdr& x = v.frames[frames[j]];
        double R[9], t[3];
        iba::se3_exp<double>(x7 + 7 * (size_t)j, R, t);
        for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) jb.Rt[4 * r + c] = R[3 * r + c]; jb.Rt[4 * r + 3] = t[r]; }
        const double* cam = own_camera ? opt->camera : &intr[6 * (size_t)frames[j]];
        jb.fx = cam[0]; jb.fv = opt->v_focal_is_fx ? cam[0] : cam[1]; jb.cx = cam[2]; jb.cy = cam[3]; jb.W = cam[4]; jb.H = cam[5];
        jb.Wi = (uint32_t)cam[4]; jb.Hi = (uint32_t)cam[5];
        jb.pt_base = x.pt_base; jb.P = x.P;
        jb.rec_base = rec; jb.img_base = pix; jb.first_block = (uint32_t)blocks; jb.first_pblock = (uint32_t)pblocks;
        rec += jb.P; pix += job_pixels(jb);
        blocks += (jb.P + (uint64_t)prj::kSlice - 1u) / (uint64_t)prj::kSlice;
        pblocks += (job_pixels(jb) + (uint64_t)prj::kThreads - 1u) / (uint64_t)prj::kThreads;
        if (blocks >= (1ull << 31) || pblocks >= (1ull << 31)) { delete res; return t_err.fail(IBA_ERR_UNSUPPORTED, who + "the jobs of one call need 2^31 blocks or more (split the call)"); }
    }
    const iba_status s = run_chain(v, res);
    if (s != IBA_OK) { t_err.msg = who + t_err.msg; delete res; return s; }
    *out = res;
    return IBA_OK;
}

void iba_projection_free(iba_projection* p) {
    if (!p) return;
    if (p->device >= 0) (void)hipSetDevice(p->device);
    delete p;
}

int32_t iba_projection_n_jobs(const iba_projection* p) { return p ? (int32_t)p->jobs.size() : 0; }

iba_status iba_projection_size(const iba_projection* p, int32_t job, int32_t* W, int32_t* H) {
    PRJ_ACCESS(p, job, "iba_projection_size");
    if (!W || !H) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_size: W or H is NULL");
    *W = (int32_t)p->jobs[(size_t)job].Wi; *H = (int32_t)p->jobs[(size_t)job].Hi;
    return IBA_OK;
}

iba_status iba_projection_pose(const iba_projection* p, int32_t job, double Rt12[12]) {
    PRJ_ACCESS(p, job, "iba_projection_pose");
    if (!Rt12) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_pose: Rt12 is NULL");
    std::memcpy(Rt12, p->jobs[(size_t)job].Rt, 12 * sizeof(double));
    return IBA_OK;
}

iba_status iba_projection_counts(const iba_projection* p, int32_t job, iba_project_counts* counts) {
    PRJ_ACCESS(p, job, "iba_projection_counts");
    if (!counts) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_counts: counts is NULL");
    const uint32_t zero[prj::kCounters] = {0};
    const uint32_t* c = p->counts.empty() ? zero : &p->counts[(size_t)job * prj::kCounters];
    counts->n_points = (int64_t)p->jobs[(size_t)job].P;
    counts->n_skipped = c[prj::C_SKIPPED]; counts->n_in_front = c[prj::C_IN_FRONT]; counts->n_inside = c[prj::C_INSIDE];
    counts->n_visible = c[prj::C_VISIBLE]; counts->n_pixels = c[prj::C_PIXELS];
    return IBA_OK;
}

iba_status iba_projection_depth(iba_projection* p, int32_t job, float* depth_HxW) {
    PRJ_ACCESS(p, job, "iba_projection_depth");
    if (!depth_HxW) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_depth: the output is NULL");
    const ProjJob& jb = p->jobs[(size_t)job];
    if (p->device < 0 || !job_pixels(jb)) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(p->device));
    IBA_CALL_TRY(hipMemcpy(depth_HxW, p->d_depth.p + jb.img_base, sizeof(float) * (size_t)job_pixels(jb), hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_projection_index(iba_projection* p, int32_t job, uint32_t* index_HxW) {
    PRJ_ACCESS(p, job, "iba_projection_index");
    if (!index_HxW) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_index: the output is NULL");
    const ProjJob& jb = p->jobs[(size_t)job];
    if (p->device < 0 || !job_pixels(jb)) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(p->device));
    IBA_CALL_TRY(hipMemcpy(index_HxW, p->d_index.p + jb.img_base, sizeof(uint32_t) * (size_t)job_pixels(jb), hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_projection_points(iba_projection* p, int32_t job, double* uv_nx2, float* z_n, uint8_t* flags_n) {
    PRJ_ACCESS(p, job, "iba_projection_points");
    const ProjJob& jb = p->jobs[(size_t)job];
    if (p->device < 0 || !jb.P) return IBA_OK;
    std::vector<ProjRec> rec((size_t)jb.P);
    IBA_CALL_TRY(hipSetDevice(p->device));
    IBA_CALL_TRY(hipMemcpy(rec.data(), p->d_rec.p + jb.rec_base, sizeof(ProjRec) * (size_t)jb.P, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < rec.size(); ++i) {
        if (uv_nx2) { uv_nx2[2 * i] = rec[i].u; uv_nx2[2 * i + 1] = rec[i].v; }
        if (z_n) z_n[i] = rec[i].z;
        if (flags_n) flags_n[i] = (uint8_t)rec[i].flags;
    }
    return IBA_OK;
}

iba_status iba_projection_colorize(iba_projection* p, int32_t job, const uint8_t* rgb_HxWx3, uint8_t* point_rgb_nx3) {
    PRJ_ACCESS(p, job, "iba_projection_colorize");
    if (!rgb_HxWx3 || !point_rgb_nx3) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_colorize: the image or the output is NULL");
    const ProjJob& jb = p->jobs[(size_t)job];
    if (p->device < 0 || !jb.P) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(p->device));
    DevBuf<uint8_t> d_img, d_out;
    IBA_CALL_TRY(d_img.upload(rgb_HxWx3, 3 * (size_t)job_pixels(jb)));
    IBA_CALL_TRY(d_out.alloc(3 * (size_t)jb.P));
    const uint32_t n_blocks = (jb.P + (uint32_t)prj::kSlice - 1u) / (uint32_t)prj::kSlice;
    IBA_CALL_TRY(timed(iba::debug_env("IBA_PROJECT_TIMING") != nullptr, &p->ms[3], [&] {
        return iba::project_visible(nullptr, p->d_jobs.p + job, 1, jb.first_block, n_blocks, p->opt.occlusion_tol, p->d_rec.p, p->d_depth.p, nullptr, d_img.p, d_out.p);
    }));
    IBA_CALL_TRY(hipMemcpy(point_rgb_nx3, d_out.p, 3 * (size_t)jb.P, hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_projection_overlay(iba_projection* p, int32_t job, const uint8_t* rgb_HxWx3, uint8_t* out_HxWx3) {
    PRJ_ACCESS(p, job, "iba_projection_overlay");
    if (!out_HxWx3) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_projection_overlay: the output is NULL");
    const ProjJob& jb = p->jobs[(size_t)job];
    const size_t bytes = 3 * (size_t)job_pixels(jb);
    if (p->device < 0 || !bytes) return IBA_OK;
    IBA_CALL_TRY(hipSetDevice(p->device));
    DevBuf<uint8_t> d_img, d_out;
    if (rgb_HxWx3) IBA_CALL_TRY(d_img.upload(rgb_HxWx3, bytes));
    IBA_CALL_TRY(d_out.alloc(bytes));
    const uint32_t n_blocks = (uint32_t)((job_pixels(jb) + (uint64_t)prj::kThreads - 1u) / (uint64_t)prj::kThreads);
    IBA_CALL_TRY(timed(iba::debug_env("IBA_PROJECT_TIMING") != nullptr, &p->ms[4], [&] {
        return iba::project_overlay(nullptr, p->d_jobs.p + job, n_blocks, p->d_depth.p, p->d_index.p, rgb_HxWx3 ? d_img.p : nullptr, d_out.p, p->opt.z_near, p->opt.z_far);
    }));
    IBA_CALL_TRY(hipMemcpy(out_HxWx3, d_out.p, bytes, hipMemcpyDeviceToHost));
    return IBA_OK;
}

// ---- debug (include/iba_mi355x_debug.h): host only ----

iba_status iba_debug_project_validate(int32_t n_frames, const double* intrinsics6, const double* x7, const int32_t* frames, int32_t J, const iba_project_options* opt) {
    const std::string why = prj::validate(opt, x7, frames, J, n_frames, intrinsics6);
    return why.empty() ? IBA_OK : t_err.fail(IBA_ERR_INVALID_ARG, "iba_project_run: " + why);
}

iba_status iba_debug_project_stub(int32_t n_jobs, iba_projection** out) {
    if (!out || n_jobs < 0) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_project_stub: out is NULL or n_jobs < 0");
    iba_projection* res = new iba_projection();
    prj::default_options(res->opt);
    res->jobs.resize((size_t)n_jobs);
    if (n_jobs) std::memset(res->jobs.data(), 0, sizeof(ProjJob) * (size_t)n_jobs);
    *out = res;
    return IBA_OK;
}

int32_t iba_debug_projection_chunks(const iba_projection* p) { return p ? p->n_chunks : 0; }

iba_status iba_debug_projection_kernel_ms(const iba_projection* p, float ms[5]) {
    if (!p || !ms) return t_err.fail(IBA_ERR_INVALID_ARG, "iba_debug_projection_kernel_ms: a NULL argument");
    std::memcpy(ms, p->ms, sizeof(p->ms));
    return IBA_OK;
}

}  // extern "C"

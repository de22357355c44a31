// Robust smoothing of a growing pose graph on the device (include/iba_mi355x.h, iba_smooth_*): the converged optimum the reference's iSAM2 stage
// approaches. Kernels: iba_smooth_kernels.hpp; the solve: iba_pgo_solve.hpp (iba_pgo's own); checks and plan: iba_smooth_host.hpp.
// The graph is kept on the host as it is appended; sync() brings the device up to it before anything runs. The LM loop (iba_graph_lm.hpp) and the
// scaffolding around the chains (iba_pgo_solve.hpp) are the ones iba_pgo uses; the loop reads kScal doubles per trial.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_device_buf.hpp"
#include "iba_pgo_solve.hpp"
#include "iba_smooth_host.hpp"
#include "iba_smooth_kernels.hpp"

namespace {

using namespace iba::smooth;
using iba::DevBuf;
using iba::pgo::kScal;
using iba::pgo::final_launch;

thread_local std::string t_err;

}  // namespace

struct iba_smooth {
    int device = 0;
    bool device_ready = false;
    bool dead = false;                     // a device failure while the graph was brought up lost the estimates: every later call answers IBA_ERR_STATE
    iba_smooth_options opt{};
    // the graph as appended (host)
    int32_t N = 0;
    std::vector<double> new_nodes;         // 16 per node not yet on the device (nodes N_dev .. N - 1)
    std::vector<int32_t> fi, fj;
    std::vector<double> zinv, ivar;        // 12 and 6 per factor
    std::vector<uint8_t> robust;
    // the device's view
    int32_t N_dev = 0, F_dev = 0;
    size_t cap_nodes = 0;
    iba::pgo::Plan plan;
    iba::pgo::Arrow ar;
    int cur = 0;                           // poses[cur] are the estimates, poses[1 - cur] the trial
    bool linearized = false;
    int nbF = 0, nbN = 0;
    DevBuf<double> poses[2], d_zinv, d_ivar, weight, r, A, g, fpart, D, b, npart, delta, upart, scal;
    DevBuf<int32_t> d_fi, d_fj;
    DevBuf<uint8_t> d_robust;
    std::vector<uint8_t> trace;
    std::string err;
    hipStream_t stream = nullptr;
};

namespace {

iba_status fail(iba_smooth* s, iba_status st, const std::string& m) { if (s) s->err = m; else t_err = m; return st; }
bool is_dead(iba_smooth* s, const char* who, iba_status* st) {
    if (!s || !s->dead) return false;
    *st = fail(s, IBA_ERR_STATE, std::string(who) + ": an earlier device failure lost the estimates; destroy the object");
    return true;
}

FactorDev factor_dev(const iba_smooth* s) { return FactorDev{s->F_dev, s->d_fi.p, s->d_fj.p, s->d_zinv.p, s->d_ivar.p, s->d_robust.p}; }

// the device brought up to the appended graph: new nodes behind the estimates, the factor arrays, the plan
iba_status sync(iba_smooth* s, const char* who) {
    const std::string name = who;
    if (s->N < 1) return fail(s, IBA_ERR_STATE, name + ": the graph has no node");
    if (!s->device_ready) {
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= s->device || s->device < 0 || hipSetDevice(s->device) != hipSuccess)
            return fail(s, IBA_ERR_NO_DEVICE, name + ": no usable gfx950 device " + std::to_string(s->device) + " (there is no CPU fallback)");
        hipError_t e = hipStreamCreate(&s->stream);
        if (e == hipSuccess) e = s->scal.alloc(kScal);
        if (e != hipSuccess) return fail(s, IBA_ERR_HIP, name + ": " + hipGetErrorString(e));
        s->device_ready = true;
    } else if (hipSetDevice(s->device) != hipSuccess) return fail(s, IBA_ERR_HIP, name + ": hipSetDevice");
    const int32_t F = (int32_t)s->fi.size();
    if (s->N == s->N_dev && F == s->F_dev) return IBA_OK;
    // the plan first: it can refuse the graph (separator cap), and then nothing on the device has changed
    iba::pgo::Plan p;
    std::string why;
    if (!make_plan(s->N, s->fi, s->fj, s->opt.segment, IBA_PGO_MAX_SEPARATORS, p, why)) return fail(s, IBA_ERR_INVALID_ARG, name + ": " + why);
    hipError_t e = hipSuccess;
    auto up = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    const size_t n = (size_t)s->N, m = (size_t)F;
    if (s->N > s->N_dev) {
        if (n > s->cap_nodes) {
            const size_t cap = n + n / 4 + 16;
            DevBuf<double> grown;
            up(grown.alloc(16 * cap));
            if (e == hipSuccess && s->N_dev) up(hipMemcpy(grown.p, s->poses[s->cur].p, 16 * (size_t)s->N_dev * sizeof(double), hipMemcpyDeviceToDevice));
            if (e == hipSuccess) { s->poses[0] = std::move(grown); s->cur = 0; }
            up(s->poses[1].alloc(16 * cap));
            up(s->D.alloc(36 * cap)); up(s->b.alloc(6 * cap)); up(s->npart.alloc(3 * cap)); up(s->delta.alloc(6 * cap)); up(s->upart.alloc(2 * ((cap + kThreads - 1) / kThreads)));
            if (e == hipSuccess) s->cap_nodes = cap;
        }
        if (e == hipSuccess) up(hipMemcpy(s->poses[s->cur].p + 16 * (size_t)s->N_dev, s->new_nodes.data(), 16 * (n - (size_t)s->N_dev) * sizeof(double), hipMemcpyHostToDevice));
    }
    if (F != s->F_dev || !s->d_fi.p) {
        up(s->d_fi.upload(s->fi)); up(s->d_fj.upload(s->fj)); up(s->d_zinv.upload(s->zinv)); up(s->d_ivar.upload(s->ivar)); up(s->d_robust.upload(s->robust));
        std::vector<double> w(m, 1.0);
        if (e == hipSuccess && s->F_dev && s->weight.p) up(hipMemcpy(w.data(), s->weight.p, (size_t)s->F_dev * sizeof(double), hipMemcpyDeviceToHost));
        up(s->weight.upload(w));
        up(s->r.alloc(6 * m)); up(s->A.alloc(36 * m)); up(s->g.alloc(6 * m)); up(s->fpart.alloc((m + kThreads - 1) / kThreads));
    }
    up(s->ar.upload(p, s->N));
    if (e != hipSuccess) { s->dead = true; s->linearized = false; return fail(s, IBA_ERR_HIP, name + ": " + hipGetErrorString(e) + " (the estimates on the device are lost: the object can only be destroyed)"); }
    s->plan = std::move(p);
    s->N_dev = s->N; s->F_dev = F;
    s->new_nodes.clear();
    s->nbF = (F + kThreads - 1) / kThreads; s->nbN = (s->N + kThreads - 1) / kThreads;
    s->linearized = false;
    return IBA_OK;
}

// linearise at poses[cur]; scal[0..3] on the host afterwards: F, |x|^2, max |b|, max diagonal of the between part
iba_status linearize(iba_smooth* s, double* scal_host, const std::string& name) {
    hipStream_t st = s->stream;
    if (s->F_dev > 0)
        hipLaunchKernelGGL(smooth_factor_kernel<true>, dim3(s->nbF), dim3(kThreads), 0, st, factor_dev(s), (const double*)s->poses[s->cur].p, s->r.p, s->weight.p, s->A.p, s->g.p, s->fpart.p);
    final_launch(st, (const double*)s->fpart.p, s->nbF, 1, 0, s->scal.p);
    hipLaunchKernelGGL(smooth_node_kernel, dim3(s->N_dev), dim3(64), 0, st, (int)s->N_dev, (const int32_t*)s->ar.inc_off.p, (const int32_t*)s->ar.inc_edge.p, (const int32_t*)s->d_fi.p,
                       (const double*)s->A.p, (const double*)s->g.p, (const double*)s->poses[s->cur].p, s->D.p, s->b.p, s->npart.p);
    final_launch(st, (const double*)s->npart.p, (int)s->N_dev, 1, 2, s->scal.p + 1);
    const iba_status rs = iba::pgo::read_scalars(s, 4, scal_host, name, "linearise");
    if (rs == IBA_OK) s->linearized = true;
    return rs;
}

// trial poses into poses[1 - cur] from delta, F there; scal[0..7] on the host afterwards
iba_status trial(iba_smooth* s, double lambda, double* scal_host, const std::string& name) {
    hipStream_t st = s->stream;
    hipLaunchKernelGGL(smooth_update_kernel, dim3(s->nbN), dim3(kThreads), 0, st, (int)s->N_dev, (const double*)s->poses[s->cur].p, (const double*)s->delta.p, (const double*)s->b.p, lambda,
                       s->poses[1 - s->cur].p, s->upart.p);
    final_launch(st, (const double*)s->upart.p, s->nbN, 2, 0, s->scal.p + 4);
    if (s->F_dev > 0)
        hipLaunchKernelGGL(smooth_factor_kernel<false>, dim3(s->nbF), dim3(kThreads), 0, st, factor_dev(s), (const double*)s->poses[1 - s->cur].p, (double*)nullptr, (double*)nullptr,
                           (double*)nullptr, (double*)nullptr, s->fpart.p);
    final_launch(st, (const double*)s->fpart.p, s->nbF, 1, 0, s->scal.p + 6);
    return iba::pgo::read_scalars(s, kScal, scal_host, name, "trial", lambda);
}

}  // namespace

extern "C" {

iba_status iba_default_smooth_options(iba_smooth_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->max_iteration = 100; o->max_iteration_lm = 20; o->segment = 128;
    o->min_relative_increment = 1e-6; o->min_relative_residual_increment = 1e-6; o->min_right_term = 1e-6; o->min_residual = 1e-6;
    o->upper_scale_factor = 2.0 / 3.0; o->lower_scale_factor = 1.0 / 3.0;
    return IBA_OK;
}

const char* iba_smooth_last_error(const iba_smooth* s) { return s ? s->err.c_str() : t_err.c_str(); }

void iba_smooth_destroy(iba_smooth* s) {
    if (!s) return;
    if (s->device_ready) {
        (void)hipSetDevice(s->device);
        if (s->stream) (void)hipStreamDestroy(s->stream);
    }
    delete s;
}

iba_status iba_smooth_create(const iba_smooth_options* opt, int device, iba_smooth** out) {
    if (out) *out = nullptr;
    if (!out) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_create: out is NULL");
    const std::string why = validate_options(opt);
    if (!why.empty()) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_create: " + why);
    if (device < 0) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_create: device " + std::to_string(device) + " < 0");
    iba_smooth* s = new iba_smooth();   // the device is opened by the first call that needs it: building a graph needs none
    s->opt = *opt; s->device = device;
    *out = s;
    return IBA_OK;
}

iba_status iba_smooth_add_node(iba_smooth* s, const double* pose16) {
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_add_node: s is NULL");
    { iba_status ds; if (is_dead(s, "iba_smooth_add_node", &ds)) return ds; }
    const std::string why = validate_pose(pose16, "pose16");
    if (!why.empty()) return fail(s, IBA_ERR_INVALID_ARG, "iba_smooth_add_node: " + why);
    if (s->N == INT32_MAX / 64) return fail(s, IBA_ERR_UNSUPPORTED, "iba_smooth_add_node: too many nodes");
    s->new_nodes.insert(s->new_nodes.end(), pose16, pose16 + 16);
    ++s->N;
    return IBA_OK;
}

static iba_status add_factor(iba_smooth* s, const char* who, int32_t i, int32_t j, const double* Z16, const double* var6, int32_t robust) {
    const std::string name = who;
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, name + ": s is NULL");
    { iba_status ds; if (is_dead(s, who, &ds)) return ds; }
    std::string why = validate_pose(Z16, "Z16");
    if (why.empty()) why = validate_var(var6);
    if (why.empty() && (j < 0 || j >= s->N)) why = "node " + std::to_string(j) + " is outside [0, " + std::to_string(s->N) + ")";
    if (why.empty() && i != -1 && (i < 0 || i >= s->N)) why = "node " + std::to_string(i) + " is outside [0, " + std::to_string(s->N) + ")";
    if (why.empty() && i == j) why = "i == j == " + std::to_string(i);
    if (why.empty() && s->fi.size() >= (size_t)(INT32_MAX / 64)) why = "too many factors";
    if (!why.empty()) return fail(s, IBA_ERR_INVALID_ARG, name + ": " + why);
    double zi[12];
    inv12(Z16, zi);
    s->fi.push_back(i); s->fj.push_back(j); s->robust.push_back(robust ? 1 : 0);
    s->zinv.insert(s->zinv.end(), zi, zi + 12);
    for (int k = 0; k < 6; ++k) s->ivar.push_back(1.0 / var6[k]);
    return IBA_OK;
}

iba_status iba_smooth_add_prior(iba_smooth* s, int32_t node, const double* Z16, const double* var6) { return add_factor(s, "iba_smooth_add_prior", -1, node, Z16, var6, 0); }

iba_status iba_smooth_add_between(iba_smooth* s, int32_t i, int32_t j, const double* Z16, const double* var6, int32_t robust) {
    if (s && i == -1) return fail(s, IBA_ERR_INVALID_ARG, "iba_smooth_add_between: node -1 is outside [0, " + std::to_string(s->N) + ")");
    return add_factor(s, "iba_smooth_add_between", i, j, Z16, var6, robust);
}

iba_status iba_smooth_linearize(iba_smooth* s, double* r, double* w, double* A, double* D, double* b, double* F) {
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_linearize: s is NULL");
    { iba_status ds; if (is_dead(s, "iba_smooth_linearize", &ds)) return ds; }
    iba_status st = sync(s, "iba_smooth_linearize");
    if (st != IBA_OK) return st;
    double sc[kScal];
    st = linearize(s, sc, "iba_smooth_linearize");
    if (st != IBA_OK) return st;
    const size_t m = (size_t)s->F_dev, n = (size_t)s->N_dev;
    iba::pgo::Download dn;
    dn(r, s->r.p, 6 * m); dn(w, s->weight.p, m); dn(A, s->A.p, 36 * m); dn(D, s->D.p, 36 * n); dn(b, s->b.p, 6 * n);
    if (dn.e != hipSuccess) return fail(s, IBA_ERR_HIP, std::string("iba_smooth_linearize: ") + hipGetErrorString(dn.e));
    if (F) *F = sc[0];
    return IBA_OK;
}

iba_status iba_smooth_solve(iba_smooth* s, double lambda, double* delta) {
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_solve: s is NULL");
    { iba_status ds; if (is_dead(s, "iba_smooth_solve", &ds)) return ds; }
    const char* state = nullptr;
    if (s->N < 1) state = "the graph has no node";
    else if (!s->linearized || s->N != s->N_dev || (int32_t)s->fi.size() != s->F_dev) state = "no linearisation of the current graph at the current estimates (call iba_smooth_linearize)";
    return iba::pgo::solve_call(s, lambda, delta, "iba_smooth_solve", state);
}

iba_status iba_smooth_update(iba_smooth* s, iba_smooth_result* res) {
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_update: s is NULL");
    { iba_status ds; if (is_dead(s, "iba_smooth_update", &ds)) return ds; }
    if (!res) return fail(s, IBA_ERR_INVALID_ARG, "iba_smooth_update: result is NULL");
    const std::string name = "iba_smooth_update";
    iba_status st = sync(s, "iba_smooth_update");
    if (st != IBA_OK) return st;
    std::memset(res, 0, sizeof(*res));
    res->struct_size = (int32_t)sizeof(*res);
    res->n_nodes = s->N_dev; res->n_factors = s->F_dev;
    s->trace.clear();
    iba::GraphLmResult lm;   // S4
    st = iba::graph_lm(iba::graph_lm_options(s->opt),
        [&](bool after_accept, double* sc) { if (after_accept) s->cur = 1 - s->cur; return linearize(s, sc, name); },
        [&](double lambda, double* ts) { s->ar.launch(s->stream, s->D.p, s->b.p, s->A.p, lambda, s->delta.p, s->scal.p); return trial(s, lambda, ts, name); }, s->trace, 0, lm);
    res->F_start = lm.residual_start; res->lambda_start = lm.lambda_start;
    if (st != IBA_OK) return st;
    res->iterations = lm.iterations; res->trials = lm.trials; res->stop = lm.stop; res->F = lm.residual; res->lambda = lm.lambda; res->max_b = lm.max_b;
    return IBA_OK;
}

iba_status iba_smooth_read(iba_smooth* s, int32_t first, int32_t count, double* nodes16, double* weight) {
    if (!s) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_smooth_read: s is NULL");
    { iba_status ds; if (is_dead(s, "iba_smooth_read", &ds)) return ds; }
    if (first < 0 || count < 0 || (int64_t)first + count > s->N)
        return fail(s, IBA_ERR_INVALID_ARG, "iba_smooth_read: nodes [" + std::to_string(first) + ", " + std::to_string((int64_t)first + count) + ") are outside [0, " + std::to_string(s->N) + ")");
    const size_t F = s->fi.size();
    hipError_t e = hipSuccess;
    if (s->device_ready && hipSetDevice(s->device) != hipSuccess) return fail(s, IBA_ERR_HIP, "iba_smooth_read: hipSetDevice");
    if (nodes16 && count) {
        // nodes already on the device from there, the ones appended since from the host list
        const int32_t on_dev = std::max(0, std::min(first + count, s->N_dev) - first);
        if (on_dev > 0) e = hipMemcpy(nodes16, s->poses[s->cur].p + 16 * (size_t)first, 16 * (size_t)on_dev * sizeof(double), hipMemcpyDeviceToHost);
        for (int32_t k = on_dev; k < count; ++k) std::memcpy(nodes16 + 16 * (size_t)k, s->new_nodes.data() + 16 * (size_t)(first + k - s->N_dev), 16 * sizeof(double));
    }
    if (e == hipSuccess && weight && F) {
        for (size_t k = 0; k < F; ++k) weight[k] = 1.0;
        if (s->F_dev > 0) e = hipMemcpy(weight, s->weight.p, (size_t)s->F_dev * sizeof(double), hipMemcpyDeviceToHost);
    }
    if (e != hipSuccess) return fail(s, IBA_ERR_HIP, std::string("iba_smooth_read: ") + hipGetErrorString(e));
    return IBA_OK;
}

iba_status iba_debug_smooth_trace(iba_smooth* s, uint8_t* trials, int32_t cap, int32_t* n) {
    if (!iba::pgo::trace_out(s ? &s->trace : nullptr, trials, cap, n)) return fail(s, IBA_ERR_INVALID_ARG, "iba_debug_smooth_trace: bad argument");
    return IBA_OK;
}

}  // extern "C"

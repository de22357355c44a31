// Pose-graph optimisation on the device (include/iba_mi355x.h, iba_pgo_*): Open3D's GlobalOptimization — LM, pruning of uncertain edges by
// line-process weight, LM again — on a graph that stays on the device. Kernels: iba_pgo_kernels.hpp; plan and checks: iba_pgo_host.hpp.
// The LM loop is iba_graph_lm.hpp's (shared with iba_smooth, as is the scaffolding of iba_pgo_solve.hpp); it reads kScal doubles per trial and nothing else.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "../../include/iba_mi355x_debug.h"
#include "iba_device_buf.hpp"
#include "iba_internal.hpp"
#include "iba_pgo_host.hpp"
#include "iba_pgo_kernels.hpp"
#include "iba_pgo_solve.hpp"

namespace {

using namespace iba::pgo;
using iba::DevBuf;

thread_local std::string t_err;

int sep_cap() {
    int cap = IBA_PGO_MAX_SEPARATORS;
    if (const char* e = iba::debug_env("IBA_PGO_MAX_SEP")) { const int v = std::atoi(e); if (v >= 1 && v <= IBA_PGO_MAX_SEPARATORS) cap = v; }
    return cap;
}

}  // namespace

struct iba_pgo {
    int device = 0;
    int32_t N = 0, E = 0;
    iba_pgo_options opt{};
    std::vector<int32_t> src, tgt;
    std::vector<uint8_t> flags;
    std::vector<double> info55;
    Plan plan;
    Arrow ar;                    // the plan on the device and the solve (shared with iba_smooth)
    double mu = 0.0;
    int cur = 0;                 // poses[cur] are the poses, poses[1 - cur] the trial
    bool linearized = false;
    int nbE = 0, nbN = 0;
    DevBuf<double> poses[2], Xinv, info, weight, zeta, A, g, epart, D, b, npart, delta, upart, scal;
    DevBuf<int32_t> d_src, d_tgt;
    DevBuf<uint8_t> d_flags;
    std::vector<uint8_t> trace;
    std::string err;
    hipStream_t stream = nullptr;
};

namespace {

iba_status fail(iba_pgo* pg, iba_status s, const std::string& m) { if (pg) pg->err = m; else t_err = m; return s; }

EdgeDev edge_dev(const iba_pgo* pg) { return EdgeDev{pg->E, pg->d_src.p, pg->d_tgt.p, pg->Xinv.p, pg->info.p, pg->d_flags.p}; }

// the plan of the active edges onto the device (create and prune time)
iba_status upload_plan(iba_pgo* pg) {
    std::vector<uint8_t> active(pg->E);
    for (int32_t e = 0; e < pg->E; ++e) active[e] = (pg->flags[e] & 2) ? 0 : 1;
    std::string why;
    if (!make_plan(pg->N, pg->src.data(), pg->tgt.data(), active.data(), pg->E, pg->opt.segment, sep_cap(), pg->plan, why)) return fail(pg, IBA_ERR_INVALID_ARG, "iba_pgo: " + why);
    pg->mu = line_process_mu(pg->opt, pg->info55.data(), pg->flags.data(), pg->E);
    hipError_t e = pg->d_flags.upload(pg->flags);
    if (e == hipSuccess) e = pg->ar.upload(pg->plan, pg->N);
    if (e != hipSuccess) return fail(pg, IBA_ERR_HIP, std::string("iba_pgo: plan upload: ") + hipGetErrorString(e));
    pg->linearized = false;
    return IBA_OK;
}

// linearise at poses[cur]; scal[0..3] on the host afterwards
iba_status linearize(iba_pgo* pg, bool recompute_w, double* scal_host) {
    hipStream_t st = pg->stream;
    if (pg->E > 0)
        hipLaunchKernelGGL(pgo_edge_kernel<true>, dim3(pg->nbE), dim3(kThreads), 0, st, edge_dev(pg), (const double*)pg->poses[pg->cur].p, pg->mu, recompute_w ? 1 : 0, pg->weight.p,
                           pg->zeta.p, pg->A.p, pg->g.p, pg->epart.p);
    final_launch(st, pg->epart.p, pg->nbE, 1, 0, pg->scal.p);
    hipLaunchKernelGGL(pgo_node_kernel, dim3(pg->N), dim3(64), 0, st, (int)pg->N, (const int32_t*)pg->ar.inc_off.p, (const int32_t*)pg->ar.inc_edge.p, (const double*)pg->A.p,
                       (const double*)pg->g.p, (const double*)pg->poses[pg->cur].p, pg->D.p, pg->b.p, pg->npart.p);
    final_launch(st, pg->npart.p, (int)pg->N, 1, 2, pg->scal.p + 1);
    const iba_status rs = read_scalars(pg, 4, scal_host, "iba_pgo", "linearise");
    if (rs == IBA_OK) pg->linearized = true;
    return rs;
}

// the launch chain of (H + lambda I) delta = b; no synchronisation
void solve_launch(iba_pgo* pg, double lambda) { pg->ar.launch(pg->stream, pg->D.p, pg->b.p, pg->A.p, lambda, pg->delta.p, pg->scal.p); }

// trial poses into poses[1 - cur] from delta, the trial residual; scal[0..7] on the host afterwards
iba_status trial(iba_pgo* pg, double lambda, double* scal_host) {
    hipStream_t st = pg->stream;
    hipLaunchKernelGGL(pgo_update_kernel, dim3(pg->nbN), dim3(kThreads), 0, st, (int)pg->N, (const double*)pg->poses[pg->cur].p, (const double*)pg->delta.p, (const double*)pg->b.p, lambda,
                       pg->poses[1 - pg->cur].p, pg->upart.p);
    final_launch(st, pg->upart.p, pg->nbN, 2, 0, pg->scal.p + 4);
    if (pg->E > 0)
        hipLaunchKernelGGL(pgo_edge_kernel<false>, dim3(pg->nbE), dim3(kThreads), 0, st, edge_dev(pg), (const double*)pg->poses[1 - pg->cur].p, pg->mu, 0, pg->weight.p,
                           (double*)nullptr, (double*)nullptr, (double*)nullptr, pg->epart.p);
    final_launch(st, pg->epart.p, pg->nbE, 1, 0, pg->scal.p + 6);
    return read_scalars(pg, kScal, scal_host, "iba_pgo", "trial", lambda);
}

// one LM pass (rule 6: iba_graph_lm.hpp), then the reference-node compensation
iba_status lm_pass(iba_pgo* pg, iba_pgo_pass* out, uint8_t trace_bit) {
    const iba_pgo_options& o = pg->opt;
    double ref_before[16];
    if (o.reference_node >= 0 && hipMemcpy(ref_before, pg->poses[pg->cur].p + 16 * (size_t)o.reference_node, sizeof(ref_before), hipMemcpyDeviceToHost) != hipSuccess)
        return fail(pg, IBA_ERR_HIP, "iba_pgo: download of the reference node");
    // rule 6 itself; the line-process weights are recomputed, and the accepted trial becomes the poses, only behind an accepted trial
    iba::GraphLmResult lm;
    const iba_status st = iba::graph_lm(iba::graph_lm_options(o),
        [&](bool after_accept, double* sc) { if (after_accept) pg->cur = 1 - pg->cur; return linearize(pg, after_accept, sc); },
        [&](double lambda, double* ts) { solve_launch(pg, lambda); return trial(pg, lambda, ts); }, pg->trace, trace_bit, lm);
    if (st != IBA_OK) return st;
    out->iterations = lm.iterations; out->trials = lm.trials; out->stop = lm.stop; out->reserved = 0; out->residual = lm.residual; out->lambda = lm.lambda;
    if (o.reference_node >= 0) {
        double ref_after[16], inv[12];
        if (hipMemcpy(ref_after, pg->poses[pg->cur].p + 16 * (size_t)o.reference_node, sizeof(ref_after), hipMemcpyDeviceToHost) != hipSuccess)
            return fail(pg, IBA_ERR_HIP, "iba_pgo: download of the reference node");
        Rigid12 C;
        inv12(ref_after, inv);
        mul12(ref_before, inv, C.m);
        hipLaunchKernelGGL(pgo_left_mul_kernel, dim3(pg->nbN), dim3(kThreads), 0, pg->stream, (int)pg->N, C, pg->poses[pg->cur].p);
        const hipError_t e = hipStreamSynchronize(pg->stream);
        if (e != hipSuccess) return fail(pg, IBA_ERR_HIP, std::string("iba_pgo: compensation kernel: ") + hipGetErrorString(e));
        pg->linearized = false;
    }
    return IBA_OK;
}

}  // namespace

// iba_pgo_solve.hpp: the one place the solve's kernels are launched from
namespace iba { namespace pgo {

void Arrow::launch(hipStream_t st, const double* D, const double* b, const double* A, double lambda, double* delta, double* scal) {
    const RunDev rd{R, run_first.p, run_last.p, chain.p, N};
    const int n = 6 * ns;
    (void)hipMemsetAsync(scal + 7, 0, sizeof(double), st);
    (void)hipMemsetAsync(S.p, 0, (size_t)n * n * sizeof(double), st);
    if (R > 0)
        hipLaunchKernelGGL(pgo_run_forward_kernel, dim3((R + 3) / 4), dim3(64), 0, st, rd, D, b, A, lambda, G.p, F.p, y.p, run_S.p, run_b.p, scal);
    hipLaunchKernelGGL(pgo_sep_assemble_kernel, dim3(nblk), dim3(64), 0, st, (const int32_t*)brow.p, (const int32_t*)bcol.p, (const int32_t*)boff.p,
                       (const int32_t*)kind.p, (const int32_t*)idx.p, D, b, A, (const double*)run_S.p, (const double*)run_b.p, lambda, n, S.p, rhs.p);
    for (int j0 = 0; j0 < n; j0 += kNB) {
        const int w = std::min(kNB, n - j0);
        hipLaunchKernelGGL(pgo_chol_panel_kernel, dim3(1), dim3(kThreads), 0, st, S.p, n, j0, w, scal);
        const int rest = n - (j0 + w);
        if (rest > 0) { const int nt = (rest + kTile - 1) / kTile; hipLaunchKernelGGL(pgo_chol_update_kernel, dim3(nt, nt), dim3(kThreads), 0, st, S.p, n, j0, w); }
    }
    hipLaunchKernelGGL(pgo_sep_solve_kernel, dim3(1), dim3(kThreads), 0, st, (const double*)S.p, n, (const double*)rhs.p, xs.p);
    hipLaunchKernelGGL(pgo_run_back_kernel, dim3((std::max(R, ns) + 63) / 64), dim3(64), 0, st, rd, ns, (const int32_t*)sep_node.p, (const int32_t*)sep_of_node.p,
                       (const double*)xs.p, (const double*)G.p, (const double*)F.p, (const double*)y.p, delta);
}

void final_launch(hipStream_t st, const double* partial, int nblocks, int nsum, int nmax, double* out) {
    hipLaunchKernelGGL(pgo_final_kernel, dim3(1), dim3(64), 0, st, partial, nblocks, nsum, nmax, out);
}

} }  // namespace iba::pgo

extern "C" {

iba_status iba_default_pgo_options(iba_pgo_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->reference_node = 0;
    o->max_corr_dist = 1.2; o->edge_prune_threshold = 0.25; o->preference_loop_closure = 1.0;
    o->max_iteration = 100; o->max_iteration_lm = 20;
    o->min_relative_increment = 1e-6; o->min_relative_residual_increment = 1e-6; o->min_right_term = 1e-6; o->min_residual = 1e-6;
    o->upper_scale_factor = 2.0 / 3.0; o->lower_scale_factor = 1.0 / 3.0;
    o->segment = 128;   // profiles/pgo_bench.md: the fastest of 8 .. 128 at N = 512 and N = 4541
    return IBA_OK;
}

const char* iba_pgo_last_error(const iba_pgo* pg) { return pg ? pg->err.c_str() : t_err.c_str(); }

void iba_pgo_destroy(iba_pgo* pg) {
    if (!pg) return;
    (void)hipSetDevice(pg->device);
    if (pg->stream) (void)hipStreamDestroy(pg->stream);
    delete pg;
}

iba_status iba_pgo_plan(int32_t N, const iba_pgo_edge* edges, int32_t E, const iba_pgo_options* opt, int32_t* separators, int32_t sep_cap_out, int32_t* n_separators,
                        int32_t* runs, int32_t run_cap, int32_t* n_runs, int32_t* K_used) {
    std::string why = validate_topology(N, edges, E);
    if (why.empty()) why = validate_options(opt, N);
    if (why.empty() && ((separators && sep_cap_out < 0) || (runs && run_cap < 0))) why = "a negative capacity";
    if (!why.empty()) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_plan: " + why);
    std::vector<int32_t> src(E), tgt(E);
    for (int32_t e = 0; e < E; ++e) { src[e] = edges[e].source; tgt[e] = edges[e].target; }
    Plan p;
    if (!make_plan(N, src.data(), tgt.data(), nullptr, E, opt->segment, sep_cap(), p, why)) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_plan: " + why);
    if (separators) for (int32_t k = 0; k < sep_cap_out && k < (int32_t)p.sep.size(); ++k) separators[k] = p.sep[k];
    if (n_separators) *n_separators = (int32_t)p.sep.size();
    if (runs) for (int32_t k = 0; k < run_cap && k < (int32_t)p.run_first.size(); ++k) { runs[2 * k] = p.run_first[k]; runs[2 * k + 1] = p.run_last[k]; }
    if (n_runs) *n_runs = (int32_t)p.run_first.size();
    if (K_used) *K_used = p.K;
    return IBA_OK;
}

iba_status iba_pgo_create(const double* nodes16, int32_t N, const iba_pgo_edge* edges, int32_t E, const iba_pgo_options* opt, int device, iba_pgo** out) {
    if (out) *out = nullptr;
    if (!out) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_create: out is NULL");
    std::string why = validate_topology(N, edges, E);
    if (why.empty()) why = validate_options(opt, N);
    if (why.empty()) why = validate_values(nodes16, N, edges, E);
    if (!why.empty()) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_create: " + why);
    iba_pgo* pg = new iba_pgo();
    pg->N = N; pg->E = E; pg->opt = *opt; pg->device = device;
    pg->src.resize(E); pg->tgt.resize(E); pg->flags.resize(E); pg->info55.resize(E);
    std::vector<double> xinv((size_t)E * 12), info((size_t)E * 36), ones((size_t)E, 1.0);
    for (int32_t e = 0; e < E; ++e) {
        pg->src[e] = edges[e].source; pg->tgt[e] = edges[e].target; pg->flags[e] = edges[e].uncertain ? 1 : 0; pg->info55[e] = edges[e].info[35];
        inv12(edges[e].T, &xinv[(size_t)e * 12]);
        for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { info[(size_t)e * 36 + i * 6 + j] = edges[e].info[i * 6 + j]; info[(size_t)e * 36 + j * 6 + i] = edges[e].info[i * 6 + j]; }
    }
    {   // the plan (and with it the separator cap) is an argument check too: before the device probe
        std::string w2; Plan p;
        if (!make_plan(N, pg->src.data(), pg->tgt.data(), nullptr, E, opt->segment, sep_cap(), p, w2)) { delete pg; return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_create: " + w2); }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0 || hipSetDevice(device) != hipSuccess) {
        delete pg;
        return fail(nullptr, IBA_ERR_NO_DEVICE, "iba_pgo_create: no usable gfx950 device " + std::to_string(device) + " (there is no CPU fallback)");
    }
    pg->nbE = (E + kThreads - 1) / kThreads; pg->nbN = (N + kThreads - 1) / kThreads;
    hipError_t e = hipSuccess;
    auto up = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    const size_t n = (size_t)N, m = (size_t)E;
    up(pg->poses[0].alloc(16 * n)); up(pg->poses[1].alloc(16 * n));
    if (e == hipSuccess) up(hipMemcpy(pg->poses[0].p, nodes16, 16 * n * sizeof(double), hipMemcpyHostToDevice));
    up(pg->d_src.upload(pg->src)); up(pg->d_tgt.upload(pg->tgt)); up(pg->Xinv.upload(xinv)); up(pg->info.upload(info)); up(pg->weight.upload(ones));
    up(pg->zeta.alloc(6 * m)); up(pg->A.alloc(36 * m)); up(pg->g.alloc(6 * m)); up(pg->epart.alloc(pg->nbE));
    up(pg->D.alloc(36 * n)); up(pg->b.alloc(6 * n)); up(pg->npart.alloc(3 * n));
    up(pg->delta.alloc(6 * n)); up(pg->upart.alloc(2 * (size_t)pg->nbN)); up(pg->scal.alloc(kScal));
    up(hipStreamCreate(&pg->stream));
    if (e != hipSuccess) { const std::string msg = hipGetErrorString(e); iba_pgo_destroy(pg); return fail(nullptr, IBA_ERR_HIP, "iba_pgo_create: " + msg); }
    const iba_status st = upload_plan(pg);
    if (st != IBA_OK) { t_err = pg->err; iba_pgo_destroy(pg); return st; }
    *out = pg;
    return IBA_OK;
}

iba_status iba_pgo_linearize(iba_pgo* pg, double* zeta, double* weight, double* A, double* b, double* residual) {
    if (!pg) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_linearize: pg is NULL");
    if (hipSetDevice(pg->device) != hipSuccess) return fail(pg, IBA_ERR_HIP, "iba_pgo_linearize: hipSetDevice");
    double sc[kScal];
    const iba_status st = linearize(pg, false, sc);
    if (st != IBA_OK) return st;
    const size_t m = (size_t)pg->E, n = (size_t)pg->N;
    Download dn;
    dn(zeta, pg->zeta.p, 6 * m); dn(weight, pg->weight.p, m); dn(A, pg->A.p, 36 * m); dn(b, pg->b.p, 6 * n);
    if (dn.e != hipSuccess) return fail(pg, IBA_ERR_HIP, std::string("iba_pgo_linearize: ") + hipGetErrorString(dn.e));
    if (residual) *residual = sc[0];
    return IBA_OK;
}

iba_status iba_pgo_solve(iba_pgo* pg, double lambda, double* delta) {
    if (!pg) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_solve: pg is NULL");
    return solve_call(pg, lambda, delta, "iba_pgo_solve", pg->linearized ? nullptr : "no linearisation at the current poses (call iba_pgo_linearize)");
}

iba_status iba_pgo_optimize(iba_pgo* pg, iba_pgo_result* res) {
    if (!pg) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_optimize: pg is NULL");
    if (!res) return fail(pg, IBA_ERR_INVALID_ARG, "iba_pgo_optimize: result is NULL");
    if (hipSetDevice(pg->device) != hipSuccess) return fail(pg, IBA_ERR_HIP, "iba_pgo_optimize: hipSetDevice");
    std::memset(res, 0, sizeof(*res));
    res->struct_size = (int32_t)sizeof(*res);
    pg->trace.clear();
    // weights of the edges in the graph to 1 (a dropped edge keeps the weight it was dropped with); with prune: rule 7 first
    const size_t m = (size_t)pg->E;
    std::vector<double> w(m);
    int32_t n_pruned = 0;
    auto reset_weights = [&](bool prune) -> iba_status {
        if (!m) return IBA_OK;
        if (hipMemcpy(w.data(), pg->weight.p, m * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess) return fail(pg, IBA_ERR_HIP, "iba_pgo_optimize: download of the weights");
        for (size_t e = 0; e < m; ++e) {
            if (prune && (pg->flags[e] & 1) && !(pg->flags[e] & 2) && w[e] < pg->opt.edge_prune_threshold) { pg->flags[e] |= 2; ++n_pruned; }
            if (!(pg->flags[e] & 2)) w[e] = 1.0;
        }
        if (hipMemcpy(pg->weight.p, w.data(), m * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(pg, IBA_ERR_HIP, "iba_pgo_optimize: upload of the weights");
        return IBA_OK;
    };
    iba_status st = reset_weights(false);
    if (st != IBA_OK) return st;
    st = lm_pass(pg, &res->pass[0], 0);
    if (st != IBA_OK) return st;
    st = reset_weights(true);
    if (st != IBA_OK) return st;
    res->n_pruned = n_pruned;
    st = upload_plan(pg);
    if (st != IBA_OK) return st;
    return lm_pass(pg, &res->pass[1], 0x80);
}

iba_status iba_pgo_read(iba_pgo* pg, double* nodes16, double* weight, uint8_t* pruned) {
    if (!pg) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_pgo_read: pg is NULL");
    if (hipSetDevice(pg->device) != hipSuccess) return fail(pg, IBA_ERR_HIP, "iba_pgo_read: hipSetDevice");
    hipError_t e = hipSuccess;
    if (nodes16) e = hipMemcpy(nodes16, pg->poses[pg->cur].p, 16 * (size_t)pg->N * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && weight && pg->E) e = hipMemcpy(weight, pg->weight.p, (size_t)pg->E * sizeof(double), hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(pg, IBA_ERR_HIP, std::string("iba_pgo_read: ") + hipGetErrorString(e));
    if (pruned) for (int32_t k = 0; k < pg->E; ++k) pruned[k] = (pg->flags[k] & 2) ? 1 : 0;
    return IBA_OK;
}

iba_status iba_debug_pgo_trace(iba_pgo* pg, uint8_t* trials, int32_t cap, int32_t* n) {
    if (!trace_out(pg ? &pg->trace : nullptr, trials, cap, n)) return fail(pg, IBA_ERR_INVALID_ARG, "iba_debug_pgo_trace: bad argument");
    return IBA_OK;
}

}  // extern "C"

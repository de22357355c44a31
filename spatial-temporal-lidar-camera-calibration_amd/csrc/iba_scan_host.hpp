// Host side of iba_scan_step / iba_scan_register / iba_scan_information (include/iba_mi355x.h; included at the end of iba_capi.hip, after
// iba_icp_host.hpp whose loop and helpers it uses). A pass = the transforms of the edges still running copied to the device from pinned
// memory, iba_scan_pass_kernel, iba_scan_sum_kernel, the sums copied back to pinned memory, ONE stream synchronise for all edges (PassWork,
// iba_flat_pass.hpp): 160 B down and 256 B up per edge and iteration, nothing of scan size.

namespace {

// an edge that can run: both scans hold points
bool scan_runs(const iba_handle* h, const iba_scan_edge& e) { return h->h_frames[(size_t)e.src_frame].P > 0 && h->h_frames[(size_t)e.tgt_frame].P > 0; }

iba_status scan_check_edges(iba_handle* h, const iba_scan_edge* edges, int32_t E, const char* who) {
    if (!edges) return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": edges are NULL");
    if (E < 1 || E > kIcpMaxB) return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": E must be in [1, 4096]");
    for (int e = 0; e < E; ++e) {
        const iba_scan_edge& g = edges[e];
        if (g.src_frame < 0 || g.src_frame >= h->n_frames || g.tgt_frame < 0 || g.tgt_frame >= h->n_frames)
            return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": edge " + std::to_string(e) + " (" + std::to_string(g.src_frame) + " -> " + std::to_string(g.tgt_frame) + ") names a frame outside the handle's " +
                                                    std::to_string(h->n_frames) + " local frames (both scans of an edge must live on this handle's shard)");
        if (g.src_frame == g.tgt_frame) return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": edge " + std::to_string(e) + " joins frame " + std::to_string(g.src_frame) + " to itself");
        if (!icp_finite16(g.T)) return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": the transform of edge " + std::to_string(e) + " is not finite");
    }
    return IBA_OK;
}
iba_status scan_check_estimation(iba_handle* h, int32_t estimation, bool step, const char* who) {
    if (estimation != IBA_SCAN_POINT_TO_POINT && estimation != IBA_SCAN_POINT_TO_PLANE && !(step && estimation == IBA_SCAN_INFORMATION))
        return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": unknown estimation " + std::to_string(estimation));
    if (estimation == IBA_SCAN_POINT_TO_PLANE && (!h->params.plane_cache || !h->plane_cost.p))
        return fail(h, IBA_ERR_INVALID_ARG, std::string(who) + ": point-to-plane reads the memoised normals of the target scan: the handle needs plane_cache = 1");
    return IBA_OK;
}
bool scan_dist_ok(double d) { return d > 0.0 && std::isfinite(d); }

iba_status scan_reserve_edges(iba_handle* h, int nb) {
    HIP_TRY(h, h->scan.reserve((size_t)nb, (size_t)nb * kScanMom));
    return IBA_OK;
}

// the edge as the kernel takes it (its place in the grid is set by scan_pass); the pivot = T * centre of the source scan's box
void scan_make_xf(const iba_handle* h, int src, int tgt, const double* T16, double dist, ScanXf& x) {
    std::memcpy(x.T, T16, 12 * sizeof(double));
    const float* bx = &h->h_frame_box[8 * (size_t)src];
    const double c[3] = {0.5 * ((double)bx[0] + (double)bx[4]), 0.5 * ((double)bx[1] + (double)bx[5]), 0.5 * ((double)bx[2] + (double)bx[6])};
    icp_pivot(T16, c, x.piv);
    x.gate2 = dist * dist; x.src = src; x.tgt = tgt; x.blk0 = 0; x.part0 = 0; x.pair0 = 0;
}

// launches the pass kernel at the given shape, then the sum kernel of the mode; the status returned is the pass launch's, the sum launch's
// is read by the caller's PassWork::finish
template <int MODE>
hipError_t scan_launch_pass_and_sum(iba_handle* h, PassShape sh, unsigned blocks, int nb, uint32_t* pairs) {
    auto& w = h->scan;
    const auto kernel = sh.threads == 64 ? iba_scan_pass_kernel<64, MODE> : iba_scan_pass_kernel<256, MODE>;
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3((unsigned)sh.threads), sh.lds, h->stream, h->dev_problem(), w.d_item.p, nb, std::max(3, (int)h->params.norm_min_pts), w.d_part.p, pairs);
    if (const hipError_t e = hipGetLastError()) return e;
    hipLaunchKernelGGL(iba_scan_sum_kernel<MODE>, dim3((unsigned)nb), dim3(256), 0, h->stream, h->dev_problem(), w.d_part.p, w.d_item.p, w.d_mom.p);
    return hipSuccess;
}

// One pass over the nb edges staged in h->scan.h_item[0 .. nb) (every one runs): their sums land in h->scan.h_mom. threads: 0 = the rule of
// DESIGN.md 5b applied to the largest target tree of the pass, 64 / 256 forces a shape (the sums do not depend on it). pairs: the edges' pair0 are set by the caller.
iba_status scan_pass(iba_handle* h, int nb, int mode, int threads, bool pairs) {
    auto& w = h->scan;
    uint32_t nodes = 1;
    for (int k = 0; k < nb; ++k) nodes = std::max(nodes, tree_nodes(h->h_frames[(size_t)w.h_item.p[k].tgt]));
    PassShape sh = pass_shape(nodes);
    if (threads == 64 || threads == 256) sh.threads = threads; else if (h->scan_threads) sh.threads = h->scan_threads;
    uint64_t blocks = 0, chunks = 0;
    for (int k = 0; k < nb; ++k) {
        const uint32_t P = h->h_frames[(size_t)w.h_item.p[k].src].P;
        w.h_item.p[k].blk0 = flat_take(blocks, P, sh.threads); w.h_item.p[k].part0 = flat_take(chunks, P, 64);
    }
    if (blocks > 0x7FFFFFFFull) return fail(h, IBA_ERR_UNSUPPORTED, "iba_scan: the batch needs more blocks than one launch takes");
    HIP_TRY(h, w.d_part.grow((size_t)chunks * 31u));
    HIP_TRY(h, w.upload((size_t)nb, h->stream));
    const auto launch = mode == kScanP2P ? scan_launch_pass_and_sum<kScanP2P> : (mode == kScanP2L ? scan_launch_pass_and_sum<kScanP2L> : scan_launch_pass_and_sum<kScanInfo>);
    HIP_TRY(h, launch(h, sh, (unsigned)blocks, nb, pairs ? w.d_pair.p : nullptr));
    HIP_TRY(h, w.finish(kScanMom * (size_t)nb, h->stream));
    h->scan_last_threads = sh.threads;
    return IBA_OK;
}

// the information pass (GetInformationMatrixFromPointClouds) over the edges `run` at the transforms T_of(e), all edges in one pass:
// take(e, m) receives the sums of edge e
template <class TOf, class Take>
iba_status scan_info_pass(iba_handle* h, const iba_scan_edge* edges, const std::vector<int>& run, double dist, TOf T_of, Take take) {
    auto& w = h->scan;
    for (size_t k = 0; k < run.size(); ++k) scan_make_xf(h, edges[run[k]].src_frame, edges[run[k]].tgt_frame, T_of(run[k]), dist, w.h_item.p[k]);
    if (const iba_status s = scan_pass(h, (int)run.size(), kScanInfo, 0, false)) return s;
    for (size_t k = 0; k < run.size(); ++k) take(run[k], w.h_mom.p + (size_t)kScanMom * k);
    return IBA_OK;
}

// one stage of RegistrationICP over the edges `run` (indices into edges / st), from st[].T
iba_status scan_stage(iba_handle* h, const iba_scan_edge* edges, const std::vector<int>& run, std::vector<IcpItem>& st, int estimation, double dist, int max_iter, double rel_fitness, double rel_rmse) {
    auto& w = h->scan;
    for (int e : run) { st[(size_t)e].iterations = 0; st[(size_t)e].status = IBA_ICP_MAX_ITER; }
    const auto pass = [&](const std::vector<int>& lv, const double* Ts, const double*& mom) -> iba_status {
        for (size_t k = 0; k < lv.size(); ++k) scan_make_xf(h, edges[lv[k]].src_frame, edges[lv[k]].tgt_frame, Ts + 16 * k, dist, w.h_item.p[k]);
        mom = w.h_mom.p;
        return scan_pass(h, (int)lv.size(), estimation, 0, false);
    };
    const auto update = [&](const IcpItem& s, double* U4) {
        return estimation == IBA_SCAN_POINT_TO_PLANE ? iba::icp::point_to_plane_from_moments(s.m, U4) : iba::icp::umeyama_from_moments(s.m, false, U4);
    };
    return icp_run_loop(st, run, kScanMom, max_iter, rel_fitness, rel_rmse, pass, update);
}

}  // namespace

iba_status iba_default_scan_options(iba_scan_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(iba_scan_options);
    o->estimation = IBA_SCAN_POINT_TO_POINT;
    o->coarse_dist = 0.0; o->coarse_max_iter = 30; o->coarse_rel_fitness = 1e-4; o->coarse_rel_rmse = 1e-4;
    o->refine_dist = 0.3; o->refine_max_iter = 30; o->refine_rel_fitness = 1e-6; o->refine_rel_rmse = 1e-6;
    o->info_dist = 0.0;
    return IBA_OK;
}

iba_status iba_scan_step(iba_handle* h, const iba_scan_edge* edges, int32_t E, double max_corr_dist, int32_t estimation, double* moments, uint32_t* pair_idx) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!moments) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_step: moments are NULL");
    if (const iba_status s = scan_check_edges(h, edges, E, "iba_scan_step")) return s;
    if (const iba_status s = scan_check_estimation(h, estimation, true, "iba_scan_step")) return s;
    if (!scan_dist_ok(max_corr_dist)) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_step: max_corr_dist must be positive and finite");
    std::memset(moments, 0, sizeof(double) * IBA_SCAN_NMOM * (size_t)E);
    std::vector<int> run;
    std::vector<uint64_t> pair0((size_t)E + 1, 0);
    for (int e = 0; e < E; ++e) { pair0[(size_t)e + 1] = pair0[(size_t)e] + h->h_frames[(size_t)edges[e].src_frame].P; if (scan_runs(h, edges[e])) run.push_back(e); }
    const uint64_t n_pair = pair0[(size_t)E];
    if (pair_idx && n_pair) std::memset(pair_idx, 0xFF, sizeof(uint32_t) * n_pair);
    if (run.empty()) return IBA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (const iba_status s = scan_reserve_edges(h, (int)run.size())) return s;
    auto& w = h->scan;
    if (pair_idx) {
        HIP_TRY(h, w.d_pair.grow((size_t)n_pair));
        HIP_TRY(h, hipMemsetAsync(w.d_pair.p, 0xFF, sizeof(uint32_t) * n_pair, h->stream));
    }
    for (size_t k = 0; k < run.size(); ++k) {
        const iba_scan_edge& g = edges[run[k]];
        scan_make_xf(h, g.src_frame, g.tgt_frame, g.T, max_corr_dist, w.h_item.p[k]);
        w.h_item.p[k].pair0 = pair0[(size_t)run[k]];
    }
    if (const iba_status s = scan_pass(h, (int)run.size(), estimation, 0, pair_idx != nullptr)) return s;
    for (size_t k = 0; k < run.size(); ++k) std::memcpy(moments + (size_t)IBA_SCAN_NMOM * (size_t)run[k], w.h_mom.p + (size_t)kScanMom * k, sizeof(double) * kScanMom);
    if (pair_idx) HIP_TRY(h, hipMemcpy(pair_idx, w.d_pair.p, sizeof(uint32_t) * n_pair, hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_scan_information(iba_handle* h, const iba_scan_edge* edges, int32_t E, double max_dist, double* info, int32_t* n_pairs) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!info || !n_pairs) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_information: NULL output");
    if (const iba_status s = scan_check_edges(h, edges, E, "iba_scan_information")) return s;
    if (!scan_dist_ok(max_dist)) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_information: max_dist must be positive and finite");
    std::memset(info, 0, sizeof(double) * 36 * (size_t)E);
    std::memset(n_pairs, 0, sizeof(int32_t) * (size_t)E);
    std::vector<int> run;
    for (int e = 0; e < E; ++e) if (scan_runs(h, edges[e])) run.push_back(e);
    if (run.empty()) return IBA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    if (const iba_status s = scan_reserve_edges(h, (int)run.size())) return s;
    return scan_info_pass(h, edges, run, max_dist, [&](int e) { return edges[e].T; },
                          [&](int e, const double* m) { iba::icp::information_from_sums(m, info + 36 * (size_t)e); n_pairs[e] = (int32_t)m[0]; });
}

iba_status iba_scan_register(iba_handle* h, const iba_scan_edge* edges, int32_t E, const iba_scan_options* o, iba_scan_result* out) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_register: results are NULL");
    if (!o) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_register: options are NULL (iba_default_scan_options fills them)");
    if (o->struct_size != (int32_t)sizeof(iba_scan_options)) return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_options.struct_size does not match this library");
    if (const iba_status s = scan_check_edges(h, edges, E, "iba_scan_register")) return s;
    if (const iba_status s = scan_check_estimation(h, o->estimation, false, "iba_scan_register")) return s;
    const bool coarse = o->coarse_dist > 0.0;
    if (!scan_dist_ok(o->refine_dist) || o->refine_max_iter < 0 || !(o->refine_rel_fitness >= 0.0) || !(o->refine_rel_rmse >= 0.0) ||
        (coarse && (!std::isfinite(o->coarse_dist) || o->coarse_max_iter < 0 || !(o->coarse_rel_fitness >= 0.0) || !(o->coarse_rel_rmse >= 0.0))) || !(std::isfinite(o->info_dist) || o->info_dist <= 0.0))
        return fail(h, IBA_ERR_INVALID_ARG, "iba_scan_options: refine_dist must be positive and finite, the iteration counts and thresholds non-negative, the distances finite");
    std::vector<IcpItem> st((size_t)E);
    std::vector<int> run;
    for (int e = 0; e < E; ++e) {
        IcpItem& s = st[(size_t)e];
        std::memcpy(s.T, edges[e].T, sizeof(double) * 16); std::memset(s.m, 0, sizeof(s.m));
        s.n_src = (int)h->h_frames[(size_t)edges[e].src_frame].P; s.status = IBA_ICP_DEGENERATE;
        if (scan_runs(h, edges[e])) run.push_back(e);
    }
    std::memset(out, 0, sizeof(iba_scan_result) * (size_t)E);
    if (!run.empty()) {
        HIP_TRY(h, hipSetDevice(h->device));
        if (const iba_status s = scan_reserve_edges(h, (int)run.size())) return s;
        if (coarse) if (const iba_status s = scan_stage(h, edges, run, st, o->estimation, o->coarse_dist, o->coarse_max_iter, o->coarse_rel_fitness, o->coarse_rel_rmse)) return s;
        if (const iba_status s = scan_stage(h, edges, run, st, o->estimation, o->refine_dist, o->refine_max_iter, o->refine_rel_fitness, o->refine_rel_rmse)) return s;
    }
    for (int e = 0; e < E; ++e) {
        const IcpItem& s = st[(size_t)e];
        icp_fill_result(s.T, s.m, s.n_src, s.iterations, s.status, out[e].reg);
        out[e].n_planar = o->estimation == IBA_SCAN_POINT_TO_PLANE ? (int32_t)s.m[2] : 0;
    }
    if (o->info_dist > 0.0 && !run.empty())   // at the final transforms
        return scan_info_pass(h, edges, run, o->info_dist, [&](int e) { return (const double*)st[(size_t)e].T; },
                              [&](int e, const double* m) { iba::icp::information_from_sums(m, out[e].info); out[e].n_info = (int32_t)m[0]; });
    return IBA_OK;
}

/* debug (include/iba_mi355x_debug.h): force the block shape of the scan pass kernel (64 / 256; 0 = the rule); the shape of the last pass */
iba_status iba_debug_scan_threads(iba_handle* h, int32_t threads) {
    if (!h || (threads != 0 && threads != 64 && threads != 256)) return IBA_ERR_INVALID_ARG;
    h->scan_threads = threads;
    return IBA_OK;
}
int32_t iba_debug_last_scan_threads(const iba_handle* h) { return h ? h->scan_last_threads : -1; }

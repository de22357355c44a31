// Host side of iba_icp_step / iba_icp_register / iba_icp_calib (include/iba_mi355x.h; included at the end of iba_capi.hip, whose handle it uses).
// A pass = the transforms of the starts still running copied to the device from pinned memory, iba_icp_pass_kernel, iba_icp_sum_kernel, the
// moment blocks copied back to pinned memory, one stream synchronise (PassWork, iba_flat_pass.hpp): 128 B down and 168 B up per start and
// iteration. The source cloud is uploaded once per call.

namespace {

constexpr int kIcpMaxB = 4096;

iba_status icp_check_target(iba_handle* h, int32_t fb, int32_t fe) {
    if (fb < 0 || fe > h->n_frames || fb >= fe) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp: frame range [" + std::to_string(fb) + ", " + std::to_string(fe) + ") is empty or outside the handle's " + std::to_string(h->n_frames) + " local frames");
    return IBA_OK;
}

// block shape of the pass kernel for this target (the largest node table among its tiles that hold points)
PassShape icp_shape(const iba_handle* h, int fb, int fe) {
    uint32_t nodes = 1;
    for (int f = fb; f < fe; ++f) if (h->h_frames[(size_t)f].P > 0) nodes = std::max(nodes, tree_nodes(h->h_frames[(size_t)f]));
    return pass_shape(nodes);
}

iba_status icp_reserve(iba_handle* h, int n, int B, int threads, bool pairs) {
    auto& w = h->icp;
    const size_t nw = ((size_t)n + (size_t)threads - 1) / (size_t)threads * (size_t)(threads / 64);
    HIP_TRY(h, w.reserve((size_t)B, (size_t)B * kIcpMom));
    HIP_TRY(h, w.d_src.grow(3 * (size_t)n));
    HIP_TRY(h, w.d_part.grow((size_t)B * nw * kIcpSums));
    if (pairs) HIP_TRY(h, w.d_pair.grow(2 * (size_t)B * (size_t)n));
    return IBA_OK;
}

// plain sequential f64 mean of the source points (the pivot of the sums is its image)
void icp_centroid(const double* src, int n, double c[3]) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = 0; i < n; ++i) { s0 += src[3 * (size_t)i]; s1 += src[3 * (size_t)i + 1]; s2 += src[3 * (size_t)i + 2]; }
    c[0] = s0 / (double)n; c[1] = s1 / (double)n; c[2] = s2 / (double)n;
}
// piv = T c by the kernel's own expression (icp_transform)
void icp_pivot(const double* T16, const double c[3], double piv[3]) {
    for (int r = 0; r < 3; ++r) piv[r] = std::fma(T16[r * 4 + 2], c[2], std::fma(T16[r * 4 + 1], c[1], std::fma(T16[r * 4], c[0], T16[r * 4 + 3])));
}
// the transform as the kernel takes it
void icp_make_xf(const double* T16, const double c[3], double gate, IcpXf& x) {
    std::memcpy(x.T, T16, 12 * sizeof(double));
    icp_pivot(T16, c, x.piv);
    x.gate2 = gate * gate;
}

// one pass over the nb transforms staged in h->icp.h_item[0 .. nb): their moment blocks land in h->icp.h_mom (the source is on the device)
iba_status icp_pass(iba_handle* h, int fb, int fe, int n, int nb, PassShape sh, bool pairs) {
    auto& w = h->icp;
    const hipStream_t st = h->stream;
    HIP_TRY(h, w.upload((size_t)nb, st));
    const dim3 grid((unsigned)(((size_t)n + (size_t)sh.threads - 1) / (size_t)sh.threads), (unsigned)nb);
    uint32_t* pf = pairs ? w.d_pair.p : nullptr; uint32_t* pi = pairs ? w.d_pair.p + (size_t)nb * (size_t)n : nullptr;
    const auto kernel = sh.threads == 64 ? iba_icp_pass_kernel<64> : iba_icp_pass_kernel<256>;
    hipLaunchKernelGGL(kernel, grid, dim3((unsigned)sh.threads), sh.lds, st, h->dev_problem(), h->d_frame_box.p, fb, fe, w.d_src.p, n, w.d_item.p, w.d_part.p, pf, pi);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_icp_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, w.d_part.p, (int)(grid.x * (unsigned)(sh.threads / 64)), w.d_item.p, w.d_mom.p);
    HIP_TRY(h, w.finish(kIcpMom * (size_t)nb, st));
    return IBA_OK;
}

bool icp_finite16(const double* T) { for (int i = 0; i < 16; ++i) if (!std::isfinite(T[i])) return false; return true; }

iba_status icp_check_options(iba_handle* h, const iba_icp_options* o) {
    if (!o) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp: options are NULL (iba_default_icp_options fills them)");
    if (o->struct_size != (int32_t)sizeof(iba_icp_options)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_options.struct_size does not match this library");
    if (!(o->max_corr_dist > 0.0) || !std::isfinite(o->max_corr_dist) || o->max_iter < 0 || !(o->relative_fitness >= 0.0) || !(o->relative_rmse >= 0.0))
        return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_options: max_corr_dist must be positive and finite, max_iter and the two thresholds non-negative");
    return IBA_OK;
}

// RegistrationICP over independent items (starts of iba_icp_register, edges of iba_scan_register), parameterised on the device pass and on the
// host update. pass(live, Ts, mom): one correspondence pass at the transforms Ts (16 doubles per live item), mom receives the moment blocks
// (nmom doubles per live item); update(item, U4): the estimation's update from item.m, false when none is defined. Finished items drop out of
// the passes; item.status is IBA_ICP_* at the end.
struct IcpItem { double T[16]; double m[32]; int iterations = 0; int n_src = 0; int status = IBA_ICP_MAX_ITER; };
template <class Pass, class Update>
iba_status icp_run_loop(std::vector<IcpItem>& st, std::vector<int> live, int nmom, int max_iter, double rel_fitness, double rel_rmse, Pass pass, Update update) {
    if (live.empty()) return IBA_OK;
    std::vector<int> next;
    std::vector<double> cand(16 * live.size());
    const double* mom = nullptr;
    // evaluation at the init (GetRegistrationResultAndCorrespondences before the loop)
    for (size_t k = 0; k < live.size(); ++k) std::memcpy(&cand[16 * k], st[(size_t)live[k]].T, sizeof(double) * 16);
    if (const iba_status s = pass(live, cand.data(), mom)) return s;
    for (size_t k = 0; k < live.size(); ++k) std::memcpy(st[(size_t)live[k]].m, mom + (size_t)nmom * k, sizeof(double) * (size_t)nmom);
    for (int it = 0; it < max_iter && !live.empty(); ++it) {
        next.clear();
        for (size_t k = 0; k < live.size(); ++k) {   // T = update * T
            IcpItem& s = st[(size_t)live[k]];
            double U4[16];
            if (!update(s, U4)) { s.status = IBA_ICP_DEGENERATE; continue; }
            double Tn[16]; iba::icp::mat4_mul(U4, s.T, Tn);
            if (!icp_finite16(Tn)) { s.status = IBA_ICP_DEGENERATE; continue; }
            std::memcpy(&cand[16 * next.size()], Tn, sizeof(Tn));
            next.push_back(live[k]);
        }
        live.swap(next);
        if (live.empty()) break;
        if (const iba_status s = pass(live, cand.data(), mom)) return s;
        next.clear();
        for (size_t k = 0; k < live.size(); ++k) {
            IcpItem& s = st[(size_t)live[k]];
            const double* m = mom + (size_t)nmom * k;
            const double df = std::fabs(iba::icp::fitness_of(s.m, s.n_src) - iba::icp::fitness_of(m, s.n_src)), dr = std::fabs(iba::icp::rmse_of(s.m) - iba::icp::rmse_of(m));
            std::memcpy(s.T, &cand[16 * k], sizeof(double) * 16); std::memcpy(s.m, m, sizeof(double) * (size_t)nmom); ++s.iterations;
            if (df < rel_fitness && dr < rel_rmse) s.status = IBA_ICP_CONVERGED;
            else next.push_back(live[k]);
        }
        live.swap(next);
    }
    for (int b : live) { IcpItem& s = st[(size_t)b]; s.status = s.m[0] >= 3.0 ? IBA_ICP_MAX_ITER : IBA_ICP_DEGENERATE; }
    return IBA_OK;
}

void icp_fill_result(const double* T, const double* m, int n_src, int iterations, int converged, iba_icp_result& r) {
    std::memcpy(r.T, T, 16 * sizeof(double));
    r.scale = iba::icp::scale_of(T);
    r.fitness = iba::icp::fitness_of(m, n_src); r.inlier_rmse = iba::icp::rmse_of(m);
    r.n_corr = (int32_t)m[0]; r.iterations = iterations; r.converged = converged;
}

}  // namespace

iba_status iba_default_icp_options(iba_icp_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(iba_icp_options);
    o->max_corr_dist = 1.0; o->max_iter = 30; o->relative_fitness = 1e-6; o->relative_rmse = 1e-6; o->with_scaling = 1;
    return IBA_OK;
}

iba_status iba_icp_step(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* src_xyz, int32_t n_src, const double* T, int32_t B,
                        double max_corr_dist, double* moments, uint32_t* pair_frame, uint32_t* pair_idx) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!T || !moments || n_src < 0 || (n_src > 0 && !src_xyz)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_step: NULL transform, moments or source");
    if (B < 1 || B > kIcpMaxB) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_step: B must be in [1, 4096]");
    if ((pair_frame == nullptr) != (pair_idx == nullptr)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_step: pair_frame and pair_idx go together (both NULL or both given)");
    if (!(max_corr_dist > 0.0) || !std::isfinite(max_corr_dist)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_step: max_corr_dist must be positive and finite");
    if (const iba_status s = icp_check_target(h, frame_begin, frame_end)) return s;
    for (int b = 0; b < B; ++b) if (!icp_finite16(T + 16 * (size_t)b)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_step: transform " + std::to_string(b) + " is not finite");
    std::memset(moments, 0, sizeof(double) * IBA_ICP_NMOM * (size_t)B);
    if (n_src == 0) return IBA_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    const bool pairs = pair_idx != nullptr;
    const PassShape sh = icp_shape(h, frame_begin, frame_end);
    if (const iba_status s = icp_reserve(h, n_src, B, sh.threads, pairs)) return s;
    auto& w = h->icp;
    HIP_TRY(h, hipMemcpyAsync(w.d_src.p, src_xyz, sizeof(double) * 3 * (size_t)n_src, hipMemcpyHostToDevice, h->stream));
    double c[3]; icp_centroid(src_xyz, n_src, c);
    for (int b = 0; b < B; ++b) icp_make_xf(T + 16 * (size_t)b, c, max_corr_dist, w.h_item.p[b]);
    if (const iba_status s = icp_pass(h, frame_begin, frame_end, n_src, B, sh, pairs)) return s;
    std::memcpy(moments, w.h_mom.p, sizeof(double) * IBA_ICP_NMOM * (size_t)B);
    if (pairs) {
        HIP_TRY(h, hipMemcpy(pair_frame, w.d_pair.p, sizeof(uint32_t) * (size_t)B * (size_t)n_src, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(pair_idx, w.d_pair.p + (size_t)B * (size_t)n_src, sizeof(uint32_t) * (size_t)B * (size_t)n_src, hipMemcpyDeviceToHost));
    }
    return IBA_OK;
}

iba_status iba_icp_register(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* src_xyz, int32_t n_src, const double* T_init, int32_t B,
                            const iba_icp_options* opt, iba_icp_result* out) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!T_init || !out || n_src < 0 || (n_src > 0 && !src_xyz)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_register: NULL transforms, results or source");
    if (B < 1 || B > kIcpMaxB) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_register: B must be in [1, 4096]");
    if (const iba_status s = icp_check_options(h, opt)) return s;
    if (const iba_status s = icp_check_target(h, frame_begin, frame_end)) return s;
    for (int b = 0; b < B; ++b) if (!icp_finite16(T_init + 16 * (size_t)b)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_register: start " + std::to_string(b) + " is not finite");
    const double zero[IBA_ICP_NMOM] = {0.0};
    if (n_src == 0) {   // nothing to register: the starts come back as they are, marked degenerate
        for (int b = 0; b < B; ++b) icp_fill_result(T_init + 16 * (size_t)b, zero, 0, 0, IBA_ICP_DEGENERATE, out[b]);
        return IBA_OK;
    }
    HIP_TRY(h, hipSetDevice(h->device));
    const PassShape sh = icp_shape(h, frame_begin, frame_end);
    if (const iba_status s = icp_reserve(h, n_src, B, sh.threads, false)) return s;
    auto& w = h->icp;
    HIP_TRY(h, hipMemcpyAsync(w.d_src.p, src_xyz, sizeof(double) * 3 * (size_t)n_src, hipMemcpyHostToDevice, h->stream));
    double c[3]; icp_centroid(src_xyz, n_src, c);
    std::vector<IcpItem> st((size_t)B);
    std::vector<int> live((size_t)B);   // the starts of the current pass, in ascending order
    for (int b = 0; b < B; ++b) { std::memcpy(st[(size_t)b].T, T_init + 16 * (size_t)b, sizeof(double) * 16); st[(size_t)b].n_src = n_src; live[(size_t)b] = b; }
    const auto pass = [&](const std::vector<int>& lv, const double* Ts, const double*& mom) -> iba_status {
        for (size_t k = 0; k < lv.size(); ++k) icp_make_xf(Ts + 16 * k, c, opt->max_corr_dist, w.h_item.p[k]);
        mom = w.h_mom.p;
        return icp_pass(h, frame_begin, frame_end, n_src, (int)lv.size(), sh, false);
    };
    const auto update = [&](const IcpItem& s, double* U4) { return iba::icp::umeyama_from_moments(s.m, opt->with_scaling != 0, U4); };
    if (const iba_status s = icp_run_loop(st, live, kIcpMom, opt->max_iter, opt->relative_fitness, opt->relative_rmse, pass, update)) return s;
    for (int b = 0; b < B; ++b) { const IcpItem& s = st[(size_t)b]; icp_fill_result(s.T, s.m, n_src, s.iterations, s.status, out[b]); }
    return IBA_OK;
}

iba_status iba_icp_calib(iba_handle* h, int32_t frame_begin, int32_t frame_end, const double* cam_xyz, int32_t n, const double rigid12_init[12], double scale_init,
                         const double* ref_lidar_pose12, const iba_icp_options* opt, double rigid12_out[12], double* scale_out, iba_icp_result* res) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!rigid12_init || !rigid12_out || !scale_out) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_calib: NULL init or output");
    if (!(scale_init > 0.0) || !std::isfinite(scale_init)) return fail(h, IBA_ERR_INVALID_ARG, "iba_icp_calib: scale_init must be positive and finite");
    double T0[16]; iba::icp::init_from_sim3(rigid12_init, scale_init, T0);
    if (ref_lidar_pose12) { double Tr[16]; iba::icp::rigid12_mul_T16(ref_lidar_pose12, T0, Tr); std::memcpy(T0, Tr, sizeof(T0)); }   // the queries move, the scans stay
    iba_icp_result r;
    if (const iba_status s = iba_icp_register(h, frame_begin, frame_end, cam_xyz, n, T0, 1, opt, &r)) return s;
    if (ref_lidar_pose12) { double inv[12], Tr[16]; iba::icp::inv_rigid12(ref_lidar_pose12, inv); iba::icp::rigid12_mul_T16(inv, r.T, Tr); std::memcpy(r.T, Tr, sizeof(Tr)); r.scale = iba::icp::scale_of(r.T); }
    iba::icp::sim3_from_result(r.T, rigid12_out, scale_out);
    if (res) *res = r;
    return IBA_OK;
}

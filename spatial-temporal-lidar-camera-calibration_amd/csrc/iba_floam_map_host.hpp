// Host side of iba_floam_map_step / iba_floam_map_register (include/iba_mi355x.h; included at the end of iba_capi.hip, after iba_icp_host.hpp
// and iba_scan_host.hpp whose checks it shares). A pair is two jobs (edge, surf) of the flat grids of iba_floam_map_kernels.hpp. An association =
// the jobs copied to the device from pinned memory, iba_floam_nn5_kernel, iba_floam_eval_kernel, iba_floam_sum_kernel, the moments copied back, ONE
// stream synchronise for all pairs (PassWork, iba_flat_pass.hpp); an LM trial = the same without the search, on the records the association left on
// the device. 272 B down and 272 B up per pair and evaluation, nothing of cloud size unless the caller asks for nn_idx / records.

namespace {

constexpr int kFloamMapMaxB = 4096;

struct FloamMapState {   // one pair of iba_floam_map_register
    double T[16], H[36], g[6], cost = 0.0;
    iba::LmStep<6> lm;                // the trust-region solve of the current association
    double Tn[16], xn2 = 0.0;         // the trial in flight
    bool enabled = false, finished = false, inner = false;
};

// "" when the options are inside the supported range; otherwise the message, as iba_floam_map_* word it under the name `w`
std::string fmap_options_error(const iba_floam_map_options* o, const std::string& w) {
    if (!o) return w + ": options are NULL (iba_default_floam_map_options fills them)";
    if (o->struct_size != (int32_t)sizeof(iba_floam_map_options)) return "iba_floam_map_options.struct_size does not match this library";
    if (o->k != 5) return w + ": k = " + std::to_string(o->k) + " neighbours are not supported (5 is the only value)";
    const double th[5] = {o->max_nn_dist2, o->edge_eig_ratio, o->edge_half_len, o->plane_max_resid, o->huber_delta};
    for (double v : th) if (!std::isfinite(v) || v < 0.0) return "iba_floam_map_options: max_nn_dist2, edge_eig_ratio, edge_half_len, plane_max_resid and huber_delta must be finite and not negative";
    if (o->outer_passes < 0 || o->inner_iterations < 0 || o->min_map_edge < 0 || o->min_map_surf < 0)
        return "iba_floam_map_options: outer_passes, inner_iterations, min_map_edge and min_map_surf must not be negative";
    return "";
}

iba_status fmap_check(iba_handle* h, const iba_floam_pair* pairs, int32_t B, const iba_floam_map_options* o, const char* who) {
    const std::string w(who);
    if (!pairs) return fail(h, IBA_ERR_INVALID_ARG, w + ": pairs are NULL");
    const std::string bad = fmap_options_error(o, w);
    if (!bad.empty() && (!o || o->struct_size != (int32_t)sizeof(iba_floam_map_options))) return fail(h, IBA_ERR_INVALID_ARG, bad);
    if (B < 1 || B > kFloamMapMaxB) return fail(h, IBA_ERR_INVALID_ARG, w + ": B must be in [1, 4096]");
    if (!bad.empty()) return fail(h, IBA_ERR_INVALID_ARG, bad);
    for (int b = 0; b < B; ++b) {
        const iba_floam_pair& p = pairs[b];
        const int32_t fr[4] = {p.src_edge_frame, p.src_surf_frame, p.map_edge_frame, p.map_surf_frame};
        for (int32_t f : fr)
            if (f < 0 || f >= h->n_frames) return fail(h, IBA_ERR_INVALID_ARG, w + ": pair " + std::to_string(b) + " names frame " + std::to_string(f) + " outside the handle's " + std::to_string(h->n_frames) + " local frames");
        if (!icp_finite16(p.T)) return fail(h, IBA_ERR_INVALID_ARG, w + ": the transform of pair " + std::to_string(b) + " is not finite");
    }
    return IBA_OK;
}

bool fmap_enabled(const iba_handle* h, const iba_floam_pair& p, const iba_floam_map_options& o) {
    return (int64_t)h->h_frames[(size_t)p.map_edge_frame].P > (int64_t)o.min_map_edge && (int64_t)h->h_frames[(size_t)p.map_surf_frame].P > (int64_t)o.min_map_surf;
}

iba_status fmap_reserve(iba_handle* h, int nb) {
    HIP_TRY(h, h->fmap.reserve(2 * (size_t)nb, (size_t)nb * kFloamMom));
    return IBA_OK;
}

// jobs 2 k, 2 k + 1 of the launch = pair lv[k] at Ts + 16 k; rec0[b] = the first record of pair b in the call's record buffer
void fmap_stage(iba_handle* h, const iba_floam_pair* pairs, const iba_floam_map_options& o, const std::vector<int>& lv, const double* Ts, const std::vector<uint64_t>& rec0) {
    auto& w = h->fmap;
    for (size_t k = 0; k < lv.size(); ++k) {
        const iba_floam_pair& p = pairs[lv[k]];
        const bool en = fmap_enabled(h, p, o);
        for (int s = 0; s < 2; ++s) {
            FloamJob& j = w.h_item.p[2 * k + (size_t)s];
            std::memcpy(j.T, Ts + 16 * k, 12 * sizeof(double));
            j.src = s ? p.src_surf_frame : p.src_edge_frame; j.map = s ? p.map_surf_frame : p.map_edge_frame;
            j.kind = s + 1; j.enabled = en ? 1 : 0; j.pad = 0;
            j.rec0 = rec0[(size_t)lv[k]] + (s ? (uint64_t)h->h_frames[(size_t)p.src_edge_frame].P : 0ull);
        }
    }
}

// One evaluation of the nb pairs staged in h->fmap.h_item: search (the records are rewritten) when `search`, then the sums at the staged poses
// on the records in place; the moments land in h->fmap.h_mom.
iba_status fmap_pass(iba_handle* h, int nb, const iba_floam_map_options& o, bool search, bool want_nn) {
    auto& w = h->fmap;
    const hipStream_t st = h->stream;
    const int nj = 2 * nb;
    uint32_t nodes = 1;
    for (int k = 0; k < nj; ++k) nodes = std::max(nodes, tree_nodes(h->h_frames[(size_t)w.h_item.p[k].map]));
    const PassShape sh = pass_shape(nodes);
    constexpr int kEvThreads = 256;
    uint64_t bn = 0, be = 0, chunks = 0;
    for (int k = 0; k < nj; ++k) {
        FloamJob& j = w.h_item.p[k];
        const uint32_t P = h->h_frames[(size_t)j.src].P;
        j.blk_nn = flat_take(bn, P, sh.threads); j.blk_ev = flat_take(be, P, kEvThreads); j.part0 = flat_take(chunks, P, 64);
    }
    if (bn > 0x7FFFFFFFull || chunks > 0x7FFFFFFFull) return fail(h, IBA_ERR_UNSUPPORTED, "iba_floam_map: the batch needs more blocks than one launch takes");
    HIP_TRY(h, w.d_part.grow((size_t)chunks * kFloamSums));
    HIP_TRY(h, w.upload((size_t)nj, st));
    const FloamFit fit{o.max_nn_dist2, o.edge_eig_ratio, o.edge_half_len, o.plane_max_resid, o.huber_delta};
    if (search && bn > 0) {
        const auto kernel = sh.threads == 64 ? iba_floam_nn5_kernel<64> : iba_floam_nn5_kernel<256>;
        hipLaunchKernelGGL(kernel, dim3((unsigned)bn), dim3((unsigned)sh.threads), sh.lds, st, h->dev_problem(), h->d_frame_box.p, w.d_item.p, nj, fit, w.d_rec.p, want_nn ? w.d_nn.p : nullptr);
        HIP_TRY(h, hipGetLastError());
    }
    if (be > 0) {
        hipLaunchKernelGGL(iba_floam_eval_kernel<kEvThreads>, dim3((unsigned)be), dim3(kEvThreads), 0, st, h->dev_problem(), w.d_item.p, nj, o.huber_delta, w.d_rec.p, w.d_part.p);
        HIP_TRY(h, hipGetLastError());
    }
    hipLaunchKernelGGL(iba_floam_sum_kernel, dim3((unsigned)nb), dim3(256), 0, st, h->dev_problem(), w.d_part.p, w.d_item.p, w.d_mom.p);
    HIP_TRY(h, w.finish(kFloamMom * (size_t)nb, st));
    return IBA_OK;
}

// the first record of every pair (edge cloud, then surf cloud) and their total
uint64_t fmap_offsets(const iba_handle* h, const iba_floam_pair* pairs, int32_t B, std::vector<uint64_t>& rec0) {
    rec0.assign((size_t)B + 1, 0);
    for (int b = 0; b < B; ++b) rec0[(size_t)b + 1] = rec0[(size_t)b] + h->h_frames[(size_t)pairs[b].src_edge_frame].P + h->h_frames[(size_t)pairs[b].src_surf_frame].P;
    return rec0[(size_t)B];
}

// the reference's Plus (lidarOptimization.cpp getTransformFromSe3): Exp(delta) as a row-major 4x4, delta = [omega, upsilon]
void fmap_exp(const double* d, double* E) {
    const double ox = d[0], oy = d[1], oz = d[2];
    const double theta = std::sqrt((ox * ox + oy * oy) + oz * oz), half = 0.5 * theta;
    const bool small = theta < 1e-10;
    double imag;
    const double real = std::cos(half);
    if (small) { const double t2 = theta * theta, t4 = t2 * t2; imag = 0.5 - 0.0208333 * t2 + 0.000260417 * t4; }
    else imag = std::sin(half) / theta;
    const double qw = real, qx = imag * ox, qy = imag * oy, qz = imag * oz;
    // Eigen's Quaternion::toRotationMatrix
    const double tx = 2.0 * qx, ty = 2.0 * qy, tz = 2.0 * qz;
    const double twx = tx * qw, twy = ty * qw, twz = tz * qw, txx = tx * qx, txy = ty * qx, txz = tz * qx, tyy = ty * qy, tyz = tz * qy, tzz = tz * qz;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    double J[9];
    if (small) std::memcpy(J, R, sizeof(J));
    else {
        const double O[9] = {0.0, -oz, oy, oz, 0.0, -ox, -oy, ox, 0.0};
        double O2[9]; iba::la3::mat3_mul(O, O, O2);
        const double a = (1.0 - std::cos(theta)) / (theta * theta), b = (theta - std::sin(theta)) / (theta * theta * theta);
        for (int i = 0; i < 9; ++i) J[i] = ((i % 4 == 0 ? 1.0 : 0.0) + a * O[i]) + b * O2[i];
    }
    double t[3]; iba::la3::mat3_vec(J, d + 3, t);
    for (int r = 0; r < 3; ++r) { for (int c = 0; c < 3; ++c) E[r * 4 + c] = R[r * 3 + c]; E[r * 4 + 3] = t[r]; }
    E[12] = 0.0; E[13] = 0.0; E[14] = 0.0; E[15] = 1.0;
}

void fmap_unpack(const double* m, double* H, double* g, double& cost) {
    int o = 4;
    for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) { H[i * 6 + j] = m[o]; H[j * 6 + i] = m[o]; ++o; }
    for (int i = 0; i < 6; ++i) g[i] = m[25 + i];
    cost = 0.5 * m[31];
}

}  // namespace

iba_status iba_default_floam_map_options(iba_floam_map_options* o) {
    if (!o) return IBA_ERR_INVALID_ARG;
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(iba_floam_map_options);
    o->k = 5;
    o->max_nn_dist2 = 1.0; o->edge_eig_ratio = 3.0; o->edge_half_len = 0.1; o->plane_max_resid = 0.2; o->huber_delta = 0.1;
    o->outer_passes = 2; o->inner_iterations = 4; o->min_map_edge = 10; o->min_map_surf = 50;
    return IBA_OK;
}

iba_status iba_floam_map_step(iba_handle* h, const iba_floam_pair* pairs, int32_t B, const iba_floam_map_options* o, double* moments, uint32_t* nn_idx, iba_floam_record* records) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!moments) return fail(h, IBA_ERR_INVALID_ARG, "iba_floam_map_step: moments are NULL");
    if (const iba_status s = fmap_check(h, pairs, B, o, "iba_floam_map_step")) return s;
    static_assert(sizeof(iba_floam_record) == sizeof(FloamRec), "the public record is the device record");
    std::vector<uint64_t> rec0;
    const uint64_t n_rec = fmap_offsets(h, pairs, B, rec0);
    HIP_TRY(h, hipSetDevice(h->device));
    if (const iba_status s = fmap_reserve(h, B)) return s;
    auto& w = h->fmap;
    HIP_TRY(h, w.d_rec.grow((size_t)n_rec));
    if (nn_idx) HIP_TRY(h, w.d_nn.grow(5 * (size_t)n_rec));
    std::vector<int> lv((size_t)B);
    std::vector<double> Ts(16 * (size_t)B);
    for (int b = 0; b < B; ++b) { lv[(size_t)b] = b; std::memcpy(&Ts[16 * (size_t)b], pairs[b].T, 16 * sizeof(double)); }
    fmap_stage(h, pairs, *o, lv, Ts.data(), rec0);
    if (const iba_status s = fmap_pass(h, B, *o, true, nn_idx != nullptr)) return s;
    std::memcpy(moments, w.h_mom.p, sizeof(double) * kFloamMom * (size_t)B);
    if (nn_idx && n_rec) HIP_TRY(h, hipMemcpy(nn_idx, w.d_nn.p, sizeof(uint32_t) * 5 * (size_t)n_rec, hipMemcpyDeviceToHost));
    if (records && n_rec) HIP_TRY(h, hipMemcpy(records, w.d_rec.p, sizeof(FloamRec) * (size_t)n_rec, hipMemcpyDeviceToHost));
    return IBA_OK;
}

iba_status iba_floam_map_register(iba_handle* h, const iba_floam_pair* pairs, int32_t B, const iba_floam_map_options* o, iba_floam_map_result* out) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, "iba_floam_map_register: results are NULL");
    if (const iba_status s = fmap_check(h, pairs, B, o, "iba_floam_map_register")) return s;
    const iba::LmOptions lm;   // the trust-region rules of iba_lm.hpp
    const auto ldlt = [](const double* A, const double* rhs, double* x) {   // false: a pivot or a step that is not positive and finite (the pair is degenerate)
        double L[36] = {0.0}, dd[6];
        bool ok = iba::icp::ldlt6_factor(A, L, dd);
        if (ok) { iba::icp::ldlt6_apply(L, dd, rhs, x); for (int i = 0; i < 6; ++i) ok = ok && std::isfinite(x[i]); }
        return ok;
    };
    std::vector<uint64_t> rec0;
    const uint64_t n_rec = fmap_offsets(h, pairs, B, rec0);
    std::vector<FloamMapState> st((size_t)B);
    std::memset(out, 0, sizeof(iba_floam_map_result) * (size_t)B);
    std::vector<int> run;
    for (int b = 0; b < B; ++b) {
        FloamMapState& s = st[(size_t)b];
        std::memcpy(s.T, pairs[b].T, sizeof(s.T));
        s.enabled = fmap_enabled(h, pairs[b], *o);
        s.finished = !s.enabled;
        out[b].status = s.enabled ? IBA_FLOAM_MAP_OK : IBA_FLOAM_MAP_DEGENERATE;
        if (s.enabled) run.push_back(b);
    }
    if (!run.empty() && o->outer_passes > 0) {
        HIP_TRY(h, hipSetDevice(h->device));
        if (const iba_status s = fmap_reserve(h, (int)run.size())) return s;
        HIP_TRY(h, h->fmap.d_rec.grow((size_t)n_rec));
    }
    auto& w = h->fmap;
    std::vector<int> lv;
    std::vector<double> Ts;
    for (int pass = 0; pass < o->outer_passes; ++pass) {
        lv.clear(); Ts.clear();
        for (int b : run) if (!st[(size_t)b].finished) { lv.push_back(b); Ts.insert(Ts.end(), st[(size_t)b].T, st[(size_t)b].T + 16); }
        if (lv.empty()) break;
        fmap_stage(h, pairs, *o, lv, Ts.data(), rec0);
        if (const iba_status s = fmap_pass(h, (int)lv.size(), *o, true, false)) return s;
        for (size_t k = 0; k < lv.size(); ++k) {   // the association of this pass and the problem it builds
            FloamMapState& s = st[(size_t)lv[k]];
            iba_floam_map_result& r = out[lv[k]];
            const double* m = w.h_mom.p + (size_t)kFloamMom * k;
            fmap_unpack(m, s.H, s.g, s.cost);
            ++r.passes; ++r.evaluations;
            r.n_edge = (int32_t)m[1]; r.n_surf = (int32_t)m[3];
            if (pass == 0) r.initial_cost = s.cost;
            r.final_cost = s.cost;
            s.inner = true;
            if (m[1] + m[3] < 6.0) { s.finished = true; s.inner = false; r.status = IBA_FLOAM_MAP_DEGENERATE; continue; }
            s.lm.begin(lm, s.H);
        }
        for (int it = 0; it < o->inner_iterations; ++it) {
            std::vector<int> tv; std::vector<double> Tt;
            bool any = false;
            for (int b : lv) {
                FloamMapState& s = st[(size_t)b];
                if (!s.inner) continue;
                any = true;
                ++out[b].iterations;
                const iba::LmProposal next = s.lm.propose(lm, s.H, s.g, ldlt);
                if (next == iba::LmProposal::kNoSolve) { s.inner = false; s.finished = true; out[b].status = IBA_FLOAM_MAP_DEGENERATE; continue; }
                if (next == iba::LmProposal::kStop) s.inner = false;
                if (next != iba::LmProposal::kTrial) continue;
                s.xn2 = 1.0 + ((s.T[3] * s.T[3] + s.T[7] * s.T[7]) + s.T[11] * s.T[11]);   // |(unit quaternion, translation)|^2 of the current pose
                double E[16];
                fmap_exp(s.lm.delta, E);
                iba::icp::mat4_mul(E, s.T, s.Tn);
                s.Tn[12] = 0.0; s.Tn[13] = 0.0; s.Tn[14] = 0.0; s.Tn[15] = 1.0;
                tv.push_back(b); Tt.insert(Tt.end(), s.Tn, s.Tn + 16);
            }
            if (!any) break;
            if (tv.empty()) continue;
            fmap_stage(h, pairs, *o, tv, Tt.data(), rec0);
            if (const iba_status s = fmap_pass(h, (int)tv.size(), *o, false, false)) return s;
            for (size_t k = 0; k < tv.size(); ++k) {
                FloamMapState& s = st[(size_t)tv[k]];
                double Hn[36], gn[6], cn;
                fmap_unpack(w.h_mom.p + (size_t)kFloamMom * k, Hn, gn, cn);
                ++out[tv[k]].evaluations;
                const iba::LmVerdict verdict = s.lm.judge(lm, s.cost, cn, s.xn2);
                if (verdict == iba::LmVerdict::kStop) s.inner = false;
                if (verdict == iba::LmVerdict::kAccept) { std::memcpy(s.T, s.Tn, sizeof(s.T)); std::memcpy(s.H, Hn, sizeof(Hn)); std::memcpy(s.g, gn, sizeof(gn)); s.cost = cn; }
            }
        }
        for (int b : lv) { st[(size_t)b].inner = false; out[b].final_cost = st[(size_t)b].cost; }
    }
    for (int b = 0; b < B; ++b) std::memcpy(out[b].T, st[(size_t)b].T, sizeof(out[b].T));
    return IBA_OK;
}

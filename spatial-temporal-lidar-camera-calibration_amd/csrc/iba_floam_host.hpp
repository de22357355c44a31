// Host side of iba_floam_extract (include/iba_mi355x.h; included at the end of iba_capi.hip, after iba_voxel_host.hpp whose rocPRIM include and
// vox_bits it shares). One call = one launch chain for the whole batch of scans (iba_floam_kernels.hpp) with three synchronisations: after the
// classification and the partition (the ring sizes come up, 272 B per scan: rule 3 is checked and the sectors are listed on the host), after the
// scans of the sector counts (the outputs are sized) and at the end. Down go the scan, block and sector lists (16 + 8 B per 256 points, 16 B per
// sector); up come the ring sizes, the offsets per sector and the two clouds. The work buffers belong to the call. floam_extract_impl is the
// same chain with the clouds left on the device for iba_floam_odom_run (iba_floam_odom_host.hpp).
#include <rocprim/device/device_radix_sort.hpp>

struct iba_floam_features {
    int32_t n = 0, lines = 0;
    std::vector<int64_t> efirst, sfirst;      // n + 1: scan s owns the edge / surf points first[s] .. first[s + 1]
    std::vector<float> exyz, sxyz;            // 3 per point
    std::vector<int32_t> eidx, sidx;          // original index in the scan
    std::vector<int64_t> stats;               // 3 per scan: non-finite, out of range, no ring
    std::vector<int32_t> ring_points;         // lines per scan
};

namespace {

constexpr int kFloamMaxScans = 1 << 20;
constexpr uint64_t kFloamMaxPoints = 0xFFFFFF00ull;   // points of one call: a sorted position is a 32-bit value

// "" when the options are inside the supported range
std::string floam_check_options(const iba_floam_options* o) {
    if (!o) return "the options are NULL";
    if (o->struct_size != (int32_t)sizeof(iba_floam_options)) return "iba_floam_options.struct_size does not match this library";
    if (o->num_lines != 16 && o->num_lines != 32 && o->num_lines != 64) return "num_lines must be 16, 32 or 64";
    if (!std::isfinite(o->min_distance) || !std::isfinite(o->max_distance)) return "min_distance / max_distance are not finite";
    if (o->min_distance > o->max_distance) return "min_distance is above max_distance";
    if (o->min_ring_points < 11) return "min_ring_points must be at least 11";
    if (o->num_sectors < 1 || o->num_sectors > 64) return "num_sectors must be in [1, 64]";
    if (o->max_edges_per_sector < 0 || o->max_edges_per_sector > 64) return "max_edges_per_sector must be in [0, 64]";
    if (o->neighbour_span != kFloamSpan) return "neighbour_span must be 5: the curvature window is written for that span alone";
    if (!std::isfinite(o->edge_curvature) || !std::isfinite(o->neighbour_gap2)) return "edge_curvature / neighbour_gap2 are not finite";
    return "";
}

}  // namespace

iba_status iba_default_floam_options(iba_floam_options* o) {
    if (!o) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_default_floam_options: the options are NULL");
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->num_lines = 64; o->min_distance = 3.0; o->max_distance = 90.0; o->min_ring_points = 131; o->num_sectors = 6; o->max_edges_per_sector = 20;
    o->neighbour_span = kFloamSpan; o->edge_curvature = 0.1; o->neighbour_gap2 = 0.05;
    return IBA_OK;
}

namespace {

struct FloamDevClouds { DevBuf<float> exyz, sxyz; };   // the gathered clouds of a call, left on the device (efirst / sfirst of the result index them)

// iba_floam_extract. keep != NULL (iba_floam_odom_run): the two clouds stay on the device in *keep and are NOT downloaded — the result then holds
// the counts, first positions and statistics only, its xyz / index arrays are empty. `who` heads the messages.
iba_status floam_extract_impl(iba_handle* h, const int32_t* frames, int32_t n, const iba_floam_options* opt, const std::string& who, FloamDevClouds* keep, iba_floam_features** out) {
    if (!h) return fail(nullptr, IBA_ERR_INVALID_ARG, who + "the handle is NULL");
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, who + "the result pointer is NULL");
    *out = nullptr;
    if (!frames) return fail(h, IBA_ERR_INVALID_ARG, who + "frames is NULL");
    const std::string bad = floam_check_options(opt);
    if (!bad.empty()) return fail(h, IBA_ERR_INVALID_ARG, who + bad);
    if (n < 1 || n > kFloamMaxScans) return fail(h, IBA_ERR_INVALID_ARG, who + "n must be in [1, 2^20]");
    std::vector<FloamScan> scans((size_t)n);
    std::vector<FloamBlock> blocks;
    uint64_t N = 0;
    for (int32_t i = 0; i < n; ++i) {
        if (frames[i] < 0 || frames[i] >= h->n_frames)
            return fail(h, IBA_ERR_INVALID_ARG, who + "scan " + std::to_string(i) + " names frame " + std::to_string(frames[i]) + " outside the handle's " + std::to_string(h->n_frames) + " local frames");
        const uint32_t P = h->h_frames[(size_t)frames[i]].P;
        scans[(size_t)i] = FloamScan{N, frames[i], 0};
        for (uint64_t b = 0; b < P; b += (uint64_t)kFloamThreads) blocks.push_back(FloamBlock{i, (uint32_t)b});
        N += P;
        if (N > kFloamMaxPoints) return fail(h, IBA_ERR_UNSUPPORTED, who + "the scans of one call hold more than 2^32 - 256 points (split the batch)");
    }
    const int lines = opt->num_lines, S = opt->num_sectors;
    const uint32_t eslots = (uint32_t)std::max(opt->max_edges_per_sector, 1);
    std::unique_ptr<iba_floam_features> res(new iba_floam_features);   // (freed on every error path below)
    res->n = n; res->lines = lines;
    res->efirst.assign((size_t)n + 1, 0); res->sfirst.assign((size_t)n + 1, 0); res->stats.assign(3 * (size_t)n, 0); res->ring_points.assign((size_t)n * (size_t)lines, 0);
    if (N == 0) { *out = res.release(); return IBA_OK; }   // every scan is empty: no launch

    const FloamShape sh{opt->min_distance, opt->max_distance, opt->edge_curvature, opt->neighbour_gap2, lines, opt->max_edges_per_sector};
    HIP_TRY(h, hipSetDevice(h->device));
    const hipStream_t st = h->stream;
    DevBuf<FloamScan> d_scans; DevBuf<FloamBlock> d_blocks; DevBuf<FloamTask> d_tasks; DevBuf<uint32_t> d_counts, d_key[2], d_val[2], d_epos, d_spos, d_ne, d_ns; DevBuf<unsigned char> d_tmp;
    DevBuf<float4> d_rp; DevBuf<float> d_exyz, d_sxyz; DevBuf<int32_t> d_eidx, d_sidx;

    // ---- rules 1-2 and the stable partition by (scan, ring) ----
    HIP_TRY(h, d_scans.alloc((size_t)n)); HIP_TRY(h, d_blocks.alloc(blocks.size())); HIP_TRY(h, d_counts.alloc((size_t)n * kFloamBins));
    HIP_TRY(h, d_key[0].alloc((size_t)N)); HIP_TRY(h, d_key[1].alloc((size_t)N)); HIP_TRY(h, d_val[0].alloc((size_t)N)); HIP_TRY(h, d_val[1].alloc((size_t)N));
    HIP_TRY(h, hipMemcpyAsync(d_scans.p, scans.data(), sizeof(FloamScan) * (size_t)n, hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(d_blocks.p, blocks.data(), sizeof(FloamBlock) * blocks.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemsetAsync(d_counts.p, 0, sizeof(uint32_t) * (size_t)n * kFloamBins, st));
    hipLaunchKernelGGL(iba_floam_classify_kernel, dim3((unsigned)blocks.size()), dim3(kFloamThreads), 0, st, h->frames.p, h->pts4.p, h->inv_perm.p, d_scans.p, d_blocks.p, sh, d_key[0].p, d_val[0].p, d_counts.p);
    HIP_TRY(h, hipGetLastError());
    rocprim::double_buffer<uint32_t> kb(d_key[0].p, d_key[1].p), vb(d_val[0].p, d_val[1].p);
    const unsigned end_bit = (unsigned)vox_bits((uint64_t)n * kFloamKeys);
    size_t tmp_bytes = 0;
    HIP_TRY(h, rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)N, 0u, end_bit, st));
    HIP_TRY(h, d_tmp.alloc(tmp_bytes));
    HIP_TRY(h, rocprim::radix_sort_pairs((void*)d_tmp.p, tmp_bytes, kb, vb, (size_t)N, 0u, end_bit, st));
    std::vector<uint32_t> counts((size_t)n * kFloamBins);
    HIP_TRY(h, hipMemcpyAsync(counts.data(), d_counts.p, sizeof(uint32_t) * counts.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));

    // ---- rules 3 and 5: the sectors of every ring that is long enough ----
    std::vector<FloamTask> tasks;
    std::vector<uint32_t> task_first((size_t)n + 1, 0);
    uint64_t surf_slots = 0;
    uint32_t maxL = 0;
    for (int32_t i = 0; i < n; ++i) {
        const uint32_t* c = counts.data() + (size_t)i * kFloamBins;
        for (int k = 0; k < 3; ++k) res->stats[3 * (size_t)i + k] = (int64_t)c[64 + k];
        uint64_t base = scans[(size_t)i].pos0, seen = 0;
        task_first[(size_t)i] = (uint32_t)tasks.size();
        for (int r = 0; r < 64; ++r) {
            const uint32_t np = c[r];
            seen += np;
            if (r < lines) res->ring_points[(size_t)i * lines + r] = (int32_t)np;
            if (np > (uint32_t)kFloamMaxRing)
                return fail(h, IBA_ERR_UNSUPPORTED, who + "scan " + std::to_string(i) + " (frame " + std::to_string(frames[i]) + "), ring " + std::to_string(r) + " holds " + std::to_string(np) +
                                                        " points; a ring list holds at most " + std::to_string(kFloamMaxRing) + " (IBA_FLOAM_MAX_RING_POINTS)");
            if (np >= (uint32_t)opt->min_ring_points) {
                const uint32_t total = np - 10u, len = total / (uint32_t)S;
                for (int s = 0; s < S; ++s) {
                    const uint32_t lo = len * (uint32_t)s;
                    const int64_t hi = s < S - 1 ? (int64_t)len * (s + 1) - 1 : (int64_t)total - 1;
                    if (hi <= (int64_t)lo) continue;                                   // a sector with no entries
                    tasks.push_back(FloamTask{(uint32_t)base, lo, (uint32_t)(hi - lo), (uint32_t)surf_slots});
                    surf_slots += (uint64_t)(hi - lo);
                    maxL = std::max(maxL, (uint32_t)(hi - lo));
                }
            }
            base += np;
        }
        const uint64_t all = seen + c[64] + c[65] + c[66];
        if (all != h->h_frames[(size_t)frames[i]].P) return fail(h, IBA_ERR_HIP, who + "the ring sizes of scan " + std::to_string(i) + " do not add up to its points");
    }
    task_first[(size_t)n] = (uint32_t)tasks.size();
    const size_t T = tasks.size();
    if (T == 0) { *out = res.release(); return IBA_OK; }   // no ring reaches min_ring_points
    if ((uint64_t)T * eslots > 0xFFFFFFFFull) return fail(h, IBA_ERR_UNSUPPORTED, who + "more than 2^32 edge slots in one call (split the batch)");

    // ---- rules 4-8 per sector, then the counts scanned ----
    const uint32_t Pmax = floam_pow2(maxL);
    const size_t lds = floam_sector_lds(Pmax);
    if (lds > 65536) HIP_TRY(h, hipFuncSetAttribute((const void*)iba_floam_sector_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    HIP_TRY(h, d_tasks.alloc(T)); HIP_TRY(h, d_rp.alloc((size_t)N)); HIP_TRY(h, d_epos.alloc(T * eslots)); HIP_TRY(h, d_spos.alloc((size_t)surf_slots));
    HIP_TRY(h, d_ne.alloc(T + 1)); HIP_TRY(h, d_ns.alloc(T + 1));
    HIP_TRY(h, hipMemcpyAsync(d_tasks.p, tasks.data(), sizeof(FloamTask) * T, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(iba_floam_ring_points_kernel, dim3((unsigned)((N + kFloamThreads - 1) / kFloamThreads)), dim3(kFloamThreads), 0, st, h->frames.p, h->pts4.p, h->inv_perm.p, d_scans.p, kb.current(),
                       vb.current(), N, d_rp.p);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_floam_sector_kernel, dim3((unsigned)T), dim3(kFloamThreads), lds, st, d_tasks.p, d_rp.p, sh, Pmax, d_epos.p, d_spos.p, d_ne.p, d_ns.p);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_vox_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, d_ne.p, (uint32_t)T, d_ne.p + T);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_vox_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, d_ns.p, (uint32_t)T, d_ns.p + T);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> eoff(T + 1), soff(T + 1);
    HIP_TRY(h, hipMemcpyAsync(eoff.data(), d_ne.p, sizeof(uint32_t) * (T + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipMemcpyAsync(soff.data(), d_ns.p, sizeof(uint32_t) * (T + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    const size_t NE = eoff[T], NS = soff[T];
    if (NE > T * eslots || NS > surf_slots) return fail(h, IBA_ERR_HIP, who + "the sector counts came back larger than their slots");

    // ---- rule 9: the two clouds in their final order ----
    HIP_TRY(h, d_exyz.alloc(3 * NE)); HIP_TRY(h, d_eidx.alloc(NE)); HIP_TRY(h, d_sxyz.alloc(3 * NS)); HIP_TRY(h, d_sidx.alloc(NS));
    hipLaunchKernelGGL(iba_floam_gather_kernel, dim3((unsigned)T), dim3(kFloamThreads), 0, st, d_tasks.p, d_rp.p, opt->max_edges_per_sector, d_epos.p, d_spos.p, d_ne.p, d_ns.p, d_exyz.p, d_eidx.p, d_sxyz.p,
                       d_sidx.p);
    HIP_TRY(h, hipGetLastError());
    if (!keep) { res->exyz.resize(3 * NE); res->eidx.resize(NE); res->sxyz.resize(3 * NS); res->sidx.resize(NS); }
    if (NE && !keep) {
        HIP_TRY(h, hipMemcpyAsync(res->exyz.data(), d_exyz.p, sizeof(float) * 3 * NE, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(res->eidx.data(), d_eidx.p, sizeof(int32_t) * NE, hipMemcpyDeviceToHost, st));
    }
    if (NS && !keep) {
        HIP_TRY(h, hipMemcpyAsync(res->sxyz.data(), d_sxyz.p, sizeof(float) * 3 * NS, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(res->sidx.data(), d_sidx.p, sizeof(int32_t) * NS, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipStreamSynchronize(st));
    for (int32_t i = 0; i <= n; ++i) { res->efirst[(size_t)i] = (int64_t)eoff[task_first[(size_t)i]]; res->sfirst[(size_t)i] = (int64_t)soff[task_first[(size_t)i]]; }
    if (keep) { keep->exyz = std::move(d_exyz); keep->sxyz = std::move(d_sxyz); }
    *out = res.release();
    return IBA_OK;
}

}  // namespace

iba_status iba_floam_extract(iba_handle* h, const int32_t* frames, int32_t n, const iba_floam_options* opt, iba_floam_features** out) {
    return floam_extract_impl(h, frames, n, opt, "iba_floam_extract: ", nullptr, out);
}

int32_t iba_floam_num(const iba_floam_features* f) { return f ? f->n : 0; }
int64_t iba_floam_n_edge(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->efirst[(size_t)s + 1] - f->efirst[(size_t)s] : -1; }
int64_t iba_floam_n_surf(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->sfirst[(size_t)s + 1] - f->sfirst[(size_t)s] : -1; }
const float* iba_floam_edge_xyz(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->exyz.data() + 3 * (size_t)f->efirst[(size_t)s] : nullptr; }
const int32_t* iba_floam_edge_index(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->eidx.data() + (size_t)f->efirst[(size_t)s] : nullptr; }
const float* iba_floam_surf_xyz(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->sxyz.data() + 3 * (size_t)f->sfirst[(size_t)s] : nullptr; }
const int32_t* iba_floam_surf_index(const iba_floam_features* f, int32_t s) { return (f && s >= 0 && s < f->n) ? f->sidx.data() + (size_t)f->sfirst[(size_t)s] : nullptr; }
iba_status iba_floam_stats(const iba_floam_features* f, int32_t s, int64_t* n_nonfinite, int64_t* n_out_of_range, int64_t* n_no_ring, int32_t* ring_points) {
    if (!f) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_floam_stats: the result is NULL");
    if (s < 0 || s >= f->n) return fail(nullptr, IBA_ERR_INVALID_ARG, "iba_floam_stats: scan " + std::to_string(s) + " is outside the result's " + std::to_string(f->n));
    if (n_nonfinite) *n_nonfinite = f->stats[3 * (size_t)s];
    if (n_out_of_range) *n_out_of_range = f->stats[3 * (size_t)s + 1];
    if (n_no_ring) *n_no_ring = f->stats[3 * (size_t)s + 2];
    if (ring_points) std::memcpy(ring_points, f->ring_points.data() + (size_t)s * f->lines, sizeof(int32_t) * (size_t)f->lines);
    return IBA_OK;
}
void iba_floam_free(iba_floam_features* f) { delete f; }

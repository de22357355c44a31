// Host side of iba_submap_handle (include/iba_mi355x.h; included at the end of iba_capi.hip, after iba_voxel_host.hpp whose vox_build it runs) and
// of iba_debug_scan_index / iba_debug_build_tree (include/iba_mi355x_debug.h).
// One call = the voxel chain of iba_submap_build without its download, then create_impl (iba_capi.hip) with the scan side built on the device
// by index_build_device: one launch chain on the SOURCE handle's stream for all frames of the new handle (iba_index_kernels.hpp) — per tree
// level a segment kernel, rocPRIM's segmented radix sort and a split kernel (at most kMaxTreeDepth = 11 levels), then the sort inside the
// leaves, the gather and the boxes. Down go 32 B per frame, up come a flag word and 32 B of frame box per frame. The work buffers are of
// the size of the clouds and live for the call only (IdxScratch). The source of the build is any buffer of f64 triples on the device
// (ScanSource::xyz; NULL = the voxel chain's clouds): iba_floam_odom_run (iba_floam_odom_host.hpp) builds its handles through the same chain.
#include <rocprim/device/device_segmented_radix_sort.hpp>

namespace {

struct IdxScratch {
    DevBuf<IdxFrame> fr; DevBuf<float4> src4; DevBuf<uint32_t> order, order2, val, seg_begin, seg_end, seg_dim, flag; DevBuf<uint64_t> key, key_out; DevBuf<unsigned char> tmp;
};

#define IDX_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) { why = std::string("iba_submap_handle: ") + #expr + ": " + hipGetErrorString(_e); return IBA_ERR_HIP; } \
    } while (0)

iba_status index_build_device(iba_handle* dst, const ScanSource& from, std::string& why) {
    iba_handle* src = from.src;
    const int M = dst->n_frames;
    const std::vector<FrameHdr>& hdr = dst->h_frames;
    const float qnan = std::numeric_limits<float>::quiet_NaN();
    dst->h_frame_box.assign(8 * (size_t)std::max(M, 1), qnan);
    const uint64_t total = (uint64_t)dst->n_pt_total;   // padded positions of all frames
    if (total > 0xFFFFFF00ull) { why = "iba_submap_handle: the sub-maps of one call hold more than 2^32 - 256 voxels (split the batch)"; return IBA_ERR_UNSUPPORTED; }
    std::vector<IdxFrame> fr((size_t)std::max(M, 1));
    std::memset(fr.data(), 0, sizeof(IdxFrame) * fr.size());
    uint32_t dmax = 0, maxP = 0; uint64_t n_chunks = 0;
    for (int s = 0; s < M; ++s) {
        IdxFrame& x = fr[(size_t)s];
        x.pt_base = (uint32_t)hdr[s].pt_base; x.P = hdr[s].P; x.src_first = from.first[s]; x.depth = hdr[s].depth; x.node_base = hdr[s].node_base; x.box_base = (uint32_t)hdr[s].box_base;
        dmax = std::max(dmax, x.depth); maxP = std::max(maxP, x.P);
        n_chunks = hdr[s].box_base + (hdr[s].P + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
    }
    IDX_TRY(hipSetDevice(src->device));
    const hipStream_t st = src->stream;
    if (total == 0) {   // every frame is empty: nothing but the frame boxes (all NaN)
        IDX_TRY(hipMemcpyAsync(dst->d_frame_box.p, dst->h_frame_box.data(), sizeof(float) * dst->h_frame_box.size(), hipMemcpyHostToDevice, st));
        IDX_TRY(hipStreamSynchronize(st));
        return IBA_OK;
    }
    IdxScratch w;
    const uint32_t n_quads = (uint32_t)(total / 4u);
    const size_t max_seg = (size_t)M << dmax;   // segments of the deepest level's children = leaves
    IDX_TRY(w.fr.upload(fr));
    IDX_TRY(w.src4.alloc((size_t)total)); IDX_TRY(w.order.alloc((size_t)total)); IDX_TRY(w.flag.alloc(1));
    IDX_TRY(hipMemsetAsync(w.flag.p, 0, sizeof(uint32_t), st));
    auto blocks = [](uint64_t n, uint32_t per) { return dim3((unsigned)((n + per - 1) / per)); };
    hipLaunchKernelGGL(iba_idx_stage_kernel, blocks(n_quads, kIdxThreads), dim3(kIdxThreads), 0, st, w.fr.p, M, n_quads, from.xyz ? from.xyz : src->vox.d_xyz.p, w.src4.p, w.order.p, w.flag.p);
    IDX_TRY(hipGetLastError());
    const uint32_t* final_order = w.order.p;
    if (dmax > 0) {
        IDX_TRY(w.order2.alloc((size_t)total)); IDX_TRY(w.val.alloc((size_t)total)); IDX_TRY(w.key.alloc((size_t)total)); IDX_TRY(w.key_out.alloc((size_t)total));
        IDX_TRY(w.seg_begin.alloc(max_seg)); IDX_TRY(w.seg_end.alloc(max_seg)); IDX_TRY(w.seg_dim.alloc(max_seg));
        size_t tmp_bytes = 0;
        for (uint32_t d = 0; d <= dmax; ++d) {   // the largest temporary storage any of the sorts asks for (a host-side question)
            size_t b = 0;
            if (d < dmax) IDX_TRY(rocprim::segmented_radix_sort_pairs(nullptr, b, w.key.p, w.key_out.p, w.val.p, w.order.p, (unsigned)total, (unsigned)((size_t)M << d), w.seg_begin.p, w.seg_end.p, 0u, 32u + (unsigned)kIdxIndexBits, st));
            else IDX_TRY(rocprim::segmented_radix_sort_keys(nullptr, b, w.order.p, w.order2.p, (unsigned)total, (unsigned)max_seg, w.seg_begin.p, w.seg_end.p, 0u, (unsigned)kIdxIndexBits, st));
            tmp_bytes = std::max(tmp_bytes, b);
        }
        IDX_TRY(w.tmp.alloc(tmp_bytes));
        for (uint32_t d = 0; d < dmax; ++d) {
            const uint64_t n_seg = (uint64_t)M << d;
            if ((maxP >> d) >= 1024u)
                hipLaunchKernelGGL(iba_idx_segment_kernel<256>, blocks(n_seg, 1), dim3(kIdxThreads), 0, st, w.fr.p, M, (int)d, w.src4.p, w.order.p, w.key.p, w.val.p, w.seg_begin.p, w.seg_end.p, w.seg_dim.p, dst->nodes.p);
            else
                hipLaunchKernelGGL(iba_idx_segment_kernel<64>, blocks(n_seg, kIdxThreads / 64), dim3(kIdxThreads), 0, st, w.fr.p, M, (int)d, w.src4.p, w.order.p, w.key.p, w.val.p, w.seg_begin.p, w.seg_end.p, w.seg_dim.p, dst->nodes.p);
            IDX_TRY(hipGetLastError());
            size_t b = tmp_bytes;
            IDX_TRY(rocprim::segmented_radix_sort_pairs((void*)w.tmp.p, b, w.key.p, w.key_out.p, w.val.p, w.order.p, (unsigned)total, (unsigned)n_seg, w.seg_begin.p, w.seg_end.p, 0u, 32u + (unsigned)kIdxIndexBits, st));
            hipLaunchKernelGGL(iba_idx_split_kernel, blocks(n_seg, kIdxThreads), dim3(kIdxThreads), 0, st, w.fr.p, M, (int)d, w.src4.p, w.order.p, w.seg_dim.p, dst->nodes.p);
            IDX_TRY(hipGetLastError());
        }
        // ascending original index inside every leaf; the frames of depth 0 are copied as they are
        IDX_TRY(hipMemcpyAsync(w.order2.p, w.order.p, sizeof(uint32_t) * (size_t)total, hipMemcpyDeviceToDevice, st));
        hipLaunchKernelGGL(iba_idx_leaf_kernel, blocks(max_seg, kIdxThreads), dim3(kIdxThreads), 0, st, w.fr.p, M, (int)dmax, w.seg_begin.p, w.seg_end.p);
        IDX_TRY(hipGetLastError());
        size_t b = tmp_bytes;
        IDX_TRY(rocprim::segmented_radix_sort_keys((void*)w.tmp.p, b, w.order.p, w.order2.p, (unsigned)total, (unsigned)max_seg, w.seg_begin.p, w.seg_end.p, 0u, (unsigned)kIdxIndexBits, st));
        final_order = w.order2.p;
    }
    hipLaunchKernelGGL(iba_idx_gather_kernel, blocks(n_quads, kIdxThreads), dim3(kIdxThreads), 0, st, w.fr.p, M, n_quads, w.src4.p, final_order, dst->xs.p, dst->ys.p, dst->zs.p, dst->pts4.p, dst->perm.p, dst->inv_perm.p);
    IDX_TRY(hipGetLastError());
    hipLaunchKernelGGL(iba_idx_chunk_box_kernel, blocks(n_chunks, kIdxThreads / 64), dim3(kIdxThreads), 0, st, w.fr.p, M, (uint32_t)n_chunks, dst->xs.p, dst->ys.p, dst->zs.p, dst->chunk_box.p);
    IDX_TRY(hipGetLastError());
    hipLaunchKernelGGL(iba_idx_frame_box_kernel, dim3((unsigned)M), dim3(kIdxThreads), 0, st, w.fr.p, dst->chunk_box.p, dst->d_frame_box.p);
    IDX_TRY(hipGetLastError());
    uint32_t flag = 0;
    IDX_TRY(hipMemcpyAsync(&flag, w.flag.p, sizeof(flag), hipMemcpyDeviceToHost, st));
    IDX_TRY(hipMemcpyAsync(dst->h_frame_box.data(), dst->d_frame_box.p, sizeof(float) * 8 * (size_t)M, hipMemcpyDeviceToHost, st));
    IDX_TRY(hipStreamSynchronize(st));
    if (flag) { why = "iba_submap_handle: a voxel coordinate is not finite after narrowing to float32 (beyond 3.4e38: move the sub-map towards the origin with its output transform)"; return IBA_ERR_UNSUPPORTED; }
    return IBA_OK;
}
#undef IDX_TRY

}  // namespace

// A scans-only handle of M frames whose points are on src's device already, in xyz (3 doubles per point, narrowed to float32 by the stage kernel;
// NULL: src->vox.d_xyz). counts == NULL: the frames lie one after the other, frame s = the points first64[s] .. first64[s + 1] (M + 1 entries);
// otherwise frame s has counts[s] points from first64[s] on (iba_floam_odom_run: frames anywhere in a staging buffer). No keypoints, no covisibility,
// identity poses, the intrinsics of a KITTI camera (none of them is read by the scan-side entry points). The message is left in
// iba_last_error(src), headed by `who`; `what` names a frame in it.
iba_status scan_handle_from_device(iba_handle* src, const double* xyz, const std::vector<int64_t>& first64, const std::vector<int64_t>* counts, int32_t M, const iba_params* params, const std::string& who, const char* what,
                                   iba_handle** out) {
    std::vector<uint64_t> pt_off((size_t)M + 1, 0ull), zeros((size_t)M + 1, 0ull);
    std::vector<uint32_t> first((size_t)M + 1, 0u);
    for (int s = 0; s < M; ++s) {
        first[(size_t)s] = (uint32_t)first64[(size_t)s];
        pt_off[(size_t)s + 1] = pt_off[(size_t)s] + (uint64_t)(counts ? (*counts)[(size_t)s] : first64[(size_t)s + 1] - first64[(size_t)s]);
    }
    for (int s = 0; s < M; ++s)
        if (pt_off[(size_t)s + 1] - pt_off[(size_t)s] >= (1ull << 22))
            return fail(src, IBA_ERR_UNSUPPORTED, who + what + " " + std::to_string(s) + " has " + std::to_string(pt_off[(size_t)s + 1] - pt_off[(size_t)s]) + " voxels; a frame holds fewer than 2^22 points (choose a larger voxel)");
    const double intr[6] = {718.856, 718.856, 607.1928, 185.2157, 1241.0, 376.0};
    std::vector<double> intrinsics(6 * (size_t)M), Tl(12 * (size_t)M, 0.0);
    std::vector<float> T34(12 * (size_t)M, 0.f);
    for (int s = 0; s < M; ++s) {
        std::memcpy(&intrinsics[6 * (size_t)s], intr, sizeof(intr));
        for (int i = 0; i < 3; ++i) { T34[12 * (size_t)s + 5 * i] = 1.f; Tl[12 * (size_t)s + 5 * i] = 1.0; }
    }
    const uint64_t match_off[1] = {0};
    iba_problem_desc d;
    std::memset(&d, 0, sizeof(d));
    d.n_frames = M; d.pt_offset = pt_off.data(); d.pts_xyz = nullptr; d.intrinsics = intrinsics.data(); d.kp_offset = zeros.data(); d.covis_offset = zeros.data();
    d.match_offset = match_off; d.Tcw = T34.data(); d.Tc_next = T34.data(); d.Tl_next = Tl.data();
    const ScanSource from{src, first.data(), xyz};
    iba_handle* h = nullptr;
    const iba_status s = create_impl(&d, params, src->device, 0, M, nullptr, &from, &h);
    if (s != IBA_OK) return fail(src, s, g_create_error.rfind(who, 0) == 0 ? g_create_error : who + g_create_error);
    h->scans_only = true;
    *out = h;
    return IBA_OK;
}

iba_status iba_submap_handle(iba_handle* src, const iba_submap_desc* subs, int32_t M, const iba_params* params, iba_handle** out) {
    if (!src) return IBA_ERR_INVALID_ARG;
    const std::string who = "iba_submap_handle: ";
    if (!out) return fail(src, IBA_ERR_INVALID_ARG, who + "the result pointer is NULL");
    *out = nullptr;
    if (!params) return fail(src, IBA_ERR_INVALID_ARG, who + "the parameters are NULL");
    if (const iba_status s = check_params(src, *params)) return s;
    iba_submap_clouds* built = nullptr;
    if (const iba_status s = vox_build(src, subs, M, who, false, &built)) return s;
    const std::unique_ptr<iba_submap_clouds> c(built);
    return scan_handle_from_device(src, nullptr, c->first, nullptr, M, params, who, "sub-map", out);
}

int64_t iba_frame_num_points(const iba_handle* h, int32_t frame) { return (h && frame >= 0 && frame < h->n_frames) ? (int64_t)h->h_frames[(size_t)frame].P : -1; }

iba_status iba_debug_scan_index(iba_handle* h, int32_t frame, uint32_t* perm, float* xyz_tree, uint32_t* node_dim, float* node_split, float* chunk_box, float frame_box[8], int32_t* depth) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (frame < 0 || frame >= h->n_frames) return fail(h, IBA_ERR_INVALID_ARG, "iba_debug_scan_index: the frame is outside the handle's local frames");
    const FrameHdr& x = h->h_frames[(size_t)frame];
    HIP_TRY(h, hipSetDevice(h->device));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t P = x.P, nn = ((size_t)1 << x.depth) - 1, nc = (P + (size_t)kChunk - 1) / (size_t)kChunk;
    if (depth) *depth = (int32_t)x.depth;
    if (perm && P) HIP_TRY(h, hipMemcpy(perm, h->perm.p + x.pt_base, sizeof(uint32_t) * P, hipMemcpyDeviceToHost));
    if (xyz_tree && P) {
        HIP_TRY(h, hipMemcpy(xyz_tree, h->xs.p + x.pt_base, sizeof(float) * P, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(xyz_tree + P, h->ys.p + x.pt_base, sizeof(float) * P, hipMemcpyDeviceToHost));
        HIP_TRY(h, hipMemcpy(xyz_tree + 2 * P, h->zs.p + x.pt_base, sizeof(float) * P, hipMemcpyDeviceToHost));
    }
    if ((node_dim || node_split) && nn) {
        std::vector<TreeNode> nd(nn);
        HIP_TRY(h, hipMemcpy(nd.data(), h->nodes.p + x.node_base, sizeof(TreeNode) * nn, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < nn; ++i) { if (node_dim) node_dim[i] = nd[i].dim; if (node_split) node_split[i] = nd[i].split; }
    }
    if (chunk_box && nc) HIP_TRY(h, hipMemcpy(chunk_box, h->chunk_box.p + 8 * (size_t)x.box_base, sizeof(float) * 8 * nc, hipMemcpyDeviceToHost));
    if (frame_box) HIP_TRY(h, hipMemcpy(frame_box, h->d_frame_box.p + 8 * (size_t)frame, sizeof(float) * 8, hipMemcpyDeviceToHost));
    return IBA_OK;
}

// host only (no device is touched): build_tree of iba_build.hpp on n points, for the CPU tier's restatement of the rules
iba_status iba_debug_build_tree(const float* xyz, uint32_t P, uint32_t* perm, uint32_t* node_dim, float* node_split, int32_t* depth) {
    if ((!xyz && P) || P >= (1u << 22)) return IBA_ERR_INVALID_ARG;
    const uint32_t D = tree_depth_for(P);
    std::vector<uint32_t> idx; std::vector<TreeNode> nodes;
    build_tree(xyz, P, D, idx, nodes);
    if (depth) *depth = (int32_t)D;
    if (perm) std::copy(idx.begin(), idx.end(), perm);
    for (size_t i = 0; i < nodes.size(); ++i) { if (node_dim) node_dim[i] = nodes[i].dim; if (node_split) node_split[i] = nodes[i].split; }
    return IBA_OK;
}

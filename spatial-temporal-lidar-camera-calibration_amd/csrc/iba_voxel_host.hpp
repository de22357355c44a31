// Host side of iba_submap_build and iba_lattice_build (include/iba_mi355x.h; included at the end of iba_capi.hip, whose handle it uses).
// One call = one launch chain for the whole batch of sub-maps (iba_voxel_kernels.hpp) with three synchronisations: after the bounds (the
// extent is checked and the key fields are sized on the host), after the count of the voxels (the outputs are sized) and at the end. Down go
// the member and sub-map blocks (128 B per member, 152 B per sub-map), up come the bounds (56 B per sub-map) and the voxel clouds: nothing of
// input-scan size crosses PCIe. The work buffers live in the handle (h->vox) and only grow.
// iba_lattice_build is the same chain on the descriptor iba_lattice_desc: PCL's cells anchored at the origin instead of Open3D's grid on the cloud's
// minimum, and a crop box applied in the first kernel (the kLattice variants of the transform / bounds / key kernels; 64 B of crop box per sub-map
// go down and the bounds are 64 B). Sort, heads and averages are the very same kernels.
#include <rocprim/device/device_radix_sort.hpp>

struct iba_submap_clouds {
    int32_t M = 0;
    std::vector<int64_t> first;     // M + 1: sub-map s owns the voxels first[s] .. first[s + 1]
    std::vector<int64_t> dropped;   // M
    std::vector<int64_t> cropped;   // M (iba_lattice_build; zeros for iba_submap_build)
    std::vector<double> xyz;        // 3 per voxel
    std::vector<int32_t> count;     // 1 per voxel
};

namespace {

constexpr int kVoxMaxSubs = 4096;
constexpr int kVoxMaxMembers = 1 << 22;        // members of one call, all sub-maps together
constexpr uint64_t kVoxMaxPoints = 0xFFFFFF00ull;   // member points of one call: a concatenation position is a 32-bit value of the sort

template <bool kLattice> auto& vox_partials(iba_handle::VoxWork& w) { if constexpr (kLattice) return w.d_lpart; else return w.d_part; }
template <bool kLattice> auto& vox_bounds(iba_handle::VoxWork& w) { if constexpr (kLattice) return w.d_lbounds; else return w.d_bounds; }

bool vox_finite12(const double* T) { for (int i = 0; i < 12; ++i) if (!std::isfinite(T[i])) return false; return true; }
int vox_bits(uint64_t v) { int b = 0; while (v) { ++b; v >>= 1; } return b; }   // bits that hold 0 .. v

// what differs between the two descriptors: the name of the struct, the cell size and its name, the crop box
const char* vox_desc_name(const iba_submap_desc&) { return "iba_submap_desc"; }
const char* vox_desc_name(const iba_lattice_desc&) { return "iba_lattice_desc"; }
const char* vox_cell_name(const iba_submap_desc&) { return "voxel"; }
const char* vox_cell_name(const iba_lattice_desc&) { return "leaf"; }
double vox_cell(const iba_submap_desc& d) { return d.voxel; }
double vox_cell(const iba_lattice_desc& d) { return d.leaf; }
const char* vox_crop_error(const iba_submap_desc&) { return nullptr; }
const char* vox_crop_error(const iba_lattice_desc& d) {
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(d.crop_lo[a]) || !std::isfinite(d.crop_hi[a])) return "crop_lo / crop_hi are not finite";
        if (!(d.crop_lo[a] <= d.crop_hi[a])) return "crop_lo must not exceed crop_hi";
    }
    return nullptr;
}

template <class Desc>
iba_status vox_check(iba_handle* h, const Desc* subs, int32_t M, const std::string& who) {
    if (!subs) return fail(h, IBA_ERR_INVALID_ARG, who + "the sub-map descriptors are NULL");
    if (M < 1 || M > kVoxMaxSubs) return fail(h, IBA_ERR_INVALID_ARG, who + "M must be in [1, 4096]");
    int64_t members = 0;
    for (int s = 0; s < M; ++s) {
        const Desc& d = subs[s];
        const std::string at = who + "sub-map " + std::to_string(s) + ": ";
        if (d.struct_size != (int32_t)sizeof(Desc)) return fail(h, IBA_ERR_INVALID_ARG, at + vox_desc_name(d) + ".struct_size does not match this library");
        if (d.n_members < 1) return fail(h, IBA_ERR_INVALID_ARG, at + "n_members must be at least 1");
        if (!d.frames || !d.poses12) return fail(h, IBA_ERR_INVALID_ARG, at + "frames / poses12 are NULL");
        if (!(vox_cell(d) > 0.0) || !std::isfinite(vox_cell(d))) return fail(h, IBA_ERR_INVALID_ARG, at + vox_cell_name(d) + " must be positive and finite");
        if (const char* e = vox_crop_error(d)) return fail(h, IBA_ERR_INVALID_ARG, at + e);
        if (d.out12 && !vox_finite12(d.out12)) return fail(h, IBA_ERR_INVALID_ARG, at + "out12 is not finite");
        for (int m = 0; m < d.n_members; ++m) {
            if (d.frames[m] < 0 || d.frames[m] >= h->n_frames)
                return fail(h, IBA_ERR_INVALID_ARG, at + "member " + std::to_string(m) + " names frame " + std::to_string(d.frames[m]) + " outside the handle's " + std::to_string(h->n_frames) + " local frames");
            if (!vox_finite12(d.poses12 + 12 * (size_t)m)) return fail(h, IBA_ERR_INVALID_ARG, at + "the pose of member " + std::to_string(m) + " is not finite");
        }
        members += d.n_members;
    }
    if (members > kVoxMaxMembers) return fail(h, IBA_ERR_UNSUPPORTED, who + "more than 2^22 members in one call");
    return IBA_OK;
}

// The launch chain of iba_submap_build. clouds = true: the voxel clouds come up into the result. false (iba_submap_handle, iba_index_host.hpp):
// they stay on the device (h->vox.d_xyz, in the order of the result's `first`) and only first / dropped are filled. `who` heads the messages.
// Desc = iba_lattice_desc: the lattice filter (rules L1-L4 of the header) through the kLattice kernels.
template <class Desc>
iba_status vox_build(iba_handle* h, const Desc* subs, int32_t M, const std::string& who, bool clouds, iba_submap_clouds** out) {
    constexpr bool kLattice = std::is_same<Desc, iba_lattice_desc>::value;
    using Partial = typename VoxPartialOf<kLattice>::type;
    if (const iba_status s = vox_check(h, subs, M, who)) return s;

    // ---- the batch as the kernels take it: members that hold points, sub-map after sub-map ----
    std::vector<VoxMember> mem;
    std::vector<VoxSub> sub((size_t)M);
    std::vector<uint64_t> n_in((size_t)M, 0);   // member points per sub-map
    uint64_t N = 0, blocks = 0;
    for (int s = 0; s < M; ++s) {
        const Desc& d = subs[s];
        VoxSub& S = sub[(size_t)s];
        std::memset(&S, 0, sizeof(S));
        S.voxel = vox_cell(d); S.has_out = d.out12 ? 1 : 0;
        if (d.out12) std::memcpy(S.out, d.out12, sizeof(S.out));
        S.blk0 = (uint32_t)blocks;
        for (int m = 0; m < d.n_members; ++m) {
            const uint32_t P = h->h_frames[(size_t)d.frames[m]].P;
            if (P == 0u) continue;
            VoxMember x;
            std::memset(&x, 0, sizeof(x));
            std::memcpy(x.T, d.poses12 + 12 * (size_t)m, sizeof(x.T));
            x.pos0 = N; x.blk0 = (uint32_t)blocks; x.frame = d.frames[m]; x.sub = s;
            mem.push_back(x);
            N += P; n_in[(size_t)s] += P; blocks += (P + (uint32_t)kVoxThreads - 1u) / (uint32_t)kVoxThreads;
            if (N > kVoxMaxPoints || blocks > 0x7FFFFFFFull) return fail(h, IBA_ERR_UNSUPPORTED, who + "the members of one call hold more than 2^32 - 256 points (split the batch)");
        }
        S.blk1 = (uint32_t)blocks;
    }
    std::unique_ptr<iba_submap_clouds> res(new iba_submap_clouds);   // (freed on every error path below)
    res->M = M; res->first.assign((size_t)M + 1, 0); res->dropped.assign((size_t)M, 0); res->cropped.assign((size_t)M, 0);
    if (N == 0) { *out = res.release(); return IBA_OK; }   // every member is an empty scan: zero voxels, no launch

    HIP_TRY(h, hipSetDevice(h->device));
    auto& w = h->vox;
    const hipStream_t st = h->stream;
    HIP_TRY(h, w.d_mem.grow(mem.size()));
    HIP_TRY(h, w.d_sub.grow((size_t)M));
    auto& d_part = vox_partials<kLattice>(w);
    auto& d_bounds = vox_bounds<kLattice>(w);
    HIP_TRY(h, d_part.grow((size_t)blocks));
    HIP_TRY(h, d_bounds.grow((size_t)M));
    HIP_TRY(h, w.d_q3.grow(3 * (size_t)N));
    HIP_TRY(h, hipMemcpyAsync(w.d_mem.p, mem.data(), sizeof(VoxMember) * mem.size(), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipMemcpyAsync(w.d_sub.p, sub.data(), sizeof(VoxSub) * (size_t)M, hipMemcpyHostToDevice, st));
    const VoxCrop* d_crop = nullptr;
    std::vector<VoxCrop> crop;   // (lives until the first synchronisation, like mem and sub)
    if constexpr (kLattice) {
        crop.resize((size_t)M);
        for (int s = 0; s < M; ++s) {
            VoxCrop& c = crop[(size_t)s];
            std::memset(&c, 0, sizeof(c));
            c.has_crop = subs[s].has_crop ? 1 : 0;
            std::memcpy(c.lo, subs[s].crop_lo, sizeof(c.lo)); std::memcpy(c.hi, subs[s].crop_hi, sizeof(c.hi));
        }
        HIP_TRY(h, w.d_crop.grow((size_t)M));
        HIP_TRY(h, hipMemcpyAsync(w.d_crop.p, crop.data(), sizeof(VoxCrop) * (size_t)M, hipMemcpyHostToDevice, st));
        d_crop = w.d_crop.p;
    }
    hipLaunchKernelGGL(iba_vox_transform_kernel<kLattice>, dim3((unsigned)blocks), dim3(kVoxThreads), 0, st, h->frames.p, h->pts4.p, h->inv_perm.p, w.d_mem.p, (int)mem.size(), d_crop, w.d_q3.p, d_part.p);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_vox_bounds_kernel<kLattice>, dim3((unsigned)M), dim3(kVoxThreads), 0, st, w.d_sub.p, d_part.p, d_bounds.p);
    HIP_TRY(h, hipGetLastError());
    std::vector<Partial> bounds((size_t)M);
    HIP_TRY(h, hipMemcpyAsync(bounds.data(), d_bounds.p, sizeof(Partial) * (size_t)M, hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));

    // ---- minb, the extent, the key fields ----
    uint64_t n_kept = 0, imax[3] = {0, 0, 0};
    for (int s = 0; s < M; ++s) {
        const Partial& b = bounds[(size_t)s];
        VoxSub& S = sub[(size_t)s];
        res->dropped[(size_t)s] = (int64_t)b.dropped;
        uint64_t kept = n_in[(size_t)s] - b.dropped;
        if constexpr (kLattice) { res->cropped[(size_t)s] = (int64_t)b.cropped; kept -= b.cropped; }
        n_kept += kept;
        if (kept == 0) continue;
        for (int a = 0; a < 3; ++a) {
            double top;   // the kernels' expression on the largest kept q: no index of this axis is above it
            if constexpr (kLattice) {   // floor(q / leaf) does not decrease with q: the least kept q has the least cell; the key holds the cell minus that
                S.minb[a] = vox_lattice_index(b.mn[a], S.voxel);
                top = vox_lattice_index(b.mx[a], S.voxel) - S.minb[a];
            } else {
                S.minb[a] = b.mn[a] - 0.5 * S.voxel;
                top = vox_index(b.mx[a], S.minb[a], S.voxel);
            }
            if (!(top >= 0.0 && top < (double)(1u << kVoxAxisBits)))
                return fail(h, IBA_ERR_UNSUPPORTED, who + "sub-map " + std::to_string(s) + ": the extent along axis " + std::to_string(a) + " is " + (top < 9.0e18 ? std::to_string((long long)top + 1) : std::string("more than 2^63")) +
                                                        " voxels; the key holds " + std::to_string(1u << kVoxAxisBits) + " per axis (choose a larger voxel or split the sub-map)");
            imax[a] = std::max(imax[a], (uint64_t)top);
        }
    }
    if (n_kept == 0) { *out = res.release(); return IBA_OK; }   // nothing but dropped points
    VoxBits bits{};
    bits.y_shift = vox_bits(imax[2]); bits.x_shift = bits.y_shift + vox_bits(imax[1]); bits.sub_shift = bits.x_shift + vox_bits(imax[0]);
    const unsigned end_bit = (unsigned)(bits.sub_shift + vox_bits((uint64_t)M));   // (sub-map M is the key of the dropped points; at most 51 + 13 bits)

    HIP_TRY(h, w.d_key[0].grow((size_t)N)); HIP_TRY(h, w.d_key[1].grow((size_t)N));
    HIP_TRY(h, w.d_val[0].grow((size_t)N)); HIP_TRY(h, w.d_val[1].grow((size_t)N));
    HIP_TRY(h, hipMemcpyAsync(w.d_sub.p, sub.data(), sizeof(VoxSub) * (size_t)M, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(iba_vox_key_kernel<kLattice>, dim3((unsigned)blocks), dim3(kVoxThreads), 0, st, h->frames.p, w.d_mem.p, (int)mem.size(), w.d_sub.p, (int)M, bits, w.d_q3.p, w.d_key[0].p, w.d_val[0].p);
    HIP_TRY(h, hipGetLastError());
    rocprim::double_buffer<uint64_t> kb(w.d_key[0].p, w.d_key[1].p);
    rocprim::double_buffer<uint32_t> vb(w.d_val[0].p, w.d_val[1].p);
    size_t tmp_bytes = 0;
    HIP_TRY(h, rocprim::radix_sort_pairs(nullptr, tmp_bytes, kb, vb, (size_t)N, 0u, end_bit, st));
    HIP_TRY(h, w.d_tmp.grow(tmp_bytes));
    tmp_bytes = w.d_tmp.n;
    HIP_TRY(h, rocprim::radix_sort_pairs((void*)w.d_tmp.p, tmp_bytes, kb, vb, (size_t)N, 0u, end_bit, st));
    const uint64_t* keys = kb.current();
    const uint32_t* vals = vb.current();

    // ---- heads, slots, averages ----
    const uint32_t nhb = (uint32_t)((n_kept + (uint64_t)kVoxHeadBlock - 1) / (uint64_t)kVoxHeadBlock);
    HIP_TRY(h, w.d_blockc.grow((size_t)nhb + 1));
    HIP_TRY(h, w.d_subfirst.grow((size_t)M + 1));
    hipLaunchKernelGGL(iba_vox_count_heads_kernel, dim3(nhb), dim3(kVoxThreads), 0, st, keys, n_kept, w.d_blockc.p);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_vox_scan_blocks_kernel, dim3(1), dim3(1024), 0, st, w.d_blockc.p, nhb, w.d_blockc.p + nhb);
    HIP_TRY(h, hipGetLastError());
    uint32_t V = 0;
    HIP_TRY(h, hipMemcpyAsync(&V, w.d_blockc.p + nhb, sizeof(V), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    if (V == 0 || (uint64_t)V > n_kept) return fail(h, IBA_ERR_HIP, who + "the voxel count came back outside (0, kept points]");
    HIP_TRY(h, w.d_seg.grow((size_t)V));
    HIP_TRY(h, w.d_xyz.grow(3 * (size_t)V));
    HIP_TRY(h, w.d_cnt.grow((size_t)V));
    HIP_TRY(h, hipMemsetAsync(w.d_subfirst.p, 0xFF, sizeof(uint32_t) * ((size_t)M + 1), st));
    hipLaunchKernelGGL(iba_vox_heads_kernel, dim3(nhb), dim3(kVoxThreads), 0, st, keys, n_kept, w.d_blockc.p, (int)bits.sub_shift, w.d_seg.p, w.d_subfirst.p);
    HIP_TRY(h, hipGetLastError());
    hipLaunchKernelGGL(iba_vox_average_kernel, dim3((V + (uint32_t)kVoxThreads - 1u) / (uint32_t)kVoxThreads), dim3(kVoxThreads), 0, st, w.d_sub.p, (int)bits.sub_shift, keys, vals, w.d_q3.p, w.d_seg.p, V, n_kept,
                       w.d_xyz.p, w.d_cnt.p);
    HIP_TRY(h, hipGetLastError());
    std::vector<uint32_t> first((size_t)M + 1);
    if (clouds) {
        res->xyz.resize(3 * (size_t)V); res->count.resize((size_t)V);
        HIP_TRY(h, hipMemcpyAsync(res->xyz.data(), w.d_xyz.p, sizeof(double) * 3 * (size_t)V, hipMemcpyDeviceToHost, st));
        HIP_TRY(h, hipMemcpyAsync(res->count.data(), w.d_cnt.p, sizeof(int32_t) * (size_t)V, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(h, hipMemcpyAsync(first.data(), w.d_subfirst.p, sizeof(uint32_t) * ((size_t)M + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(h, hipStreamSynchronize(st));
    res->first[(size_t)M] = (int64_t)V;
    for (int s = M - 1; s >= 0; --s) res->first[(size_t)s] = first[(size_t)s] == kVoxNoSlot ? res->first[(size_t)s + 1] : (int64_t)first[(size_t)s];   // (a sub-map without voxels owns an empty range)
    *out = res.release();
    return IBA_OK;
}

}  // namespace

iba_status iba_submap_build(iba_handle* h, const iba_submap_desc* subs, int32_t M, iba_submap_clouds** out) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, "iba_submap_build: the result pointer is NULL");
    *out = nullptr;
    return vox_build(h, subs, M, "iba_submap_build: ", true, out);
}

iba_status iba_lattice_build(iba_handle* h, const iba_lattice_desc* subs, int32_t M, iba_submap_clouds** out) {
    if (!h) return IBA_ERR_INVALID_ARG;
    if (!out) return fail(h, IBA_ERR_INVALID_ARG, "iba_lattice_build: the result pointer is NULL");
    *out = nullptr;
    return vox_build(h, subs, M, "iba_lattice_build: ", true, out);
}

int32_t iba_submap_num(const iba_submap_clouds* c) { return c ? c->M : 0; }
int64_t iba_submap_n_voxels(const iba_submap_clouds* c, int32_t s) { return (c && s >= 0 && s < c->M) ? c->first[(size_t)s + 1] - c->first[(size_t)s] : -1; }
int64_t iba_submap_n_dropped(const iba_submap_clouds* c, int32_t s) { return (c && s >= 0 && s < c->M) ? c->dropped[(size_t)s] : -1; }
int64_t iba_submap_n_cropped(const iba_submap_clouds* c, int32_t s) { return (c && s >= 0 && s < c->M) ? c->cropped[(size_t)s] : -1; }
const double* iba_submap_xyz(const iba_submap_clouds* c, int32_t s) { return (c && s >= 0 && s < c->M) ? c->xyz.data() + 3 * (size_t)c->first[(size_t)s] : nullptr; }
const int32_t* iba_submap_counts(const iba_submap_clouds* c, int32_t s) { return (c && s >= 0 && s < c->M) ? c->count.data() + (size_t)c->first[(size_t)s] : nullptr; }
void iba_submap_free(iba_submap_clouds* c) { delete c; }

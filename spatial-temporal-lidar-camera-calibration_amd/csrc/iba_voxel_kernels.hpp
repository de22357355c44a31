// Device side of iba_submap_build (include/iba_mi355x.h): resident scans + poses -> voxel-averaged clouds, a BATCH OF SUB-MAPS per launch chain.
// A sub-map is a list of members (local frame, pose); its points in CONCATENATION order are the members in list order, each member's points in
// the scan's ORIGINAL index order. Position g of the batch = the sub-maps one after the other (VoxMember::pos0 + original index).
//
//  iba_vox_transform_kernel   flat grid over the 256-point blocks of every member (VoxMember::blk0 ascending: a block finds its member by
//      bisection). Thread = one original index o: the point is gathered from the resident pts4 through inv_perm (float32, widened), q = pose * p
//      by vox_apply — four separately rounded f64 operations per row, NO fma — and staged as three doubles at position g. A point with a
//      non-finite coordinate before or after the transform is dropped (q staged as NaN). The block's min / max of the kept q per axis and its
//      dropped count: the lanes of a wave by ordered compares over DPP-free shuffles, the four waves through LDS, ONE partial per block.
//  iba_vox_bounds_kernel      grid (sub-maps), 256 threads: the partials of the sub-map's blocks (contiguous: VoxSub::blk0 .. blk1) reduced by
//      compares and an integer sum. A min / max is exact in any order. The host reads the result (the one place the extent can be refused),
//      forms minb = min - 0.5 voxel and the width of every key field, and sends both back.
//  iba_vox_key_kernel         the same grid as the first kernel: index = floor((q - minb) / voxel) per axis (IEEE f64 division and floor), key =
//      sub-map | ix | iy | iz packed from the top in fields as wide as this BATCH needs (the sort then takes as few passes as the data allow; the
//      order of the keys is lexicographic (sub-map, ix, iy, iz) whatever the widths), value = g. A dropped point takes the key of a sub-map one
//      past the last: it sorts behind every kept point.
//  (rocPRIM's device radix sort by key, stable: equal keys keep ascending g = concatenation order)
//  iba_vox_count_heads_kernel / iba_vox_scan_blocks_kernel / iba_vox_heads_kernel   a head = a sorted position whose key differs from its
//      predecessor's. Heads per 2048-position block, an exclusive scan of the block counts by ONE block (a running total carried over 1024-entry
//      rounds), then each block ranks its own heads and writes seg_start[slot] = position; the first head of a sub-map writes the sub-map's
//      first slot. Integer work only.
//  iba_vox_average_kernel     thread = one voxel: the staged q of its segment added SEQUENTIALLY in sorted (= concatenation) order — the order
//      is the definition of the result, it is never traded for a tree —, divided by double(count), moved by the sub-map's output transform with
//      vox_apply. The loads of the next eight points are issued before the adds of the current eight (they do not depend on the sum): the adds
//      stay a chain, the gathers overlap. No floating-point atomics anywhere.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_types.hpp"

namespace iba {

constexpr int kVoxThreads = 256;
constexpr int kVoxAxisBits = 17;                 // most bits of one index field: 2^17 = 131072 voxels per axis
constexpr int kVoxHeadItems = 8;                 // sorted positions per thread of the head kernels
constexpr int kVoxHeadBlock = kVoxThreads * kVoxHeadItems;
constexpr uint32_t kVoxNoSlot = 0xFFFFFFFFu;

struct VoxMember {       // one member of one sub-map (host -> device)
    double T[12];        // row-major 3x4, scan frame -> common frame
    uint64_t pos0;       // position of its first point in the batch's concatenation
    uint32_t blk0;       // first block of the member in the flat grid
    int32_t frame, sub;  // local frame, sub-map
    int32_t pad;
};
struct VoxSub {          // one sub-map
    double out[12];      // output transform (has_out)
    double voxel;
    double minb[3];      // min over kept q - 0.5 voxel (written by the host between the bounds and the key kernel); iba_lattice_build: the least cell index per axis
    uint32_t blk0, blk1; // its blocks in the flat grid
    int32_t has_out, pad;
};
struct VoxPartial { double mn[3], mx[3]; uint64_t dropped; };   // of one block / one sub-map
struct VoxLatPartial { double mn[3], mx[3]; uint64_t dropped, cropped; };   // the same of iba_lattice_build: points outside the crop box counted on their own
struct VoxCrop { double lo[3], hi[3]; int32_t has_crop, pad; };             // one sub-map's crop box (iba_lattice_build)
template <bool kLattice> struct VoxPartialOf { using type = VoxPartial; };
template <> struct VoxPartialOf<true> { using type = VoxLatPartial; };
struct VoxBits { int32_t sub_shift, x_shift, y_shift, pad; };   // iz sits at bit 0

// row r of T * (x, y, z, 1): ((T0 x + T1 y) + T2 z) + T3, every operation rounded on its own (tests/submap_ref.py restates it in numpy, which has no fma)
__host__ __device__ __forceinline__ double vox_row(const double* T, int r, double x, double y, double z) {
#pragma clang fp contract(off)
    const double a = T[4 * r] * x;
    const double b = T[4 * r + 1] * y;
    const double c = T[4 * r + 2] * z;
    const double ab = a + b;
    const double abc = ab + c;
    return abc + T[4 * r + 3];
}
__host__ __device__ __forceinline__ void vox_apply(const double* T, double x, double y, double z, double& q0, double& q1, double& q2) {
    q0 = vox_row(T, 0, x, y, z); q1 = vox_row(T, 1, x, y, z); q2 = vox_row(T, 2, x, y, z);
}
// Open3D's voxel index of one axis: floor((q - minb) / voxel)
__host__ __device__ __forceinline__ double vox_index(double q, double minb, double voxel) {
#pragma clang fp contract(off)
    const double d = q - minb;
    return floor(d / voxel);
}

// PCL's cell of one axis with the origin as the anchor: floor(q / leaf) (iba_lattice_build, rule L3)
__host__ __device__ __forceinline__ double vox_lattice_index(double q, double leaf) {
#pragma clang fp contract(off)
    return floor(q / leaf);
}

__device__ __forceinline__ int vox_member_of_block(const VoxMember* __restrict__ mem, int n_mem, uint32_t blk) {
    int lo = 0, hi = n_mem - 1;   // the last member whose first block is not beyond this one (the host lists no member without points: every blk0 is distinct)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (mem[mid].blk0 <= blk) lo = mid; else hi = mid - 1; }
    return lo;
}

__device__ __forceinline__ double vox_shfl_xor(double v, int m) { return __shfl_xor(v, m, 64); }

// kLattice (iba_lattice_build): a finite q outside its sub-map's crop box (both ends inclusive) is staged as NaN like a dropped point and counted
// on its own; it takes part in no bound and, in the key kernel, costs no key beyond the drop bucket. crops is read by that variant only.
template <bool kLattice>
__global__ __launch_bounds__(kVoxThreads) void iba_vox_transform_kernel(const FrameHdr* __restrict__ frames, const float4* __restrict__ pts4, const uint32_t* __restrict__ inv_perm,
                                                                       const VoxMember* __restrict__ mem, int n_mem, const VoxCrop* __restrict__ crops, double* __restrict__ q3,
                                                                       typename VoxPartialOf<kLattice>::type* __restrict__ partials) {
    __shared__ double s_mn[4][3], s_mx[4][3];
    __shared__ uint32_t s_dr[4], s_cr[4];
    const VoxMember& X = mem[vox_member_of_block(mem, n_mem, blockIdx.x)];
    const FrameHdr& fh = frames[X.frame];
    const uint32_t o = (blockIdx.x - X.blk0) * (uint32_t)kVoxThreads + threadIdx.x;   // original index in the member's scan
    const bool act = o < fh.P;
    const double inf = __builtin_huge_val();
    double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    uint32_t dropped = 0u, cropped = 0u;
    if (act) {
        const float4 p = pts4[fh.pt_base + inv_perm[fh.pt_base + o]];
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        double q[3];
        vox_apply(X.T, x, y, z, q[0], q[1], q[2]);
        const bool keep = isfinite(x) && isfinite(y) && isfinite(z) && isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]);
        bool inside = true;
        if constexpr (kLattice) {
            const VoxCrop& C = crops[X.sub];
            if (C.has_crop) inside = C.lo[0] <= q[0] && q[0] <= C.hi[0] && C.lo[1] <= q[1] && q[1] <= C.hi[1] && C.lo[2] <= q[2] && q[2] <= C.hi[2];
        }
        double* dst = q3 + 3 * (X.pos0 + o);
        if (keep && inside) {
            dst[0] = q[0]; dst[1] = q[1]; dst[2] = q[2];
#pragma unroll
            for (int a = 0; a < 3; ++a) { mn[a] = q[a]; mx[a] = q[a]; }
        } else {
            const double nan = __builtin_nan("");
            dst[0] = nan; dst[1] = nan; dst[2] = nan;
            if (keep) cropped = 1u; else dropped = 1u;
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = vox_shfl_xor(mn[a], m), hi = vox_shfl_xor(mx[a], m);
            mn[a] = lo < mn[a] ? lo : mn[a]; mx[a] = hi > mx[a] ? hi : mx[a];
        }
        dropped += (uint32_t)__shfl_xor((int)dropped, m, 64);
        if constexpr (kLattice) cropped += (uint32_t)__shfl_xor((int)cropped, m, 64);
    }
    const int w = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_mn[w][a] = mn[a]; s_mx[w][a] = mx[a]; }
        s_dr[w] = dropped;
        if constexpr (kLattice) s_cr[w] = cropped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        typename VoxPartialOf<kLattice>::type r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double lo = s_mn[0][a], hi = s_mx[0][a];
#pragma unroll
            for (int k = 1; k < 4; ++k) { lo = s_mn[k][a] < lo ? s_mn[k][a] : lo; hi = s_mx[k][a] > hi ? s_mx[k][a] : hi; }
            r.mn[a] = lo; r.mx[a] = hi;
        }
        r.dropped = (uint64_t)((s_dr[0] + s_dr[1]) + (s_dr[2] + s_dr[3]));
        if constexpr (kLattice) r.cropped = (uint64_t)((s_cr[0] + s_cr[1]) + (s_cr[2] + s_cr[3]));
        partials[blockIdx.x] = r;
    }
}

template <bool kLattice>
__global__ __launch_bounds__(kVoxThreads) void iba_vox_bounds_kernel(const VoxSub* __restrict__ subs, const typename VoxPartialOf<kLattice>::type* __restrict__ partials,
                                                                    typename VoxPartialOf<kLattice>::type* __restrict__ out) {
    using Partial = typename VoxPartialOf<kLattice>::type;
    __shared__ double s_mn[4][3], s_mx[4][3];
    __shared__ unsigned long long s_dr[4], s_cr[4];
    const VoxSub& S = subs[blockIdx.x];
    const double inf = __builtin_huge_val();
    double mn[3] = {inf, inf, inf}, mx[3] = {-inf, -inf, -inf};
    unsigned long long dropped = 0ull, cropped = 0ull;
    for (uint32_t b = S.blk0 + threadIdx.x; b < S.blk1; b += (uint32_t)kVoxThreads) {
        const Partial p = partials[b];
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = p.mn[a] < mn[a] ? p.mn[a] : mn[a]; mx[a] = p.mx[a] > mx[a] ? p.mx[a] : mx[a]; }
        dropped += p.dropped;
        if constexpr (kLattice) cropped += p.cropped;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double lo = vox_shfl_xor(mn[a], m), hi = vox_shfl_xor(mx[a], m);
            mn[a] = lo < mn[a] ? lo : mn[a]; mx[a] = hi > mx[a] ? hi : mx[a];
        }
        dropped += (unsigned long long)__shfl_xor((long long)dropped, m, 64);
        if constexpr (kLattice) cropped += (unsigned long long)__shfl_xor((long long)cropped, m, 64);
    }
    const int w = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_mn[w][a] = mn[a]; s_mx[w][a] = mx[a]; }
        s_dr[w] = dropped;
        if constexpr (kLattice) s_cr[w] = cropped;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial r;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            double lo = s_mn[0][a], hi = s_mx[0][a];
#pragma unroll
            for (int k = 1; k < 4; ++k) { lo = s_mn[k][a] < lo ? s_mn[k][a] : lo; hi = s_mx[k][a] > hi ? s_mx[k][a] : hi; }
            r.mn[a] = lo; r.mx[a] = hi;
        }
        r.dropped = (uint64_t)((s_dr[0] + s_dr[1]) + (s_dr[2] + s_dr[3]));
        if constexpr (kLattice) r.cropped = (uint64_t)((s_cr[0] + s_cr[1]) + (s_cr[2] + s_cr[3]));
        out[blockIdx.x] = r;
    }
}

// kLattice: the cell is floor(q / leaf) and the key field holds it minus the sub-map's least cell of that axis (VoxSub::minb, two exact integers)
template <bool kLattice>
__global__ __launch_bounds__(kVoxThreads) void iba_vox_key_kernel(const FrameHdr* __restrict__ frames, const VoxMember* __restrict__ mem, int n_mem, const VoxSub* __restrict__ subs, int n_sub,
                                                                 VoxBits bits, const double* __restrict__ q3, uint64_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const VoxMember& X = mem[vox_member_of_block(mem, n_mem, blockIdx.x)];
    const uint32_t o = (blockIdx.x - X.blk0) * (uint32_t)kVoxThreads + threadIdx.x;
    if (o >= frames[X.frame].P) return;
    const VoxSub& S = subs[X.sub];
    const uint64_t g = X.pos0 + o;
    const double q0 = q3[3 * g], q1 = q3[3 * g + 1], q2 = q3[3 * g + 2];
    uint64_t key;
    if (q0 == q0) {   // (a dropped or cropped point was staged as NaN)
        uint64_t ix, iy, iz;
        if constexpr (kLattice) {
            ix = (uint64_t)(long long)(vox_lattice_index(q0, S.voxel) - S.minb[0]);
            iy = (uint64_t)(long long)(vox_lattice_index(q1, S.voxel) - S.minb[1]);
            iz = (uint64_t)(long long)(vox_lattice_index(q2, S.voxel) - S.minb[2]);
        } else {
            ix = (uint64_t)(long long)vox_index(q0, S.minb[0], S.voxel);
            iy = (uint64_t)(long long)vox_index(q1, S.minb[1], S.voxel);
            iz = (uint64_t)(long long)vox_index(q2, S.minb[2], S.voxel);
        }
        key = ((uint64_t)X.sub << bits.sub_shift) | (ix << bits.x_shift) | (iy << bits.y_shift) | iz;
    } else {
        key = (uint64_t)n_sub << bits.sub_shift;
    }
    keys[g] = key;
    vals[g] = (uint32_t)g;
}

// heads of the block's kVoxHeadBlock sorted positions; thread t owns the kVoxHeadItems consecutive positions from base + t * kVoxHeadItems
__device__ __forceinline__ uint32_t vox_head_flags(const uint64_t* __restrict__ keys, uint64_t n, uint64_t i0) {
    uint32_t f = 0u;
    if (i0 < n) {
        uint64_t prev = i0 > 0 ? keys[i0 - 1] : ~keys[0];
#pragma unroll
        for (int k = 0; k < kVoxHeadItems; ++k) {
            if (i0 + k < n) { const uint64_t c = keys[i0 + k]; if (c != prev) f |= 1u << k; prev = c; }
        }
    }
    return f;
}

__global__ __launch_bounds__(kVoxThreads) void iba_vox_count_heads_kernel(const uint64_t* __restrict__ keys, uint64_t n, uint32_t* __restrict__ block_count) {
    __shared__ uint32_t s_c[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kVoxHeadBlock + (uint64_t)threadIdx.x * kVoxHeadItems;
    uint32_t c = (uint32_t)__popc(vox_head_flags(keys, n, i0));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) c += (uint32_t)__shfl_xor((int)c, m, 64);
    if ((threadIdx.x & 63u) == 0u) s_c[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) block_count[blockIdx.x] = (s_c[0] + s_c[1]) + (s_c[2] + s_c[3]);
}

// exclusive scan of block_count[0 .. nb) in place by one block of 1024 threads; total[0] = the sum
__global__ __launch_bounds__(1024) void iba_vox_scan_blocks_kernel(uint32_t* __restrict__ block_count, uint32_t nb, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_w[16];
    __shared__ uint32_t s_carry;
    const uint32_t t = threadIdx.x, lane = t & 63u, w = t >> 6;
    if (t == 0) s_carry = 0u;
    __syncthreads();
    for (uint32_t base = 0; base < nb; base += 1024u) {
        const uint32_t i = base + t;
        const uint32_t v = i < nb ? block_count[i] : 0u;
        uint32_t inc = v;   // inclusive scan inside the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= (uint32_t)d) inc += u; }
        if (lane == 63u) s_w[w] = inc;
        __syncthreads();
        uint32_t before = s_carry;
        for (uint32_t k = 0; k < w; ++k) before += s_w[k];
        if (i < nb) block_count[i] = before + inc - v;
        __syncthreads();
        if (t == 1023u) s_carry = before + inc;
        __syncthreads();
    }
    if (t == 0) total[0] = s_carry;
}

__global__ __launch_bounds__(kVoxThreads) void iba_vox_heads_kernel(const uint64_t* __restrict__ keys, uint64_t n, const uint32_t* __restrict__ block_offset, int sub_shift,
                                                                   uint32_t* __restrict__ seg_start, uint32_t* __restrict__ sub_first) {
    __shared__ uint32_t s_w[4];
    const uint64_t i0 = (uint64_t)blockIdx.x * kVoxHeadBlock + (uint64_t)threadIdx.x * kVoxHeadItems;
    const uint32_t f = vox_head_flags(keys, n, i0);
    const uint32_t c = (uint32_t)__popc(f), lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t inc = c;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) { const uint32_t u = (uint32_t)__shfl_up((int)inc, d, 64); if (lane >= (uint32_t)d) inc += u; }
    if (lane == 63u) s_w[w] = inc;
    __syncthreads();
    uint32_t slot = block_offset[blockIdx.x] + inc - c;
    for (uint32_t k = 0; k < w; ++k) slot += s_w[k];
#pragma unroll
    for (int k = 0; k < kVoxHeadItems; ++k) {
        if (f & (1u << k)) {
            const uint64_t i = i0 + k;
            seg_start[slot] = (uint32_t)i;
            const uint32_t s = (uint32_t)(keys[i] >> sub_shift);
            if (i == 0 || (uint32_t)(keys[i - 1] >> sub_shift) != s) sub_first[s] = slot;
            ++slot;
        }
    }
}

__global__ __launch_bounds__(kVoxThreads) void iba_vox_average_kernel(const VoxSub* __restrict__ subs, int sub_shift, const uint64_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                     const double* __restrict__ q3, const uint32_t* __restrict__ seg_start, uint32_t n_vox, uint64_t n_kept,
                                                                     double* __restrict__ xyz, int32_t* __restrict__ count) {
    const uint32_t v = blockIdx.x * (uint32_t)kVoxThreads + threadIdx.x;
    if (v >= n_vox) return;
    const uint64_t b = seg_start[v], e = v + 1u < n_vox ? seg_start[v + 1u] : n_kept;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    uint64_t i = b;
    for (; i + 8 <= e; i += 8) {
        double x[8], y[8], z[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const double* p = q3 + 3 * (uint64_t)vals[i + k]; x[k] = p[0]; y[k] = p[1]; z[k] = p[2]; }
#pragma unroll
        for (int k = 0; k < 8; ++k) { sx += x[k]; sy += y[k]; sz += z[k]; }
    }
    for (; i < e; ++i) { const double* p = q3 + 3 * (uint64_t)vals[i]; sx += p[0]; sy += p[1]; sz += p[2]; }
    const double n = (double)(e - b);
    double m0 = sx / n, m1 = sy / n, m2 = sz / n;
    const VoxSub& S = subs[(uint32_t)(keys[b] >> sub_shift)];
    if (S.has_out) { const double a0 = m0, a1 = m1, a2 = m2; vox_apply(S.out, a0, a1, a2, m0, m1, m2); }
    xyz[3 * (uint64_t)v] = m0; xyz[3 * (uint64_t)v + 1] = m1; xyz[3 * (uint64_t)v + 2] = m2;
    count[v] = (int32_t)(e - b);
}

}  // namespace iba

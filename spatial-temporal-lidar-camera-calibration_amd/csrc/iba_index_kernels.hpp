// Device side of iba_submap_handle (include/iba_mi355x.h): the scan-side arrays of a handle — the implicit balanced kd-tree of iba_build.hpp,
// the leaf-ordered points, the chunk and frame boxes — built on the device from the voxel clouds iba_submap_build's chain leaves there, for
// ALL frames of the new handle together. The result is a pure function of the float32 points and must equal, byte for byte, what iba_create
// uploads for the same points. The rules are build_tree's (iba_build.hpp), restated:
//
//  Depth.    D = tree_depth_for(P): known on the host from the voxel counts. Frames of a call have different depths; level d runs for the
//            frames with D > d.
//  Level d, segment (d, k) of a frame = tree positions [k P >> d, (k + 1) P >> d), mid = (2k + 1) P >> (d + 1):
//            float min / max per axis over the segment (exact in any order), the extents as FLOAT subtractions max - min, the split dimension =
//            the first axis whose extent is strictly the largest, the segment partitioned at rank mid, split = the value at rank mid. The
//            host's branches for mid <= lo (split = min) and mid >= hi (split = max) are kept; a segment of a level below D holds more than
//            kLeafTarget points, so they are reached by no input (they would also depend on the order std::nth_element leaves behind).
//  Order.    Within a segment (value along the split dimension, original index), with -0.0f == +0.0f: the tie then goes to the index. The sort
//            key is ordered(value) << 22 | index (P < 2^22), where ordered() maps a float to an unsigned integer that keeps the order of the
//            floats and maps BOTH zeros to one key. The stored split is not taken from the key: it is the bits of the coordinate of the point
//            that stands at rank mid after the sort.
//            The host partitions with std::nth_element; a full sort of the segment puts the same element at rank mid and the same SETS on its
//            two sides, and nothing below depends on the order inside a side: the next level sorts its segments again, and
//  Final.    inside a leaf [j P >> D, (j + 1) P >> D) the points stand in ascending original index.
//
//  iba_idx_stage_kernel      thread = four consecutive original indices of one frame (bisection over the frames' first positions): the voxel
//      average narrowed from f64 to f32 (round to nearest even, the conversion of the host's cast), staged as (x, y, z, index bits) at the
//      frame's base + original index; order[] = identity; the NaN padding up to Ppad. A coordinate that is not finite after narrowing raises
//      a flag word by an integer atomic OR (the host refuses the call).
//  iba_idx_segment_kernel    a group of 64 or 256 threads per (frame, k) of the level: bounds of the segment by compares (wave shuffles, then
//      LDS for the four waves of a large group), the split dimension, the segment's range for the sort, then key / value of every position of
//      the segment. No atomics, no dependence on which group runs first: every word is written by exactly one thread.
//  (rocPRIM's segmented radix sort of the pairs on bits 0 .. 54: every segment of the level in one call, the values land in order[].
//   Positions outside the level's segments — finished frames — are not touched.)
//  iba_idx_split_kernel      thread = one segment: the node (split bits of the point at rank mid, dimension).
//  iba_idx_leaf_kernel       thread = one leaf: its range, for the segmented sort of the ORIGINAL INDICES inside every leaf (bits 0 .. 22).
//  iba_idx_gather_kernel     thread = four consecutive tree positions: one 16-byte store each to xs, ys, zs, perm and four to pts4; inv_perm is
//      the one scattered 4-byte store (a permutation: no two threads write one word).
//  iba_idx_chunk_box_kernel  one wave per 64-position chunk, iba_idx_frame_box_kernel one block per frame. The host takes a bound by
//      `if (v < mn) mn = v` in ascending position: of values that compare equal (-0.0f and +0.0f) the FIRST stays. The reductions therefore
//      carry (value, position) and break a tie by the lower position, which makes the bytes independent of the reduction's shape.
// Everything is written once per call by a fixed thread: the same bytes on every call.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_build.hpp"
#include "iba_types.hpp"

namespace iba {

constexpr int kIdxThreads = 256;
constexpr int kIdxIndexBits = 22;                  // original index field of the sort key (iba_create refuses scans of 2^22 points)
constexpr uint32_t kIdxQnanBits = 0x7FC00000u;     // std::numeric_limits<float>::quiet_NaN(), the host build's padding
static_assert(kChunk == 64, "iba_idx_chunk_box_kernel reduces one chunk per wave");

struct IdxFrame {         // one frame of the new handle (host -> device), 32 B
    uint32_t pt_base;     // first tree position (padded space: FrameHdr::pt_base)
    uint32_t P;
    uint32_t src_first;   // first voxel of the sub-map in the voxel chain's output
    uint32_t depth;
    uint32_t node_base, box_base;
    uint32_t pad0, pad1;
};

__device__ __forceinline__ float idx_qnan() { return __uint_as_float(kIdxQnanBits); }

// order-preserving key of a float; -0.0f and +0.0f share one key
__host__ __device__ __forceinline__ uint32_t idx_ordered(uint32_t bits) {
    if ((bits << 1) == 0u) bits = 0u;
    return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}

// the last frame whose first position is not beyond `pos` (empty frames share a first position with their successor: the LAST of them that
// still holds points is wanted, so the bisection runs on the END of the frames instead)
__device__ __forceinline__ int idx_frame_of_pos(const IdxFrame* __restrict__ fr, int M, uint32_t pos) {
    int lo = 0, hi = M - 1;   // the first frame whose padded end is beyond pos
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t end = fr[mid].pt_base + ((fr[mid].P + 3u) & ~3u);
        if (end > pos) hi = mid; else lo = mid + 1;
    }
    return lo;
}
__device__ __forceinline__ int idx_frame_of_chunk(const IdxFrame* __restrict__ fr, int M, uint32_t c) {
    int lo = 0, hi = M - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const uint32_t end = fr[mid].box_base + (fr[mid].P + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
        if (end > c) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kIdxThreads) void iba_idx_stage_kernel(const IdxFrame* __restrict__ fr, int M, uint32_t n_quads, const double* __restrict__ vox_xyz,
                                                                   float4* __restrict__ src4, uint32_t* __restrict__ order, uint32_t* __restrict__ flag) {
    const uint32_t q = blockIdx.x * (uint32_t)kIdxThreads + threadIdx.x;
    if (q >= n_quads) return;
    const uint32_t pos = 4u * q;
    const IdxFrame F = fr[idx_frame_of_pos(fr, M, pos)];
    const uint32_t i0 = pos - F.pt_base;
    uint32_t ord[4];
    bool bad = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        float4 p = make_float4(idx_qnan(), idx_qnan(), idx_qnan(), 0.f);
        ord[j] = 0u;
        if (i < F.P) {
            const double* s = vox_xyz + 3 * ((size_t)F.src_first + i);
            p.x = (float)s[0]; p.y = (float)s[1]; p.z = (float)s[2]; p.w = __uint_as_float(i);
            bad = bad || !(isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
            ord[j] = i;
        }
        src4[pos + (uint32_t)j] = p;
    }
    *reinterpret_cast<uint4*>(order + pos) = make_uint4(ord[0], ord[1], ord[2], ord[3]);
    if (bad) atomicOr(flag, 1u);
}

// G threads per segment (64: a wave, 256: the block). Grid: ceil((M << d) / (kIdxThreads / G)) blocks.
template <int G>
__global__ __launch_bounds__(kIdxThreads) void iba_idx_segment_kernel(const IdxFrame* __restrict__ fr, int M, int d, const float4* __restrict__ src4, const uint32_t* __restrict__ order,
                                                                     uint64_t* __restrict__ key, uint32_t* __restrict__ val, uint32_t* __restrict__ seg_begin, uint32_t* __restrict__ seg_end,
                                                                     uint32_t* __restrict__ seg_dim, TreeNode* __restrict__ nodes) {
    __shared__ float s_b[4][6];
    const uint32_t seg = blockIdx.x * (uint32_t)(kIdxThreads / G) + threadIdx.x / (uint32_t)G;
    const uint32_t lane = threadIdx.x % (uint32_t)G;
    const uint32_t n_seg = (uint32_t)M << d;
    if (seg >= n_seg) return;                       // (uniform over the group; with G = 256 over the block)
    const uint32_t f = seg >> d, k = seg & ((1u << d) - 1u);
    const IdxFrame F = fr[f];
    if (F.depth <= (uint32_t)d) {                   // a finished frame: no segment at this level
        if (lane == 0) { seg_begin[seg] = 0u; seg_end[seg] = 0u; seg_dim[seg] = 0x80000000u; }
        return;
    }
    const uint32_t lo = (uint32_t)(((uint64_t)k * F.P) >> d), hi = (uint32_t)(((uint64_t)(k + 1u) * F.P) >> d);
    const uint32_t mid = (uint32_t)(((uint64_t)(2u * k + 1u) * F.P) >> (d + 1));
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t t = lo + lane; t < hi; t += (uint32_t)G) {
        const float4 p = src4[F.pt_base + order[F.pt_base + t]];
        const float v[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) { mn[a] = v[a] < mn[a] ? v[a] : mn[a]; mx[a] = v[a] > mx[a] ? v[a] : mx[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float o1 = __shfl_xor(mn[a], m, 64), o2 = __shfl_xor(mx[a], m, 64);
            mn[a] = o1 < mn[a] ? o1 : mn[a]; mx[a] = o2 > mx[a] ? o2 : mx[a];
        }
    if (G == 256) {
        const uint32_t w = threadIdx.x >> 6;
        if ((threadIdx.x & 63u) == 0u) { for (int a = 0; a < 3; ++a) { s_b[w][a] = mn[a]; s_b[w][3 + a] = mx[a]; } }
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = s_b[0][a]; mx[a] = s_b[0][3 + a];
            for (int w2 = 1; w2 < 4; ++w2) { mn[a] = s_b[w2][a] < mn[a] ? s_b[w2][a] : mn[a]; mx[a] = s_b[w2][3 + a] > mx[a] ? s_b[w2][3 + a] : mx[a]; }
        }
    }
    uint32_t dim = 0u; float ext = mx[0] - mn[0];
    for (uint32_t a = 1; a < 3u; ++a) if (mx[a] - mn[a] > ext) { ext = mx[a] - mn[a]; dim = a; }
    const bool sorts = mid > lo && mid < hi;
    if (lane == 0) {
        seg_begin[seg] = sorts ? F.pt_base + lo : 0u; seg_end[seg] = sorts ? F.pt_base + hi : 0u;
        seg_dim[seg] = dim | (sorts ? 0u : 0x80000000u);
        if (!sorts) {
            float split = 0.f;
            if (hi > lo) split = (mid <= lo) ? mn[dim] : mx[dim];
            nodes[F.node_base + ((1u << d) - 1u) + k] = TreeNode{split, dim};
        }
    }
    if (!sorts) return;
    for (uint32_t t = lo + lane; t < hi; t += (uint32_t)G) {
        const uint32_t o = order[F.pt_base + t];
        const float4 p = src4[F.pt_base + o];
        const float v = dim == 0u ? p.x : (dim == 1u ? p.y : p.z);
        key[F.pt_base + t] = ((uint64_t)idx_ordered(__float_as_uint(v)) << kIdxIndexBits) | (uint64_t)o;
        val[F.pt_base + t] = o;
    }
}

__global__ __launch_bounds__(kIdxThreads) void iba_idx_split_kernel(const IdxFrame* __restrict__ fr, int M, int d, const float4* __restrict__ src4, const uint32_t* __restrict__ order,
                                                                   const uint32_t* __restrict__ seg_dim, TreeNode* __restrict__ nodes) {
    const uint32_t seg = blockIdx.x * (uint32_t)kIdxThreads + threadIdx.x;
    if (seg >= ((uint32_t)M << d)) return;
    const uint32_t dim = seg_dim[seg];
    if (dim & 0x80000000u) return;                  // a finished frame, or a node the segment kernel has written
    const uint32_t f = seg >> d, k = seg & ((1u << d) - 1u);
    const IdxFrame F = fr[f];
    const uint32_t mid = (uint32_t)(((uint64_t)(2u * k + 1u) * F.P) >> (d + 1));
    const float4 p = src4[F.pt_base + order[F.pt_base + mid]];
    nodes[F.node_base + ((1u << d) - 1u) + k] = TreeNode{dim == 0u ? p.x : (dim == 1u ? p.y : p.z), dim};
}

__global__ __launch_bounds__(kIdxThreads) void iba_idx_leaf_kernel(const IdxFrame* __restrict__ fr, int M, int dmax, uint32_t* __restrict__ seg_begin, uint32_t* __restrict__ seg_end) {
    const uint32_t seg = blockIdx.x * (uint32_t)kIdxThreads + threadIdx.x;
    if (seg >= ((uint32_t)M << dmax)) return;
    const uint32_t f = seg >> dmax, j = seg & ((1u << dmax) - 1u);
    const IdxFrame F = fr[f];
    uint32_t b = 0u, e = 0u;
    if (F.depth > 0u && j < (1u << F.depth)) {      // (the one leaf of a frame of depth 0 is already in ascending index)
        b = F.pt_base + (uint32_t)(((uint64_t)j * F.P) >> F.depth); e = F.pt_base + (uint32_t)(((uint64_t)(j + 1u) * F.P) >> F.depth);
    }
    seg_begin[seg] = b; seg_end[seg] = e;
}

__global__ __launch_bounds__(kIdxThreads) void iba_idx_gather_kernel(const IdxFrame* __restrict__ fr, int M, uint32_t n_quads, const float4* __restrict__ src4, const uint32_t* __restrict__ order,
                                                                    float* __restrict__ xs, float* __restrict__ ys, float* __restrict__ zs, float4* __restrict__ pts4,
                                                                    uint32_t* __restrict__ perm, uint32_t* __restrict__ inv_perm) {
    const uint32_t q = blockIdx.x * (uint32_t)kIdxThreads + threadIdx.x;
    if (q >= n_quads) return;
    const uint32_t pos = 4u * q;
    const IdxFrame F = fr[idx_frame_of_pos(fr, M, pos)];
    const uint32_t i0 = pos - F.pt_base;
    const uint4 o4 = *reinterpret_cast<const uint4*>(order + pos);
    const uint32_t o[4] = {o4.x, o4.y, o4.z, o4.w};
    float x[4], y[4], z[4]; uint32_t pm[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = i0 + (uint32_t)j;
        float4 p = make_float4(idx_qnan(), idx_qnan(), idx_qnan(), 0.f);
        pm[j] = 0u;
        if (i < F.P) {
            p = src4[F.pt_base + o[j]];
            pm[j] = o[j];
            inv_perm[F.pt_base + o[j]] = i;
        } else {
            inv_perm[pos + (uint32_t)j] = 0u;       // (padding: no original index maps here)
        }
        x[j] = p.x; y[j] = p.y; z[j] = p.z;
        pts4[pos + (uint32_t)j] = p;
    }
    *reinterpret_cast<float4*>(xs + pos) = make_float4(x[0], x[1], x[2], x[3]);
    *reinterpret_cast<float4*>(ys + pos) = make_float4(y[0], y[1], y[2], y[3]);
    *reinterpret_cast<float4*>(zs + pos) = make_float4(z[0], z[1], z[2], z[3]);
    *reinterpret_cast<uint4*>(perm + pos) = make_uint4(pm[0], pm[1], pm[2], pm[3]);
}

// (value, position) with the host's sequential rule: of equal values the one at the lower position stays
__device__ __forceinline__ void idx_first_min(float& v, uint32_t& at, float v2, uint32_t at2) { if (v2 < v || (v2 == v && at2 < at)) { v = v2; at = at2; } }
__device__ __forceinline__ void idx_first_max(float& v, uint32_t& at, float v2, uint32_t at2) { if (v2 > v || (v2 == v && at2 < at)) { v = v2; at = at2; } }

__global__ __launch_bounds__(kIdxThreads) void iba_idx_chunk_box_kernel(const IdxFrame* __restrict__ fr, int M, uint32_t n_chunks, const float* __restrict__ xs, const float* __restrict__ ys,
                                                                       const float* __restrict__ zs, float* __restrict__ chunk_box) {
    const uint32_t c = blockIdx.x * (uint32_t)(kIdxThreads / 64) + (threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63u;
    if (c >= n_chunks) return;                      // (uniform over the wave)
    const IdxFrame F = fr[idx_frame_of_chunk(fr, M, c)];
    const uint32_t i = (c - F.box_base) * (uint32_t)kChunk + lane;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t amn[3] = {lane, lane, lane}, amx[3] = {lane, lane, lane};
    if (i < F.P) {
        const float v[3] = {xs[F.pt_base + i], ys[F.pt_base + i], zs[F.pt_base + i]};
#pragma unroll
        for (int a = 0; a < 3; ++a) { if (v[a] < mn[a]) mn[a] = v[a]; if (v[a] > mx[a]) mx[a] = v[a]; }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float v1 = __shfl_xor(mn[a], m, 64); const uint32_t a1 = (uint32_t)__shfl_xor((int)amn[a], m, 64);
            const float v2 = __shfl_xor(mx[a], m, 64); const uint32_t a2 = (uint32_t)__shfl_xor((int)amx[a], m, 64);
            idx_first_min(mn[a], amn[a], v1, a1); idx_first_max(mx[a], amx[a], v2, a2);
        }
    if (lane == 0) {
        float rmax = 0.f;
        for (int a = 0; a < 3; ++a) rmax = fmaxf(rmax, fmaxf(fabsf(mn[a]), fabsf(mx[a])));
        float4* bx = reinterpret_cast<float4*>(chunk_box + 8 * (size_t)c);
        bx[0] = make_float4(mn[0], mn[1], mn[2], idx_qnan());
        bx[1] = make_float4(mx[0], mx[1], mx[2], (mn[0] <= mx[0]) ? rmax : idx_qnan());
    }
}

__global__ __launch_bounds__(kIdxThreads) void iba_idx_frame_box_kernel(const IdxFrame* __restrict__ fr, const float* __restrict__ chunk_box, float* __restrict__ frame_box) {
    __shared__ float s_v[4][6];
    __shared__ uint32_t s_a[4][6];
    const IdxFrame F = fr[blockIdx.x];
    const uint32_t nc = (F.P + (uint32_t)kChunk - 1u) / (uint32_t)kChunk;
    float v[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
    uint32_t at[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    for (uint32_t c = threadIdx.x; c < nc; c += (uint32_t)kIdxThreads) {
        const float4* bx = reinterpret_cast<const float4*>(chunk_box + 8 * ((size_t)F.box_base + c));
        const float4 lo = bx[0], hi = bx[1];
        idx_first_min(v[0], at[0], lo.x, c); idx_first_min(v[1], at[1], lo.y, c); idx_first_min(v[2], at[2], lo.z, c);
        idx_first_max(v[3], at[3], hi.x, c); idx_first_max(v[4], at[4], hi.y, c); idx_first_max(v[5], at[5], hi.z, c);
    }
#pragma unroll
    for (int a = 0; a < 6; ++a)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const float v1 = __shfl_xor(v[a], m, 64); const uint32_t a1 = (uint32_t)__shfl_xor((int)at[a], m, 64);
            if (a < 3) idx_first_min(v[a], at[a], v1, a1); else idx_first_max(v[a], at[a], v1, a1);
        }
    const uint32_t w = threadIdx.x >> 6;
    if ((threadIdx.x & 63u) == 0u) for (int a = 0; a < 6; ++a) { s_v[w][a] = v[a]; s_a[w][a] = at[a]; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int a = 0; a < 6; ++a)
            for (uint32_t w2 = 1; w2 < 4u; ++w2) { if (a < 3) idx_first_min(v[a], at[a], s_v[w2][a], s_a[w2][a]); else idx_first_max(v[a], at[a], s_v[w2][a], s_a[w2][a]); }
        float4* out = reinterpret_cast<float4*>(frame_box + 8 * (size_t)blockIdx.x);
        const float n = idx_qnan();
        out[0] = F.P ? make_float4(v[0], v[1], v[2], n) : make_float4(n, n, n, n);
        out[1] = F.P ? make_float4(v[3], v[4], v[5], n) : make_float4(n, n, n, n);
    }
}

}  // namespace iba

// Kernels of iba_floam_extract (include/iba_mi355x.h, "F-LOAM feature extraction"; host side: iba_floam_host.hpp). The rules of the header are the
// contract; tests/floam_ref.py restates them in numpy and the result is compared byte for byte. One call = one chain for the whole batch of scans:
//  iba_floam_classify_kernel  thread = one ORIGINAL point index of one scan (read through inv_perm, as iba_vox_transform_kernel does): rules 1-2. Writes
//      the sort key scan * 65 + ring (ring 64: the point is skipped) and the original index as the sort's value; counts the points per ring and the
//      three skip reasons in an LDS histogram, one integer atomic per non-empty bin and block into counts[scan][68].
//  (rocPRIM's stable radix sort on the keys: the ring lists in original index order, scan after scan, ring after ring. The host reads counts back,
//      checks rule 3 and lists the sectors: a FloamTask each.)
//  iba_floam_ring_points_kernel  thread = one sorted position: the point (x, y, z, original index bits) in ring order, 16 B each.
//  iba_floam_sector_kernel    block = one (scan, ring, sector): rules 4-8. Curvature per entry from the ring-ordered points (the float32 chain, every
//      operation rounded on its own), (value bits, position) sorted ascending by a bitonic network in LDS (a value is never negative, so its f64 bits
//      order as an integer; padding sorts last), the greedy walk from the top with the marks as an LDS bitmap: every wave looks at the same next 64
//      sorted entries at once and a ballot names the first unmarked one (at most 21 picks; the 10 neighbour gaps of a pick are taken by 10 lanes and
//      two ballots say where each direction stops), then the surf list by ballot-prefix compaction in ascending order. Results go to slots that the
//      host sized per sector (max_edges_per_sector, sector length) as sorted positions.
//  (iba_vox_scan_blocks_kernel, twice: exclusive scans of the edge and surf counts per sector)
//  iba_floam_gather_kernel    block = one sector: its edge and surf points to their final places, rings ascending, sectors ascending (rule 9).
// No floating-point atomics; no result depends on what else is in the batch.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_types.hpp"

namespace iba {

constexpr int kFloamThreads = 256;
constexpr int kFloamMaxRing = 8192;            // IBA_FLOAM_MAX_RING_POINTS
constexpr int kFloamBins = 68;                 // per scan: points per ring [64], non-finite, out of range, no ring, unused
constexpr uint32_t kFloamKeys = 65;            // keys per scan: 64 rings + the skipped points
constexpr int kFloamSpan = 5;                  // neighbour_span: the only window the curvature is written for

struct FloamScan { uint64_t pos0; int32_t frame, pad; };    // one scan of the batch: where its points start in the concatenation, its local frame
struct FloamBlock { int32_t scan; uint32_t first; };         // one block of the classify kernel: original indices first .. first + 255 of the scan
struct FloamShape {
    double min_distance, max_distance, edge_curvature, neighbour_gap2;
    int32_t num_lines, max_edges;
};
struct FloamTask {             // one sector
    uint32_t ring_base;        // sorted position of the ring's first point
    uint32_t start, len;       // its curvature entries [start, start + len): entry t is ring position start + t + 5
    uint32_t surf_slot;        // first surf slot (the edge slots are task * max(max_edges, 1))
};

// rules 1-2: the ring of one point, 64 when it is skipped; why = 0 kept, 1 non-finite, 2 out of range, 3 no ring
__device__ __forceinline__ uint32_t floam_ring(float xf, float yf, float zf, const FloamShape& sh, int& why) {
#pragma clang fp contract(off)
    if (!(isfinite(xf) && isfinite(yf) && isfinite(zf))) { why = 1; return 64u; }
    const double x = (double)xf, y = (double)yf, z = (double)zf;
    const double xx = x * x;
    const double yy = y * y;
    const double d = sqrt(xx + yy);
    if (d < sh.min_distance || d > sh.max_distance) { why = 2; return 64u; }
    const double q = z / d;
    const double a180 = atan(q) * 180.0;
    const double angle = a180 / 3.14159265358979323846;
    why = 3;
    if (angle != angle) return 64u;
    int id;
    if (sh.num_lines == 16) {
        id = (int)((angle + 15.0) / 2.0 + 0.5);
    } else if (sh.num_lines == 32) {
        id = (int)((angle + 92.0 / 3.0) * 3.0 / 4.0);
    } else {
        if (angle > 2.0 || angle < -24.33) return 64u;
        id = angle >= -8.83 ? (int)((2.0 - angle) * 3.0 + 0.5) : 32 + (int)((-8.83 - angle) * 2.0 + 0.5);
    }
    if (id < 0 || id >= sh.num_lines) return 64u;
    why = 0;
    return (uint32_t)id;
}

__global__ __launch_bounds__(kFloamThreads) void iba_floam_classify_kernel(const FrameHdr* __restrict__ frames, const float4* __restrict__ pts4, const uint32_t* __restrict__ inv_perm,
                                                                          const FloamScan* __restrict__ scans, const FloamBlock* __restrict__ blocks, FloamShape sh,
                                                                          uint32_t* __restrict__ keys, uint32_t* __restrict__ vals, uint32_t* __restrict__ counts) {
    __shared__ uint32_t s_cnt[kFloamBins];
    if (threadIdx.x < (unsigned)kFloamBins) s_cnt[threadIdx.x] = 0u;
    __syncthreads();
    const FloamBlock b = blocks[blockIdx.x];
    const FloamScan sc = scans[b.scan];
    const FrameHdr& fh = frames[sc.frame];
    const uint32_t o = b.first + threadIdx.x;
    if (o < fh.P) {
        const float4 p = pts4[fh.pt_base + inv_perm[fh.pt_base + o]];
        int why;
        const uint32_t ring = floam_ring(p.x, p.y, p.z, sh, why);
        keys[sc.pos0 + o] = (uint32_t)b.scan * kFloamKeys + ring;
        vals[sc.pos0 + o] = o;
        atomicAdd(&s_cnt[why == 0 ? ring : 63u + (uint32_t)why], 1u);
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)kFloamBins && s_cnt[threadIdx.x]) atomicAdd(&counts[(size_t)b.scan * kFloamBins + threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(kFloamThreads) void iba_floam_ring_points_kernel(const FrameHdr* __restrict__ frames, const float4* __restrict__ pts4, const uint32_t* __restrict__ inv_perm,
                                                                             const FloamScan* __restrict__ scans, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ vals,
                                                                             uint64_t n, float4* __restrict__ ring_pts) {
    const uint64_t i = (uint64_t)blockIdx.x * kFloamThreads + threadIdx.x;
    if (i >= n) return;
    const uint32_t k = keys[i];
    if (k % kFloamKeys == 64u) return;                         // a skipped point: no sector reads its position
    const FrameHdr& fh = frames[scans[k / kFloamKeys].frame];
    const uint32_t o = vals[i];
    float4 p = pts4[fh.pt_base + inv_perm[fh.pt_base + o]];
    p.w = __uint_as_float(o);
    ring_pts[i] = p;
}

// rule 4 for one axis: the reference's expression left to right in float32
__device__ __forceinline__ float floam_chain(float m5, float m4, float m3, float m2, float m1, float c, float p1, float p2, float p3, float p4, float p5) {
#pragma clang fp contract(off)
    float s = m5 + m4;
    s = s + m3;
    s = s + m2;
    s = s + m1;
    const float t = 10.0f * c;
    s = s - t;
    s = s + p1;
    s = s + p2;
    s = s + p3;
    s = s + p4;
    s = s + p5;
    return s;
}
__device__ __forceinline__ double floam_sq3(float dx, float dy, float dz) {
#pragma clang fp contract(off)
    const double x = (double)dx, y = (double)dy, z = (double)dz;
    const double xx = x * x;
    const double yy = y * y;
    const double zz = z * z;
    const double xy = xx + yy;
    return xy + zz;
}
// rule 7: the squared gap between two ring points
__device__ __forceinline__ double floam_gap2(const float4 a, const float4 b) {
#pragma clang fp contract(off)
    const float dx = a.x - b.x;
    const float dy = a.y - b.y;
    const float dz = a.z - b.z;
    return floam_sq3(dx, dy, dz);
}

__host__ __device__ __forceinline__ uint32_t floam_pow2(uint32_t n) { uint32_t p = 64u; while (p < n) p <<= 1; return p; }   // sorted entries of a sector of n
__host__ __device__ __forceinline__ size_t floam_sector_lds(uint32_t P) { return (size_t)P * 10u + (size_t)((P + 10u + 31u) / 32u + 1u) * 4u; }

// dynamic LDS: u64 val[P] | u32 marks[(P + 41) / 32 + 1] | u16 pos[P]  (P = floam_pow2 of the launch's longest sector)
__global__ __launch_bounds__(kFloamThreads) void iba_floam_sector_kernel(const FloamTask* __restrict__ tasks, const float4* __restrict__ ring_pts, FloamShape sh, uint32_t Pmax,
                                                                        uint32_t* __restrict__ edge_pos, uint32_t* __restrict__ surf_pos, uint32_t* __restrict__ n_edge,
                                                                        uint32_t* __restrict__ n_surf) {
    extern __shared__ unsigned long long s_dyn[];
    __shared__ uint32_t s_w[kFloamThreads / 64];
    unsigned long long* s_val = s_dyn;
    uint32_t* s_mark = (uint32_t*)(s_val + Pmax);
    const uint32_t mark_words = (Pmax + 10u + 31u) / 32u + 1u;
    unsigned short* s_pos = (unsigned short*)(s_mark + mark_words);

    const FloamTask T = tasks[blockIdx.x];
    const uint32_t L = T.len, P = floam_pow2(L), tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const float4* __restrict__ rp = ring_pts + T.ring_base;   // ring positions 0 .. n - 1
    const unsigned long long inf_bits = 0x7FF0000000000000ull;

    // ---- rule 4: curvature of entry t = ring position j = start + t + 5 (position within the sector window: t + 5) ----
    for (uint32_t t = tid; t < P; t += kFloamThreads) {
        unsigned long long bits = ~0ull;
        unsigned short ps = 0xFFFFu;
        if (t < L) {
            const float4* q = rp + T.start + t;                // q[0 .. 10] = ring positions j - 5 .. j + 5
            const float4 a0 = q[0], a1 = q[1], a2 = q[2], a3 = q[3], a4 = q[4], c = q[5], b1 = q[6], b2 = q[7], b3 = q[8], b4 = q[9], b5 = q[10];
            const float dx = floam_chain(a0.x, a1.x, a2.x, a3.x, a4.x, c.x, b1.x, b2.x, b3.x, b4.x, b5.x);
            const float dy = floam_chain(a0.y, a1.y, a2.y, a3.y, a4.y, c.y, b1.y, b2.y, b3.y, b4.y, b5.y);
            const float dz = floam_chain(a0.z, a1.z, a2.z, a3.z, a4.z, c.z, b1.z, b2.z, b3.z, b4.z, b5.z);
            const double v = floam_sq3(dx, dy, dz);
            bits = (v != v) ? inf_bits : (unsigned long long)__double_as_longlong(v);   // a NaN counts as +inf; v is never negative
            ps = (unsigned short)t;
        }
        s_val[t] = bits; s_pos[t] = ps;
    }
    for (uint32_t w = tid; w < mark_words; w += kFloamThreads) s_mark[w] = 0u;
    __syncthreads();

    // ---- rule 6: ascending by (value, position) ----
    for (uint32_t k = 2u; k <= P; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0u; j >>= 1) {
            for (uint32_t i = tid; i < P; i += kFloamThreads) {
                const uint32_t x = i ^ j;
                if (x > i) {
                    const unsigned long long vi = s_val[i], vx = s_val[x];
                    const unsigned short pi = s_pos[i], px = s_pos[x];
                    const bool gt = vi > vx || (vi == vx && pi > px);
                    if (gt == ((i & k) == 0u)) { s_val[i] = vx; s_val[x] = vi; s_pos[i] = px; s_pos[x] = pi; }
                }
            }
            __syncthreads();
        }
    }

    // ---- rule 7: every wave walks the same entries, thread 0 writes ----
    const uint32_t edge_slot = blockIdx.x * (uint32_t)(sh.max_edges > 0 ? sh.max_edges : 1);
    int cur = (int)L - 1, count = 0;
    while (cur >= 0) {
        const int e = cur - (int)lane;
        bool open = false;
        if (e >= 0) { const uint32_t m = (uint32_t)s_pos[e] + 5u; open = ((s_mark[m >> 5] >> (m & 31u)) & 1u) == 0u; }
        const unsigned long long bal = __ballot(open);
        if (bal == 0ull) { cur -= 64; continue; }
        const int e0 = cur - (int)__builtin_ctzll(bal);
        const unsigned long long v0 = s_val[e0];
        const uint32_t t0 = (uint32_t)s_pos[e0];
        if (__longlong_as_double((long long)v0) <= sh.edge_curvature) break;
        ++count;
        const bool over = count > sh.max_edges;
        // the gaps of the pick: lanes 0-4 upwards (k = lane + 1), lanes 5-9 downwards (k = -(lane - 4))
        bool wide = false;
        if (!over && lane < 10u) {
            const float4* c = rp + T.start + t0 + 5u;          // the pick's ring position
            const int k = lane < 5u ? (int)lane + 1 : -((int)lane - 4);
            const float4 a = c[k], b = lane < 5u ? c[k - 1] : c[k + 1];
            wide = floam_gap2(a, b) > sh.neighbour_gap2;
        }
        const unsigned long long wb = __ballot(wide);
        const uint32_t up = (uint32_t)(wb & 31ull), dn = (uint32_t)((wb >> 5) & 31ull);
        const uint32_t n_up = over ? 0u : (up ? (uint32_t)__builtin_ctz(up) : 5u), n_dn = over ? 0u : (dn ? (uint32_t)__builtin_ctz(dn) : 5u);
        __syncthreads();                                       // every wave has read the marks of this round
        if (tid == 0u) {
            for (uint32_t m = t0 + 5u - n_dn; m <= t0 + 5u + n_up; ++m) s_mark[m >> 5] |= 1u << (m & 31u);
            if (!over) edge_pos[edge_slot + (uint32_t)count - 1u] = T.ring_base + T.start + t0 + 5u;
        }
        __syncthreads();
        if (over) break;
        cur = e0 - 1;
    }
    __syncthreads();
    const uint32_t ne = (uint32_t)(count > sh.max_edges ? sh.max_edges : count);

    // ---- rule 8: the unmarked entries in ascending order ----
    uint32_t base = 0u;
    for (uint32_t t = 0u; t < L; t += kFloamThreads) {
        const uint32_t i = t + tid;
        bool keep = false;
        uint32_t ti = 0u;
        if (i < L) { ti = (uint32_t)s_pos[i]; const uint32_t m = ti + 5u; keep = ((s_mark[m >> 5] >> (m & 31u)) & 1u) == 0u; }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0u) s_w[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = base, all = 0u;
#pragma unroll
        for (uint32_t w = 0u; w < (uint32_t)(kFloamThreads / 64); ++w) { const uint32_t c = s_w[w]; if (w < wave) before += c; all += c; }
        if (keep) surf_pos[T.surf_slot + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = T.ring_base + T.start + ti + 5u;
        base += all;
        __syncthreads();
    }
    if (tid == 0u) { n_edge[blockIdx.x] = ne; n_surf[blockIdx.x] = base; }
}

__global__ __launch_bounds__(kFloamThreads) void iba_floam_gather_kernel(const FloamTask* __restrict__ tasks, const float4* __restrict__ ring_pts, int32_t max_edges,
                                                                        const uint32_t* __restrict__ edge_pos, const uint32_t* __restrict__ surf_pos, const uint32_t* __restrict__ edge_off,
                                                                        const uint32_t* __restrict__ surf_off, float* __restrict__ edge_xyz, int32_t* __restrict__ edge_idx,
                                                                        float* __restrict__ surf_xyz, int32_t* __restrict__ surf_idx) {
    const uint32_t k = blockIdx.x;
    const uint32_t e0 = edge_off[k], ne = edge_off[k + 1] - e0, s0 = surf_off[k], ns = surf_off[k + 1] - s0;
    const uint32_t eslot = k * (uint32_t)(max_edges > 0 ? max_edges : 1), sslot = tasks[k].surf_slot;
    for (uint32_t i = threadIdx.x; i < ne; i += kFloamThreads) {
        const float4 p = ring_pts[edge_pos[eslot + i]];
        float* d = edge_xyz + 3 * (size_t)(e0 + i);
        d[0] = p.x; d[1] = p.y; d[2] = p.z; edge_idx[e0 + i] = (int32_t)__float_as_uint(p.w);
    }
    for (uint32_t i = threadIdx.x; i < ns; i += kFloamThreads) {
        const float4 p = ring_pts[surf_pos[sslot + i]];
        float* d = surf_xyz + 3 * (size_t)(s0 + i);
        d[0] = p.x; d[1] = p.y; d[2] = p.z; surf_idx[s0 + i] = (int32_t)__float_as_uint(p.w);
    }
}

}  // namespace iba

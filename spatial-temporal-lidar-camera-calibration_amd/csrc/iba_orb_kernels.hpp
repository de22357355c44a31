// ORB extraction, the device half (include/iba_mi355x.h, rules O2, O4, O5, O7, O8, O9). Every launch runs over flat tables the host built for a chunk
// of images: rows (one per image and level), 64 x 16 pixel tiles, cells, keypoints. All pixel work is integer; the only float decisions are the
// arctangent polynomial and the descriptor's rotated sample positions, both written once in iba_orb_host.hpp for host and device.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_orb_host.hpp"

namespace iba {
namespace orb {

constexpr int kThreads = 256;
constexpr int kTileW = 64, kTileH = 16;      // a block's pixels: 64 x 4 threads, four rows each
constexpr int kHalo = 3;                     // FAST circle radius = blur radius
constexpr int kCellMax = 59;                 // the widest tested region of a cell: width < 60 with one column
constexpr int kCellStride = 64;

struct OrbRow {                // one level of one image
    uint64_t pix;              // where the level starts in the chunk's pyramid, score and blurred planes
    int32_t W, H;
    int32_t src;               // the row of the level above it (-1: level 0)
    uint32_t xtab, ytab;       // its resize tables (pairs s, c1)
    int32_t pad;
};
struct OrbTile { int32_t row, tx, ty, pad; };
struct OrbCell { int32_t row, x0, x1, y0, y1; };     // the tested region in level pixels
struct OrbKp   { int32_t row, x, y, score; };        // level pixels
struct OrbUmax { int32_t u[16]; };

// O2: one lane per output pixel; the tables hold every float decision
__global__ __launch_bounds__(kThreads) void orb_resize_kernel(const OrbRow* __restrict__ rows, const OrbTile* __restrict__ tiles, const int2* __restrict__ tab, uint8_t* __restrict__ pyr) {
    const OrbTile t = tiles[blockIdx.x];
    const OrbRow r = rows[t.row];
    const OrbRow s = rows[r.src];
    const int x = t.tx * kTileW + (int)(threadIdx.x & 63);
    if (x >= r.W) return;
    const int2 cx = tab[r.xtab + (uint32_t)x];
    const int xa = cx.x, xb = min(cx.x + 1, s.W - 1), a1 = cx.y, a0 = 2048 - cx.y;
    const uint8_t* __restrict__ sp = pyr + s.pix;
    for (int k = 0; k < 4; ++k) {
        const int y = t.ty * kTileH + (int)(threadIdx.x >> 6) + 4 * k;
        if (y >= r.H) break;
        const int2 cy = tab[r.ytab + (uint32_t)y];
        const int ya = cy.x, yb = min(cy.x + 1, s.H - 1), b1 = cy.y, b0 = 2048 - cy.y;
        const uint8_t* p0 = sp + (size_t)ya * (size_t)s.W;
        const uint8_t* p1 = sp + (size_t)yb * (size_t)s.W;
        const int S0 = (int)p0[xa] * a0 + (int)p0[xb] * a1, S1 = (int)p1[xa] * a0 + (int)p1[xb] * a1;
        pyr[r.pix + (size_t)y * (size_t)r.W + (size_t)x] = (uint8_t)((((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2);
    }
}

// a tile of a level with its halo into LDS; coordinates outside the level are clamped (score) or reflected (blur, reflect-101)
template <bool REFLECT>
__device__ inline void load_tile(const OrbRow& r, const OrbTile& t, const uint8_t* __restrict__ plane, uint8_t (*tile)[kTileW + 2 * kHalo + 2]) {
    constexpr int TW = kTileW + 2 * kHalo, TH = kTileH + 2 * kHalo;
    const uint8_t* __restrict__ sp = plane + r.pix;
    for (int i = (int)threadIdx.x; i < TW * TH; i += kThreads) {
        const int ly = i / TW, lx = i - ly * TW;
        int x = t.tx * kTileW + lx - kHalo, y = t.ty * kTileH + ly - kHalo;
        if (REFLECT) {
            if (x < 0) x = -x;
            if (x >= r.W) x = 2 * r.W - 2 - x;
            if (y < 0) y = -y;
            if (y >= r.H) y = 2 * r.H - 2 - y;
        }
        x = min(max(x, 0), r.W - 1); y = min(max(y, 0), r.H - 1);
        tile[ly][lx] = sp[(size_t)y * (size_t)r.W + (size_t)x];
    }
}

// O4: the score of the centre p with the 16 circle values v: the largest t with 9 contiguous all > p + t or all < p - t (0 or less: none)
__device__ inline int fast_score(int p, const int (&v)[16]) {
    int d[25];
#pragma unroll
    for (int k = 0; k < 16; ++k) d[k] = v[k] - p;
#pragma unroll
    for (int k = 16; k < 25; ++k) d[k] = d[k - 16];
    int best = -256;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        int lo = d[k], hi = d[k];
#pragma unroll
        for (int j = 1; j < 9; ++j) { lo = min(lo, d[k + j]); hi = max(hi, d[k + j]); }
        best = max(best, max(lo, -hi));
    }
    return best - 1;
}

__global__ __launch_bounds__(kThreads) void orb_score_kernel(const OrbRow* __restrict__ rows, const OrbTile* __restrict__ tiles, const uint8_t* __restrict__ pyr, uint8_t* __restrict__ score, int min_th) {
    __shared__ uint8_t tile[kTileH + 2 * kHalo][kTileW + 2 * kHalo + 2];
    const OrbTile t = tiles[blockIdx.x];
    const OrbRow r = rows[t.row];
    load_tile<false>(r, t, pyr, tile);
    __syncthreads();
    const int lx = (int)(threadIdx.x & 63), x = t.tx * kTileW + lx;
    if (x >= r.W) return;
    constexpr int cx[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int cy[16] = {-3, -3, -2, -1, 0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3};
    for (int k = 0; k < 4; ++k) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, y = t.ty * kTileH + ly;
        if (y >= r.H) break;
        int out = 0;
        if (x >= kHalo && x < r.W - kHalo && y >= kHalo && y < r.H - kHalo) {
            const int p = tile[ly + kHalo][lx + kHalo];
            // the cheap reject: nine contiguous circle pixels hold at least two of the four compass pixels
            const int c0 = (int)tile[ly + kHalo - 3][lx + kHalo] - p, c1 = (int)tile[ly + kHalo][lx + kHalo + 3] - p;
            const int c2 = (int)tile[ly + kHalo + 3][lx + kHalo] - p, c3 = (int)tile[ly + kHalo][lx + kHalo - 3] - p;
            const int bright = (c0 > min_th) + (c1 > min_th) + (c2 > min_th) + (c3 > min_th);
            const int dark = (c0 < -min_th) + (c1 < -min_th) + (c2 < -min_th) + (c3 < -min_th);
            if (bright >= 2 || dark >= 2) {
                int v[16];
#pragma unroll
                for (int q = 0; q < 16; ++q) v[q] = tile[ly + kHalo + cy[q]][lx + kHalo + cx[q]];
                const int s = fast_score(p, v);
                out = s >= min_th ? s : 0;
            }
        }
        score[r.pix + (size_t)y * (size_t)r.W + (size_t)x] = (uint8_t)out;
    }
}

// O5: one block per cell. WRITE = false counts the kept pixels at ini_th (and at min_th when there is none: a fallback cell); WRITE = true writes them
// at the cell's offset in row-major order, by ballot prefix inside a wave and wave totals through LDS.
template <bool WRITE>
__global__ __launch_bounds__(kThreads) void orb_cell_kernel(const OrbRow* __restrict__ rows, const OrbCell* __restrict__ cells, const uint8_t* __restrict__ score, int ini_th, int min_th,
                                                            int32_t* __restrict__ cell_cnt, int32_t* __restrict__ cell_fb, const int32_t* __restrict__ cell_off,
                                                            int2* __restrict__ cand_xy, int32_t* __restrict__ cand_score) {
    __shared__ uint8_t tile[kCellMax + 2][kCellStride];
    __shared__ int32_t s_cnt[2];
    __shared__ int32_t s_wave[kThreads / 64];
    const OrbCell c = cells[blockIdx.x];
    const OrbRow r = rows[c.row];
    const int w = c.x1 - c.x0, h = c.y1 - c.y0;      // 1..kCellMax each (checked on the host)
    const uint8_t* __restrict__ sp = score + r.pix;
    for (int i = (int)threadIdx.x; i < (h + 2) * kCellStride; i += kThreads) {
        const int ly = i / kCellStride, lx = i - ly * kCellStride;
        const bool inside = ly >= 1 && ly <= h && lx >= 1 && lx <= w;
        tile[ly][lx] = inside ? sp[(size_t)(c.y0 + ly - 1) * (size_t)r.W + (size_t)(c.x0 + lx - 1)] : (uint8_t)0;
    }
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int n = w * h, lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int th = WRITE ? (cell_fb[blockIdx.x] ? min_th : ini_th) : 0;
    int base = WRITE ? cell_off[blockIdx.x] : 0;
    for (int i0 = 0; i0 < n; i0 += kThreads) {       // (uniform trip count: the barriers below are reached by every thread)
        const int i = i0 + (int)threadIdx.x;
        int s = 0, px = 0, py = 0;
        bool is_max = false;
        if (i < n) {
            py = i / w; px = i - py * w;
            s = tile[py + 1][px + 1];
            if (s > 0) {
                int m = max(max((int)tile[py][px], (int)tile[py][px + 1]), (int)tile[py][px + 2]);
                m = max(m, max((int)tile[py + 1][px], (int)tile[py + 1][px + 2]));
                m = max(m, max(max((int)tile[py + 2][px], (int)tile[py + 2][px + 1]), (int)tile[py + 2][px + 2]));
                is_max = s > m;
            }
        }
        if (!WRITE) {
            const unsigned long long b_ini = __ballot(is_max && s >= ini_th), b_min = __ballot(is_max && s >= min_th);
            if (lane == 0) { if (b_ini) atomicAdd(&s_cnt[0], __popcll(b_ini)); if (b_min) atomicAdd(&s_cnt[1], __popcll(b_min)); }
        } else {
            const bool keep = is_max && s >= th;
            const unsigned long long b = __ballot(keep);
            if (lane == 0) s_wave[wave] = __popcll(b);
            __syncthreads();
            int before = 0, total = 0;
            for (int q = 0; q < kThreads / 64; ++q) { const int v = s_wave[q]; if (q < wave) before += v; total += v; }
            if (keep) {
                const int at = base + before + __popcll(b & ((1ull << lane) - 1ull));
                cand_xy[at] = make_int2(c.x0 + px - kMinB, c.y0 + py - kMinB);
                cand_score[at] = s;
            }
            base += total;
            __syncthreads();
        }
    }
    if (!WRITE) {
        __syncthreads();
        if (threadIdx.x == 0) {
            const int fb = s_cnt[0] == 0;
            cell_cnt[blockIdx.x] = fb ? s_cnt[1] : s_cnt[0];
            cell_fb[blockIdx.x] = fb;
        }
    }
}

// exclusive scan of the cell counts by one block: off[0 .. n], off[n] = the total
__global__ __launch_bounds__(1024) void orb_scan_kernel(const int32_t* __restrict__ cnt, int32_t* __restrict__ off, int n) {
    __shared__ int32_t part[1024];
    const int per = (n + 1023) / 1024, a = min((int)threadIdx.x * per, n), b = min(a + per, n);
    int sum = 0;
    for (int i = a; i < b; ++i) sum += cnt[i];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = (int)threadIdx.x >= d ? part[threadIdx.x - d] : 0;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    int at = part[threadIdx.x] - sum;
    for (int i = a; i < b; ++i) { off[i] = at; at += cnt[i]; }
    if (threadIdx.x == 1023) off[n] = part[1023];
}

// O7: one wave per keypoint: two patch rows per step (32 lanes each), integer moments, a butterfly sum, the polynomial on lane 0
__global__ __launch_bounds__(kThreads) void orb_orient_kernel(const OrbRow* __restrict__ rows, const OrbKp* __restrict__ kps, int n_kp, const uint8_t* __restrict__ pyr, OrbUmax um, float* __restrict__ angle) {
    const int k = (int)blockIdx.x * (kThreads / 64) + (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
    if (k >= n_kp) return;
    const OrbKp kp = kps[k];
    const OrbRow r = rows[kp.row];
    const uint8_t* __restrict__ c = pyr + r.pix + (size_t)kp.y * (size_t)r.W + (size_t)kp.x;
    const int u = (lane & 31) - kHalfPatch;
    int m10 = 0, m01 = 0;
    for (int v0 = -kHalfPatch; v0 <= kHalfPatch; v0 += 2) {
        const int v = v0 + (lane >> 5);
        if (v <= kHalfPatch && u <= kHalfPatch) {
            const int lim = um.u[v < 0 ? -v : v];
            if (u >= -lim && u <= lim) {
                const int val = c[(ptrdiff_t)v * (ptrdiff_t)r.W + (ptrdiff_t)u];
                m10 += u * val; m01 += v * val;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) { m10 += __shfl_xor(m10, d, 64); m01 += __shfl_xor(m01, d, 64); }
    if (lane == 0) angle[k] = orb_atan2_deg((float)m01, (float)m10);
}

// O8: the 7-tap blur of the levels that have keypoints, two integer passes through LDS
__global__ __launch_bounds__(kThreads) void orb_blur_kernel(const OrbRow* __restrict__ rows, const OrbTile* __restrict__ tiles, const int32_t* __restrict__ row_kp, const uint8_t* __restrict__ pyr, uint8_t* __restrict__ blur) {
    __shared__ uint8_t tile[kTileH + 2 * kHalo][kTileW + 2 * kHalo + 2];
    __shared__ uint16_t hs[kTileH + 2 * kHalo][kTileW];
    const OrbTile t = tiles[blockIdx.x];
    if (row_kp[t.row] == 0) return;
    const OrbRow r = rows[t.row];
    load_tile<true>(r, t, pyr, tile);
    __syncthreads();
    constexpr int wgt[7] = {18, 34, 49, 54, 49, 34, 18};
    for (int i = (int)threadIdx.x; i < (kTileH + 2 * kHalo) * kTileW; i += kThreads) {
        const int ly = i >> 6, lx = i & 63;
        int sum = 0;
#pragma unroll
        for (int q = 0; q < 7; ++q) sum += wgt[q] * (int)tile[ly][lx + q];
        hs[ly][lx] = (uint16_t)sum;
    }
    __syncthreads();
    const int lx = (int)(threadIdx.x & 63), x = t.tx * kTileW + lx;
    if (x >= r.W) return;
    for (int k = 0; k < 4; ++k) {
        const int ly = (int)(threadIdx.x >> 6) + 4 * k, y = t.ty * kTileH + ly;
        if (y >= r.H) break;
        int sum = 0;
#pragma unroll
        for (int q = 0; q < 7; ++q) sum += wgt[q] * (int)hs[ly + q][lx];
        blur[r.pix + (size_t)y * (size_t)r.W + (size_t)x] = (uint8_t)((sum + 32768) >> 16);
    }
}

// O9: 32 lanes per keypoint, one descriptor byte (eight tests) per lane
__global__ __launch_bounds__(kThreads) void orb_desc_kernel(const OrbRow* __restrict__ rows, const OrbKp* __restrict__ kps, int n_kp, const float* __restrict__ angle, const uint8_t* __restrict__ blur,
                                                            const char4* __restrict__ pattern, uint8_t* __restrict__ desc) {
    const int k = (int)blockIdx.x * (kThreads / 32) + (int)(threadIdx.x >> 5), byte = (int)(threadIdx.x & 31);
    if (k >= n_kp) return;
    const OrbKp kp = kps[k];
    const OrbRow r = rows[kp.row];
    float a, b;
    orb_angle_ab(angle[k], &a, &b);
    const uint8_t* __restrict__ c = blur + r.pix + (size_t)kp.y * (size_t)r.W + (size_t)kp.x;
    int out = 0;
    for (int q = 0; q < 8; ++q) {
        const char4 p = pattern[8 * byte + q];
        const float x0 = (float)p.x, y0 = (float)p.y, x1 = (float)p.z, y1 = (float)p.w;
        const int r0 = (int)rintf(x0 * b + y0 * a), c0 = (int)rintf(x0 * a - y0 * b);
        const int r1 = (int)rintf(x1 * b + y1 * a), c1 = (int)rintf(x1 * a - y1 * b);
        const int t0 = c[(ptrdiff_t)r0 * (ptrdiff_t)r.W + (ptrdiff_t)c0], t1 = c[(ptrdiff_t)r1 * (ptrdiff_t)r.W + (ptrdiff_t)c1];
        out |= (t0 < t1) << q;
    }
    desc[(size_t)k * 32u + (size_t)byte] = (uint8_t)out;
}

}  // namespace orb
}  // namespace iba

// Device side of the scan-to-image projection (include/iba_mi355x.h, iba_project_*, rules P2-P8), and its launches. Four kernels:
//   iba_project_splat_kernel    the flat grid of iba_flat_pass.hpp over (job, 4096-point slice), thread = point: the leaf-ordered 16-byte point and
//                               its original index, P2 / P3 with the evaluator's quotients (div2), the (2r + 1)^2 integer atomic mins of P4, the
//                               point's record at its ORIGINAL index; the job's R | t and camera from a table staged in LDS
//   iba_project_resolve_kernel  thread = pixel: keys -> depth and index images, n_pixels (P5)
//   iba_project_visible_kernel  thread = point (original order): P6, and with an uploaded image P7
//   iba_project_overlay_kernel  thread = pixel: P8
// Every reduction is an integer minimum or an integer count: no result depends on the order in which blocks or lanes arrive, so two runs give
// the same bytes. Counts go by wave ballot into LDS and from there by ONE global atomic per counter and block.
// First version: no LDS tile in front of the global atomics, no merging of lanes that hit the same pixel.
// The launches (project_*) need no handle: pointers and a stream. They are compiled with the evaluation kernels (iba_capi.hip), whose div2 and
// flat_job they use, and declared in iba_internal.hpp for iba_project.hip.
#pragma once
#include "iba_flat_pass.hpp"
#include "iba_internal.hpp"
#include "iba_project_host.hpp"

namespace iba {

using project::ProjJob;
using project::ProjRec;

// wave ballot of `pred` added to the block's LDS counter by the wave's first lane (every lane of the wave calls)
__device__ __forceinline__ void proj_count(uint32_t* s_cnt, bool pred) {
    const unsigned long long m = __ballot(pred);
    if ((threadIdx.x & 63u) == 0u && m) atomicAdd(s_cnt, (uint32_t)__popcll(m));
}

__global__ __launch_bounds__(project::kThreads) void iba_project_splat_kernel(const float4* __restrict__ pts4, const ProjJob* __restrict__ jobs, int nj, uint32_t bias, int r, double z_min,
                                                                            double z_max, unsigned long long* __restrict__ keys, ProjRec* __restrict__ recs, uint32_t* __restrict__ cnt) {
    __shared__ ProjJob s_job;
    __shared__ uint32_t s_cnt[3];
    const uint32_t blk = blockIdx.x + bias;
    const int j = flat_job<&ProjJob::first_block>(jobs, nj, blk);
    {
        const uint64_t* src = reinterpret_cast<const uint64_t*>(jobs + j);
        uint64_t* dst = reinterpret_cast<uint64_t*>(&s_job);
        for (uint32_t i = threadIdx.x; i < sizeof(ProjJob) / 8u; i += project::kThreads) dst[i] = src[i];
        if (threadIdx.x < 3u) s_cnt[threadIdx.x] = 0u;
    }
    __syncthreads();
    const ProjJob& jb = s_job;
    const uint32_t base = (blk - jb.first_block) * (uint32_t)project::kSlice;
    const int Wi = (int)jb.Wi, Hi = (int)jb.Hi;
    for (uint32_t it = 0; it < (uint32_t)(project::kSlice / project::kThreads); ++it) {
        const uint32_t pos = base + it * (uint32_t)project::kThreads + threadIdx.x;
        const bool live = pos < jb.P;
        float4 p = float4{0.f, 0.f, 0.f, 0.f};
        if (live) p = pts4[jb.pt_base + pos];
        const uint32_t orig = __float_as_uint(p.w);
        const bool finite = isfinite(p.x) && isfinite(p.y) && isfinite(p.z);
        const double x = (double)p.x, y = (double)p.y, z = (double)p.z;
        const double qx = ((jb.Rt[0] * x + jb.Rt[1] * y) + jb.Rt[2] * z) + jb.Rt[3];
        const double qy = ((jb.Rt[4] * x + jb.Rt[5] * y) + jb.Rt[6] * z) + jb.Rt[7];
        const double qz = ((jb.Rt[8] * x + jb.Rt[9] * y) + jb.Rt[10] * z) + jb.Rt[11];
        const bool front = live && finite && z_min < qz && qz < z_max;
        double u = 0.0, v = 0.0;
        if (front) div2(jb.fx * qx + jb.cx * qz, jb.fv * qy + jb.cy * qz, qz, u, v);
        const bool inside = front && 0.0 <= u && u < jb.W && 0.0 <= v && v < jb.H;
        const float z32 = front ? (float)qz : 0.f;
        if (live && orig < jb.P) {
            ProjRec rec;
            rec.u = u; rec.v = v; rec.z = z32;
            rec.flags = (front ? IBA_PROJECT_IN_FRONT : 0u) | (inside ? IBA_PROJECT_INSIDE : 0u);
            recs[jb.rec_base + orig] = rec;
        }
        if (inside) {
            const int iu = (int)floor(u), iv = (int)floor(v);
            const unsigned long long key = ((unsigned long long)__float_as_uint(z32) << 32) | (unsigned long long)orig;
            const int x0 = max(iu - r, 0), x1 = min(iu + r, Wi - 1), y0 = max(iv - r, 0), y1 = min(iv + r, Hi - 1);
            for (int yy = y0; yy <= y1; ++yy)
                for (int xx = x0; xx <= x1; ++xx)
                    (void)__hip_atomic_fetch_min(keys + jb.key_base + (uint64_t)yy * (uint64_t)Wi + (uint64_t)xx, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        proj_count(&s_cnt[0], live && !finite);
        proj_count(&s_cnt[1], front);
        proj_count(&s_cnt[2], inside);
    }
    __syncthreads();
    if (threadIdx.x < 3u && s_cnt[threadIdx.x]) atomicAdd(cnt + (size_t)j * project::kCounters + project::C_SKIPPED + threadIdx.x, s_cnt[threadIdx.x]);
}

__global__ __launch_bounds__(project::kThreads) void iba_project_resolve_kernel(const ProjJob* __restrict__ jobs, int nj, uint32_t bias, const unsigned long long* __restrict__ keys,
                                                                              float* __restrict__ depth, uint32_t* __restrict__ index, uint32_t* __restrict__ cnt) {
    __shared__ uint32_t s_cnt;
    const uint32_t blk = blockIdx.x + bias;
    const int j = flat_job<&ProjJob::first_pblock>(jobs, nj, blk);
    const ProjJob& jb = jobs[j];
    if (threadIdx.x == 0u) s_cnt = 0u;
    __syncthreads();
    const uint64_t pix = (uint64_t)(blk - jb.first_pblock) * (uint64_t)project::kThreads + threadIdx.x;
    const bool live = pix < (uint64_t)jb.Wi * (uint64_t)jb.Hi;
    bool holds = false;
    if (live) {
        const unsigned long long key = keys[jb.key_base + pix];
        holds = key != ~0ull;
        depth[jb.img_base + pix] = holds ? __uint_as_float((uint32_t)(key >> 32)) : 0.f;
        index[jb.img_base + pix] = (uint32_t)key;   // (all ones for an empty pixel)
    }
    proj_count(&s_cnt, holds);
    __syncthreads();
    if (threadIdx.x == 0u && s_cnt) atomicAdd(cnt + (size_t)j * project::kCounters + project::C_PIXELS, s_cnt);
}

// COLOUR = false: P6 for the jobs of a chunk, n_visible counted. true: one job again (the same flags), its points coloured from rgb (P7).
template <bool COLOUR>
__global__ __launch_bounds__(project::kThreads) void iba_project_visible_kernel(const ProjJob* __restrict__ jobs, int nj, uint32_t bias, double tol, ProjRec* __restrict__ recs,
                                                                              const float* __restrict__ depth, uint32_t* __restrict__ cnt, const uint8_t* __restrict__ rgb,
                                                                              uint8_t* __restrict__ point_rgb) {
    __shared__ uint32_t s_cnt;
    const uint32_t blk = blockIdx.x + bias;
    const int j = flat_job<&ProjJob::first_block>(jobs, nj, blk);
    const ProjJob& jb = jobs[j];
    if (threadIdx.x == 0u) s_cnt = 0u;
    __syncthreads();
    const uint32_t base = (blk - jb.first_block) * (uint32_t)project::kSlice;
    const int Wi = (int)jb.Wi, Hi = (int)jb.Hi;
    for (uint32_t it = 0; it < (uint32_t)(project::kSlice / project::kThreads); ++it) {
        const uint32_t i = base + it * (uint32_t)project::kThreads + threadIdx.x;
        const bool live = i < jb.P;
        bool vis = false;
        if (live) {
            ProjRec& rec = recs[jb.rec_base + i];
            const uint32_t fl = rec.flags & ~IBA_PROJECT_VISIBLE;
            const double u = rec.u, v = rec.v;
            int x0 = 0, y0 = 0;
            if (fl & IBA_PROJECT_INSIDE) {
                x0 = (int)floor(u); y0 = (int)floor(v);
                const float zwin = depth[jb.img_base + (uint64_t)y0 * (uint64_t)Wi + (uint64_t)x0];
                vis = (double)rec.z <= (double)zwin * (1.0 + tol);
            }
            rec.flags = fl | (vis ? IBA_PROJECT_VISIBLE : 0u);
            if (COLOUR) {
                uint8_t out[3] = {0, 0, 0};
                if (vis) {
                    const int x1 = min(x0 + 1, Wi - 1), y1 = min(y0 + 1, Hi - 1);
                    const double a = u - (double)x0, b = v - (double)y0;
                    const uint8_t* p00 = rgb + 3 * ((size_t)y0 * (size_t)Wi + (size_t)x0);
                    const uint8_t* p01 = rgb + 3 * ((size_t)y1 * (size_t)Wi + (size_t)x0);
                    const uint8_t* p10 = rgb + 3 * ((size_t)y0 * (size_t)Wi + (size_t)x1);
                    const uint8_t* p11 = rgb + 3 * ((size_t)y1 * (size_t)Wi + (size_t)x1);
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        const double c00 = (double)p00[c], c01 = (double)p01[c], c10 = (double)p10[c], c11 = (double)p11[c];
                        const double val = ((1.0 - a) * ((1.0 - b) * c00 + b * c01)) + (a * ((1.0 - b) * c10 + b * c11));
                        out[c] = (uint8_t)floor(val + 0.5);
                    }
                }
                point_rgb[3 * (size_t)i] = out[0]; point_rgb[3 * (size_t)i + 1] = out[1]; point_rgb[3 * (size_t)i + 2] = out[2];
            }
        }
        if (!COLOUR) proj_count(&s_cnt, vis);
    }
    if (!COLOUR) {
        __syncthreads();
        if (threadIdx.x == 0u && s_cnt) atomicAdd(cnt + (size_t)j * project::kCounters + project::C_VISIBLE, s_cnt);
    }
}

// one job: blocks of kThreads pixels from its pixel 0
__global__ __launch_bounds__(project::kThreads) void iba_project_overlay_kernel(const ProjJob* __restrict__ job, const float* __restrict__ depth, const uint32_t* __restrict__ index,
                                                                              const uint8_t* __restrict__ rgb, uint8_t* __restrict__ out, double z_near, double z_far) {
    const ProjJob& jb = *job;
    const uint64_t pix = (uint64_t)blockIdx.x * (uint64_t)project::kThreads + threadIdx.x;
    if (pix >= (uint64_t)jb.Wi * (uint64_t)jb.Hi) return;
    uint8_t c[3] = {0, 0, 0};
    if (index[jb.img_base + pix] != 0xFFFFFFFFu) {
        const double z = (double)depth[jb.img_base + pix];
        const double zn = fmin(fmax((z - z_near) / (z_far - z_near), 0.0), 1.0);
        project::gradient(zn, c);
    } else if (rgb) {
        c[0] = rgb[3 * pix]; c[1] = rgb[3 * pix + 1]; c[2] = rgb[3 * pix + 2];
    }
    out[3 * pix] = c[0]; out[3 * pix + 1] = c[1]; out[3 * pix + 2] = c[2];
}

// ---- the launches (declared in iba_internal.hpp); a launch of no blocks is skipped ----

hipError_t project_splat(hipStream_t st, const float4* pts4, const ProjJob* d_jobs, int nj, uint32_t bias, uint32_t n_blocks, int r, double z_min, double z_max,
                         unsigned long long* keys, ProjRec* recs, uint32_t* cnt) {
    if (!n_blocks) return hipSuccess;
    hipLaunchKernelGGL(iba_project_splat_kernel, dim3(n_blocks), dim3(project::kThreads), 0, st, pts4, d_jobs, nj, bias, r, z_min, z_max, keys, recs, cnt);
    return hipGetLastError();
}
hipError_t project_resolve(hipStream_t st, const ProjJob* d_jobs, int nj, uint32_t bias, uint32_t n_blocks, const unsigned long long* keys, float* depth, uint32_t* index, uint32_t* cnt) {
    if (!n_blocks) return hipSuccess;
    hipLaunchKernelGGL(iba_project_resolve_kernel, dim3(n_blocks), dim3(project::kThreads), 0, st, d_jobs, nj, bias, keys, depth, index, cnt);
    return hipGetLastError();
}
hipError_t project_visible(hipStream_t st, const ProjJob* d_jobs, int nj, uint32_t bias, uint32_t n_blocks, double tol, ProjRec* recs, const float* depth, uint32_t* cnt,
                           const uint8_t* rgb, uint8_t* point_rgb) {
    if (!n_blocks) return hipSuccess;
    if (rgb) hipLaunchKernelGGL(iba_project_visible_kernel<true>, dim3(n_blocks), dim3(project::kThreads), 0, st, d_jobs, nj, bias, tol, recs, depth, cnt, rgb, point_rgb);
    else hipLaunchKernelGGL(iba_project_visible_kernel<false>, dim3(n_blocks), dim3(project::kThreads), 0, st, d_jobs, nj, bias, tol, recs, depth, cnt, rgb, point_rgb);
    return hipGetLastError();
}
hipError_t project_overlay(hipStream_t st, const ProjJob* d_job, uint32_t n_blocks, const float* depth, const uint32_t* index, const uint8_t* rgb, uint8_t* out, double z_near, double z_far) {
    if (!n_blocks) return hipSuccess;
    hipLaunchKernelGGL(iba_project_overlay_kernel, dim3(n_blocks), dim3(project::kThreads), 0, st, d_job, depth, index, rgb, out, z_near, z_far);
    return hipGetLastError();
}

}  // namespace iba

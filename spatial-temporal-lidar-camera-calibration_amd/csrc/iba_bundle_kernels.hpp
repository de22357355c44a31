// Bundle adjustment, the kernels (include/iba_mi355x.h, iba_bundle*; rules B1-B10 there, their arithmetic in iba_bundle_math.hpp). One launch chain per
// LM evaluation over the flat tables of ALL jobs of a chunk: every kernel gives the items of iba_bundle_math.hpp to lanes (an edge, a point: one lane;
// a camera's sums, a block of the reduced system: one wave, summed by the DPP tree of iba_pose_kernels.hpp; a job's chi2, its factorisation: one
// workgroup) and returns at once for a job whose sequencer asks for nothing. No workgroup waits for another: kernel boundaries are the only grid-wide
// synchronisation. No floating-point atomics; the integer atomics count outliers, steps beyond pi and the jobs still running, and raise a job's
// failure flag.
#pragma once
#include <hip/hip_runtime.h>

#include "iba_bundle_host.hpp"
#include "iba_wave_sum.hpp"

namespace iba {
namespace bundle {

constexpr int kThreads = 256;
constexpr int kSolveThreads = kMaxReduced;      // one lane per row of the reduced system
constexpr int kMaxGrid = 4096;

__global__ __launch_bounds__(kThreads) void edge_kernel(Tab t, int n, DevOpt o) {
    const int e = blockIdx.x * kThreads + threadIdx.x;
    if (e < n) edge_item(t, e, o);
}
__global__ __launch_bounds__(kThreads) void point_kernel(Tab t, int n) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < n) point_item(t, p);
}
// one wave per camera
__global__ __launch_bounds__(kThreads) void camera_kernel(Tab t, int n) {
    const int cam = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (cam >= n || !camera_runs(t, cam)) return;
    double acc[kCamSums];
    const double cnt = wave_sum_f64((double)camera_lane(t, cam, lane, acc));   // a count below 2^24: exact
#pragma unroll
    for (int k = 0; k < kCamSums; ++k) {
        const double s = wave_sum_f64(acc[k]);
        if (lane == 63) t.cam_sums[(size_t)kCamSums * cam + k] = s;
    }
    if (lane == 63) t.cam_cnt[cam] = (int32_t)cnt;
}
// one workgroup per job: the job's chi2 and largest diagonal, the sequencer's first half on one lane, then the copies it asks for
__global__ __launch_bounds__(kThreads) void front_kernel(Tab t, int n_jobs, DevOpt o) {
    __shared__ double part[kThreads / kWave], mx[kThreads];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (blockIdx.x == 0 && tid == 0) *t.running = 0;
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const int kind = t.ctl[j].kind;
        if (kind == kDone) continue;
        const bool sums = kind == kLinearise || kind == kTrial;
        if (sums) { const double s = wave_sum_f64(chi_lane(t, t.job[j], tid)); if (lane == 63) part[wave] = s; }
        if (kind == kLinearise) mx[tid] = diag_lane(t, t.job[j], tid);
        __syncthreads();
        if (tid == 0) {
            double chi = 0.0, md = 0.0;
            if (sums) chi = (part[0] + part[1]) + (part[2] + part[3]);
            if (kind == kLinearise) for (int l = 0; l < kThreads; ++l) md = larger(md, mx[l]);
            sequence_front(t, j, o, chi, md);
        }
        __syncthreads();
        copy_item(t, j, tid, kThreads);
        __syncthreads();
    }
}
__global__ __launch_bounds__(kThreads) void inverse_kernel(Tab t, int n) {
    const int p = blockIdx.x * kThreads + threadIdx.x;
    if (p < n) inverse_item(t, p);
}
// one wave per block of the reduced system
__global__ __launch_bounds__(kThreads) void block_kernel(Tab t, int n) {
    const int blk = blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (blk >= n || !block_runs(t, blk)) return;
    double acc[kBlockSums];
    block_lane(t, blk, lane, acc);
#pragma unroll
    for (int k = 0; k < kBlockSums; ++k) acc[k] = wave_sum_f64(acc[k]);
    if (lane == 63) block_store(t, blk, acc);
}
// B7 in parallel: lane i owns row i. Column j of the factor needs the columns before it, so a barrier separates the columns; every entry is still
// its a_ij with the products subtracted one at a time, k ascending (the backward substitution: k descending), as reduced_solve does on the host.
__global__ __launch_bounds__(kSolveThreads) void solve_kernel(Tab t, int n_jobs) {
    __shared__ double col[kMaxReduced], vec[kMaxReduced];
    const int i = threadIdx.x;
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        Ctl& c = t.ctl[j];
        if (!c.propose || c.fail) continue;
        const JobRec q = t.job[j];
        const int n = 6 * c.n_part;
        double* S = t.S + q.s0;
        for (int cam = q.cam0 + i; cam < q.cam0 + q.n_cam; cam += kSolveThreads) {
            const int r = t.rank[cam];
            if (r >= 0) for (int k = 0; k < 6; ++k) vec[6 * r + k] = t.bs[6 * (size_t)cam + k];
        }
        __syncthreads();
        bool ok = true;
        for (int jj = 0; jj < n; ++jj) {
            double s = 0.0;
            if (i >= jj && i < n) {
                s = S[sidx(n, i, jj)];
                for (int k = 0; k < jj; ++k) s = s - S[sidx(n, i, k)] * S[sidx(n, jj, k)];
                col[i] = s;
            }
            __syncthreads();
            const double piv = col[jj];
            if (!pivot_ok(piv)) { ok = false; break; }
            const double ljj = std::sqrt(piv);
            if (i == jj) S[sidx(n, i, jj)] = ljj;
            else if (i > jj && i < n) S[sidx(n, i, jj)] = s / ljj;
            __syncthreads();
        }
        if (!ok) {
            if (i == 0) c.fail = 1;
            __syncthreads();
            continue;
        }
        double v = i < n ? vec[i] : 0.0;
        for (int k = 0; k < n; ++k) {
            if (i == k) col[k] = v / S[sidx(n, k, k)];
            __syncthreads();
            if (i > k && i < n) v = v - S[sidx(n, i, k)] * col[k];
        }
        __syncthreads();
        v = i < n ? col[i] : 0.0;
        for (int k = n - 1; k >= 0; --k) {
            if (i == k) vec[k] = v / S[sidx(n, k, k)];
            __syncthreads();
            if (i < k) v = v - S[sidx(n, k, i)] * vec[k];
        }
        __syncthreads();
        for (int cam = q.cam0 + i; cam < q.cam0 + q.n_cam; cam += kSolveThreads) {
            const int r = t.rank[cam];
            if (r >= 0) for (int k = 0; k < 6; ++k) t.dp[6 * (size_t)cam + k] = vec[6 * r + k];
        }
        __syncthreads();
    }
}
// the points' steps and trial positions, then the cameras' trial poses
__global__ __launch_bounds__(kThreads) void update_kernel(Tab t, int n_points, int n_cameras) {
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i < n_points) backsub_item(t, i);
    else if (i - n_points < n_cameras) camera_update_item(t, i - n_points);
}
// the sequencer's second half, one lane per job
__global__ __launch_bounds__(kThreads) void back_kernel(Tab t, int n_jobs, DevOpt o) {
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_jobs) sequence_back(t, j, o);
}

}  // namespace bundle
}  // namespace iba

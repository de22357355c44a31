// Motion-only pose optimisation, the kernels (include/iba_mi355x.h, iba_pose*; rules P1-P8 there, their arithmetic in iba_pose_math.hpp). One workgroup
// of 256 lanes per job, grid-stride over the jobs of a chunk. A job's edges sit in LDS up to `cap` (<= IBA_POSE_ONCHIP_EDGES) and are re-read from
// global memory above it, by the same arithmetic in the same order. Per evaluation the lanes add their edges (edge i on lane i mod 256, ascending),
// the wave sums by DPP, the four waves' partial sums meet in LDS; lane 0 runs the sequencer (lm_next: factor, solve, update, verdict) on work arrays
// in LDS and leaves the kind of the next evaluation in LDS. A round is ONE loop of evaluations: every wave reads that word as a scalar after the
// barrier, so every branch around a barrier is a uniform scalar branch. No floating-point atomics; the only atomic is the integer count of a round's
// outliers in LDS.
#pragma once
#include <hip/hip_runtime.h>

#include "iba_pose_host.hpp"
#include "iba_wave_sum.hpp"

namespace iba {
namespace pose {

constexpr int kThreads = kLanes;
constexpr int kMaxGrid = 512;
constexpr int kCap = IBA_POSE_ONCHIP_EDGES;

struct JobRec { int32_t base, n; float fx, fy, cx, cy; double T[12]; };
struct DevOpt { int32_t rounds, iterations, robust_rounds; float chi2_threshold; double delta; };

struct Shared {
    float xyz[3 * kCap], obs[2 * kCap], w[kCap];
    uint8_t bad[kCap];
    double part[kThreads / 64][kSums];
    double sums[kSums], trial[kSums], T[12];
    Lm lm;
    LmWork work;
    int32_t nbad, phase;
};

// a control word that lane 0 left in LDS before a barrier, as a wave-uniform scalar: the branches around the barriers are scalar branches
__device__ __forceinline__ int uniform(int x) { return __builtin_amdgcn_readfirstlane(x); }

struct JobView {                // a job's slices of the chunk's arrays
    const float* xyz; const float* obs; const float* w;
    uint8_t* bad;               // 1 = not active; global, read for the edges at or above cap
    int32_t n, cap;
    Cam K;
};

// an edge from LDS (ONCHIP, i < cap) or from global memory; the two are never chosen per access: a lane walks its on-chip edges, then the others
template <int ONCHIP>
__device__ __forceinline__ void load_edge(const Shared& sh, const JobView& v, int i, double* e) {
    if (ONCHIP) {
        e[0] = sh.xyz[3 * i]; e[1] = sh.xyz[3 * i + 1]; e[2] = sh.xyz[3 * i + 2]; e[3] = sh.obs[2 * i]; e[4] = sh.obs[2 * i + 1]; e[5] = sh.w[i];
    } else {
        e[0] = v.xyz[3 * i]; e[1] = v.xyz[3 * i + 1]; e[2] = v.xyz[3 * i + 2]; e[3] = v.obs[2 * i]; e[4] = v.obs[2 * i + 1]; e[5] = v.w[i];
    }
}
template <int FULL, int ONCHIP>
__device__ __forceinline__ void add_edge(const Shared& sh, const JobView& v, int i, double* acc, const double* T, int robust, double delta) {
    if (ONCHIP ? sh.bad[i] : v.bad[i]) return;
    double e[6];
    load_edge<ONCHIP>(sh, v, i, e);
    accumulate<FULL>(acc, T, v.K, e[0], e[1], e[2], e[3], e[4], e[5], robust, delta);
}
template <int ONCHIP>
__device__ __forceinline__ double edge_chi2(const Shared& sh, const JobView& v, int i, const double* T) {
    double e[6], ex, ey, c;
    load_edge<ONCHIP>(sh, v, i, e);
    edge(T, v.K, e[0], e[1], e[2], e[3], e[4], e[5], &ex, &ey, &c, nullptr);
    return c;
}

// the on-chip part of a job into LDS; flags: the job's `bad` bytes as they stand in global memory
__device__ __forceinline__ void load_job(Shared& sh, const JobView& v) {
    const int m = v.n < v.cap ? v.n : v.cap;
    for (int i = threadIdx.x; i < m; i += kThreads) {
        sh.xyz[3 * i] = v.xyz[3 * i]; sh.xyz[3 * i + 1] = v.xyz[3 * i + 1]; sh.xyz[3 * i + 2] = v.xyz[3 * i + 2];
        sh.obs[2 * i] = v.obs[2 * i]; sh.obs[2 * i + 1] = v.obs[2 * i + 1]; sh.w[i] = v.w[i]; sh.bad[i] = v.bad[i];
    }
}

// P3, collective: the sums at the pose Tl (LDS) into out (LDS, kSums; FULL = 0 writes out[27] alone). Ends behind a barrier.
template <int FULL>
__device__ __forceinline__ void job_sums(Shared& sh, const JobView& v, const double* Tl, int robust, double delta, double* out) {
    double T[12], acc[kSums];
#pragma unroll
    for (int k = 0; k < 12; ++k) T[k] = Tl[k];
#pragma unroll
    for (int k = 0; k < kSums; ++k) acc[k] = 0.0;
    const int m = v.n < v.cap ? v.n : v.cap;
    int i = threadIdx.x;
    for (; i < m; i += kThreads) add_edge<FULL, 1>(sh, v, i, acc, T, robust, delta);
    for (; i < v.n; i += kThreads) add_edge<FULL, 0>(sh, v, i, acc, T, robust, delta);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = FULL ? 0 : kSums - 1; k < kSums; ++k) { const double t = wave_sum_f64(acc[k]); if (lane == 63) sh.part[wave][k] = t; }
    __syncthreads();
    if ((int)threadIdx.x < kSums && (FULL || threadIdx.x == kSums - 1))
        out[threadIdx.x] = (sh.part[0][threadIdx.x] + sh.part[1][threadIdx.x]) + (sh.part[2][threadIdx.x] + sh.part[3][threadIdx.x]);
    __syncthreads();
}

__device__ __forceinline__ JobView view_of(const JobRec& rec, const float* xyz, const float* obs, const float* w, uint8_t* bad, int cap) {
    JobView v;
    v.xyz = xyz + 3 * (size_t)rec.base; v.obs = obs + 2 * (size_t)rec.base; v.w = w + rec.base; v.bad = bad + rec.base;
    v.n = rec.n; v.cap = cap;
    v.K = Cam{(double)rec.fx, (double)rec.fy, (double)rec.cx, (double)rec.cy};
    return v;
}

// ---- iba_pose_optimize: the whole schedule of P4-P8 per job. outlier is zero on entry; outs holds every job's start (host: start_out). ----
__global__ __launch_bounds__(kThreads) void pose_optimize_kernel(const JobRec* __restrict__ recs, int n_jobs, const float* __restrict__ xyz, const float* __restrict__ obs,
                                                                 const float* __restrict__ w, uint8_t* outlier, float* __restrict__ chi2, JobOut* __restrict__ outs, DevOpt o, int cap) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const JobRec rec = recs[j];
        if (rec.n < 3) continue;                      // P8: the host's start_out is the answer
        const JobView v = view_of(rec, xyz, obs, w, outlier, cap);
        load_job(sh, v);
        if (tid == 0) sh.lm.big = 0;
        for (int round = 0; round < o.rounds; ++round) {
            const int robust = round < o.robust_rounds ? 1 : 0;
            if (tid < 12) sh.T[tid] = recs[j].T[tid]; // every round restarts from the start pose
            if (tid == 0) { sh.nbad = 0; sh.phase = 0; lm_round_start(&sh.lm); }
            __syncthreads();
            // the optimisation as a sequence of evaluations: lane 0 leaves the next one's kind in LDS (lm_next), every wave reads it as a scalar
            for (;;) {
                const int phase = uniform(sh.phase);
                if (phase == 2) break;
                if (phase == 0) job_sums<1>(sh, v, sh.T, robust, o.delta, sh.sums);
                else job_sums<0>(sh, v, sh.work.Tn, robust, o.delta, sh.trial);
                if (tid == 0) sh.phase = lm_next(&sh.lm, &sh.work, sh.sums, sh.trial[kSums - 1], sh.T, phase, o.iterations);
                __syncthreads();
            }
            // P7: every edge at the round's final accepted pose; a lane owns its edges' flags
            {
                double T[12];
#pragma unroll
                for (int k = 0; k < 12; ++k) T[k] = sh.T[k];
                const int m = v.n < v.cap ? v.n : v.cap;
                int nb = 0, i = tid;
                for (; i < m; i += kThreads) {
                    const double c = edge_chi2<1>(sh, v, i, T);
                    const int bad = is_outlier(c, o.chi2_threshold);
                    sh.bad[i] = (uint8_t)bad; v.bad[i] = (uint8_t)bad;
                    chi2[(size_t)rec.base + i] = canonf((float)c);
                    nb += bad;
                }
                for (; i < v.n; i += kThreads) {
                    const double c = edge_chi2<0>(sh, v, i, T);
                    const int bad = is_outlier(c, o.chi2_threshold);
                    v.bad[i] = (uint8_t)bad;
                    chi2[(size_t)rec.base + i] = canonf((float)c);
                    nb += bad;
                }
                if (nb) atomicAdd(&sh.nbad, nb);
            }
            __syncthreads();
            if (tid == 0) {
                JobOut& q = outs[j];
                q.r.chi2[round] = canon(sh.lm.current); q.r.n_bad[round] = sh.nbad; q.r.lm_iterations[round] = sh.lm.its; q.r.trials[round] = sh.lm.trials;
                for (int k = 0; k < 12; ++k) q.stage[12 * round + k] = sh.T[k];
                q.r.rounds_run = round + 1;
                q.r.n_inliers = rec.n - sh.nbad;
            }
            __syncthreads();                          // the next round's start pose overwrites the sh.T that lane 0 has just read
            if (rec.n < 10) break;                    // optimizer.edges().size() < 10
        }
        if (tid == 0) {
            JobOut& q = outs[j];
            for (int k = 0; k < 12; ++k) { q.r.Tcw12[k] = sh.T[k]; q.r.Tcw12f[k] = (float)sh.T[k]; }
            q.big_steps = sh.lm.big;
        }
        __syncthreads();                              // the next job overwrites the LDS this one read
    }
}

// ---- iba_pose_eval: one linearisation per job at its pose. bad = the complement of the caller's active mask. out: n_jobs x kSums. ----
__global__ __launch_bounds__(kThreads) void pose_eval_kernel(const JobRec* __restrict__ recs, int n_jobs, const float* __restrict__ xyz, const float* __restrict__ obs,
                                                             const float* __restrict__ w, uint8_t* bad, int robust, double delta, double* __restrict__ out,
                                                             double* __restrict__ chi2_edges, int cap) {
    __shared__ Shared sh;
    const int tid = threadIdx.x;
    for (int j = blockIdx.x; j < n_jobs; j += gridDim.x) {
        const JobRec rec = recs[j];
        const JobView v = view_of(rec, xyz, obs, w, bad, cap);
        load_job(sh, v);
        if (tid < 12) sh.T[tid] = recs[j].T[tid];
        __syncthreads();
        job_sums<1>(sh, v, sh.T, robust, delta, sh.sums);
        if (tid < kSums) out[(size_t)j * kSums + tid] = canon(sh.sums[tid]);
        if (chi2_edges) {
            double T[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) T[k] = sh.T[k];
            const int m = v.n < v.cap ? v.n : v.cap;
            int i = tid;
            for (; i < m; i += kThreads) chi2_edges[(size_t)rec.base + i] = canon(edge_chi2<1>(sh, v, i, T));
            for (; i < v.n; i += kThreads) chi2_edges[(size_t)rec.base + i] = canon(edge_chi2<0>(sh, v, i, T));
        }
        __syncthreads();
    }
}

}  // namespace pose
}  // namespace iba

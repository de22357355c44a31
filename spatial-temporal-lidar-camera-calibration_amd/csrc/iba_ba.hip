// ORB-only extrinsic bundle adjustment: one 7-vector vertex, N unary reprojection edges.
// Reference: calibEdge / CalibVertex (Optimizer.cc:40-205), OptimizeExtrinsicLocal / OptimizeExtrinsicGlobal
// (Optimizer.cc:1399-1564, 1566-1744), called from ba_calib.cpp:71,79.
//
// Device: one lane per edge (grid-stride). The residual is the reference's functor evaluated on forward-mode duals
// (what G2O_MAKE_AUTO_AD_FUNCTIONS does with ceres::Jet), the robust weight is g2o's RobustKernelHuber applied the way
// BaseUnaryEdge::constructQuadraticForm does (rho' scales the information), 28 + 7 + 1 sums per lane are reduced with
// DPP wave sums and a fixed-order block / grid sum (bitwise reproducible). HBM traffic is 60 B per edge; the kernel is
// bound by the ~1.5 k double-precision operations per edge (3 Rodrigues rotations on 7-wide duals).
// Host: g2o's OptimizationAlgorithmLevenberg restated (tau = 1e-5, Nielsen's rho / lambda update with the 1/3..2/3 clamp,
// 10 trials after a failure) and the reference's four rounds. g2o is third party and absent: PARITY WITH IT IS UNPINNED;
// tests compare with oracle/ba_oracle.cpp + an independent Python restatement of the same schedule.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_device_buf.hpp"
#include "iba_lm.hpp"
#include "iba_wave_sum.hpp"

namespace {

struct DJ { double a, v[7]; };   // value and d/dx[0..6]
__device__ __forceinline__ DJ dj(double s) { DJ r; r.a = s; for (int i = 0; i < 7; ++i) r.v[i] = 0; return r; }
__device__ __forceinline__ DJ dj_var(double s, int k) { DJ r = dj(s); r.v[k] = 1.0; return r; }
__device__ __forceinline__ DJ operator+(const DJ& f, const DJ& g) { DJ h; h.a = f.a + g.a; for (int i = 0; i < 7; ++i) h.v[i] = f.v[i] + g.v[i]; return h; }
__device__ __forceinline__ DJ operator-(const DJ& f, const DJ& g) { DJ h; h.a = f.a - g.a; for (int i = 0; i < 7; ++i) h.v[i] = f.v[i] - g.v[i]; return h; }
__device__ __forceinline__ DJ operator-(const DJ& f) { DJ h; h.a = -f.a; for (int i = 0; i < 7; ++i) h.v[i] = -f.v[i]; return h; }
__device__ __forceinline__ DJ operator*(const DJ& f, const DJ& g) { DJ h; h.a = f.a * g.a; for (int i = 0; i < 7; ++i) h.v[i] = f.a * g.v[i] + f.v[i] * g.a; return h; }
__device__ __forceinline__ DJ operator/(const DJ& f, const DJ& g) {
    DJ h; const double gi = 1.0 / g.a, fg = f.a * gi; h.a = fg;
    for (int i = 0; i < 7; ++i) h.v[i] = (f.v[i] - fg * g.v[i]) * gi;
    return h;
}
__device__ __forceinline__ DJ dj_sqrt(const DJ& f) { DJ h; const double t = sqrt(f.a), ti = 1.0 / (2.0 * t); h.a = t; for (int i = 0; i < 7; ++i) h.v[i] = f.v[i] * ti; return h; }
__device__ __forceinline__ DJ dj_cos(const DJ& f) { DJ h; h.a = cos(f.a); const double s = -sin(f.a); for (int i = 0; i < 7; ++i) h.v[i] = s * f.v[i]; return h; }
__device__ __forceinline__ DJ dj_sin(const DJ& f) { DJ h; h.a = sin(f.a); const double c = cos(f.a); for (int i = 0; i < 7; ++i) h.v[i] = c * f.v[i]; return h; }

struct DV3 { DJ x, y, z; };
__device__ __forceinline__ DV3 dcross(const DV3& a, const DV3& b) { return DV3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ DJ ddot(const DV3& a, const DV3& b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
// the angle-axis block of calibEdge::operator() (Optimizer.cc:95-112, 116-133, 136-155, 158-177)
__device__ __forceinline__ DV3 drotate(const DV3& w, const DV3& p) {
    const DJ theta = dj_sqrt(ddot(w, w));
    if (theta.a > 0.0) {
        const DV3 v = {w.x / theta, w.y / theta, w.z / theta};
        const DJ cth = dj_cos(theta), sth = dj_sin(theta);
        const DV3 vxp = dcross(v, p);
        const DJ vdp = ddot(v, p);
        // 1 - cos(theta) as sin^2 / (1 + cos) where cos > 0: the literal difference of the reference is good to one epsilon of 1
        // only, and dv ~ 1 / theta multiplies it, which costs the Jacobian eps / theta at a small non-zero theta
        DJ omc; omc.a = cth.a > 0.0 ? sth.a * sth.a / (1.0 + cth.a) : 1.0 - cth.a;
        for (int i = 0; i < 7; ++i) omc.v[i] = sth.a * theta.v[i];
        return DV3{p.x * cth + vxp.x * sth + v.x * vdp * omc, p.y * cth + vxp.y * sth + v.y * vdp * omc, p.z * cth + vxp.z * sth + v.z * vdp * omc};
    }
    const DV3 wxp = dcross(w, p);
    return DV3{p.x + wxp.x, p.y + wxp.y, p.z + wxp.z};
}

struct BaDev {
    int64_t n_edges;
    const double* frame_Tlw6; const double* frame_intr;
    const int32_t* edge_frame; const double* edge_Xw; const double* edge_obs; const double* edge_info;
};
struct BaX { double x[7]; };
constexpr int kBaThreads = 256, kBaSums = 36;   // 28 (upper H) + 7 (b) + 1 (robust chi2)

__global__ __launch_bounds__(kBaThreads) void ba_edge_kernel(BaDev d, BaX X, const uint8_t* __restrict__ active, int robust, double delta,
                                                              double* __restrict__ block_sums, double* __restrict__ chi2_edges) {
    __shared__ double s_part[kBaThreads / 64][kBaSums];
    double acc[kBaSums];
#pragma unroll
    for (int i = 0; i < kBaSums; ++i) acc[i] = 0.0;
    DJ c[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) c[i] = dj_var(X.x[i], i);
    const DV3 wlc = {-c[0], -c[1], -c[2]}, tneg = {-c[3], -c[4], -c[5]};
    const DV3 tlc = drotate(wlc, tneg);                       // T_lc translation: the same for every edge
    const DV3 wcl = {c[0], c[1], c[2]};
    for (int64_t i = (int64_t)blockIdx.x * kBaThreads + threadIdx.x; i < d.n_edges; i += (int64_t)gridDim.x * kBaThreads) {
        const int f = d.edge_frame[i];
        const double* Xw = d.edge_Xw + 3 * i;
        const double* T6 = d.frame_Tlw6 + 6 * (size_t)f;
        const double* in = d.frame_intr + 4 * (size_t)f;
        const DV3 Xc0 = {c[6] * dj(Xw[0]), c[6] * dj(Xw[1]), c[6] * dj(Xw[2])};
        DV3 Xl0 = drotate(wlc, Xc0);
        Xl0 = DV3{Xl0.x + tlc.x, Xl0.y + tlc.y, Xl0.z + tlc.z};
        const DV3 wlw = {dj(T6[0]), dj(T6[1]), dj(T6[2])};
        DV3 Xli = drotate(wlw, Xl0);
        Xli = DV3{Xli.x + dj(T6[3]), Xli.y + dj(T6[4]), Xli.z + dj(T6[5])};
        DV3 Xci = drotate(wcl, Xli);
        Xci = DV3{Xci.x + c[3], Xci.y + c[4], Xci.z + c[5]};
        const DJ pu = dj(in[0]) * Xci.x / Xci.z + dj(in[2]);
        const DJ pv = dj(in[1]) * Xci.y / Xci.z + dj(in[3]);
        const DJ e0 = dj(d.edge_obs[2 * i]) - pu, e1 = dj(d.edge_obs[2 * i + 1]) - pv;
        const double info = d.edge_info[i];
        const double chi2 = info * (e0.a * e0.a + e1.a * e1.a);
        if (chi2_edges) chi2_edges[i] = chi2;
        if (active && !active[i]) continue;
        double rho0 = chi2, rho1 = 1.0;
        if (robust) {   // RobustKernelHuber::robustify
            const double dsqr = delta * delta;
            if (chi2 > dsqr) { const double sq = sqrt(chi2); rho0 = 2 * sq * delta - dsqr; rho1 = delta / sq; }
        }
        const double w = rho1 * info;
        int at = 0;
#pragma unroll
        for (int p = 0; p < 7; ++p) {
#pragma unroll
            for (int q = p; q < 7; ++q) acc[at++] += w * (e0.v[p] * e0.v[q] + e1.v[p] * e1.v[q]);
        }
#pragma unroll
        for (int p = 0; p < 7; ++p) acc[28 + p] -= w * (e0.v[p] * e0.a + e1.v[p] * e1.a);
        acc[35] += rho0;
    }
    // the tail iba::block_sum_store states, written out: that helper takes all K wave sums at once, and with 36 of them in flight this kernel compiles
    // to other code than with each one stored as it is formed
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < kBaSums; ++i) { const double t = iba::wave_sum_f64(acc[i]); if (lane == 63) s_part[wave][i] = t; }
    __syncthreads();
    if (threadIdx.x < kBaSums) {
        double t = s_part[0][threadIdx.x];
        for (int w = 1; w < kBaThreads / 64; ++w) t += s_part[w][threadIdx.x];
        block_sums[(size_t)blockIdx.x * kBaSums + threadIdx.x] = t;
    }
}
__global__ __launch_bounds__(64) void ba_reduce_kernel(const double* __restrict__ block_sums, int nblocks, double* __restrict__ out) {
    const int i = threadIdx.x;
    if (i >= kBaSums) return;
    double t = 0;
    for (int b = 0; b < nblocks; ++b) t += block_sums[(size_t)b * kBaSums + i];   // fixed order
    out[i] = t;
}

}  // namespace

struct iba_ba_handle {
    int device = 0;
    int64_t n_edges = 0;
    int n_frames = 0;
    iba::DevBuf<double> Tlw6, intr, Xw, obs, info, block_sums, out, chi2;
    iba::DevBuf<int32_t> frame;
    iba::DevBuf<uint8_t> active;
    std::vector<int32_t> slot;
    int nblocks = 0;
    std::string err;
    hipStream_t stream = nullptr;
};

namespace {
iba_status ba_fail(iba_ba_handle* h, iba_status s, const std::string& m) { if (h) h->err = m; return s; }
}

extern "C" {

const char* iba_ba_last_error(const iba_ba_handle* h) { return h ? h->err.c_str() : "iba_ba: creation failed (no gfx950 device / bad descriptor)"; }

void iba_ba_destroy(iba_ba_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamDestroy(h->stream);
    delete h;
}

iba_status iba_ba_create(const iba_ba_desc* d, int device, iba_ba_handle** out) {
    if (out) *out = nullptr;
    if (!d || !out || d->n_edges < 0 || d->n_frames < 1 || !d->frame_Tlw6 || !d->frame_intr || (d->n_edges && (!d->edge_frame || !d->edge_Xw || !d->edge_obs || !d->edge_info)))
        return IBA_ERR_INVALID_ARG;
    for (int64_t i = 0; i < d->n_edges; ++i)
        if (d->edge_frame[i] < 0 || d->edge_frame[i] >= d->n_frames || (d->edge_slot && d->edge_slot[i] < 0)) return IBA_ERR_INVALID_ARG;   // the slot indexes the outlier flags
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= device || device < 0) return IBA_ERR_NO_DEVICE;   // no CPU fallback
    if (hipSetDevice(device) != hipSuccess) return IBA_ERR_NO_DEVICE;
    iba_ba_handle* h = new iba_ba_handle();
    h->device = device; h->n_edges = d->n_edges; h->n_frames = d->n_frames;
    const size_t N = (size_t)d->n_edges, F = (size_t)d->n_frames;
    h->nblocks = (int)std::min<size_t>(2048, std::max<size_t>(1, (N + kBaThreads - 1) / kBaThreads));
    hipError_t e = hipSuccess;
    auto up = [&](hipError_t r) { if (e == hipSuccess) e = r; };
    up(h->Tlw6.upload(d->frame_Tlw6, 6 * F)); up(h->intr.upload(d->frame_intr, 4 * F)); up(h->frame.upload(d->edge_frame, N));
    up(h->Xw.upload(d->edge_Xw, 3 * N)); up(h->obs.upload(d->edge_obs, 2 * N)); up(h->info.upload(d->edge_info, N));
    std::vector<double> z((size_t)h->nblocks * kBaSums, 0.0);
    up(h->block_sums.upload(z.data(), z.size())); up(h->out.upload(z.data(), kBaSums));
    std::vector<double> zc(std::max<size_t>(N, 1), 0.0);
    up(h->chi2.upload(zc.data(), N));
    std::vector<uint8_t> on(std::max<size_t>(N, 1), 1);
    up(h->active.upload(on.data(), N));
    up(hipStreamCreate(&h->stream));
    if (e != hipSuccess) { iba_ba_destroy(h); return IBA_ERR_HIP; }
    h->slot.resize(N);
    for (size_t i = 0; i < N; ++i) h->slot[i] = d->edge_slot ? d->edge_slot[i] : (int32_t)i;
    *out = h;
    return IBA_OK;
}

iba_status iba_ba_eval(iba_ba_handle* h, const double* x, const uint8_t* active, int32_t robust, double* H, double* b, double* chi2_robust, double* chi2_edges) {
    if (!h || !x || !H || !b || !chi2_robust) return ba_fail(h, IBA_ERR_INVALID_ARG, "null argument");
    if (hipSetDevice(h->device) != hipSuccess) return ba_fail(h, IBA_ERR_HIP, "hipSetDevice");
    const size_t N = (size_t)h->n_edges;
    if (active && N && hipMemcpyAsync(h->active.p, active, N, hipMemcpyHostToDevice, h->stream) != hipSuccess) return ba_fail(h, IBA_ERR_HIP, "upload of the active mask");
    BaDev d{h->n_edges, h->Tlw6.p, h->intr.p, h->frame.p, h->Xw.p, h->obs.p, h->info.p};
    BaX X; std::memcpy(X.x, x, sizeof(X.x));
    const double delta = std::sqrt(5.991);   // deltaMono (Optimizer.cc:1453, 1626)
    hipLaunchKernelGGL(ba_edge_kernel, dim3(h->nblocks), dim3(kBaThreads), 0, h->stream, d, X, active ? h->active.p : (const uint8_t*)nullptr, (int)robust, delta,
                       h->block_sums.p, chi2_edges ? h->chi2.p : (double*)nullptr);
    hipLaunchKernelGGL(ba_reduce_kernel, dim3(1), dim3(64), 0, h->stream, h->block_sums.p, h->nblocks, h->out.p);
    double sums[kBaSums];
    if (hipMemcpyAsync(sums, h->out.p, sizeof(sums), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return ba_fail(h, IBA_ERR_HIP, "download of the sums");
    if (chi2_edges && N && hipMemcpyAsync(chi2_edges, h->chi2.p, N * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) return ba_fail(h, IBA_ERR_HIP, "download of chi2");
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return ba_fail(h, IBA_ERR_HIP, std::string("ba kernels: ") + hipGetErrorString(e));
    int at = 0;
    for (int p = 0; p < 7; ++p) for (int q = p; q < 7; ++q) { H[p * 7 + q] = sums[at]; H[q * 7 + p] = sums[at]; ++at; }
    for (int p = 0; p < 7; ++p) b[p] = sums[28 + p];
    *chi2_robust = sums[35];
    return IBA_OK;
}

iba_status iba_ba_optimize(iba_ba_handle* h, const double* x0, iba_ba_result* res) {
    if (!h || !x0 || !res) return ba_fail(h, IBA_ERR_INVALID_ARG, "null argument");
    const size_t N = (size_t)h->n_edges;
    std::memset(res, 0, sizeof(*res));
    res->n_edges = (int32_t)N;
    std::memcpy(res->x, x0, sizeof(res->x));
    if (N < 3) return IBA_OK;   // nInitialCorrespondences < 3 (Optimizer.cc:1508)
    std::vector<uint8_t> active(N, 1);            // level 0
    std::vector<double> chi2_stored(N, 0.0), chi2_now(N);
    size_t nflags = 0;
    for (size_t i = 0; i < N; ++i) nflags = std::max(nflags, (size_t)h->slot[i] + 1);
    std::vector<uint8_t> outlier_flag(nflags, 0);   // vbOutlier, indexed by the edge's slot (aliases across keyframes)
    double x[7];
    int robust = 1, nbad = 0;
    iba_status st = IBA_OK;
    for (int round = 0; round < 4; ++round) {
        std::memcpy(x, x0, sizeof(x));           // v->setEstimate(p_tcl): every round restarts from the initial estimate
        // ---- optimizer.optimize(10): g2o OptimizationAlgorithmLevenberg ----
        double lambda = 0, ni = 2;
        double H[49], b[7], chi;
        for (int it = 0; it < 10; ++it) {
            st = iba_ba_eval(h, x, active.data(), robust, H, b, &chi, nullptr); if (st != IBA_OK) return st;
            ++res->evaluations; ++res->lm_iterations;
            double current = chi;
            if (it == 0) { double md = 0; for (int k = 0; k < 7; ++k) md = std::max(md, std::fabs(H[k * 8])); lambda = 1e-5 * md; ni = 2; }   // computeLambdaInit
            double rho = 0;
            int qmax = 0;
            bool finite_lambda = true;
            do {
                double A[49], dx[7], xn[7];
                std::memcpy(A, H, sizeof(A));
                for (int k = 0; k < 7; ++k) A[k * 8] += lambda;
                const bool ok2 = iba::chol_solve7(A, b, dx);
                double temp = std::numeric_limits<double>::max();
                if (ok2) {
                    for (int k = 0; k < 7; ++k) xn[k] = x[k] + dx[k];   // CalibVertex::oplusImpl: additive
                    double Hn[49], bn[7];
                    st = iba_ba_eval(h, xn, active.data(), robust, Hn, bn, &temp, nullptr); if (st != IBA_OK) return st;
                    ++res->evaluations;
                }
                rho = current - temp;
                double scale = 1e-3;   // computeScale() + 1e-3
                if (ok2) for (int k = 0; k < 7; ++k) scale += dx[k] * (lambda * dx[k] + b[k]);
                rho /= scale;
                if (rho > 0 && std::isfinite(temp)) {
                    double alpha = 1.0 - std::pow(2 * rho - 1, 3);
                    alpha = std::min(alpha, 2.0 / 3.0);
                    lambda *= std::max(1.0 / 3.0, alpha);
                    ni = 2;
                    current = temp;
                    std::memcpy(x, xn, sizeof(x));
                } else {
                    lambda *= ni; ni *= 2;
                    if (!std::isfinite(lambda)) { finite_lambda = false; break; }
                }
                ++qmax;
            } while (rho < 0 && qmax < 10);
            if (qmax == 10 || rho == 0 || !finite_lambda) break;   // Terminate
        }
        // ---- classification (Optimizer.cc:1524-1550) ----
        double chi_final;
        st = iba_ba_eval(h, x, active.data(), robust, H, b, &chi_final, chi2_now.data()); if (st != IBA_OK) return st;
        ++res->evaluations;
        res->chi2[round] = chi_final;
        nbad = 0;
        for (size_t i = 0; i < N; ++i) {
            const size_t idx = (size_t)h->slot[i];
            if (active[i] || outlier_flag[idx]) chi2_stored[i] = chi2_now[i];   // active edges carry the final errors; flagged ones are recomputed
            if ((float)chi2_stored[i] > 5.991f) { outlier_flag[idx] = 1; active[i] = 0; ++nbad; }   // `const float chi2 = e->chi2()`
            else { outlier_flag[idx] = 0; active[i] = 1; }
        }
        res->n_bad[round] = nbad;
        if (round == 2) robust = 0;   // e->setRobustKernel(0)
        if (N < 10) break;            // optimizer.edges().size() < 10
    }
    std::memcpy(res->x, x, sizeof(x));
    res->n_inliers = (int32_t)N - nbad;
    return IBA_OK;
}

}  // extern "C"

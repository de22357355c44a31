// Motion-only pose optimisation, the arithmetic of rules P1-P8 (include/iba_mi355x.h, iba_pose*): ONE text for the kernels (iba_pose_kernels.hpp),
// the host restatement (iba_pose_host.hpp) and the stand-alone sanitizer self-test, which compiles this file with plain g++. Everything on the
// byte-for-byte path is + - x / sqrt on float64, every operation rounded, left to right, no contraction; libm is called only beyond theta = pi (P6).
#pragma once
#include <cmath>
#include <cstdint>

#include "iba_icp_math.hpp"

#if defined(__HIPCC__)
#define IBA_POSE_HD __host__ __device__ inline
#else
#define IBA_POSE_HD inline
#endif
#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace iba {
namespace pose {

constexpr int kLanes = 256;                 // P3: the lanes of a job's sums
constexpr int kSums = 28;                   // 21 (H, upper triangle by rows) + 6 (b) + 1 (robust chi2)
constexpr int kMaxRounds = 8;
constexpr int kMaxTrials = 10;
constexpr int kSeriesTerms = 14;            // P6
constexpr double kPi2 = 9.869604401089358;  // the double nearest pi^2
constexpr double kMax = 1.7976931348623157e308;

IBA_POSE_HD bool finite_(double x) { return x >= -kMax && x <= kMax; }
// a NaN that is stored into an output is stored as this one
IBA_POSE_HD double canon(double x) {
    if (x == x) return x;
    const uint64_t b = 0x7FF8000000000000ull;
    double c;
    __builtin_memcpy(&c, &b, 8);
    return c;
}
IBA_POSE_HD float canonf(float x) {
    if (x == x) return x;
    const uint32_t b = 0x7FC00000u;
    float c;
    __builtin_memcpy(&c, &b, 4);
    return c;
}
// index of H(p, q), p <= q, in the upper triangle by rows
IBA_POSE_HD int hidx(int p, int q) { return p * 6 - p * (p - 1) / 2 + (q - p); }

struct Cam { double fx, fy, cx, cy; };

// ---- P1: one edge at pose T (3 x 4 row-major): error, chi2, and where J != nullptr the 2 x 6 Jacobian (row-major 12, rotation columns first) ----
IBA_POSE_HD void edge(const double* T, const Cam& K, double X, double Y, double Z, double ox, double oy, double w, double* ex, double* ey, double* chi2, double* J) {
    const double px = ((T[0] * X + T[1] * Y) + T[2] * Z) + T[3];
    const double py = ((T[4] * X + T[5] * Y) + T[6] * Z) + T[7];
    const double pz = ((T[8] * X + T[9] * Y) + T[10] * Z) + T[11];
    const double e0 = ox - ((K.fx * px) / pz + K.cx), e1 = oy - ((K.fy * py) / pz + K.cy);
    *ex = e0; *ey = e1;
    *chi2 = w * (e0 * e0 + e1 * e1);
    if (!J) return;
    const double iz = 1.0 / pz, iz2 = iz * iz;
    J[0] = ((px * py) * iz2) * K.fx;
    J[1] = (-(1.0 + (px * px) * iz2)) * K.fx;
    J[2] = (py * iz) * K.fx;
    J[3] = (-iz) * K.fx;
    J[4] = 0.0;
    J[5] = (px * iz2) * K.fx;
    J[6] = (1.0 + (py * py) * iz2) * K.fy;
    J[7] = (-((px * py) * iz2)) * K.fy;
    J[8] = (-(px * iz)) * K.fy;
    J[9] = 0.0;
    J[10] = (-iz) * K.fy;
    J[11] = (py * iz2) * K.fy;
}

// ---- P2: RobustKernelHuber as BaseUnaryEdge::constructQuadraticForm applies it: rho (what the chi2 sum takes) and rho' (what scales the information) ----
IBA_POSE_HD void huber(double chi2, int robust, double delta, double* rho0, double* rho1) {
    *rho0 = chi2; *rho1 = 1.0;
    if (!robust) return;
    const double dsqr = delta * delta;
    if (chi2 > dsqr) { const double sq = std::sqrt(chi2); *rho0 = (2.0 * sq) * delta - dsqr; *rho1 = delta / sq; }
}

// one active edge into a lane's 28 sums (P3: ascending edge index inside a lane); FULL = 0 takes the chi2 sum alone (a trial needs no more)
template <int FULL>
IBA_POSE_HD void accumulate(double* acc, const double* T, const Cam& K, double X, double Y, double Z, double ox, double oy, double w, int robust, double delta) {
    double ex, ey, chi2, J[12], rho0, rho1;
    edge(T, K, X, Y, Z, ox, oy, w, &ex, &ey, &chi2, FULL ? J : nullptr);
    huber(chi2, robust, delta, &rho0, &rho1);
    if (FULL) {
        const double wr = rho1 * w;
        int at = 0;
#pragma unroll
        for (int p = 0; p < 6; ++p) {
#pragma unroll
            for (int q = p; q < 6; ++q) { acc[at] = acc[at] + wr * (J[p] * J[q] + J[6 + p] * J[6 + q]); ++at; }
        }
#pragma unroll
        for (int p = 0; p < 6; ++p) acc[21 + p] = acc[21 + p] - wr * (J[p] * ex + J[6 + p] * ey);
    }
    acc[27] = acc[27] + rho0;
}

// ---- P6: the three coefficients as fixed series in s = theta^2, the last two steps compensated (Dekker, + - x / only) ----
IBA_POSE_HD void two_sum(double a, double b, double* s, double* e) { const double t = a + b, bb = t - a; *s = t; *e = (a - (t - bb)) + (b - bb); }
IBA_POSE_HD void two_prod(double a, double b, double* p, double* e) {
    const double q = a * b;
    const double ca = 134217729.0 * a, ah = ca - (ca - a), al = a - ah;
    const double cb = 134217729.0 * b, bh = cb - (cb - b), bl = b - bh;
    *p = q; *e = ((ah * bh - q) + ah * bl + al * bh) + al * bl;
}
// (h, l) = 1 - (s / d) (ah + al)
IBA_POSE_HD void series_step(double s, double d, double ah, double al, double* h, double* l) {
    double p, e, pp, ee, hh, ll;
    two_prod(s, ah, &p, &e); e = e + s * al;
    two_sum(p, e, &p, &e);
    const double q = p / d;
    two_prod(q, d, &pp, &ee);
    const double r = ((p - pp) - ee) + e, ql = r / d;
    two_sum(1.0, -q, &hh, &ll); ll = ll - ql;
    two_sum(hh, ll, h, l);
}
// off = 1: sin(theta) / theta; 2: (1 - cos(theta)) / theta^2; 3: (theta - sin(theta)) / theta^3
IBA_POSE_HD double series(double s, int off) {
    double a = 1.0;
    for (int k = kSeriesTerms - 1; k > 2; --k) a = 1.0 - (s / (double)((2 * k + off - 1) * (2 * k + off))) * a;
    double h, l;
    series_step(s, (double)((3 + off) * (4 + off)), a, 0.0, &h, &l);
    series_step(s, (double)((1 + off) * (2 + off)), h, l, &h, &l);
    return off == 2 ? h * 0.5 : (off == 3 ? h / 6.0 : h);
}

// ---- P6: Tn = Exp(dx) T, dx = (omega, upsilon); returns 1 where theta > pi took libm ----
IBA_POSE_HD int exp_update(const double* dx, const double* T, double* Tn) {
    const double w0 = dx[0], w1 = dx[1], w2 = dx[2];
    const double s = (w0 * w0 + w1 * w1) + w2 * w2;
    double A, B, C;
    int big = 0;
    if (s > kPi2) {
        const double th = std::sqrt(s);
        A = std::sin(th) / th; B = (1.0 - std::cos(th)) / s; C = (th - std::sin(th)) / (s * th);
        big = 1;
    } else {
        A = series(s, 1); B = series(s, 2); C = series(s, 3);
    }
    const double O[9] = {0.0, -w2, w1, w2, 0.0, -w0, -w1, w0, 0.0};
    const double O2[9] = {-(w1 * w1 + w2 * w2), w0 * w1, w0 * w2, w0 * w1, -(w0 * w0 + w2 * w2), w1 * w2, w0 * w2, w1 * w2, -(w0 * w0 + w1 * w1)};
    double Re[9], V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        const double id = (i == 0 || i == 4 || i == 8) ? 1.0 : 0.0;
        Re[i] = (id + A * O[i]) + B * O2[i];
        V[i] = (id + B * O[i]) + C * O2[i];
    }
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double te = (V[r * 3] * dx[3] + V[r * 3 + 1] * dx[4]) + V[r * 3 + 2] * dx[5];
#pragma unroll
        for (int c = 0; c < 3; ++c) Tn[r * 4 + c] = (Re[r * 3] * T[c] + Re[r * 3 + 1] * T[4 + c]) + Re[r * 3 + 2] * T[8 + c];
        Tn[r * 4 + 3] = ((Re[r * 3] * T[3] + Re[r * 3 + 1] * T[7]) + Re[r * 3 + 2] * T[11]) + te;
    }
    return big;
}

// ---- P4, P5: g2o's OptimizationAlgorithmLevenberg on one 6-vector vertex. The state of one optimize(); the work arrays are the caller's (the kernel
// keeps both in LDS, where one lane walks them) ----
struct Lm { double lambda, ni, current, rho; int32_t qmax, stop, again, ok, it, its, trials, big; };
struct LmWork { double A[36], L[36], d[6], dx[6], Tn[12]; };

// the start of LM iteration `it` from the sums at the current pose
IBA_POSE_HD void lm_begin(Lm* s, const double* sums, int it) {
    s->current = sums[27];
    if (it == 0) {
        double md = 0.0;
        for (int k = 0; k < 6; ++k) { const double d = std::fabs(sums[hidx(k, k)]); if (d > md) md = d; }
        s->lambda = 1e-5 * md; s->ni = 2.0;
    }
    s->qmax = 0; s->rho = 0.0; s->stop = 0; s->again = 0;
}
// one trial's step: (H + lambda I) dx = b, Tn = Exp(dx) T. ok = 0: the factorisation failed (a failed trial, nothing to evaluate)
IBA_POSE_HD int lm_propose(Lm* s, const double* sums, const double* T, LmWork* w) {
    for (int r = 0; r < 6; ++r)
        for (int c = 0; c < 6; ++c) w->A[r * 6 + c] = sums[r <= c ? hidx(r, c) : hidx(c, r)] + (r == c ? s->lambda : 0.0);
    s->ok = icp::ldlt6_factor(w->A, w->L, w->d) ? 1 : 0;
    if (!s->ok) return 0;
    icp::ldlt6_apply(w->L, w->d, sums + 21, w->dx);
    return exp_update(w->dx, T, w->Tn);
}
// the verdict on a trial whose scale is known (P5): ok = 0 is a failed factorisation (scale and chi_trial unused). Returns 1 where the trial is
// accepted; sets again / stop. The core of lm_judge, and of the bundle adjustment's sequencer (iba_bundle_math.hpp), whose scale runs over more unknowns.
IBA_POSE_HD int lm_verdict(Lm* s, int ok, double scale_ok, double chi_trial) {
    const double temp = ok ? chi_trial : kMax;
    double rho = s->current - temp;
    const double scale = ok ? scale_ok : 1e-3;
    rho = rho / scale;
    s->rho = rho;
    int accept = 0;
    if (ok && rho > 0.0 && finite_(temp)) {
        const double t = 2.0 * rho - 1.0;
        double alpha = 1.0 - (t * t) * t;
        if (2.0 / 3.0 < alpha) alpha = 2.0 / 3.0;
        if (!(1.0 / 3.0 < alpha)) alpha = 1.0 / 3.0;
        s->lambda = s->lambda * alpha; s->ni = 2.0; s->current = temp;
        accept = 1;
    } else {
        s->lambda = s->lambda * s->ni; s->ni = s->ni * 2.0;
        if (!finite_(s->lambda)) { s->again = 0; s->stop = 1; return 0; }
    }
    ++s->qmax;
    s->again = (rho < 0.0 && s->qmax < kMaxTrials) ? 1 : 0;
    if (!s->again) s->stop = (s->qmax == kMaxTrials || rho == 0.0) ? 1 : 0;
    return accept;
}
// the verdict on the trial: chi_trial is the chi2 sum at Tn (unused where ok == 0). Returns 1 where Tn is accepted; sets again / stop.
IBA_POSE_HD int lm_judge(Lm* s, const double* sums, const LmWork* w, double chi_trial) {
    double scale = 1e-3;
    if (s->ok) for (int k = 0; k < 6; ++k) scale = scale + w->dx[k] * (s->lambda * w->dx[k] + sums[21 + k]);
    return lm_verdict(s, s->ok, scale, chi_trial);
}

// The sequencer of one optimize(): what the one lane (or the host) does between two evaluations. phase 0: `sums` holds the linearisation at T; phase 1:
// chi_trial is the chi2 sum at w->Tn. Returns what to evaluate next: 0 = linearise at T, 1 = the chi2 sum at w->Tn, 2 = the optimisation has ended.
// Failed factorisations are judged here, without an evaluation in between.
IBA_POSE_HD void lm_round_start(Lm* s) { s->it = 0; s->its = 0; s->trials = 0; s->stop = 0; s->again = 0; s->ok = 0; s->qmax = 0; }
IBA_POSE_HD int lm_next(Lm* s, LmWork* w, const double* sums, double chi_trial, double* T, int phase, int iterations) {
    bool propose = true;
    if (phase == 0) {
        lm_begin(s, sums, s->it);
        ++s->its;
    } else {
        if (lm_judge(s, sums, w, chi_trial)) for (int k = 0; k < 12; ++k) T[k] = w->Tn[k];
        propose = s->again != 0;
    }
    while (propose) {
        s->big += lm_propose(s, sums, T, w);
        ++s->trials;
        if (s->ok) return 1;
        lm_judge(s, sums, w, 0.0);
        propose = s->again != 0;
    }
    ++s->it;
    return (s->stop || s->it >= iterations) ? 2 : 0;
}

// P7: the classification of one edge from its chi2 at the round's final pose
IBA_POSE_HD int is_outlier(double chi2, float threshold) { return (float)chi2 > threshold ? 1 : 0; }

}  // namespace pose
}  // namespace iba

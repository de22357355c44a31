// Host-side caller of the Jacobian path: the outer re-association loop of iba_local (iba_local.cpp:434-460)
// with a Ceres-style Levenberg-Marquardt inner solve on the 7x7 normal equations the device returns.
// Ceres itself is a third-party dependency of the reference (absent here); this follows its published
// trust-region LM (LevenbergMarquardtStrategy + TrustRegionMinimizer): Jacobi column scaling,
// (H + diag(H)/radius) dx = -g, step acceptance by relative decrease, radius update
// radius /= max(1/3, 1 - (2 rho - 1)^3), and its three convergence tests in the minimizer's own order (gradient tolerance
// at the top of an iteration; parameter and function tolerance after the candidate's evaluation and before acceptance).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>

namespace iba {

struct LmOptions {
    int max_outer_iterations = 30;      // max_iba_iter
    int max_inner_iterations = 30;      // options.max_num_iterations (iba_local.cpp:437)
    double min_diff = 1e-6;             // iba_min_diff: allClose(last, cur) on the 7-vector (iba_local.cpp:454)
    double function_tolerance = 1e-6, gradient_tolerance = 1e-10, parameter_tolerance = 1e-8;   // Ceres defaults
    double initial_trust_region_radius = 1e4, max_trust_region_radius = 1e16, min_trust_region_radius = 1e-32;
    double min_relative_decrease = 1e-3, min_lm_diagonal = 1e-6, max_lm_diagonal = 1e32;
};
struct LmResult {
    double x[7];
    int outer_iterations = 0, inner_iterations = 0, evaluations = 0, converged = 0;
    double initial_cost = 0, final_cost = 0;
};

// solves A x = b for symmetric positive definite 7x7 A (row-major); returns false if not SPD
inline bool chol_solve7(const double* A, const double* b, double* x) {
    double L[49]; std::memset(L, 0, sizeof(L));
    for (int i = 0; i < 7; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = A[i * 7 + j];
            for (int k = 0; k < j; ++k) s -= L[i * 7 + k] * L[j * 7 + k];
            if (i == j) { if (!(s > 0)) return false; L[i * 7 + i] = std::sqrt(s); }
            else L[i * 7 + j] = s / L[j * 7 + j];
        }
    double y[7];
    for (int i = 0; i < 7; ++i) { double s = b[i]; for (int k = 0; k < i; ++k) s -= L[i * 7 + k] * y[k]; y[i] = s / L[i * 7 + i]; }
    for (int i = 6; i >= 0; --i) { double s = y[i]; for (int k = i + 1; k < 7; ++k) s -= L[k * 7 + i] * x[k]; x[i] = s / L[i * 7 + i]; }
    return true;
}

// One trust-region solve on N parameters, in the two halves a caller whose trials share one evaluation pass needs apart (iba_floam_map_register:
// many pairs, one device pass per trial round); calibrate_lm runs them back to back. The solver, what a failed solve means, |x|^2 and the
// Plus operation are the caller's.
enum class LmProposal { kTrial, kRetry, kStop, kNoSolve };   // what propose returns
enum class LmVerdict { kAccept, kReject, kStop };            // what judge returns
template <int N>
struct LmStep {
    double radius = 0.0, decrease = 2.0, scale[N];
    double delta[N], model = 0.0, step2 = 0.0;   // the trial in flight: the step in the caller's parameters, its model decrease, |step|^2
    void begin(const LmOptions& o, const double* H) {   // Jacobi scaling, fixed at the first Jacobian of the solve (Ceres)
        radius = o.initial_trust_region_radius; decrease = 2.0;
        for (int i = 0; i < N; ++i) scale[i] = 1.0 / (1.0 + std::sqrt(std::max(H[i * N + i], 0.0)));
    }
    // the radius after a step that is not taken; false: it has reached its floor
    bool shrink(const LmOptions& o) { radius = std::max(o.min_trust_region_radius, radius / decrease); decrease *= 2.0; return !(radius <= o.min_trust_region_radius); }
    // Propose: the gradient test (kStop), the scaled damped system through solve(A, rhs, x) (false: kNoSolve, nothing changed), the model
    // decrease; a model that is not positive shrinks the radius (kRetry, or kStop at its floor). kTrial: delta, model and step2 are set.
    template <class Solve>
    LmProposal propose(const LmOptions& o, const double* H, const double* g, Solve solve) {
        double gmax = 0.0; for (int i = 0; i < N; ++i) gmax = std::max(gmax, std::fabs(g[i]));
        if (gmax <= o.gradient_tolerance) return LmProposal::kStop;
        double Hs[N * N], gs[N], A[N * N], ngs[N], ds[N];
        for (int i = 0; i < N; ++i) { gs[i] = scale[i] * g[i]; for (int j = 0; j < N; ++j) Hs[i * N + j] = scale[i] * H[i * N + j] * scale[j]; }
        std::memcpy(A, Hs, sizeof(A));
        for (int i = 0; i < N; ++i) { A[i * N + i] += std::min(std::max(Hs[i * N + i], o.min_lm_diagonal), o.max_lm_diagonal) / radius; ngs[i] = -gs[i]; }
        if (!solve(A, ngs, ds)) return LmProposal::kNoSolve;
        model = 0.0;
        for (int i = 0; i < N; ++i) { double hd = 0.0; for (int j = 0; j < N; ++j) hd += Hs[i * N + j] * ds[j]; model -= ds[i] * (gs[i] + 0.5 * hd); }
        if (!(model > 0.0)) return shrink(o) ? LmProposal::kRetry : LmProposal::kStop;
        step2 = 0.0;
        for (int i = 0; i < N; ++i) { delta[i] = scale[i] * ds[i]; step2 += delta[i] * delta[i]; }
        return LmProposal::kTrial;
    }
    // Judge the evaluated trial, in TrustRegionMinimizer::Minimize's order: the parameter- and the function-tolerance tests against the
    // CURRENT point's cost — a run that stops on either keeps x (the candidate is not committed, and the stop can come on a step that would
    // have been rejected) — and only then accept (kAccept: the caller commits the trial) or reject (kReject, or kStop at the radius' floor).
    LmVerdict judge(const LmOptions& o, double cost, double trial_cost, double xn2) {
        if (std::sqrt(step2) <= o.parameter_tolerance * (std::sqrt(xn2) + o.parameter_tolerance)) return LmVerdict::kStop;
        if (std::fabs(cost - trial_cost) <= o.function_tolerance * cost) return LmVerdict::kStop;
        const double rho = (cost - trial_cost) / model;
        if (!(rho > o.min_relative_decrease)) return shrink(o) ? LmVerdict::kReject : LmVerdict::kStop;
        const double t = 2.0 * rho - 1.0;
        radius = std::min(o.max_trust_region_radius, radius / std::max(1.0 / 3.0, 1.0 - t * t * t)); decrease = 2.0;
        return LmVerdict::kAccept;
    }
};

// Build(x): freeze the association at x. Eval(x, H, g, cost): residual blocks of the frozen association at x.
template <class Build, class Eval>
inline bool calibrate_lm(const double* x0, const LmOptions& o, Build build, Eval eval, LmResult& r) {
    double x[7]; std::memcpy(x, x0, sizeof(x));
    double last[7]; std::memcpy(last, x0, sizeof(last));
    r = LmResult();
    for (int outer = 0; outer < o.max_outer_iterations; ++outer) {
        if (!build(x)) return false;
        double H[49], g[7], cost;
        if (!eval(x, H, g, cost)) return false;
        ++r.evaluations;
        if (outer == 0) r.initial_cost = cost;
        LmStep<7> step;
        step.begin(o, H);
        for (int it = 0; it < o.max_inner_iterations; ++it) {
            ++r.inner_iterations;
            LmProposal next = step.propose(o, H, g, chol_solve7);
            if (next == LmProposal::kNoSolve) next = step.shrink(o) ? LmProposal::kRetry : LmProposal::kStop;   // not SPD: damp harder
            if (next == LmProposal::kStop) break;
            if (next == LmProposal::kRetry) continue;
            double xn[7], xn2 = 0;
            for (int i = 0; i < 7; ++i) { xn[i] = x[i] + step.delta[i]; xn2 += x[i] * x[i]; }
            double Hn[49], gn[7], cn;
            if (!eval(xn, Hn, gn, cn)) return false;
            ++r.evaluations;
            const LmVerdict verdict = step.judge(o, cost, cn, xn2);
            if (verdict == LmVerdict::kStop) break;
            if (verdict == LmVerdict::kAccept) { std::memcpy(x, xn, sizeof(x)); std::memcpy(H, Hn, sizeof(H)); std::memcpy(g, gn, sizeof(g)); cost = cn; }
        }
        r.final_cost = cost; r.outer_iterations = outer + 1;
        bool close = true;   // allClose (IBACalib2.hpp:9-18)
        for (int i = 0; i < 7; ++i) if (std::fabs(last[i] - x[i]) > o.min_diff) close = false;
        if (close) { r.converged = 1; break; }
        std::memcpy(last, x, sizeof(last));
    }
    std::memcpy(r.x, x, sizeof(x));
    return true;
}

}  // namespace iba

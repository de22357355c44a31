// The Levenberg-Marquardt loop of the graph units (include/iba_mi355x.h: rule 6 of iba_pgo_*, S4 of iba_smooth_*), stated once. Plain C++: the unit
// gives two callables that run its launch chains and hand back scalars, so the loop's decisions run without a device (csrc/san/host_selftest.cpp).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/iba_mi355x.h"

namespace iba {

constexpr int kGraphLmScal = 8;   // the scalars of one trial; the driver reads 4 delta . (lambda delta + b), 5 |delta|^2, 6 the trial's residual

struct GraphLmOptions {
    int max_iteration, max_iteration_lm;
    double min_relative_increment, min_relative_residual_increment, min_right_term, min_residual, upper_scale_factor, lower_scale_factor;
};
// iba_pgo_options and iba_smooth_options name the eight knobs identically
template <class Options>
GraphLmOptions graph_lm_options(const Options& o) {
    return GraphLmOptions{o.max_iteration, o.max_iteration_lm, o.min_relative_increment, o.min_relative_residual_increment, o.min_right_term, o.min_residual,
                          o.upper_scale_factor, o.lower_scale_factor};
}

struct GraphLmResult {
    int iterations = 0, trials = 0, stop = IBA_PGO_STOP_NONE;
    double residual = 0.0, lambda = 0.0;
    double residual_start = 0.0, lambda_start = 0.0;   // set once the first linearisation is there, whatever happens after it
    double max_b = 0.0;                                // at the last linearisation
};

// linearize(after_accept, sc): linearise at the current estimates, sc[0..3] = residual, |x|^2, max |b|, max diagonal. after_accept: the trial of the
//   last trial() call was accepted and is to become the estimates first (false: the call that opens the loop).
// trial(lambda, ts): solve at lambda, form the trial estimates, ts[0..kGraphLmScal).
// Both return iba_status; the first that is not IBA_OK ends the loop and is returned (out then holds the start values at most).
// A byte per trial goes to trace: 0 rejected, 1 accepted, 2 stopped on the increment, each OR trace_bit.
template <class Linearize, class Trial>
iba_status graph_lm(const GraphLmOptions& o, Linearize linearize, Trial trial, std::vector<uint8_t>& trace, uint8_t trace_bit, GraphLmResult& out) {
    double sc[4];
    iba_status st = linearize(false, sc);
    if (st != IBA_OK) return st;
    double r = sc[0], lambda = 1e-5 * sc[3], nu = 2.0;
    out.residual_start = r; out.lambda_start = lambda;
    int stop = IBA_PGO_STOP_NONE, iterations = 0, trials = 0;
    while (stop == IBA_PGO_STOP_NONE) {
        if (sc[2] < o.min_right_term) { stop = IBA_PGO_STOP_RIGHT_TERM; break; }
        if (iterations >= o.max_iteration) { stop = IBA_PGO_STOP_MAX_ITERATION; break; }
        const double xnorm = std::sqrt(sc[1]);
        for (int k = 0; k < o.max_iteration_lm; ++k) {
            double ts[kGraphLmScal];
            st = trial(lambda, ts);
            if (st != IBA_OK) return st;
            ++trials;
            if (std::sqrt(ts[5]) < o.min_relative_increment * (xnorm + o.min_relative_increment)) { stop = IBA_PGO_STOP_INCREMENT; trace.push_back(2 | trace_bit); break; }
            const double r_new = ts[6], rho = (r - r_new) / (ts[4] + 1e-3);
            if (rho > 0.0) {
                const double t = 2.0 * rho - 1.0;
                lambda *= std::max(o.lower_scale_factor, std::min(1.0 - t * t * t, o.upper_scale_factor));
                nu = 2.0;
                trace.push_back(1 | trace_bit);
                const double r_before = r;
                st = linearize(true, sc);
                if (st != IBA_OK) return st;
                r = sc[0];
                if (r_before - r_new < o.min_relative_residual_increment * r_before) stop = IBA_PGO_STOP_RESIDUAL_INCREMENT;
                break;
            }
            trace.push_back(0 | trace_bit);
            lambda *= nu; nu *= 2.0;
        }
        ++iterations;   // after a stop on the increment too
        if (stop == IBA_PGO_STOP_NONE && r < o.min_residual) stop = IBA_PGO_STOP_RESIDUAL;
    }
    out.iterations = iterations; out.trials = trials; out.stop = stop; out.residual = r; out.lambda = lambda; out.max_b = sc[2];
    return IBA_OK;
}

}  // namespace iba

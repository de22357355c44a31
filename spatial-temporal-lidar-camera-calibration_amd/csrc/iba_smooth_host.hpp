// Host side of the robust pose-graph smoother (include/iba_mi355x.h, iba_smooth_*). Plain C++, no HIP: the argument checks and the plan of a
// factor list — the arrowhead plan of iba_pgo_host.hpp over the between factors, with the priors added to the incidence lists of the node gather.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_pgo_host.hpp"

namespace iba { namespace smooth {

inline std::string validate_options(const iba_smooth_options* o) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_smooth_options)) return "opt->struct_size is " + std::to_string(o->struct_size) + ", this library's iba_smooth_options has " + std::to_string(sizeof(iba_smooth_options));
    const double v[] = {o->min_relative_increment, o->min_relative_residual_increment, o->min_right_term, o->min_residual, o->upper_scale_factor, o->lower_scale_factor};
    for (double x : v) if (!std::isfinite(x)) return "an option is not finite";
    if (o->segment < 1) return "segment " + std::to_string(o->segment) + " < 1";
    if (o->max_iteration < 0 || o->max_iteration_lm < 0) return "max_iteration / max_iteration_lm < 0";
    return "";
}

inline std::string validate_pose(const double* T, const char* name) {
    if (!T) return std::string(name) + " is NULL";
    std::string why;
    if (!pgo::rigid16_ok(T, why)) return std::string(name) + " " + why;
    return "";
}

inline std::string validate_var(const double* var) {
    if (!var) return "var6 is NULL";
    for (int k = 0; k < 6; ++k) if (!std::isfinite(var[k]) || !(var[k] > 0.0)) return "var6[" + std::to_string(k) + "] is not finite or not > 0";
    return "";
}

// Factors in call order: fi < 0 a prior on fj. The plan sees a between factor (i, j) as the edge j -> i and no prior; the incidence lists are then
// rebuilt over ALL factors: factor * 2 + (the node is the factor's i), ascending factor.
inline bool make_plan(int32_t N, const std::vector<int32_t>& fi, const std::vector<int32_t>& fj, int32_t segment, int32_t cap, pgo::Plan& p, std::string& err) {
    const int32_t F = (int32_t)fi.size();
    std::vector<uint8_t> active(F);
    std::vector<int32_t> src(F), tgt(F);
    for (int32_t f = 0; f < F; ++f) { active[f] = fi[f] >= 0 ? 1 : 0; src[f] = fj[f]; tgt[f] = fi[f] >= 0 ? fi[f] : fj[f]; }
    if (!pgo::make_plan(N, src.data(), tgt.data(), active.data(), F, segment, cap, p, err)) return false;
    p.inc_off.assign(N + 1, 0);
    for (int32_t f = 0; f < F; ++f) { ++p.inc_off[fj[f] + 1]; if (fi[f] >= 0) ++p.inc_off[fi[f] + 1]; }
    for (int32_t i = 0; i < N; ++i) p.inc_off[i + 1] += p.inc_off[i];
    p.inc_edge.assign(p.inc_off[N] > 0 ? p.inc_off[N] : 1, 0);
    std::vector<int32_t> at(p.inc_off.begin(), p.inc_off.end() - 1);
    for (int32_t f = 0; f < F; ++f) { p.inc_edge[at[fj[f]]++] = f * 2; if (fi[f] >= 0) p.inc_edge[at[fi[f]]++] = f * 2 + 1; }
    return true;
}

} }  // namespace iba::smooth

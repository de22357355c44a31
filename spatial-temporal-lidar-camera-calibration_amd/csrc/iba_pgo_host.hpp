// Host side of the pose-graph optimiser (include/iba_mi355x.h, iba_pgo_*). Plain C++, no HIP: the argument checks, the arrowhead plan (chain and
// cross edges, separators, runs, the list the separator system is assembled from, the incidence lists of the gather) and mu of the line process.
// tests/pgo_ref.py restates the plan in Python; iba_pgo_plan answers it without a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/iba_mi355x.h"

namespace iba { namespace pgo {

struct Plan {
    int K = 0;
    std::vector<int32_t> sep, sep_of_node;        // separators ascending; node -> its index in sep or -1
    std::vector<int32_t> run_first, run_last;     // interior runs, ascending
    std::vector<int32_t> chain;                   // [N]: chain edge between i and i + 1, -1 without one
    std::vector<int32_t> inc_off, inc_edge;       // per node: edge * 2 + (node is the target), ascending edge
    std::vector<int32_t> brow, bcol, boff, kind, idx;   // the separator system: see pgo_sep_assemble_kernel
};

inline std::string validate_options(const iba_pgo_options* o, int32_t N) {
    if (!o) return "opt is NULL";
    if (o->struct_size != (int32_t)sizeof(iba_pgo_options)) return "opt->struct_size is " + std::to_string(o->struct_size) + ", this library's iba_pgo_options has " + std::to_string(sizeof(iba_pgo_options));
    const double v[] = {o->max_corr_dist, o->edge_prune_threshold, o->preference_loop_closure, o->min_relative_increment, o->min_relative_residual_increment,
                        o->min_right_term, o->min_residual, o->upper_scale_factor, o->lower_scale_factor};
    for (double x : v) if (!std::isfinite(x)) return "an option is not finite";
    if (o->reference_node < -1 || o->reference_node >= N) return "reference_node " + std::to_string(o->reference_node) + " is outside [-1, " + std::to_string(N) + ")";
    if (o->segment < 1) return "segment " + std::to_string(o->segment) + " < 1";
    if (o->max_iteration < 0 || o->max_iteration_lm < 0) return "max_iteration / max_iteration_lm < 0";
    return "";
}

inline std::string validate_topology(int32_t N, const iba_pgo_edge* edges, int32_t E) {
    if (N < 1) return "N = " + std::to_string(N) + " < 1";
    if (E < 0) return "E = " + std::to_string(E) + " < 0";
    if (E && !edges) return "edges is NULL";
    for (int32_t e = 0; e < E; ++e) {
        const int32_t s = edges[e].source, t = edges[e].target;
        if (s < 0 || s >= N || t < 0 || t >= N) return "edge " + std::to_string(e) + ": (" + std::to_string(s) + ", " + std::to_string(t) + ") is outside [0, " + std::to_string(N) + ")";
        if (s == t) return "edge " + std::to_string(e) + ": source == target == " + std::to_string(s);
    }
    return "";
}

inline bool rigid16_ok(const double* T, std::string& why) {
    for (int k = 0; k < 16; ++k) if (!std::isfinite(T[k])) { why = "is not finite"; return false; }
    if (T[12] != 0.0 || T[13] != 0.0 || T[14] != 0.0 || T[15] != 1.0) { why = "has a last row other than 0 0 0 1"; return false; }
    return true;
}

inline std::string validate_values(const double* nodes16, int32_t N, const iba_pgo_edge* edges, int32_t E) {
    if (!nodes16) return "nodes16 is NULL";
    std::string why;
    for (int32_t i = 0; i < N; ++i) if (!rigid16_ok(nodes16 + 16 * (size_t)i, why)) return "node " + std::to_string(i) + " " + why;
    for (int32_t e = 0; e < E; ++e) {
        if (!rigid16_ok(edges[e].T, why)) return "edge " + std::to_string(e) + ": T " + why;
        for (int i = 0; i < 6; ++i) for (int j = i; j < 6; ++j) if (!std::isfinite(edges[e].info[i * 6 + j])) return "edge " + std::to_string(e) + ": info is not finite";
    }
    return "";
}

// The plan over the edges with active[e] != 0 (active == nullptr: all). false with a message when the separators cannot be brought under cap.
inline bool make_plan(int32_t N, const int32_t* src, const int32_t* tgt, const uint8_t* active, int32_t E, int32_t segment, int32_t cap, Plan& p, std::string& err) {
    p = Plan();
    p.chain.assign(N, -1);
    std::vector<uint8_t> endpoint(N, 0);
    for (int32_t e = 0; e < E; ++e) {
        if (active && !active[e]) continue;
        const int32_t lo = src[e] < tgt[e] ? src[e] : tgt[e], hi = src[e] < tgt[e] ? tgt[e] : src[e];
        if (hi == lo + 1 && p.chain[lo] < 0) { p.chain[lo] = e; continue; }
        endpoint[lo] = 1; endpoint[hi] = 1;
    }
    int32_t n_end = 0;
    for (int32_t i = 0; i < N; ++i) n_end += endpoint[i];
    if (n_end > cap) { err = "the cross edges touch " + std::to_string(n_end) + " nodes, beyond the separator cap " + std::to_string(cap); return false; }
    int64_t K = segment;
    for (;;) {
        int64_t n = 0;
        for (int32_t i = 0; i < N; ++i) n += (endpoint[i] || i % K == 0) ? 1 : 0;
        if (n <= cap) break;
        if (K >= N) { err = "the cross edges touch " + std::to_string(n_end) + " nodes: with node 0 that is beyond the separator cap " + std::to_string(cap); return false; }
        K *= 2;
    }
    p.K = (int)K;
    p.sep_of_node.assign(N, -1);
    for (int32_t i = 0; i < N; ++i) if (endpoint[i] || i % K == 0) { p.sep_of_node[i] = (int32_t)p.sep.size(); p.sep.push_back(i); }
    for (int32_t i = 0; i < N; ++i) {
        if (p.sep_of_node[i] >= 0) continue;
        if (p.run_first.empty() || p.run_last.back() != i - 1) { p.run_first.push_back(i); p.run_last.push_back(i); }
        else p.run_last.back() = i;
    }
    // incidence lists
    p.inc_off.assign(N + 1, 0);
    for (int32_t e = 0; e < E; ++e) { if (active && !active[e]) continue; ++p.inc_off[src[e] + 1]; ++p.inc_off[tgt[e] + 1]; }
    for (int32_t i = 0; i < N; ++i) p.inc_off[i + 1] += p.inc_off[i];
    p.inc_edge.assign(p.inc_off[N] > 0 ? p.inc_off[N] : 1, 0);
    { std::vector<int32_t> at(p.inc_off.begin(), p.inc_off.end() - 1);
      for (int32_t e = 0; e < E; ++e) { if (active && !active[e]) continue; p.inc_edge[at[src[e]]++] = e * 2; p.inc_edge[at[tgt[e]]++] = e * 2 + 1; } }
    // separator system
    std::map<std::pair<int32_t, int32_t>, std::vector<std::pair<int32_t, int32_t>>> blocks;
    for (size_t q = 0; q < p.sep.size(); ++q) blocks[{(int32_t)q, (int32_t)q}].push_back({0, p.sep[q]});
    for (int32_t e = 0; e < E; ++e) {
        if (active && !active[e]) continue;
        const int32_t a = p.sep_of_node[src[e]], b = p.sep_of_node[tgt[e]];
        if (a < 0 || b < 0) continue;
        blocks[{a > b ? a : b, a > b ? b : a}].push_back({1, e});
    }
    for (size_t r = 0; r < p.run_first.size(); ++r) {
        const int32_t L = p.sep_of_node[p.run_first[r] - 1];
        blocks[{L, L}].push_back({2, (int32_t)r});
        if (p.run_last[r] + 1 < N) {
            const int32_t R = p.sep_of_node[p.run_last[r] + 1];
            blocks[{R, R}].push_back({3, (int32_t)r});
            blocks[{R, L}].push_back({4, (int32_t)r});
        }
    }
    p.boff.push_back(0);
    for (auto& kv : blocks) {
        p.brow.push_back(kv.first.first); p.bcol.push_back(kv.first.second);
        for (auto& it : kv.second) { p.kind.push_back(it.first); p.idx.push_back(it.second); }
        p.boff.push_back((int32_t)p.kind.size());
    }
    return true;
}

// rule 4: mu over the active uncertain edges, in edge order
inline double line_process_mu(const iba_pgo_options& o, const double* info55, const uint8_t* flags, int32_t E) {
    double s = 0.0; int64_t n = 0;
    for (int32_t e = 0; e < E; ++e) if ((flags[e] & 1) && !(flags[e] & 2)) { s += info55[e]; ++n; }
    return n ? o.preference_loop_closure * (o.max_corr_dist * o.max_corr_dist) * (s / (double)n) : 0.0;
}

} }  // namespace iba::pgo

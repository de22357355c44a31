// The block-arrowhead solve of (H + lambda I) delta = b as one object: a Plan on the device, the work buffers of the elimination and the launch chain
// over the kernels of iba_pgo_kernels.hpp. iba_pgo and iba_smooth both hold one: the same kernels, the same launches, the same bytes. The kernels are
// compiled into iba_pgo.hip alone, where launch() and final_launch() are defined; this header carries no device code.
// Behind it, the host scaffolding both units put around that chain (the LM loop itself is iba_graph_lm.hpp). H there is a unit's handle; the helpers
// use the members both handles name alike (device, stream, ar, D, b, A, delta, scal, err) and leave the message in H::err.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "iba_device_buf.hpp"
#include "iba_graph_lm.hpp"
#include "iba_pgo_host.hpp"
#include "iba_pgo_math.hpp"

namespace iba { namespace pgo {

struct Arrow {
    int N = 0, R = 0, ns = 0, nblk = 0;
    DevBuf<int32_t> inc_off, inc_edge, chain, run_first, run_last, sep_node, sep_of_node, brow, bcol, boff, kind, idx;
    DevBuf<double> G, F, y, run_S, run_b, S, rhs, xs;

    // the plan of N nodes onto the device and buffers of its sizes (G, F, y only when N grew past them)
    hipError_t upload(const Plan& p, int n_nodes) {
        N = n_nodes; R = (int)p.run_first.size(); ns = (int)p.sep.size(); nblk = (int)p.brow.size();
        const size_t n = 6 * (size_t)ns;
        hipError_t e = hipSuccess;
        auto up = [&](hipError_t r) { if (e == hipSuccess) e = r; };
        up(inc_off.upload(p.inc_off)); up(inc_edge.upload(p.inc_edge)); up(chain.upload(p.chain));
        up(run_first.upload(p.run_first)); up(run_last.upload(p.run_last));
        up(sep_node.upload(p.sep)); up(sep_of_node.upload(p.sep_of_node));
        up(brow.upload(p.brow)); up(bcol.upload(p.bcol)); up(boff.upload(p.boff)); up(kind.upload(p.kind)); up(idx.upload(p.idx));
        up(run_S.alloc(108 * (size_t)R)); up(run_b.alloc(12 * (size_t)R));
        up(S.alloc(n * n)); up(rhs.alloc(n)); up(xs.alloc(n));
        up(G.grow(36 * (size_t)N)); up(F.grow(36 * (size_t)N)); up(y.grow(6 * (size_t)N));
        return e;
    }

    // the launch chain; no synchronisation. D N x 36, b N x 6, A the factor blocks the plan's edge indices name, scal the kScal scalars (7: a pivot failed)
    void launch(hipStream_t st, const double* D, const double* b, const double* A, double lambda, double* delta, double* scal);
};

// pgo_final_kernel on st: out[k] = the sum (k < nsum) or max (the next nmax) over the blocks of partial[block * (nsum + nmax) + k]
void final_launch(hipStream_t st, const double* partial, int nblocks, int nsum, int nmax, double* out);

static_assert(kScal == kGraphLmScal, "the LM driver reads the trial's scalars in kScal's layout");

inline std::string not_positive_definite(const std::string& who, double lambda) {
    return who + ": H + lambda I is not positive definite to working precision (lambda = " + std::to_string(lambda) + ")";
}

// The end of a chain whose result is scalars: the first n of h->scal to the host and the chain's one synchronise. `stage` names the chain in the
// message. n == kScal: the chain had a solve in it, and scal[7] says whether one of its pivots failed.
template <class H>
iba_status read_scalars(H* h, int n, double* host, const std::string& who, const char* stage, double lambda = 0.0) {
    if (hipMemcpyAsync(host, h->scal.p, n * sizeof(double), hipMemcpyDeviceToHost, h->stream) != hipSuccess) { h->err = who + ": download of the scalars"; return IBA_ERR_HIP; }
    const hipError_t e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) { h->err = who + ": " + stage + " kernels: " + hipGetErrorString(e); return IBA_ERR_HIP; }
    if (n == kScal && host[7] != 0.0) { h->err = not_positive_definite(who, lambda); return IBA_ERR_UNSUPPORTED; }
    return IBA_OK;
}

// The body of iba_*_solve behind the entry point's test of the handle itself. `state`: why the handle has no linearisation to solve, nullptr when
// it has one; the entry point works it out, and it is reported behind the argument checks, where both units have always had it.
template <class H>
iba_status solve_call(H* h, double lambda, double* delta, const std::string& who, const char* state) {
    const auto fail = [&](iba_status st, const std::string& m) { h->err = who + ": " + m; return st; };
    if (!delta) return fail(IBA_ERR_INVALID_ARG, "delta is NULL");
    if (!std::isfinite(lambda) || lambda < 0.0) return fail(IBA_ERR_INVALID_ARG, "lambda is not finite or negative");
    if (state) return fail(IBA_ERR_STATE, state);
    if (hipSetDevice(h->device) != hipSuccess) return fail(IBA_ERR_HIP, "hipSetDevice");
    h->ar.launch(h->stream, h->D.p, h->b.p, h->A.p, lambda, h->delta.p, h->scal.p);
    double flag = 0.0;
    hipError_t e = hipMemcpyAsync(delta, h->delta.p, 6 * (size_t)h->ar.N * sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&flag, h->scal.p + 7, sizeof(double), hipMemcpyDeviceToHost, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess) return fail(IBA_ERR_HIP, hipGetErrorString(e));
    if (flag != 0.0) { h->err = not_positive_definite(who, lambda); return IBA_ERR_UNSUPPORTED; }
    return IBA_OK;
}

// iba_debug_*_trace: the bytes the last LM run pushed (nullptr: no handle). false: a bad argument.
inline bool trace_out(const std::vector<uint8_t>* trace, uint8_t* trials, int32_t cap, int32_t* n) {
    if (!trace || !n || cap < 0 || (cap && !trials)) return false;
    for (int32_t k = 0; k < cap && k < (int32_t)trace->size(); ++k) trials[k] = (*trace)[k];
    *n = (int32_t)trace->size();
    return true;
}

// Blocking downloads in sequence: a null destination or an empty source is passed over, and so is everything after the first failure (kept in e)
struct Download {
    hipError_t e = hipSuccess;
    void operator()(double* dst, const double* src, size_t count) { if (dst && count && e == hipSuccess) e = hipMemcpy(dst, src, count * sizeof(double), hipMemcpyDeviceToHost); }
};

} }  // namespace iba::pgo

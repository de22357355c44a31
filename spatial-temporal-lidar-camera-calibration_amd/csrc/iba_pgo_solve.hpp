// The block-arrowhead solve of (H + lambda I) delta = b as one object: a Plan on the device, the work buffers of the elimination and the launch chain
// over the kernels of iba_pgo_kernels.hpp. iba_pgo and iba_smooth both hold one: the same kernels, the same launches, the same bytes. The kernels are
// compiled into iba_pgo.hip alone, where launch() and final_launch() are defined; this header carries no device code.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "iba_device_buf.hpp"
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

} }  // namespace iba::pgo

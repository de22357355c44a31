// The balanced tree over a wave's 64 lanes by DPP, for float64 (rule P3 of iba_pose, B3 and B6 of iba_bundle): device code, shared by
// iba_pose_kernels.hpp and iba_bundle_kernels.hpp.
#pragma once
#include <hip/hip_runtime.h>

namespace iba {
namespace pose {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp(double x) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(x);
    int lo = (int)(unsigned)b, hi = (int)(unsigned)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double((long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo));
}
// the balanced tree over a wave's 64 lanes (row_shr 1 2 4 8, row_bcast 15 and 31), total in lane 63; a lane without a source adds +0.0
__device__ __forceinline__ double wave_sum(double x) {
    x += dpp<0x111, 0xf>(x); x += dpp<0x112, 0xf>(x); x += dpp<0x114, 0xf>(x); x += dpp<0x118, 0xf>(x);
    x += dpp<0x142, 0xa>(x); x += dpp<0x143, 0xc>(x);
    return x;
}

}  // namespace pose
}  // namespace iba

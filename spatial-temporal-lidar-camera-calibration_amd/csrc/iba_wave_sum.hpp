// The reductions over a wave's 64 lanes by DPP (row_shr 1 2 4 8, row_bcast 15 and 31: a balanced tree on the VALU, no LDS traffic) and the block tail
// behind them: device code, the one text of it for every unit. The association order of the f64 sum is fixed by that tree and is a parity rule of the
// whole project (rule 6 of iba_pgo, S4 of iba_smooth, P3 of iba_pose, B3 and B6 of iba_bundle, the sums of the evaluation chain and of the passes):
// every sum that is compared bit for bit goes through here.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace iba {

template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned long long dpp_u64(unsigned long long b) {
    int lo = (int)(unsigned int)b, hi = (int)(unsigned int)(b >> 32);
    lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, ROW_MASK, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, ROW_MASK, 0xf, false);
    return ((unsigned long long)(unsigned int)hi << 32) | (unsigned long long)(unsigned int)lo;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp(double x) { return __longlong_as_double((long long)dpp_u64<CTRL, ROW_MASK>((unsigned long long)__double_as_longlong(x))); }

// total in lane 63, fixed association order => bitwise reproducible; a lane without a source adds +0.0
__device__ __forceinline__ double wave_sum_f64(double x) {
    x += dpp<0x111, 0xf>(x); x += dpp<0x112, 0xf>(x); x += dpp<0x114, 0xf>(x); x += dpp<0x118, 0xf>(x);   // row_shr 1,2,4,8
    x += dpp<0x142, 0xa>(x);   // row_bcast:15 -> rows 1,3
    x += dpp<0x143, 0xc>(x);   // row_bcast:31 -> rows 2,3
    return x;
}
// the largest in lane 63; the inputs are >= 0, so the 0 a lane without a source reads is neutral
__device__ __forceinline__ double wave_max_f64(double x) {
    x = fmax(x, dpp<0x111, 0xf>(x)); x = fmax(x, dpp<0x112, 0xf>(x)); x = fmax(x, dpp<0x114, 0xf>(x)); x = fmax(x, dpp<0x118, 0xf>(x));
    x = fmax(x, dpp<0x142, 0xa>(x)); x = fmax(x, dpp<0x143, 0xc>(x));
    return x;
}
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t x) {   // inclusive prefix over the lanes of the wave (the total in lane 63)
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x111, 0xf, 0xf, false); x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x112, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x114, 0xf, 0xf, false); x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x118, 0xf, 0xf, false);
    x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xa, 0xf, false); x += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xc, 0xf, false);
    return x;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long x) {
    x += dpp_u64<0x111, 0xf>(x); x += dpp_u64<0x112, 0xf>(x); x += dpp_u64<0x114, 0xf>(x); x += dpp_u64<0x118, 0xf>(x);
    x += dpp_u64<0x142, 0xa>(x); x += dpp_u64<0x143, 0xc>(x);
    return x;
}

// The block tail behind K wave sums: v[k] is the wave's total of sum k in lane 63 (what wave_sum_f64 leaves there). Lane 63 puts the totals in LDS,
// a barrier, then thread k < K adds the waves in ascending order and writes out[block * K + k]. Every thread of a block of THREADS calls it, once.
template <int K, int THREADS>
__device__ __forceinline__ void block_sum_store(const double (&v)[K], double* __restrict__ out) {
    __shared__ double s_part[THREADS / 64][K];
    if ((threadIdx.x & 63) == 63) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_part[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x < K) {
        double t = s_part[0][threadIdx.x];
        for (int w = 1; w < THREADS / 64; ++w) t += s_part[w][threadIdx.x];
        out[K * (size_t)blockIdx.x + threadIdx.x] = t;
    }
}

}  // namespace iba

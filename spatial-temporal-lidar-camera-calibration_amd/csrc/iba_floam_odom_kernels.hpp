// Device side of iba_floam_odom_run (include/iba_mi355x.h) beyond the chains it borrows (iba_floam_kernels.hpp, iba_voxel_kernels.hpp,
// iba_index_kernels.hpp, iba_floam_map_kernels.hpp):
//  iba_floam_odom_move_kernel   grid (256-point blocks of the longest segment, segments): a segment is a run of float32 points of the gathered
//      feature clouds. Thread = one point: widened to f64, moved by the segment's pose with vox_apply (rule L1's expression: four separately
//      rounded operations per row, no fma) unless the segment asks for the plain copy, narrowed to float32 (round to nearest even) and stored
//      WIDENED again as three doubles — the form the index build stages its frames from (its own narrowing is then exact). This is rule O3
//      (initMapWithPoints) and the way the raw feature clouds become frames. Every word is written by exactly one thread.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "iba_voxel_kernels.hpp"

namespace iba {

struct OdomSegment {     // host -> device
    double T[12];        // row-major 3x4 (move = 1)
    uint64_t src0;       // first point of the run in the float cloud
    uint64_t dst0;       // first point of the run in the output
    uint32_t n;          // points
    int32_t kind;        // 0: the edge cloud, 1: the surf cloud
    int32_t move, pad;   // 1: apply T; 0: the plain widening
};

__global__ __launch_bounds__(kVoxThreads) void iba_floam_odom_move_kernel(const OdomSegment* __restrict__ segs, const float* __restrict__ edge_xyz, const float* __restrict__ surf_xyz,
                                                                         double* __restrict__ out) {
    const OdomSegment& S = segs[blockIdx.y];
    const uint32_t i = blockIdx.x * (uint32_t)kVoxThreads + threadIdx.x;
    if (i >= S.n) return;
    const float* p = (S.kind ? surf_xyz : edge_xyz) + 3 * (S.src0 + i);
    double q0 = (double)p[0], q1 = (double)p[1], q2 = (double)p[2];
    if (S.move) { const double x = q0, y = q1, z = q2; vox_apply(S.T, x, y, z, q0, q1, q2); }
    double* dst = out + 3 * (S.dst0 + i);
    dst[0] = (double)(float)q0; dst[1] = (double)(float)q1; dst[2] = (double)(float)q2;
}

}  // namespace iba

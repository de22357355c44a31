// Host half of the scan-to-image projection (include/iba_mi355x.h, iba_project_*): the defaults, the validation that answers before the device
// is touched, the palette of the overlay (shared with the overlay kernel: the same expressions on both sides) and the cut of a call's jobs into
// chunks. Plain C++: nothing here needs a device.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"

#if defined(__HIPCC__)
#define IBA_PROJ_HD __host__ __device__
#else
#define IBA_PROJ_HD
#endif

namespace iba {
namespace project {

constexpr int kSlice = 4096;                // points of a job one splat / visible block takes
constexpr int kThreads = 256;               // threads of every projection kernel's block
constexpr int kCounters = 8;                // uint32 counters per job on the device: the first five are used
enum Counter { C_SKIPPED = 0, C_IN_FRONT, C_INSIDE, C_VISIBLE, C_PIXELS };

// One job as the kernels read it (a multiple of 8 bytes: the splat stages it in LDS word by word). The block numbers are cumulative over ALL
// jobs of the call, so a launch over the jobs [a, b) passes jobs + a and the first block of job a as its bias.
struct ProjJob {
    double Rt[12];                   // R | t, row-major 3 x 4 (P1)
    double fx, fv, cx, cy, W, H;     // fv: the focal length v is formed with (fy, or fx under v_focal_is_fx)
    uint64_t pt_base;                // the frame's first tree position in the handle's 16-byte points
    uint64_t rec_base;               // the job's first record (original point order)
    uint64_t img_base;               // the job's first pixel in the depth and index images of the result
    uint64_t key_base;               // ... and in the key image of its chunk
    uint32_t P, Wi, Hi;              // points of the frame; the image size as integers
    uint32_t first_block;            // first splat / visible block: ceil(P / kSlice) blocks
    uint32_t first_pblock;           // first resolve block: ceil(Wi Hi / kThreads) blocks
    uint32_t pad;
};
static_assert(sizeof(ProjJob) % 8 == 0, "staged in LDS as 8-byte words");

struct ProjRec { double u, v; float z; uint32_t flags; };   // per point, at its original index
static_assert(sizeof(ProjRec) == 24, "24 bytes per point");

constexpr int kMaxSplat = 4;
constexpr double kMaxPixels = 67108864.0;   // 2^26 per image
constexpr uint64_t kBytesPerPixel = 16;     // key 8 + depth 4 + index 4: what a chunk's images cost per pixel and job

// P8: the five-stop ramp blue, cyan, green, yellow, red; zn is clamped to [0, 1] here (NaN: 0)
IBA_PROJ_HD inline void gradient(double zn, uint8_t* rgb) {
    const double stop[5][3] = {{0.0, 0.0, 255.0}, {0.0, 255.0, 255.0}, {0.0, 255.0, 0.0}, {255.0, 255.0, 0.0}, {255.0, 0.0, 0.0}};
    if (!(zn > 0.0)) zn = 0.0;
    if (zn > 1.0) zn = 1.0;
    const double s = 4.0 * zn;
    int k = (int)floor(s);
    if (k > 3) k = 3;
    const double f = s - (double)k;
    for (int c = 0; c < 3; ++c) rgb[c] = (uint8_t)floor(((1.0 - f) * stop[k][c] + f * stop[k + 1][c]) + 0.5);
}

inline void default_options(iba_project_options& o) {
    std::memset(&o, 0, sizeof(o));
    o.struct_size = (int32_t)sizeof(o);
    o.splat = 1; o.occlusion_tol = 0.02; o.z_min = 0.1; o.z_max = 120.0; o.v_focal_is_fx = 0;
    o.z_near = 2.0; o.z_far = 60.0;
}

// fx, fy, cx, cy, W, H usable as a camera: "" or what is wrong with it
inline std::string camera_fault(const double* c) {
    for (int i = 0; i < 6; ++i) if (!std::isfinite(c[i])) return "an entry is not finite";
    if (!(c[0] > 0.0) || !(c[1] > 0.0)) return "fx and fy must be positive";
    if (!(c[4] >= 1.0) || !(c[5] >= 1.0) || c[4] != std::floor(c[4]) || c[5] != std::floor(c[5])) return "W and H must be whole numbers >= 1";
    if (!(c[4] * c[5] <= kMaxPixels)) return "W * H is beyond 2^26 pixels";
    return "";
}

inline bool camera_all_zero(const double* c) { for (int i = 0; i < 6; ++i) if (c[i] != 0.0) return false; return true; }

// Everything iba_project_run refuses, in the order the header lists it. intrinsics6: n_frames x 6 of the handle's local frames, or nullptr for a
// handle without intrinsics (scans only). "" = valid.
inline std::string validate(const iba_project_options* opt, const double* x7, const int32_t* frames, int32_t J, int32_t n_frames, const double* intrinsics6) {
    if (!opt) return "opt is NULL";
    if (opt->struct_size != (int32_t)sizeof(iba_project_options)) return "iba_project_options.struct_size is not set (use iba_default_project_options)";
    if (!x7) return "x7 is NULL";
    if (!frames) return "frames is NULL";
    if (J < 1) return "J must be at least 1";
    for (int32_t j = 0; j < J; ++j)
        if (frames[j] < 0 || frames[j] >= n_frames) return "job " + std::to_string(j) + ": frame " + std::to_string(frames[j]) + " is outside the handle's " + std::to_string(n_frames) + " local frames";
    for (int64_t i = 0; i < 7 * (int64_t)J; ++i)
        if (!std::isfinite(x7[i])) return "job " + std::to_string(i / 7) + ": x[" + std::to_string(i % 7) + "] is not finite";
    if (opt->splat < 0 || opt->splat > kMaxSplat) return "splat must be in 0..4";
    if (!std::isfinite(opt->occlusion_tol) || opt->occlusion_tol < 0.0) return "occlusion_tol must be finite and >= 0";
    if (!std::isfinite(opt->z_min) || !std::isfinite(opt->z_max) || !(opt->z_min > 0.0) || !(opt->z_min < opt->z_max)) return "the depth range must be finite with 0 < z_min < z_max";
    if (!std::isfinite(opt->z_near) || !std::isfinite(opt->z_far) || !(opt->z_near < opt->z_far)) return "the gradient's range must be finite with z_near < z_far";
    if (opt->v_focal_is_fx != 0 && opt->v_focal_is_fx != 1) return "v_focal_is_fx must be 0 or 1";
    bool any_nonfinite = false;
    for (int i = 0; i < 6; ++i) any_nonfinite |= !std::isfinite(opt->camera[i]);
    if (any_nonfinite) return "camera: an entry is not finite";
    if (!camera_all_zero(opt->camera)) {
        for (int i = 0; i < 6; ++i) if (opt->camera[i] == 0.0) return "camera is partly zero (all six zero = the frame's intrinsics; otherwise all six must be set)";
        const std::string why = camera_fault(opt->camera);
        if (!why.empty()) return "camera: " + why;
        return "";
    }
    for (int32_t j = 0; j < J; ++j) {
        const std::string why = intrinsics6 ? camera_fault(intrinsics6 + 6 * (size_t)frames[j]) : std::string("a scans-only handle carries none");
        if (!why.empty()) return "job " + std::to_string(j) + ": frame " + std::to_string(frames[j]) + " has no intrinsics (" + why + ") and camera is all 0";
    }
    return "";
}

// chunk c = jobs [cut[c], cut[c + 1]): consecutive jobs while their images stay within `budget` bytes; a chunk holds at least one job
inline std::vector<int32_t> cut_chunks(std::vector<uint64_t> pixels, uint64_t budget) {
    for (uint64_t& p : pixels) p *= kBytesPerPixel;
    return iba::cut_chunks(pixels, budget);
}

}  // namespace project
}  // namespace iba

// The front end of a per-call unit (iba_project.hip, iba_orb.hip, iba_orb_match.hip, iba_twoview.hip, iba_pose.hip, iba_bundle.hip): a unit without a handle checks
// its call on the host, cuts the work into chunks under a byte budget (iba_chunks.hpp), runs one launch chain per chunk, synchronises once and
// returns a host-side result object. What those units share is here: the error slot, IBA_CALL_TRY, the events of a timed call, the guard that
// keeps a chain's host arrays alive until its stream is idle, the budget rule and the index check of an accessor. HIP host code.
//
// A unit declares ONE `thread_local iba::CallError t_err;` (IBA_CALL_TRY names it) and returns t_err.msg.c_str() from its iba_*_last_error.
// In a function that queues asynchronous copies the order of the declarations is: host arrays, DevBufs, SyncOnExit.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/iba_mi355x.h"
#include "iba_chunks.hpp"
#include "iba_internal.hpp"

namespace iba {

// the message of the thread's last failed call of one unit
struct CallError {
    std::string msg;
    iba_status fail(iba_status s, const std::string& m) { msg = m; return s; }
    iba_status fail_hip(const char* what, hipError_t e) { (void)hipGetLastError(); return fail(IBA_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    // the index of an accessor into a result of `count` items: who ends in ": ", noun is "job", "pair" or "image"
    iba_status check_index(bool null_result, int32_t index, size_t count, const std::string& who, const char* noun) {
        if (null_result) return fail(IBA_ERR_INVALID_ARG, who + "the result is NULL");
        if (index < 0 || (size_t)index >= count) return fail(IBA_ERR_INVALID_ARG, who + noun + " " + std::to_string(index) + " is outside the result's " + std::to_string(count) + " " + noun + "s");
        return IBA_OK;
    }
};

#define IBA_CALL_TRY(expr)                                              \
    do {                                                                \
        const hipError_t _e = (expr);                                   \
        if (_e != hipSuccess) return t_err.fail_hip(#expr, _e);         \
    } while (0)

// events of a timed call (debug), destroyed with the scope
struct EventSet {
    std::vector<hipEvent_t> e;
    ~EventSet() { for (hipEvent_t x : e) (void)hipEventDestroy(x); }
    hipError_t create(size_t n) {
        for (size_t i = 0; i < n; ++i) { hipEvent_t x = nullptr; const hipError_t err = hipEventCreate(&x); if (err != hipSuccess) return err; e.push_back(x); }
        return hipSuccess;
    }
};

// Declared after the host arrays and the DevBufs of a chain, so it runs first on unwind: no return, early or not, leaves a copy in flight that
// names one of them. disarm() after the chain's own successful hipStreamSynchronize: the success path then waits once, not twice.
struct SyncOnExit {
    explicit SyncOnExit(hipStream_t s) : st(s) {}
    SyncOnExit(const SyncOnExit&) = delete;
    SyncOnExit& operator=(const SyncOnExit&) = delete;
    ~SyncOnExit() { if (armed && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError(); }
    void disarm() { armed = false; }
    hipStream_t st;
    bool armed = true;
};

// the chunk budget of a call on `device`: cap_bytes, or a quarter of the free device memory where that is less; env_name (debug) overrides it
inline hipError_t call_budget(int device, uint64_t cap_bytes, const char* env_name, uint64_t* budget) {
    hipError_t err = hipSetDevice(device);
    size_t free_b = 0, total_b = 0;
    if (err == hipSuccess) err = hipMemGetInfo(&free_b, &total_b);
    if (err != hipSuccess) return err;
    *budget = std::min<uint64_t>(cap_bytes, (uint64_t)free_b / 4);
    if (const char* e = debug_env(env_name)) *budget = std::strtoull(e, nullptr, 10);
    return hipSuccess;
}

}  // namespace iba

// The one chunk cutter of the per-call units (iba_project, iba_orb, iba_orb_match, iba_twoview, iba_pose, iba_bundle): a call's items (jobs, images, pairs) cut
// into chunks of consecutive items under a byte budget. Plain C++: the sanitizer self-tests compile it with g++ through the *_host.hpp headers.
#pragma once
#include <cstdint>
#include <vector>

namespace iba {

// cut[c] .. cut[c + 1] = the items of chunk c: consecutive items while their bytes stay within `budget` and their number within
// `max_items`; a chunk holds at least one item; no items: {0, 0}
inline std::vector<int32_t> cut_chunks(const std::vector<uint64_t>& bytes, uint64_t budget, int32_t max_items = INT32_MAX) {
    std::vector<int32_t> cut(1, 0);
    uint64_t at = 0;                              // the open chunk's bytes; beyond the budget only where its first item alone is
    for (size_t i = 0; i < bytes.size(); ++i) {
        const size_t held = i - (size_t)cut.back();
        if (held > 0 && (held >= (size_t)max_items || at > budget || bytes[i] > budget - at)) { cut.push_back((int32_t)i); at = 0; }
        at += bytes[i];                           // (no wrap: at <= budget and bytes[i] <= budget - at, or at == 0)
    }
    cut.push_back((int32_t)bytes.size());
    return cut;
}

}  // namespace iba

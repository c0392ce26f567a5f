// gsm_frame_sort_check.h -- the host checks of gsm_debug_frame_sort_create / _run and the guard on
// the tile starts between the tile passes and the depth sort (the plan a run reports: SortPlan::kind,
// gsm_sort_plan.h).  Plain C++17 over
// include/gsm_debug.h alone: no HIP, so a stand-alone CPU program (tests/host/frame_sort_check_test.cpp) runs every
// row without a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gsm_debug.h"

namespace gsm {

// the widest tile field the frame sort takes: one wide pass of 11 bits + one 8-bit pass (kTilesWideMaxBits)
constexpr uint32_t kFrameSortMaxTiles = 1u << 19;
// tile ids of tile << 16 | depth keys
constexpr uint32_t kFrameSortMaxTiles16 = 1u << 16;

inline gsm_status frame_sort_create_check(uint32_t capacity, uint32_t maxTiles, const void* out) {
    if (!out) return GSM_ERR_INVALID_ARGUMENT;
    if (capacity == 0u) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
    if (maxTiles == 0u || maxTiles > kFrameSortMaxTiles) return GSM_ERR_INVALID_TILE_COUNT;
    return GSM_OK;
}

// gsm_debug_frame_sort_run's rows after the handle's, in the header's order
inline gsm_status frame_sort_run_check(uint32_t capacity, uint32_t maxTiles, const gsm_debug_frame_sort_desc* desc,
                                       const void* keys, const void* values, uint32_t n,
                                       const gsm_debug_frame_sort_out* out) {
    if (!desc || !out) return GSM_ERR_INVALID_ARGUMENT;
    if (n > capacity) return GSM_ERR_INVALID_ARGUMENT;
    if (n > 0u && (!keys || !values)) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (((uintptr_t)keys | (uintptr_t)values) & 3u) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (desc->shift != 0u && desc->shift != 16u) return GSM_ERR_INVALID_ARGUMENT;
    if (desc->depth_sort > 1u || desc->full > 1u) return GSM_ERR_INVALID_ARGUMENT;
    if (desc->depth_sort && desc->shift != 16u) return GSM_ERR_INVALID_ARGUMENT;  // (no depth field to sort)
    if (desc->num_tiles == 0u || desc->num_tiles > desc->all_tiles || desc->all_tiles > maxTiles)
        return GSM_ERR_INVALID_ARGUMENT;
    if (desc->shift == 16u && desc->all_tiles > kFrameSortMaxTiles16) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

// The tile starts as k_tile_sort needs them before it may run on them: non-decreasing over [0, numTiles] and at
// most n, so every run [tileStart[t], tileStart[t + 1]) lies inside the n sorted pairs.
inline bool frame_sort_starts_in_range(const uint32_t* tileStart, uint32_t numTiles, uint32_t n) {
    if (!tileStart) return false;
    for (uint32_t t = 0; t < numTiles; ++t)
        if (tileStart[t] > tileStart[t + 1]) return false;
    return tileStart[numTiles] <= n;
}

}  // namespace gsm

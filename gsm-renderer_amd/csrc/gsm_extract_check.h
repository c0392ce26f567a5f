// gsm_extract_check.h -- the host checks of gsm_global_extract and gsm_global_state_histogram, and
// the two keep-set helpers.  Plain C++17 over include/gsm_renderer.h alone: no HIP, so a stand-alone CPU program
// (tests/host/extract_check_test.cpp) runs every row without a device.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gsm_renderer.h"

namespace gsm {

// bytes of one input record / one harmonics element of a handle's precision
inline uint32_t extract_record_bytes(bool half) { return half ? 32u : 48u; }
inline uint32_t extract_element_bytes(bool half) { return half ? 2u : 4u; }
inline uint64_t extract_harmonics_row_bytes(bool half, uint32_t shComponents) {
    return 3ull * shComponents * extract_element_bytes(half);
}

struct ByteRange {
    uintptr_t begin;
    uint64_t bytes;  // 0: the range is not there (a NULL pointer, no rows) and meets nothing
};
inline ByteRange byte_range(const void* p, uint64_t rows, uint64_t rowBytes) {
    return ByteRange{(uintptr_t)p, p ? rows * rowBytes : 0ull};
}
inline bool ranges_meet(const ByteRange& a, const ByteRange& b) {
    return a.bytes && b.bytes && (uint64_t)a.begin < (uint64_t)b.begin + b.bytes &&
           (uint64_t)b.begin < (uint64_t)a.begin + a.bytes;
}

// gsm_global_extract's rows after the handle's, in the header's order
inline gsm_status extract_check(uint32_t maxGaussians, bool half, const gsm_gaussian_input* in,
                                const gsm_global_state* state, const uint32_t* keep,
                                const gsm_global_extract_out* out, const uint32_t* kept) {
    // (the count of a NULL input cannot be read: that is the missing buffer)
    if (in && in->gaussian_count > maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!in || !state || !keep || !out || !kept) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    const uint32_t count = in->gaussian_count, sh = in->sh_components, capacity = out->capacity;
    if (count > 0 && (!in->gaussians || (sh > 0 && !in->harmonics))) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (count > 0 && capacity > 0 && (!out->gaussians || (sh > 0 && !out->harmonics)))
        return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if ((((uintptr_t)kept) & 3u) || (((uintptr_t)out->ids) & 3u)) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (((uintptr_t)out->gaussians) & 15u) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (sh > 0 && (((uintptr_t)out->harmonics) & (extract_element_bytes(half) - 1u))) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (state->default_state > 255u) return GSM_ERR_INVALID_ARGUMENT;
    const uint64_t rec = extract_record_bytes(half), row = extract_harmonics_row_bytes(half, sh);
    const ByteRange writes[5] = {byte_range(out->gaussians, capacity, rec), byte_range(out->harmonics, capacity, row),
                                 byte_range(out->state, capacity, 1), byte_range(out->ids, capacity, 4),
                                 byte_range(kept, 1, 4)};
    const ByteRange reads[3] = {byte_range(in->gaussians, count, rec), byte_range(in->harmonics, count, row),
                                byte_range(state->state, count, 1)};
    for (int w = 0; w < 5; ++w) {
        for (int r = 0; r < 3; ++r)
            if (ranges_meet(writes[w], reads[r])) return GSM_ERR_INVALID_ARGUMENT;
        for (int v = w + 1; v < 5; ++v)
            if (ranges_meet(writes[w], writes[v])) return GSM_ERR_INVALID_ARGUMENT;
    }
    return GSM_OK;
}

// gsm_global_state_histogram's rows after the handle's
inline gsm_status state_histogram_check(uint32_t maxGaussians, const uint8_t* state, uint32_t count,
                                        const uint32_t* histogram) {
    if (count > maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!histogram || (count > 0 && !state)) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (((uintptr_t)histogram) & 3u) return GSM_ERR_INVALID_BUFFER_SIZE;
    return GSM_OK;
}

// gsm_global_keep_visible / gsm_global_keep_masked
inline void keep_visible(const gsm_global_style* styles, uint32_t styleCount, uint32_t keep[8]) {
    if (!keep) return;
    for (int k = 0; k < 8; ++k) keep[k] = 0xFFFFFFFFu;
    if (!styles) return;
    if (styleCount > 256u) styleCount = 256u;
    for (uint32_t s = 0; s < styleCount; ++s)
        if (styles[s].hidden) keep[s >> 5] &= ~(1u << (s & 31u));
}
inline void keep_masked(uint32_t testMask, uint32_t testValue, uint32_t keep[8]) {
    if (!keep) return;
    for (int k = 0; k < 8; ++k) keep[k] = 0u;
    for (uint32_t s = 0; s < 256u; ++s)
        if ((s & testMask & 0xFFu) == (testValue & 0xFFu)) keep[s >> 5] |= 1u << (s & 31u);
}

}  // namespace gsm

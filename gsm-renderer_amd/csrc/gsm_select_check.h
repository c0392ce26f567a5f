// gsm_select_check.h -- the host checks of gsm_global_select_where and gsm_global_state_bounds and
// the query's defaults.  Plain C++17 over include/gsm_renderer.h alone: no HIP, so a stand-alone CPU program
// (tests/host/select_check_test.cpp) runs every row without a device.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>

#include "../../include/gsm_renderer.h"

namespace gsm {

// gsm_global_select_query_default: no shape, identity rows, both ranges (-inf, +inf), every state
inline void select_query_default(gsm_global_select_query* q) {
    if (!q) return;
    const float inf = std::numeric_limits<float>::infinity();
    q->shape = GSM_SELECT_ALL;
    q->flags = 0u;
    for (int i = 0; i < 12; ++i) q->to_shape[i] = (i % 5 == 0) ? 1.0f : 0.0f;  // (row r holds its 1 at column r)
    q->opacity_min = q->scale_min = -inf;
    q->opacity_max = q->scale_max = inf;
    q->test_mask = q->test_value = 0u;
}

// a range is applied unless it is exactly (-inf, +inf)
inline bool select_range_applied(float lo, float hi) {
    const float inf = std::numeric_limits<float>::infinity();
    return !(lo == -inf && hi == inf);
}

// gsm_global_select_where's rows after the handle's, in the header's order
inline gsm_status select_where_check(uint32_t maxGaussians, const gsm_gaussian_input* in,
                                     const gsm_global_select_query* q, const uint8_t* state,
                                     const gsm_global_style* styles, uint32_t styleCount, const uint32_t* matched) {
    // (the count of a NULL input cannot be read: that is the missing buffer)
    if (in && in->gaussian_count > maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!in || !q) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (in->gaussian_count > 0 && (!in->gaussians || !state)) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (((uintptr_t)matched) & 3u) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (q->shape > GSM_SELECT_ELLIPSOID || (q->flags & ~GSM_SELECT_OUTSIDE)) return GSM_ERR_INVALID_ARGUMENT;
    if (q->shape == GSM_SELECT_ALL && (q->flags & GSM_SELECT_OUTSIDE)) return GSM_ERR_INVALID_ARGUMENT;
    if (std::isnan(q->opacity_min) || std::isnan(q->opacity_max) || std::isnan(q->scale_min) ||
        std::isnan(q->scale_max))
        return GSM_ERR_INVALID_ARGUMENT;
    if (q->shape != GSM_SELECT_ALL)
        for (int i = 0; i < 12; ++i)
            if (!std::isfinite(q->to_shape[i])) return GSM_ERR_INVALID_ARGUMENT;
    if (styles ? (styleCount == 0 || styleCount > 256u) : styleCount != 0) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

// gsm_global_state_bounds' rows after the handle's
inline gsm_status state_bounds_check(uint32_t maxGaussians, const gsm_gaussian_input* in,
                                     const gsm_global_state* state, const uint32_t* keep,
                                     const gsm_global_bounds* bounds) {
    if (in && in->gaussian_count > maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!in || !state || !keep || !bounds) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (in->gaussian_count > 0 && !in->gaussians) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (((uintptr_t)bounds) & 3u) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (state->default_state > 255u) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

}  // namespace gsm

// The host checks of gsm_global_select_where and gsm_global_state_bounds and the query's defaults
// (gsm-renderer_amd/csrc/gsm_select_check.h) on the CPU: every row of both check tables, and the order of the rows
// by giving two faults at once.  A stand-alone program over that header alone (no HIP, no device): the device
// pointers are made-up addresses that nothing dereferences.  tests/test_select_where.py builds it with
// -fsanitize=address,undefined and runs it.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>

#include "gsm_select_check.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void* at(uintptr_t a) { return (void*)a; }
static const float kInf = std::numeric_limits<float>::infinity();
static const float kNaN = std::numeric_limits<float>::quiet_NaN();

struct Where {
    gsm_gaussian_input in;
    gsm_global_select_query q;
    uint8_t* state;
    gsm_global_style styles[256];
    const gsm_global_style* stylesPtr;
    uint32_t styleCount;
    uint32_t* matched;
    uint32_t maxGaussians;
    gsm_status run() const {
        return gsm::select_where_check(maxGaussians, &in, &q, state, stylesPtr, styleCount, matched);
    }
};

// 1000 gaussians, a box query, no styles, every pointer given
static Where good() {
    Where c;
    std::memset(&c, 0, sizeof(c));
    c.in.gaussians = at(0x100000);
    c.in.gaussian_count = 1000;
    gsm::select_query_default(&c.q);
    c.q.shape = GSM_SELECT_BOX;
    c.state = (uint8_t*)at(0x300001);  // (a state array has no alignment)
    c.stylesPtr = nullptr;
    c.styleCount = 0;
    c.matched = (uint32_t*)at(0x800000);
    c.maxGaussians = 1000;
    return c;
}

static void test_query_default() {
    gsm_global_select_query q;
    std::memset(&q, 0xA5, sizeof(q));
    gsm::select_query_default(&q);
    EXPECT(q.shape == GSM_SELECT_ALL && q.flags == 0u);
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) EXPECT(q.to_shape[4 * r + c] == (r == c ? 1.0f : 0.0f));
    EXPECT(q.opacity_min == -kInf && q.opacity_max == kInf && q.scale_min == -kInf && q.scale_max == kInf);
    EXPECT(q.test_mask == 0u && q.test_value == 0u);
    EXPECT(!gsm::select_range_applied(q.opacity_min, q.opacity_max));
    EXPECT(gsm::select_range_applied(-kInf, 1.0f) && gsm::select_range_applied(0.0f, kInf));
    EXPECT(gsm::select_range_applied(kInf, -kInf));  // (reversed: applied, and matches nothing)
    gsm::select_query_default(nullptr);              // (a NULL query: nothing to fill)
}

static void test_where_rows() {
    Where c = good();
    EXPECT(c.run() == GSM_OK);
    // count
    c.in.gaussian_count = 1001;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    // input, query
    c = good();
    EXPECT(gsm::select_where_check(1000, nullptr, &c.q, c.state, nullptr, 0, c.matched) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::select_where_check(1000, &c.in, nullptr, c.state, nullptr, 0, c.matched) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    // gaussians, state: only with a count; harmonics never
    c = good(); c.in.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.state = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.in.gaussians = nullptr; c.state = nullptr; c.in.gaussian_count = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.in.harmonics = nullptr; c.in.sh_components = 16;
    EXPECT(c.run() == GSM_OK);
    // matched: nullable, 4-byte aligned
    c = good(); c.matched = nullptr;
    EXPECT(c.run() == GSM_OK);
    for (uintptr_t off = 1; off < 4; ++off) {
        c = good(); c.matched = (uint32_t*)at(0x800000 + off);
        EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    }
    // the query
    c = good(); c.q.shape = 3;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.q.shape = GSM_SELECT_ELLIPSOID; c.q.flags = GSM_SELECT_OUTSIDE;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.q.flags = 2;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.q.flags = 0x80000001u;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.q.shape = GSM_SELECT_ALL; c.q.flags = GSM_SELECT_OUTSIDE;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    float gsm_global_select_query::* const bounds[4] = {&gsm_global_select_query::opacity_min, &gsm_global_select_query::opacity_max,
                                                        &gsm_global_select_query::scale_min, &gsm_global_select_query::scale_max};
    for (auto b : bounds) {
        c = good(); c.q.*b = kNaN;
        EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
        c = good(); c.q.shape = GSM_SELECT_ALL; c.q.*b = kNaN;
        EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
        c = good(); c.q.*b = kInf;  // (infinite bounds are values, in either place)
        EXPECT(c.run() == GSM_OK);
        c = good(); c.q.*b = -kInf;
        EXPECT(c.run() == GSM_OK);
    }
    c = good(); c.q.opacity_min = 1.0f; c.q.opacity_max = 0.0f;  // (reversed: matches nothing, not refused)
    EXPECT(c.run() == GSM_OK);
    for (int i = 0; i < 12; ++i) {
        const float bad[3] = {kNaN, kInf, -kInf};
        for (float v : bad) {
            c = good(); c.q.to_shape[i] = v;
            EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
            c = good(); c.q.shape = GSM_SELECT_ELLIPSOID; c.q.to_shape[i] = v;
            EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
            c = good(); c.q.shape = GSM_SELECT_ALL; c.q.to_shape[i] = v;  // (no shape: to_shape is not read)
            EXPECT(c.run() == GSM_OK);
        }
    }
    // the styles
    c = good(); c.styleCount = 3;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.stylesPtr = c.styles; c.styleCount = 0;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.stylesPtr = c.styles; c.styleCount = 257;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.stylesPtr = c.styles; c.styleCount = 256;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.stylesPtr = c.styles; c.styleCount = 1;
    EXPECT(c.run() == GSM_OK);
}

static void test_where_order() {
    // two faults at once: the earlier row decides
    Where c = good();
    c.in.gaussian_count = 1001;
    EXPECT(gsm::select_where_check(1000, &c.in, nullptr, c.state, nullptr, 0, c.matched) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good(); c.in.gaussian_count = 1001; c.in.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good(); c.state = nullptr; c.matched = (uint32_t*)at(0x800002);
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good();
    EXPECT(gsm::select_where_check(1000, &c.in, nullptr, c.state, nullptr, 3, (uint32_t*)at(0x800002)) ==
           GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.matched = (uint32_t*)at(0x800002); c.q.shape = 3;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.matched = (uint32_t*)at(0x800002); c.styleCount = 3;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    // (the query's row and the styles' row give the same status: both at once is still that status)
    c = good(); c.q.opacity_max = kNaN; c.styleCount = 3;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
}

struct Bounds {
    gsm_gaussian_input in;
    gsm_global_state st;
    uint32_t keep[8];
    gsm_global_bounds* bounds;
    uint32_t maxGaussians;
    gsm_status run() const { return gsm::state_bounds_check(maxGaussians, &in, &st, keep, bounds); }
};

static Bounds good_bounds() {
    Bounds c;
    std::memset(&c, 0, sizeof(c));
    c.in.gaussians = at(0x100000);
    c.in.gaussian_count = 1000;
    c.st.state = (const uint8_t*)at(0x300003);
    for (int k = 0; k < 8; ++k) c.keep[k] = 0xFFFFFFFFu;
    c.bounds = (gsm_global_bounds*)at(0x900004);  // (4-byte aligned is enough)
    c.maxGaussians = 1000;
    return c;
}

static void test_bounds_rows() {
    Bounds c = good_bounds();
    EXPECT(c.run() == GSM_OK);
    c.in.gaussian_count = 1001;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good_bounds();
    EXPECT(gsm::state_bounds_check(1000, nullptr, &c.st, c.keep, c.bounds) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::state_bounds_check(1000, &c.in, nullptr, c.keep, c.bounds) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::state_bounds_check(1000, &c.in, &c.st, nullptr, c.bounds) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::state_bounds_check(1000, &c.in, &c.st, c.keep, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good_bounds(); c.in.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good_bounds(); c.in.gaussians = nullptr; c.in.gaussian_count = 0;
    EXPECT(c.run() == GSM_OK);
    c = good_bounds(); c.st.state = nullptr; c.st.default_state = 255;  // ({NULL, s}: every gaussian's state)
    EXPECT(c.run() == GSM_OK);
    for (uintptr_t off = 1; off < 4; ++off) {
        c = good_bounds(); c.bounds = (gsm_global_bounds*)at(0x900000 + off);
        EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    }
    c = good_bounds(); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good_bounds(); c.st.state = nullptr; c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    // the order
    c = good_bounds(); c.in.gaussian_count = 1001;
    EXPECT(gsm::state_bounds_check(1000, &c.in, nullptr, c.keep, c.bounds) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good_bounds(); c.in.gaussians = nullptr;
    EXPECT(gsm::state_bounds_check(1000, &c.in, &c.st, c.keep, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good_bounds(); c.in.gaussians = nullptr; c.bounds = (gsm_global_bounds*)at(0x900002);
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good_bounds(); c.bounds = (gsm_global_bounds*)at(0x900002); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
}

int main() {
    test_query_default();
    test_where_rows();
    test_where_order();
    test_bounds_rows();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}

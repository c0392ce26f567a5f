// The host checks of gsm_global_extract and gsm_global_state_histogram and the keep-set helpers
// (gsm-renderer_amd/csrc/gsm_extract_check.h) on the CPU: every row of both check tables, the order of the rows by
// giving two faults at once, and the helpers against their rule for all 256 states.  A stand-alone program over
// that header alone (no HIP, no device): the device pointers are made-up addresses that nothing dereferences.
// tests/test_extract.py builds it with -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>

#include "gsm_extract_check.h"

static int failures = 0;
#define EXPECT(cond)                                                  \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                               \
        }                                                             \
    } while (0)

static void* at(uintptr_t a) { return (void*)a; }

struct Call {
    gsm_gaussian_input in;
    gsm_global_state st;
    uint32_t keep[8];
    gsm_global_extract_out out;
    uint32_t* kept;
    uint32_t maxGaussians;
    bool half;
    gsm_status run() const { return gsm::extract_check(maxGaussians, half, &in, &st, keep, &out, kept); }
};

// 1000 gaussians of SH 16 in fp16 (32-byte records, 96-byte rows), every range apart
static Call good() {
    Call c;
    std::memset(&c, 0, sizeof(c));
    c.in.gaussians = at(0x100000);
    c.in.harmonics = at(0x200000);
    c.in.gaussian_count = 1000;
    c.in.sh_components = 16;
    c.st.state = (const uint8_t*)at(0x300000);
    for (int k = 0; k < 8; ++k) c.keep[k] = 0xFFFFFFFFu;
    c.out.gaussians = at(0x400000);
    c.out.harmonics = at(0x500000);
    c.out.state = (uint8_t*)at(0x600000);
    c.out.ids = (uint32_t*)at(0x700000);
    c.out.capacity = 1000;
    c.kept = (uint32_t*)at(0x800000);
    c.maxGaussians = 1000;
    c.half = true;
    return c;
}

static void test_extract_rows() {
    Call c = good();
    EXPECT(c.run() == GSM_OK);
    // count
    c.in.gaussian_count = 1001;
    EXPECT(c.run() == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    // the structs, keep, kept
    c = good();
    EXPECT(gsm::extract_check(1000, true, nullptr, &c.st, c.keep, &c.out, c.kept) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::extract_check(1000, true, &c.in, nullptr, c.keep, &c.out, c.kept) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::extract_check(1000, true, &c.in, &c.st, nullptr, &c.out, c.kept) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::extract_check(1000, true, &c.in, &c.st, c.keep, nullptr, c.kept) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::extract_check(1000, true, &c.in, &c.st, c.keep, &c.out, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    // the input's buffers, only with a count
    c = good(); c.in.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.in.harmonics = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.in.harmonics = nullptr; c.out.harmonics = nullptr; c.in.sh_components = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.in.gaussians = nullptr; c.in.harmonics = nullptr; c.in.gaussian_count = 0;
    EXPECT(c.run() == GSM_OK);
    // the outputs' buffers, only with a count and a capacity
    c = good(); c.out.gaussians = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.out.harmonics = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.out.gaussians = nullptr; c.out.harmonics = nullptr; c.out.capacity = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.out.gaussians = nullptr; c.out.harmonics = nullptr; c.in.gaussian_count = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.out.state = nullptr; c.out.ids = nullptr; c.st.state = nullptr; c.st.default_state = 255;
    EXPECT(c.run() == GSM_OK);
    // alignment
    c = good(); c.kept = (uint32_t*)at(0x800002);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.ids = (uint32_t*)at(0x700001);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.gaussians = at(0x400008);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.harmonics = at(0x500001);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.harmonics = at(0x500002);  // (one half past a 16-byte boundary: aligned to its element)
    EXPECT(c.run() == GSM_OK);
    c = good(); c.half = false; c.out.harmonics = at(0x500002);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.half = false; c.out.harmonics = at(0x500004);
    EXPECT(c.run() == GSM_OK);
    c = good(); c.in.sh_components = 0; c.out.harmonics = at(0x500001);  // (ignored without harmonics)
    EXPECT(c.run() == GSM_OK);
    // default_state (checked with and without an array)
    c = good(); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.st.state = nullptr; c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    // overlap: an output inside the input records; its last byte on the input's first; just apart on both sides
    c = good(); c.out.gaussians = at(0x100000 + 32 * 10);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.out.gaussians = at(0x100000 - 32 * 1000 + 16);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.out.gaussians = at(0x100000 - 32 * 1000);
    EXPECT(c.run() == GSM_OK);
    c = good(); c.out.gaussians = at(0x100000 + 32 * 1000);
    EXPECT(c.run() == GSM_OK);
    // ... in the harmonics, in the state array
    c = good(); c.out.ids = (uint32_t*)at(0x200000 + 96 * 999);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.out.state = (uint8_t*)at(0x300000 + 999);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.kept = (uint32_t*)at(0x300000 + 996);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.kept = (uint32_t*)at(0x300000 + 1000);
    EXPECT(c.run() == GSM_OK);
    // ... two outputs that share bytes; kept inside an output
    c = good(); c.out.ids = (uint32_t*)at(0x600000 + 996);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.out.harmonics = at(0x400000 + 32 * 999);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.kept = (uint32_t*)at(0x700000 + 4 * 999);
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    // ... the ranges follow the count and the capacity: a shorter one no longer meets
    c = good(); c.out.gaussians = at(0x100000 + 32 * 10); c.in.gaussian_count = 10;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.out.ids = (uint32_t*)at(0x600000 + 996); c.out.capacity = 996;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.out.harmonics = at(0x100000); c.in.sh_components = 0;  // (no harmonics: that range is not there)
    EXPECT(c.run() == GSM_OK);
}

static void test_extract_order() {
    // two faults at once: the earlier row decides
    Call c = good();
    c.in.gaussian_count = 1001;
    EXPECT(gsm::extract_check(1000, true, &c.in, nullptr, c.keep, &c.out, c.kept) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    c = good(); c.in.gaussians = nullptr; c.kept = (uint32_t*)at(0x800002);
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.out.gaussians = nullptr; c.out.ids = (uint32_t*)at(0x700001);
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.kept = (uint32_t*)at(0x800002); c.st.default_state = 256;
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.gaussians = at(0x100008); c.st.default_state = 256;  // (misaligned and inside the input)
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.out.harmonics = at(0x500001); c.out.state = (uint8_t*)at(0x300000);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
}

static void test_histogram_rows() {
    const uint8_t* st = (const uint8_t*)at(0x300000);
    uint32_t* h = (uint32_t*)at(0x900000);
    EXPECT(gsm::state_histogram_check(1000, st, 1000, h) == GSM_OK);
    EXPECT(gsm::state_histogram_check(1000, st + 1, 1000, h) == GSM_OK);
    EXPECT(gsm::state_histogram_check(1000, nullptr, 0, h) == GSM_OK);
    EXPECT(gsm::state_histogram_check(1000, st, 1001, h) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    EXPECT(gsm::state_histogram_check(1000, st, 1000, nullptr) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::state_histogram_check(1000, nullptr, 1, h) == GSM_ERR_MISSING_REQUIRED_BUFFER);
    EXPECT(gsm::state_histogram_check(1000, st, 1000, (uint32_t*)at(0x900002)) == GSM_ERR_INVALID_BUFFER_SIZE);
    // the order
    EXPECT(gsm::state_histogram_check(1000, nullptr, 1001, h) == GSM_ERR_INVALID_GAUSSIAN_COUNT);
    EXPECT(gsm::state_histogram_check(1000, nullptr, 1, (uint32_t*)at(0x900002)) == GSM_ERR_MISSING_REQUIRED_BUFFER);
}

static bool bit(const uint32_t keep[8], uint32_t s) { return (keep[s >> 5] >> (s & 31u)) & 1u; }

static void test_keep_helpers() {
    gsm_global_style styles[300];
    std::memset(styles, 0, sizeof(styles));
    for (uint32_t s = 0; s < 300; ++s) styles[s].hidden = (uint8_t)((s * 7u + 3u) % 5u == 0 ? (s % 3u) + 1u : 0u);
    const uint32_t counts[] = {0, 1, 7, 256, 300};
    for (uint32_t n : counts) {
        uint32_t keep[8];
        std::memset(keep, 0xA5, sizeof(keep));
        gsm::keep_visible(styles, n, keep);
        for (uint32_t s = 0; s < 256; ++s) EXPECT(bit(keep, s) == !(s < n && styles[s].hidden != 0));
    }
    uint32_t keep[8];
    std::memset(keep, 0, sizeof(keep));
    gsm::keep_visible(nullptr, 9, keep);
    for (uint32_t s = 0; s < 256; ++s) EXPECT(bit(keep, s));
    const uint32_t pairs[][2] = {{0, 0}, {0, 1}, {1, 1}, {1, 0}, {0x80, 0x80}, {0x80, 0}, {0xFF, 0x9C}, {0xFF, 0x100},
                                 {0x1FF, 0x19C}, {1, 3}};
    for (const auto& p : pairs) {
        std::memset(keep, 0xA5, sizeof(keep));
        gsm::keep_masked(p[0], p[1], keep);
        for (uint32_t s = 0; s < 256; ++s) EXPECT(bit(keep, s) == ((s & p[0] & 0xFFu) == (p[1] & 0xFFu)));
    }
    gsm::keep_visible(styles, 3, nullptr);  // (a NULL set: nothing to fill)
    gsm::keep_masked(1, 1, nullptr);
}

int main() {
    test_extract_rows();
    test_extract_order();
    test_histogram_rows();
    test_keep_helpers();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}

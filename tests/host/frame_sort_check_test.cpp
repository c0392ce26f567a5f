// The host checks of gsm_debug_frame_sort_create / _run and the guard on the tile starts
// (gsm-renderer_amd/csrc/gsm_frame_sort_check.h) on the CPU: every row of both check tables, the order of the rows by
// giving two faults at once, and the guard on real arrays (so the sanitizers see its reads).  The plan a run reports
// for every tile count at a pass boundary: tests/host/sort_plan_test.cpp, on the planners' output.  A stand-alone program over that header alone (no HIP, no device): the device pointers
// are made-up addresses that nothing dereferences.  tests/test_frame_sort.py builds it with
// -fsanitize=address,undefined and runs it.
#include <cstdio>
#include <cstring>
#include <vector>

#include "gsm_frame_sort_check.h"

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
    uint32_t capacity, maxTiles, n;
    gsm_debug_frame_sort_desc d;
    const void *keys, *values;
    gsm_debug_frame_sort_out out;
    gsm_status run() const { return gsm::frame_sort_run_check(capacity, maxTiles, &d, keys, values, n, &out); }
};

// 1000 of 4096 Global keys over 510 of 8160 tiles, depth sorted
static Call good() {
    Call c;
    std::memset(&c, 0, sizeof(c));
    c.capacity = 4096;
    c.maxTiles = 8160;
    c.n = 1000;
    c.d.shift = 16;
    c.d.num_tiles = 510;
    c.d.all_tiles = 8160;
    c.d.depth_sort = 1;
    c.d.full = 1;
    c.keys = at(0x100000);
    c.values = at(0x200000);
    return c;
}

static void test_create_rows() {
    void* h = nullptr;
    EXPECT(gsm::frame_sort_create_check(4096, 8160, &h) == GSM_OK);
    EXPECT(gsm::frame_sort_create_check(1, 1, &h) == GSM_OK);
    EXPECT(gsm::frame_sort_create_check(0xFFFFFFFFu, 1u << 19, &h) == GSM_OK);
    EXPECT(gsm::frame_sort_create_check(4096, 8160, nullptr) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::frame_sort_create_check(0, 8160, &h) == GSM_ERR_INVALID_ASSIGNMENT_CAPACITY);
    EXPECT(gsm::frame_sort_create_check(4096, 0, &h) == GSM_ERR_INVALID_TILE_COUNT);
    EXPECT(gsm::frame_sort_create_check(4096, (1u << 19) + 1u, &h) == GSM_ERR_INVALID_TILE_COUNT);
    // the order
    EXPECT(gsm::frame_sort_create_check(0, 0, nullptr) == GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::frame_sort_create_check(0, 0, &h) == GSM_ERR_INVALID_ASSIGNMENT_CAPACITY);
}

static void test_run_rows() {
    Call c = good();
    EXPECT(c.run() == GSM_OK);
    EXPECT(gsm::frame_sort_run_check(c.capacity, c.maxTiles, nullptr, c.keys, c.values, c.n, &c.out) ==
           GSM_ERR_INVALID_ARGUMENT);
    EXPECT(gsm::frame_sort_run_check(c.capacity, c.maxTiles, &c.d, c.keys, c.values, c.n, nullptr) ==
           GSM_ERR_INVALID_ARGUMENT);
    // the count
    c = good(); c.n = 4096;
    EXPECT(c.run() == GSM_OK);
    c.n = 4097;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.n = 0; c.keys = c.values = nullptr;  // (no keys: nothing to read)
    EXPECT(c.run() == GSM_OK);
    // the pairs
    c = good(); c.keys = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.values = nullptr;
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.keys = at(0x100002);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    c = good(); c.values = at(0x200001);
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
    // the descriptor
    const uint32_t shifts[] = {1, 8, 15, 17, 32};
    for (uint32_t s : shifts) {
        c = good(); c.d.shift = s;
        EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    }
    c = good(); c.d.shift = 0; c.d.depth_sort = 0;
    EXPECT(c.run() == GSM_OK);
    c = good(); c.d.shift = 0;  // (a depth sort of keys without a depth field)
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.depth_sort = 2;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.full = 2;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.depth_sort = 0; c.d.full = 0;
    EXPECT(c.run() == GSM_OK);
    // the tiles
    c = good(); c.d.num_tiles = 0;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.num_tiles = 8160;
    EXPECT(c.run() == GSM_OK);
    c.d.num_tiles = 8161;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.all_tiles = 8161;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.d.all_tiles = 0; c.d.num_tiles = 0;
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.maxTiles = 1u << 19; c.d.all_tiles = 65536;
    EXPECT(c.run() == GSM_OK);
    c.d.all_tiles = 65537;  // (16-bit tile ids beside the depth)
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c.d.shift = 0; c.d.depth_sort = 0;
    EXPECT(c.run() == GSM_OK);
    c.d.all_tiles = c.d.num_tiles = 1u << 19;
    EXPECT(c.run() == GSM_OK);
}

static void test_run_order() {
    Call c = good(); c.n = 4097; c.keys = nullptr;  // count before the pairs
    EXPECT(c.run() == GSM_ERR_INVALID_ARGUMENT);
    c = good(); c.keys = nullptr; c.values = at(0x200001);  // missing before misaligned
    EXPECT(c.run() == GSM_ERR_MISSING_REQUIRED_BUFFER);
    c = good(); c.keys = at(0x100001); c.d.shift = 3;  // the pairs before the descriptor
    EXPECT(c.run() == GSM_ERR_INVALID_BUFFER_SIZE);
}

static void test_starts_guard() {
    using gsm::frame_sort_starts_in_range;
    EXPECT(!frame_sort_starts_in_range(nullptr, 1, 0));
    // heap arrays of exactly numTiles + 1 words: a read past them is the address sanitizer's to report
    std::vector<uint32_t> s = {0, 0, 3, 3, 10};
    EXPECT(frame_sort_starts_in_range(s.data(), 4, 10));
    EXPECT(frame_sort_starts_in_range(s.data(), 4, 11));
    EXPECT(!frame_sort_starts_in_range(s.data(), 4, 9));  // the end past n
    EXPECT(frame_sort_starts_in_range(s.data(), 3, 3));   // (a frame of fewer tiles: the prefix alone)
    s = {0, 4, 3, 3, 10};
    EXPECT(!frame_sort_starts_in_range(s.data(), 4, 10));  // a start that steps back
    EXPECT(frame_sort_starts_in_range(s.data(), 1, 10));
    s = {0, 0, 3, 0xFFFFFFFFu, 10};
    EXPECT(!frame_sort_starts_in_range(s.data(), 4, 10));
    s = {7};
    EXPECT(!frame_sort_starts_in_range(s.data(), 0, 6));
    EXPECT(frame_sort_starts_in_range(s.data(), 0, 7));
    std::vector<uint32_t> z(524289, 0u);
    EXPECT(frame_sort_starts_in_range(z.data(), 524288, 0));
    z[524288] = 1;
    EXPECT(!frame_sort_starts_in_range(z.data(), 524288, 0));
}

int main() {
    test_create_rows();
    test_run_rows();
    test_run_order();
    test_starts_guard();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}

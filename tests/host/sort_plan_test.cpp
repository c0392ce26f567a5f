// sort_plan_test.cpp -- the radix sorts' pass plans (gsm_sort_plan.h) on the CPU: which passes a sort of gsm_sort.hip
// runs, each pass's digit, grid, row set, LDS bytes, totals offset and part in the tile starts, the plan a frame sort
// reports, and the fit against a workspace.  Every expected value below is a literal written by hand from the launch
// code the header replaced (never computed by the functions under test).
// Built and run by tests/test_sort_plan.py (g++ -std=c++17 -Wall -Wextra -Werror); prints the failed rows, exits 1.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "gsm_sort_plan.h"

using gsm::SortPass;
using gsm::SortPlan;
using gsm::SortStarts;

static int failures = 0, checks = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        ++checks;                                                 \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

// a plan's kind, pass count and result index
static void expect_plan(int line, const SortPlan& p, uint32_t kind, uint32_t count, int result) {
    ++checks;
    if (p.valid && p.kind == kind && p.count == count && p.result == result) return;
    ++failures;
    std::printf("FAILED line %d: valid %d kind %u count %u result %d, expected 1 %u %u %d\n", line, (int)p.valid, p.kind,
                p.count, p.result, kind, count, result);
}
// one pass: narrow (0) or wide (1), bits, shift, base, row set, LDS bytes, totals offset, part in the starts, low bits,
// and the tiles of a STARTS pass
static void expect_pass(int line, const SortPlan& plan, uint32_t i, int wide, uint32_t bits, uint32_t shift, uint32_t base,
                        int set, uint32_t lds, uint32_t totalsAt, SortStarts starts, uint32_t lowBits = 0,
                        uint32_t numTiles = 0, uint32_t allTiles = 0) {
    ++checks;
    const SortPass& p = plan.pass[i];
    if (i < plan.count && (int)p.wide == wide && p.bits == bits && p.shift == shift && p.base == base && p.superSet == set &&
        p.ldsBytes == lds && p.totalsAt == totalsAt && p.starts == starts && p.lowBits == lowBits &&
        p.numTiles == numTiles && p.allTiles == allTiles)
        return;
    ++failures;
    std::printf("FAILED line %d pass %u of %u: wide %d bits %u shift %u base %u set %d lds %u totals %u starts %u low %u tiles %u/%u,"
                " expected %d %u %u %u %d %u %u %u %u %u/%u\n",
                line, i, plan.count, (int)p.wide, p.bits, p.shift, p.base, p.superSet, p.ldsBytes, p.totalsAt,
                (unsigned)p.starts, p.lowBits, p.numTiles, p.allTiles, wide, bits, shift, base, set, lds, totalsAt,
                (unsigned)starts, lowBits, numTiles, allTiles);
}
#define PLAN(...) expect_plan(__LINE__, __VA_ARGS__)
#define PASS(...) expect_pass(__LINE__, __VA_ARGS__)

constexpr uint32_t C = 100000;  // 25 chunks of 4096 keys
constexpr uint32_t ONE_NARROW = 1, TWO_NARROW = 2, ONE_WIDE = 3, WIDE_THEN_NARROW = 4;  // gsm_frame_sort_plan

static void test_constants_and_grids() {
    CHECK(GSM_FRAME_SORT_ONE_NARROW == 1 && GSM_FRAME_SORT_TWO_NARROW == 2 && GSM_FRAME_SORT_ONE_WIDE == 3 &&
          GSM_FRAME_SORT_WIDE_THEN_NARROW == 4);
    CHECK(gsm::kRadixBlock == 256 && gsm::kRadixItems == 16 && gsm::kRadixChunk == 4096);
    CHECK(gsm::kWideMaxBits == 11 && gsm::kWideBins == 2048 && gsm::kSortTotalsWords == 2048);
    CHECK(gsm::kWideItems == 16 && gsm::kWideChunk == 4096 && gsm::kWideRowPad == 64);
    CHECK(gsm::kSuperGroup == 32 && gsm::kSuperRows == 32 && gsm::kSuperSetWords == 8192 && gsm::kSuperWords == 16384);
    CHECK(gsm::kTilesWideMaxBits == 19 && gsm::kSortNoSpace == -1);
    // binTotals of two narrow tile passes: the last pass's totals, the first's at +256, its bucket starts at +512
    CHECK(gsm::kSortFirstTotalsAt == 256 && gsm::kSortBucketsAt == 512 && gsm::kSortTwoNarrowWords == 768);
    const uint32_t caps[] = {0, 1, 4096, 4097, 100000, 1u << 20, 4096u * 1024u, 4096u * 1024u + 1u, 0xFFFFF000u};
    const uint32_t grids[] = {1, 1, 1, 2, 25, 256, 1024, 1024, 1024};
    for (int i = 0; i < 9; ++i) {
        CHECK(gsm::radix_grid_for_capacity(caps[i]) == grids[i]);
        CHECK(gsm::wide_grid_for_capacity(caps[i]) == grids[i]);
    }
    // a pass's words of `hist`: the two row sets (16384), then 2^bits words a block, the wide rows padded by 64
    CHECK(gsm::sort_pass_hist_words(false, 8, 25) == 22784);
    CHECK(gsm::sort_pass_hist_words(false, 6, 25) == 17984);
    CHECK(gsm::sort_pass_hist_words(true, 11, 25) == 69184);
    CHECK(gsm::sort_pass_hist_words(true, 9, 25) == 30784);
}

// ---- the tile plans: every all_tiles / num_tiles / shift / wide-switch row of PLANS in tests/test_frame_sort.py ----
static void one_narrow(int line, uint32_t tiles, uint32_t shift, uint32_t bits) {
    for (int wide = 0; wide < 2; ++wide)
        for (int scanless = 0; scanless < 2; ++scanless) {  // neither switch changes a one-pass narrow plan
            const SortPlan p = gsm::plan_sort_tiles(C, shift, 0, tiles, tiles, wide, scanless);
            expect_plan(line, p, ONE_NARROW, 1, 1);
            expect_pass(line, p, 0, 0, bits, shift, 0, -1, 0, 0, SortStarts::FromOneBucket, 0, 0, tiles);
            ++checks;
            if (p.pass[0].grid != 25 || p.pass[0].binWords != 256) ++failures, std::printf("FAILED line %d: grid, bins\n", line);
        }
}
static void two_narrow(int line, uint32_t all, uint32_t num, uint32_t shift, bool wide, uint32_t lo, uint32_t hi) {
    SortPlan p = gsm::plan_sort_tiles(C, shift, 0, num, all, wide, true);
    expect_plan(line, p, TWO_NARROW, 2, 0);
    expect_pass(line, p, 0, 0, lo, shift, 0, 0, 1024, 256, SortStarts::BucketsOut);
    expect_pass(line, p, 1, 0, hi, shift + lo, 0, 1, 0, 0, SortStarts::FromBuckets, lo, 0, all);
    ++checks;
    if (p.pass[0].grid != 25 || p.pass[1].grid != 25 || p.pass[0].binWords != 768 || p.pass[1].binWords != 768)
        ++failures, std::printf("FAILED line %d: grid, bins\n", line);
    p = gsm::plan_sort_tiles(C, shift, 0, num, all, wide, false);  // GSM_SORT_SCAN=kernel: both with k_radix_scan
    expect_plan(line, p, TWO_NARROW, 2, 0);
    expect_pass(line, p, 0, 0, lo, shift, 0, -1, 1024, 256, SortStarts::BucketsOut);
    expect_pass(line, p, 1, 0, hi, shift + lo, 0, -1, 0, 0, SortStarts::FromBuckets, lo, 0, all);
}
static void one_wide(int line, uint32_t all, uint32_t num, uint32_t shift, uint32_t base, uint32_t bits) {
    for (int scanless = 0; scanless < 2; ++scanless) {
        const SortPlan p = gsm::plan_sort_tiles(C, shift, base, num, all, true, scanless);
        expect_plan(line, p, ONE_WIDE, 1, 1);
        expect_pass(line, p, 0, 1, bits, shift, base, -1, 0, 0, SortStarts::WideTiles, 0, num, all);
        ++checks;
        if (p.pass[0].grid != 25 || p.pass[0].binWords != (bits == 9 ? 512u : bits == 10 ? 1024u : 2048u))
            ++failures, std::printf("FAILED line %d: grid, bins\n", line);
    }
}
static void wide_then_narrow(int line, uint32_t all, uint32_t lo, uint32_t buckets) {
    const SortPlan p = gsm::plan_sort_tiles_wide(C, all);
    expect_plan(line, p, WIDE_THEN_NARROW, 2, 0);
    expect_pass(line, p, 0, 1, lo, 0, 0, -1, 0, 0, SortStarts::WideBuckets, 0, buckets, buckets);
    expect_pass(line, p, 1, 0, 8, lo, 0, -1, 0, 0, SortStarts::FromBigBuckets, lo, 0, all);
    ++checks;
    if (p.pass[0].grid != 25 || p.pass[1].grid != 25 || p.pass[0].binWords != buckets || p.pass[1].binWords != 256)
        ++failures, std::printf("FAILED line %d: grid, bins\n", line);
}

static void test_tile_plans() {
    // one narrow pass: fields of fewer than 4 bits are clamped to 4
    one_narrow(__LINE__, 1, 16, 4);
    one_narrow(__LINE__, 2, 16, 4);
    one_narrow(__LINE__, 16, 16, 4);
    one_narrow(__LINE__, 17, 16, 5);
    one_narrow(__LINE__, 33, 16, 6);
    one_narrow(__LINE__, 65, 16, 7);
    one_narrow(__LINE__, 129, 16, 8);
    one_narrow(__LINE__, 256, 16, 8);
    one_narrow(__LINE__, 129, 0, 8);
    // two narrow passes: more than 2048 tiles in the frame ...
    two_narrow(__LINE__, 2049, 2049, 16, true, 6, 6);
    two_narrow(__LINE__, 4080, 4080, 16, true, 6, 6);
    two_narrow(__LINE__, 16200, 16200, 16, true, 7, 7);
    two_narrow(__LINE__, 65536, 65536, 16, true, 8, 8);
    two_narrow(__LINE__, 4080, 4080, 0, true, 6, 6);
    two_narrow(__LINE__, 16200, 2049, 16, true, 7, 7);  // (a slab of more than 2048 tiles)
    // ... or wide digits off (the one wide pass refused)
    two_narrow(__LINE__, 257, 257, 16, false, 5, 4);
    two_narrow(__LINE__, 300, 300, 16, false, 5, 4);
    two_narrow(__LINE__, 1800, 1800, 16, false, 6, 5);
    two_narrow(__LINE__, 16200, 1800, 16, false, 7, 7);
    // tile fields of 9 to 16 bits
    two_narrow(__LINE__, 512, 512, 16, false, 5, 4);
    two_narrow(__LINE__, 1024, 1024, 16, false, 5, 5);
    two_narrow(__LINE__, 2048, 2048, 16, false, 6, 5);
    two_narrow(__LINE__, 4096, 4096, 16, false, 6, 6);
    two_narrow(__LINE__, 8192, 8192, 16, false, 7, 6);
    two_narrow(__LINE__, 16384, 16384, 16, false, 7, 7);
    two_narrow(__LINE__, 32768, 32768, 16, false, 8, 7);
    two_narrow(__LINE__, 65536, 65536, 16, false, 8, 8);
    // one wide pass: 9, 10 and 11 bits; a frame smaller than its configuration; a slab that starts at tile 7000
    one_wide(__LINE__, 257, 257, 16, 0, 9);
    one_wide(__LINE__, 1000, 1000, 16, 0, 10);
    one_wide(__LINE__, 2048, 2048, 16, 0, 11);
    one_wide(__LINE__, 16200, 1800, 16, 0, 11);
    one_wide(__LINE__, 1000, 1000, 0, 0, 10);
    one_wide(__LINE__, 16200, 1800, 16, 7000, 11);
    one_wide(__LINE__, 300, 100, 16, 0, 9);  // (7 bits of local tiles: clamped to 9)
    // one wide pass, then 8 bits: the tile counts of PLANS (17, 17, 17, 18 and 19 bits) ...
    wide_then_narrow(__LINE__, 65537, 9, 512);
    wide_then_narrow(__LINE__, 65792, 9, 512);
    wide_then_narrow(__LINE__, 131072, 9, 512);
    wide_then_narrow(__LINE__, 262144, 10, 1024);
    wide_then_narrow(__LINE__, 524288, 11, 2048);
    // ... and the first count of each width
    wide_then_narrow(__LINE__, 131073, 10, 1024);
    wide_then_narrow(__LINE__, 262145, 11, 2048);
    // above kTilesWideMaxBits: no plan, and it fits nothing
    const SortPlan over = gsm::plan_sort_tiles_wide(C, 524289);
    CHECK(!over.valid && over.count == 0);
    CHECK(!gsm::sort_plan_fits(over, (size_t)1 << 30, 1u << 20, true, true));
    CHECK(!gsm::plan_sort_tiles_wide(C, 0xFFFFFFFFu).valid);
}

// The plan a frame sort reports (gsm_debug_frame_sort_out::plan = SortPlan::kind), for every tile count at a pass
// boundary: one pass (result 1) is the narrow one up to 256 tiles and the wide one above, two passes (result 0) the
// two narrow ones up to 65,536 tiles and wide-then-narrow above.
static void test_reported_plan() {
    const uint32_t one[] = {1, 2, 16, 17, 33, 65, 129, 256};
    for (uint32_t t : one) PLAN(gsm::plan_sort_tiles(C, 16, 0, t, t, true, true), ONE_NARROW, 1, 1);
    const uint32_t mid[] = {257, 300, 1000, 2048, 2049, 16200, 65536};
    for (uint32_t t : mid) {  // (one pass over more than 2048 tiles: a frame of at most 2048 of them)
        PLAN(gsm::plan_sort_tiles(C, 16, 0, t < 2048 ? t : 2048, t, true, true), ONE_WIDE, 1, 1);
        PLAN(gsm::plan_sort_tiles(C, 16, 0, t, t, false, true), TWO_NARROW, 2, 0);
    }
    const uint32_t big[] = {65537, 65792, 131072, 262144, 524288};
    for (uint32_t t : big) PLAN(gsm::plan_sort_tiles_wide(C, t), WIDE_THEN_NARROW, 2, 0);
}

// ---- plan_sort_bits ----
static void test_bits_plans() {
    const SortStarts N = SortStarts::None;
    // 32 bits, wide: 11, 11, 10 -- never scanless
    for (int scanless = 0; scanless < 2; ++scanless) {
        const SortPlan p = gsm::plan_sort_bits(C, 0, 32, true, scanless);
        PLAN(p, 0, 3, 1);
        PASS(p, 0, 1, 11, 0, 0, -1, 0, 0, N);
        PASS(p, 1, 1, 11, 11, 0, -1, 0, 0, N);
        PASS(p, 2, 1, 10, 22, 0, -1, 0, 0, N);
        CHECK(p.pass[0].binWords == 2048 && p.pass[2].binWords == 1024 && p.pass[0].grid == 25);
        CHECK(p.pass[0].histWords == 69184 && p.pass[2].histWords == 16384 + 1088 * 25);
    }
    // 32 bits, narrow: 8, 8, 8, 8 on row sets 0, 1, 0, 1
    SortPlan p = gsm::plan_sort_bits(C, 0, 32, false, true);
    PLAN(p, 0, 4, 0);
    PASS(p, 0, 0, 8, 0, 0, 0, 1024, 0, N);
    PASS(p, 1, 0, 8, 8, 0, 1, 1024, 0, N);
    PASS(p, 2, 0, 8, 16, 0, 0, 1024, 0, N);
    PASS(p, 3, 0, 8, 24, 0, 1, 1024, 0, N);
    CHECK(p.pass[0].binWords == 256 && p.pass[3].histWords == 22784);
    p = gsm::plan_sort_bits(C, 0, 32, false, false);  // the scanless switch off: every pass with k_radix_scan
    PLAN(p, 0, 4, 0);
    for (uint32_t i = 0; i < 4; ++i) PASS(p, i, 0, 8, 8 * i, 0, -1, 1024, 0, N);
    // 16 bits with either switch: 8, 8 (two wide passes would save none)
    for (int wide = 0; wide < 2; ++wide) {
        p = gsm::plan_sort_bits(C, 0, 16, wide, true);
        PLAN(p, 0, 2, 0);
        PASS(p, 0, 0, 8, 0, 0, 0, 1024, 0, N);
        PASS(p, 1, 0, 8, 8, 0, 1, 1024, 0, N);
        p = gsm::plan_sort_bits(C, 0, 16, wide, false);
        PASS(p, 0, 0, 8, 0, 0, -1, 1024, 0, N);
        PASS(p, 1, 0, 8, 8, 0, -1, 1024, 0, N);
    }
    // 20 bits at shift 4: 7, 7, 6 narrow (an odd count: not scanless), 10, 10 wide
    p = gsm::plan_sort_bits(C, 4, 20, false, true);
    PLAN(p, 0, 3, 1);
    PASS(p, 0, 0, 7, 4, 0, -1, 1024, 0, N);
    PASS(p, 1, 0, 7, 11, 0, -1, 1024, 0, N);
    PASS(p, 2, 0, 6, 18, 0, -1, 1024, 0, N);
    CHECK(p.pass[0].binWords == 128 && p.pass[2].binWords == 64);
    p = gsm::plan_sort_bits(C, 4, 20, true, true);
    PLAN(p, 0, 2, 0);
    PASS(p, 0, 1, 10, 4, 0, -1, 0, 0, N);
    PASS(p, 1, 1, 10, 14, 0, -1, 0, 0, N);
    // 12 bits: 6, 6 with either switch
    for (int wide = 0; wide < 2; ++wide) {
        p = gsm::plan_sort_bits(C, 0, 12, wide, true);
        PLAN(p, 0, 2, 0);
        PASS(p, 0, 0, 6, 0, 0, 0, 1024, 0, N);
        PASS(p, 1, 0, 6, 6, 0, 1, 1024, 0, N);
    }
    // the clamps: 3 bits in one pass of 4; 17 bits wide in 9 + 9 (8 left, clamped); 9 bits narrow in 5 + 4, and in one
    // wide pass with the switch on
    p = gsm::plan_sort_bits(C, 0, 3, true, true);
    PLAN(p, 0, 1, 1);
    PASS(p, 0, 0, 4, 0, 0, -1, 1024, 0, N);
    p = gsm::plan_sort_bits(C, 0, 17, true, true);
    PLAN(p, 0, 2, 0);
    PASS(p, 0, 1, 9, 0, 0, -1, 0, 0, N);
    PASS(p, 1, 1, 9, 9, 0, -1, 0, 0, N);
    p = gsm::plan_sort_bits(C, 0, 9, false, true);
    PLAN(p, 0, 2, 0);
    PASS(p, 0, 0, 5, 0, 0, 0, 1024, 0, N);
    PASS(p, 1, 0, 4, 5, 0, 1, 1024, 0, N);
    p = gsm::plan_sort_bits(C, 0, 9, true, true);
    PLAN(p, 0, 1, 1);
    PASS(p, 0, 1, 9, 0, 0, -1, 0, 0, N);
    // no bits, no passes; more bits than four passes hold: no plan
    PLAN(gsm::plan_sort_bits(C, 0, 0, true, true), 0, 0, 0);
    CHECK(!gsm::plan_sort_bits(C, 0, 33, false, true).valid);
}

// ---- plan_sort_pairs ----
static void test_pairs_plans() {
    const SortStarts N = SortStarts::None;
    SortPlan p = gsm::plan_sort_pairs(C, 0, 3, true);  // an odd digit count: no scanless
    PLAN(p, 0, 3, 1);
    for (uint32_t i = 0; i < 3; ++i) PASS(p, i, 0, 8, 8 * i, 0, -1, 1024, 0, N);
    CHECK(p.pass[0].binWords == 256 && p.pass[2].binWords == 256 && p.pass[1].grid == 25);
    p = gsm::plan_sort_pairs(C, 0, 4, true);
    PLAN(p, 0, 4, 0);
    PASS(p, 0, 0, 8, 0, 0, 0, 1024, 0, N);
    PASS(p, 1, 0, 8, 8, 0, 1, 1024, 0, N);
    PASS(p, 2, 0, 8, 16, 0, 0, 1024, 0, N);
    PASS(p, 3, 0, 8, 24, 0, 1, 1024, 0, N);
    p = gsm::plan_sort_pairs(C, 1, 4, true);
    PLAN(p, 0, 4, 0);
    PASS(p, 0, 0, 8, 8, 0, 0, 1024, 0, N);
    PASS(p, 1, 0, 8, 16, 0, 1, 1024, 0, N);
    PASS(p, 2, 0, 8, 24, 0, 0, 1024, 0, N);
    PASS(p, 3, 0, 8, 32, 0, 1, 1024, 0, N);
    p = gsm::plan_sort_pairs(C, 0, 4, false);
    for (uint32_t i = 0; i < 4; ++i) PASS(p, i, 0, 8, 8 * i, 0, -1, 1024, 0, N);
    p = gsm::plan_sort_pairs(C, 2, 2, true);
    PLAN(p, 0, 2, 0);
    PASS(p, 0, 0, 8, 16, 0, 0, 1024, 0, N);
    PASS(p, 1, 0, 8, 24, 0, 1, 1024, 0, N);
    p = gsm::plan_sort_pairs(C, 1, 1, true);
    PLAN(p, 0, 1, 1);
    PASS(p, 0, 0, 8, 8, 0, -1, 1024, 0, N);
}

// ---- the fit ----
// every plan above, at a capacity
static std::vector<SortPlan> plans_at(uint32_t cap) {
    std::vector<SortPlan> v;
    const uint32_t tiles[] = {1, 2, 16, 17, 33, 65, 129, 256, 257, 300, 512, 1000, 1024, 1800, 2048, 2049, 4080,
                              4096, 8192, 16200, 16384, 32768, 65536};
    for (uint32_t t : tiles)
        for (int sw = 0; sw < 4; ++sw)
            for (uint32_t shift = 0; shift <= 16; shift += 16) v.push_back(gsm::plan_sort_tiles(cap, shift, 0, t, t, sw & 1, sw & 2));
    for (int sw = 0; sw < 4; ++sw) {
        v.push_back(gsm::plan_sort_tiles(cap, 16, 0, 1800, 16200, sw & 1, sw & 2));
        v.push_back(gsm::plan_sort_tiles(cap, 16, 7000, 1800, 16200, sw & 1, sw & 2));
        v.push_back(gsm::plan_sort_tiles(cap, 16, 0, 2049, 16200, sw & 1, sw & 2));
        v.push_back(gsm::plan_sort_tiles(cap, 16, 0, 100, 300, sw & 1, sw & 2));
        const uint32_t bits[] = {0, 3, 9, 12, 16, 17, 20, 32};
        for (uint32_t b : bits) v.push_back(gsm::plan_sort_bits(cap, 0, b, sw & 1, sw & 2));
        v.push_back(gsm::plan_sort_bits(cap, 4, 20, sw & 1, sw & 2));
    }
    const uint32_t big[] = {65537, 65792, 131072, 131073, 262144, 262145, 524288};
    for (uint32_t t : big) v.push_back(gsm::plan_sort_tiles_wide(cap, t));
    for (int first = 0; first < 2; ++first)
        for (int sl = 0; sl < 2; ++sl) {
            v.push_back(gsm::plan_sort_pairs(cap, first, 3, sl));
            v.push_back(gsm::plan_sort_pairs(cap, first, 4, sl));
        }
    return v;
}
static bool has_wide_11(const SortPlan& p) {
    for (uint32_t i = 0; i < p.count; ++i)
        if (p.pass[i].wide && p.pass[i].bits == 11) return true;
    return false;
}

static void test_fit() {
    // sort_workspace_bytes: 16384 words of row sets + 2112 words (an 11-bit wide row) a block, 4 bytes each
    const uint32_t caps[] = {1, 4096, 4097, 1u << 20, 4096u * 1024u + 1u};
    const size_t bytes[] = {73984, 73984, 82432, 2228224, 8716288};
    for (int c = 0; c < 5; ++c) {
        CHECK(gsm::sort_workspace_bytes(caps[c]) == bytes[c]);
        int widest = 0;
        for (const SortPlan& p : plans_at(caps[c])) {
            // the workspace covers the widest pass any planner emits at that capacity ...
            CHECK(gsm::sort_plan_fits(p, bytes[c], 2048, true, true));
            // ... and, one word shorter, no plan with the widest pass (11 bits wide); every other plan still fits
            CHECK(gsm::sort_plan_fits(p, bytes[c] - 4, 2048, true, true) == !has_wide_11(p));
            widest += has_wide_11(p);
            // no workspace, no bins
            if (p.count) {
                CHECK(!gsm::sort_plan_fits(p, bytes[c], 2048, false, true));
                CHECK(!gsm::sort_plan_fits(p, bytes[c], 2048, true, false));
                CHECK(!gsm::sort_plan_fits(p, 0, 2048, true, true));
                CHECK(!gsm::sort_plan_fits(p, bytes[c], 0, true, true));
            }
        }
        CHECK(widest >= 8);  // (the one-wide plans of 1800 and 2048 tiles alone are 8)
    }
    // a narrow pass's own footprint: 8 bits on 25 blocks is 22784 words
    const SortPlan pairs = gsm::plan_sort_pairs(C, 0, 4, true);
    CHECK(gsm::sort_plan_fits(pairs, 22784 * 4, 256, true, true));
    CHECK(!gsm::sort_plan_fits(pairs, 22784 * 4 - 4, 256, true, true));
    CHECK(!gsm::sort_plan_fits(pairs, 22784 * 4, 255, true, true));
    // the bins: a two-narrow tile plan needs 768 (two passes' totals and the bucket starts), one narrow pass 256, a
    // wide pass 2^bits, a bits plan's narrow pass 2^bits
    const SortPlan two = gsm::plan_sort_tiles(C, 16, 0, 4080, 4080, true, true);
    CHECK(!gsm::sort_plan_fits(two, 1u << 20, 256, true, true));
    CHECK(!gsm::sort_plan_fits(two, 1u << 20, 767, true, true));
    CHECK(gsm::sort_plan_fits(two, 1u << 20, 768, true, true));
    const SortPlan one = gsm::plan_sort_tiles(C, 16, 0, 16, 16, true, true);
    CHECK(!gsm::sort_plan_fits(one, 1u << 20, 255, true, true));
    CHECK(gsm::sort_plan_fits(one, 1u << 20, 256, true, true));
    const SortPlan wide = gsm::plan_sort_tiles(C, 16, 0, 1000, 1000, true, true);
    CHECK(!gsm::sort_plan_fits(wide, 1u << 20, 1023, true, true));
    CHECK(gsm::sort_plan_fits(wide, 1u << 20, 1024, true, true));
    const SortPlan twelve = gsm::plan_sort_bits(C, 0, 12, false, true);
    CHECK(!gsm::sort_plan_fits(twelve, 1u << 20, 63, true, true));
    CHECK(gsm::sort_plan_fits(twelve, 1u << 20, 64, true, true));
    // the wide-then-narrow plan: 512 bins for 65537 tiles; null hist, null bins, null buckets
    const SortPlan wn = gsm::plan_sort_tiles_wide(C, 65537);
    CHECK(gsm::sort_plan_fits(wn, 1u << 20, 512, true, true, true));
    CHECK(!gsm::sort_plan_fits(wn, 1u << 20, 511, true, true, true));
    CHECK(!gsm::sort_plan_fits(wn, 1u << 20, 512, false, true, true));
    CHECK(!gsm::sort_plan_fits(wn, 1u << 20, 512, true, false, true));
    CHECK(!gsm::sort_plan_fits(wn, 1u << 20, 512, true, true, false));
    CHECK(gsm::sort_plan_fits(two, 1u << 20, 768, true, true, false));  // (no other plan reads `buckets`)
    CHECK(gsm::sort_plan_fits(wide, 1u << 20, 1024, true, true, false));
    // a plan of no passes reads nothing
    CHECK(gsm::sort_plan_fits(gsm::plan_sort_bits(C, 0, 0, true, true), 0, 0, false, false, false));
    // narrow passes read at most 1024 blocks' rows: a pass made by hand on 1025 does not fit, a wide one is not asked
    SortPlan hand;
    hand.add(gsm::sort_narrow_pass(C, 0, 8, -1, SortStarts::None, 256));
    hand.pass[0].grid = 1024;
    CHECK(gsm::sort_plan_fits(hand, 1u << 24, 2048, true, true));
    hand.pass[0].grid = 1025;
    CHECK(!gsm::sort_plan_fits(hand, 1u << 24, 2048, true, true));
    hand.pass[0].wide = true;
    CHECK(gsm::sort_plan_fits(hand, 1u << 24, 2048, true, true));
    // a fifth pass does not fit the plan
    SortPlan five;
    for (int i = 0; i < 5; ++i) five.add(gsm::sort_narrow_pass(C, 0, 8, -1, SortStarts::None, 256));
    CHECK(!five.valid && five.count == 4);
}

int main() {
    test_constants_and_grids();
    test_tile_plans();
    test_reported_plan();
    test_bits_plans();
    test_pairs_plans();
    test_fit();
    if (failures) {
        std::printf("%d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("all checks passed (%d)\n", checks);
    return 0;
}

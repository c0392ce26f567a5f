// gsm_sort_plan.h -- which passes a radix sort of gsm_sort.hip runs, each with what its launches read, and whether
// they fit the workspace (host only, plain C++17: no HIP; gsm_debug.h for the GSM_FRAME_SORT_* values).  An entry of
// gsm_sort.hip asks its planner and hands the plan to run_sort_plan, which checks sort_plan_fits and launches what the
// plan says; tests/host/sort_plan_test.cpp holds the planners to tables written by hand.  DESIGN.md 34.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/gsm_debug.h"

namespace gsm {

// What the kernels of gsm_sort.hip and the plan share.
constexpr int kRadixBlock = 256;
constexpr int kRadixItems = 16;  // keys per thread per chunk (4096-key chunks)
constexpr int kRadixChunk = kRadixBlock * kRadixItems;
// wide radix digits: up to 11 bits, 2048 bins, in chunks of kWideChunk keys (kWideItems per thread; 8 measured
// slower): their per-chunk digit bookkeeping is heavier, so their blocks are fewer per CU
constexpr uint32_t kWideMaxBits = 11, kWideBins = 1u << kWideMaxBits;
constexpr int kWideItems = 16;
constexpr int kWideChunk = kRadixBlock * kWideItems;
static_assert(kWideItems % 4 == 0 && kWideItems <= kRadixItems, "wide chunks: 16-B loads, <= the narrow chunk");
// the wide passes' block-major count rows of 2^bits words are padded by 256 B (rows of a power-of-two stride all
// start on the same HBM channel group)
constexpr uint32_t kWideRowPad = 64;
// the scanless narrow passes' super-group rows (gsm_sort.hip): kSuperGroup consecutive blocks share a row of 256
// words, two row sets in front of every pass's block counts
constexpr uint32_t kSuperGroup = 32;
constexpr uint32_t kSuperRows = 1024 / kSuperGroup;  // radix_grid_for_capacity caps the grid at 1024
constexpr size_t kSuperSetWords = (size_t)kSuperRows * 256;
constexpr size_t kSuperWords = 2 * kSuperSetWords;
// a tile sort's `binTotals`: the last narrow pass's digit totals, the first's at kSortFirstTotalsAt and its bucket
// starts at kSortBucketsAt (<= 256 words each), or one wide pass's 2048 digit totals
constexpr size_t kSortTotalsWords = kWideBins;
constexpr uint32_t kSortFirstTotalsAt = 256, kSortBucketsAt = 512, kSortTwoNarrowWords = 768;
constexpr uint32_t kTilesWideMaxBits = kWideMaxBits + 8u;  // one wide pass + one 8-bit pass
constexpr int kSortNoSpace = -1;

inline uint32_t radix_grid_for_capacity(uint32_t capacity) {
    // <= 1024 blocks: k_radix_scan holds a digit's column in 4 registers per thread
    uint32_t g = (capacity + kRadixChunk - 1) / kRadixChunk;
    return g > 1024 ? 1024 : g < 1 ? 1 : g;
}
inline uint32_t wide_grid_for_capacity(uint32_t capacity) {
    uint32_t g = (capacity + kWideChunk - 1) / kWideChunk;  // (<= 1024 rows: sort_workspace_bytes)
    return g > 1024 ? 1024 : g < 1 ? 1 : g;
}
// The workspace footprint of one pass in words of `hist` -- narrow: digit-major counts hist[d][block] (k_radix_upsweep
// / k_radix_scan); wide: block-major rows of 2^bits + kWideRowPad words (k_wide_upsweep); both behind the scanless
// super-group row sets.
inline size_t sort_pass_hist_words(bool wide, uint32_t bits, uint32_t grid) {
    const size_t rows = wide ? ((size_t)1 << bits) + kWideRowPad : ((size_t)1 << bits);
    return kSuperWords + rows * grid;
}
// Bytes of a sort's workspace (`hist`) for a capacity, zeroed once at allocation: the super-group row sets, then the
// per-block digit counts of the widest pass any planner below emits -- 256 digits (narrow) or 2^kWideMaxBits.
inline size_t sort_workspace_bytes(uint32_t capacity) {
    const size_t narrow = sort_pass_hist_words(false, 8, radix_grid_for_capacity(capacity));
    const size_t wide = sort_pass_hist_words(true, kWideMaxBits, wide_grid_for_capacity(capacity));
    return (narrow > wide ? narrow : wide) * sizeof(uint32_t);
}

// A pass's part in the tile starts (TileStarts and k_wide_downsweep's STARTS, gsm_sort.hip).
enum class SortStarts : uint32_t {
    None,
    BucketsOut,      // narrow, the first of two: block 0 writes the bucket starts to binTotals + kSortBucketsAt
    FromOneBucket,   // narrow, the only pass: the tile starts from one bucket (no bucket array, lowBits 0)
    FromBuckets,     // narrow, the last of two: the tile starts from binTotals + kSortBucketsAt, 2^lowBits buckets
    WideTiles,       // wide, the only pass: block 0 writes tileStart[0 .. allTiles]
    WideBuckets,     // wide, before an 8-bit pass: block 0 writes its digits' bases to `buckets` as 2^bits "tiles"
    FromBigBuckets,  // narrow after WideBuckets: the tile starts from `buckets`, up to 2048 of them (BIGL)
};
// the STARTS instances of the downsweeps
inline bool sort_writes_starts(SortStarts s) { return s != SortStarts::None && s != SortStarts::BucketsOut; }
inline bool sort_uses_buckets(SortStarts s) { return s == SortStarts::WideBuckets || s == SortStarts::FromBigBuckets; }

// Everything one pass's launches read.
struct SortPass {
    bool wide = false;  // k_wide_* (9..11 bits) or k_radix_* (4..8)
    uint32_t bits = 0, shift = 0;
    uint32_t base = 0;  // wide: digit = ((key >> shift) - base) & (2^bits - 1), a slab's first tile
    uint32_t grid = 0;
    int superSet = -1;      // narrow: the scanless row set, 0 or 1; -1: the k_radix_scan launch
    uint32_t ldsBytes = 0;  // dynamic LDS of the downsweep
    uint32_t totalsAt = 0;  // where in binTotals the pass keeps its digit totals
    SortStarts starts = SortStarts::None;
    uint32_t lowBits = 0;                // FromBuckets, FromBigBuckets: bits of the pass before (its digits, the buckets)
    uint32_t numTiles = 0, allTiles = 0;  // the STARTS passes' tiles (narrow: allTiles alone)
    size_t histWords = 0, binWords = 0;   // what the pass needs of `hist` and of `binTotals`
};

struct SortPlan {
    SortPass pass[4];
    uint32_t count = 0;
    int result = 0;     // the ping-pong index of the sorted pairs
    uint32_t kind = 0;  // the GSM_FRAME_SORT_* value of a tile plan, 0 otherwise
    bool valid = true;  // false: a field no plan covers (more than 4 passes, or above kTilesWideMaxBits)
    void add(const SortPass& p) {
        if (count == 4) {
            valid = false;
            return;
        }
        pass[count++] = p;
        result = (int)(count & 1u);
    }
};

// 1 KiB of dynamic LDS on the narrow downsweeps without tile starts: > 40 KiB a block, 3 blocks per CU like the STARTS
// pass -- the first 4K tile pass at 4 blocks per CU measured 2.5 us slower (64.4-65.9 against 62.2-62.4 us; 1080p
// unchanged; r06, profiles/r06_sort_occupancy_ab.txt)
inline SortPass sort_narrow_pass(uint32_t capacity, uint32_t shift, uint32_t bits, int superSet, SortStarts starts,
                                 size_t binWords) {
    SortPass p;
    p.bits = bits, p.shift = shift, p.grid = radix_grid_for_capacity(capacity), p.superSet = superSet, p.starts = starts;
    p.ldsBytes = sort_writes_starts(starts) ? 0u : 1024u;
    p.histWords = sort_pass_hist_words(false, bits, p.grid), p.binWords = binWords;
    return p;
}
inline SortPass sort_wide_pass(uint32_t capacity, uint32_t shift, uint32_t bits, uint32_t base, SortStarts starts,
                               uint32_t numTiles, uint32_t allTiles) {
    SortPass p;
    p.wide = true, p.bits = bits, p.shift = shift, p.base = base, p.grid = wide_grid_for_capacity(capacity);
    p.starts = starts, p.numTiles = numTiles, p.allTiles = allTiles;
    p.histWords = sort_pass_hist_words(true, bits, p.grid), p.binWords = (size_t)1 << bits;
    return p;
}

// bits of the ids of `tiles` tiles, within [from, to]
inline uint32_t sort_bits_for(uint32_t tiles, uint32_t from, uint32_t to) {
    uint32_t b = from;
    while (b < to && ((tiles - 1u) >> b)) b++;
    return b;
}
// Near-equal digit widths: the next of `passesLeft` digits over `bitsLeft` bits, at least `least` (4 narrow, 9 wide:
// a digit wider than the bits left reads zero bits above the field).
inline uint32_t sort_digit_width(uint32_t bitsLeft, uint32_t passesLeft, uint32_t least) {
    const uint32_t b = (bitsLeft + passesLeft - 1) / passesLeft;
    return b < least ? least : b;
}

// radix_sort_bits: bits [shift, shift + bits) in ceil(bits / 8) narrow passes, or -- `wide` and where that saves a
// whole pass (32-bit keys: 3 passes of 11/11/10 bits instead of 4) -- ceil(bits / 11) wide ones.  Scanless only with
// an even number of narrow passes (pass i on row set i & 1: every call starts and ends with set 0 zero).
inline SortPlan plan_sort_bits(uint32_t capacity, uint32_t shift, uint32_t bits, bool wide, bool scanless) {
    const uint32_t narrowPasses = (bits + 7) / 8, widePasses = (bits + kWideMaxBits - 1) / kWideMaxBits;
    const bool useWide = wide && widePasses < narrowPasses;
    const uint32_t passes = useWide ? widePasses : narrowPasses;
    const bool sets = !useWide && scanless && passes % 2 == 0;
    SortPlan plan;
    for (uint32_t p = 0, done = 0; p < passes; ++p) {
        const uint32_t b = sort_digit_width(bits - done, passes - p, useWide ? 9u : 4u);
        if (useWide) plan.add(sort_wide_pass(capacity, shift + done, b, 0u, SortStarts::None, 0u, 0u));
        else
            plan.add(sort_narrow_pass(capacity, shift + done, b, sets ? (int)(p & 1u) : -1, SortStarts::None,
                                      (size_t)1 << b));
        done += b;
    }
    return plan;
}

// radix_sort_pairs: numDigits whole bytes from byte firstDigit, narrow
inline SortPlan plan_sort_pairs(uint32_t capacity, int firstDigit, int numDigits, bool scanless) {
    return plan_sort_bits(capacity, (uint32_t)firstDigit * 8u, (uint32_t)numDigits * 8u, false, scanless);
}

// radix_sort_tiles: the tile field at `shift` of keys that hold tiles [tileBase, tileBase + numTiles) of allTiles
// (<= 65,536), the tile starts written by the last pass.  With <= 2048 tiles in that range (a multi-GPU slab) and wide
// digits on, one wide pass sorts it, digits counted from tileBase; otherwise the narrow passes of plan_sort_bits over
// the whole field (which do not read tileBase): one, or two of 5..8 and 4..8 bits (balanced: 6 + 8 / 8 + 6 at 4K and
// 5 + 7 / 7 + 5 at 1080p measured slower).  The two are scanless whenever the switch is on.
inline SortPlan plan_sort_tiles(uint32_t capacity, uint32_t shift, uint32_t tileBase, uint32_t numTiles,
                                uint32_t allTiles, bool wide, bool scanless) {
    const uint32_t bits = sort_bits_for(allTiles, 1, 16), localBits = sort_bits_for(numTiles, 1, 16);
    SortPlan plan;
    if (wide && bits > 8 && localBits <= kWideMaxBits) {
        plan.kind = GSM_FRAME_SORT_ONE_WIDE;
        plan.add(sort_wide_pass(capacity, shift, sort_digit_width(localBits, 1, 9), tileBase, SortStarts::WideTiles,
                                numTiles, allTiles));
    } else if (bits <= 8) {  // one pass, one bucket
        plan.kind = GSM_FRAME_SORT_ONE_NARROW;
        plan.add(sort_narrow_pass(capacity, shift, sort_digit_width(bits, 1, 4), -1, SortStarts::FromOneBucket, 256));
    } else {
        plan.kind = GSM_FRAME_SORT_TWO_NARROW;
        const uint32_t lo = sort_digit_width(bits, 2, 4), hi = sort_digit_width(bits - lo, 1, 4);
        plan.add(sort_narrow_pass(capacity, shift, lo, scanless ? 0 : -1, SortStarts::BucketsOut, kSortTwoNarrowWords));
        plan.pass[0].totalsAt = kSortFirstTotalsAt;
        plan.add(sort_narrow_pass(capacity, shift + lo, hi, scanless ? 1 : -1, SortStarts::FromBuckets,
                                  kSortTwoNarrowWords));
        plan.pass[1].lowBits = lo;
    }
    plan.pass[plan.count - 1].allTiles = allTiles;
    return plan;
}

// radix_sort_tiles_wide: the tile field of a grid above 65,536 tiles (DepthFirst tile_id_bits 32), 17..19 bits at
// shift 0, in two passes.  One wide pass over the low lo = bits - 8 bits (9..11) whose block 0 also writes its digits'
// global bases -- the low-digit buckets' starts, as a STARTS pass' "tile starts" of 2^lo tiles -- into `buckets`
// (2^lo + 1 words), then one 8-bit pass over the high digit that writes the tile starts from those buckets
// (k_radix_downsweep BIGL), never scanless.  The plan does not depend on the wide switch (three narrow passes could
// not write the starts).  The reference sorts such a field in ceil(bits / 8) = 3 passes (TileSortEncoder.swift:60-62).
inline SortPlan plan_sort_tiles_wide(uint32_t capacity, uint32_t allTiles) {
    const uint32_t bits = sort_bits_for(allTiles, 17, 32);
    SortPlan plan;
    plan.kind = GSM_FRAME_SORT_WIDE_THEN_NARROW;
    if (bits > kTilesWideMaxBits) {
        plan.valid = false;
        return plan;
    }
    const uint32_t lo = bits - 8u;
    plan.add(sort_wide_pass(capacity, 0u, lo, 0u, SortStarts::WideBuckets, 1u << lo, 1u << lo));
    plan.add(sort_narrow_pass(capacity, lo, 8, -1, SortStarts::FromBigBuckets, 256));
    plan.pass[1].lowBits = lo, plan.pass[1].allTiles = allTiles;
    return plan;
}

// The only workspace check: every pass's footprint against what the caller holds.  Nothing is launched for a plan
// that does not fit -- a knob or a grid rule changed without the allocation (the r05 wide-pass A/B fault class,
// VERDICT r05 item 5).
inline bool sort_plan_fits(const SortPlan& plan, size_t histBytes, size_t binWords, bool haveHist, bool haveBins,
                           bool haveBuckets = true) {
    if (!plan.valid) return false;
    for (uint32_t i = 0; i < plan.count; ++i) {
        const SortPass& p = plan.pass[i];
        if (!haveHist || !haveBins || (sort_uses_buckets(p.starts) && !haveBuckets)) return false;
        if (p.histWords * sizeof(uint32_t) > histBytes || p.binWords > binWords) return false;
        // narrow passes read <= 1024 blocks' rows (k_radix_scan's column in registers, the super rows)
        if (!p.wide && p.grid > kSuperRows * kSuperGroup) return false;
    }
    return true;
}

}  // namespace gsm

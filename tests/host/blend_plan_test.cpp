// blend_plan_test.cpp -- the Global blend's launch plan (gsm_blend_plan.h) on the CPU: which of the nine kernel
// families a frame gets, with how many pairs per lane, waves and workgroups, and which flags word.  Every expected
// value below is a literal written by hand from the launch code the header replaced (never computed by the functions
// under test); flag words are sums of the bits' literal values.
// Built and run by tests/test_blend_plan.py (g++ -std=c++17 -Wall -Wextra -Werror); prints the failed rows, exits 1.
#include <cstdint>
#include <cstdio>
#include <functional>

#include "gsm_blend_plan.h"

using gsm::BlendPlan;
using gsm::BlendShape;
using gsm::BlendWalk;
using gsm::FrameKind;

static int failures = 0, checks = 0;
#define CHECK(cond)                                               \
    do {                                                          \
        ++checks;                                                 \
        if (!(cond)) {                                            \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                           \
        }                                                         \
    } while (0)

// a Single frame of `tiles` tiles on `cus` CUs: RGBA16F (format 0) into a 16-byte aligned colour target, no depth, no
// options, claim 1 -- the flags word of its plain walk is 1 + 2 + 256 = 259
static BlendShape shape(int cus, uint32_t tiles) {
    BlendShape s;
    s.numTiles = tiles;
    s.color = 0x1000;
    s.colorPitch = 0x100;
    s.numCUs = cus;
    return s;
}
typedef std::function<void(BlendShape&)> Edit;
static BlendShape with(BlendShape s, const Edit& e) {
    e(s);
    return s;
}
// depth, pick and occluder as aligned as any rule asks
static void depth16(BlendShape& s) { s.depth = 0x2000, s.depthPitch = 0x40; }
static void pick8(BlendShape& s) { s.pick = 0x3000, s.pickPitch = 0x80; }
static void occ8(BlendShape& s) { s.occluder = 0x4000, s.occluderPitch = 0x80, s.sortedVals = true; }

static void expect(int line, const BlendShape& s, BlendWalk walk, int P, int waves, uint32_t grid, int flags,
                   int targetFlags, int kernel) {
    const BlendPlan p = gsm::plan_blend(s);
    ++checks;
    if (p.walk == walk && p.P == P && p.waves == waves && p.grid == grid && p.flags == flags &&
        p.targetFlags == targetFlags && p.kernel == kernel)
        return;
    ++failures;
    std::printf("FAILED line %d: walk %u P %d waves %d grid %u flags %d targetFlags %d kernel %d, expected %u %d %d %u %d %d %d\n",
                line, (unsigned)p.walk, p.P, p.waves, p.grid, p.flags, p.targetFlags, p.kernel, (unsigned)walk, P, waves,
                grid, flags, targetFlags, kernel);
}
#define EXPECT(...) expect(__LINE__, __VA_ARGS__)
#define NOTHING(s) expect(__LINE__, s, BlendWalk::None, 0, 0, 0u, 0, 0, 0)

// (units are a multiple of 4 at P = 1 and of 2 at P = 2, so the rows next to a threshold of units are the nearest
// tile counts on either side of it)
static void shapes_4_cus() {
    const int C = 4;  // P = 1 up to 32 tiles; 12 waves from 96 units, 16 from 384
    NOTHING(shape(C, 0));
    // quadrant / half tile: 32 tiles -> 128 quadrant units, 33 -> 66 half tiles
    EXPECT(shape(C, 32), BlendWalk::Px, 1, 12, 4u, 259, 0, 1);
    EXPECT(shape(C, 33), BlendWalk::Px, 2, 8, 4u, 259, 0, 2);
    // 8 / 12 waves at 96 units: 23 and 24 tiles of quadrants (92, 96), 47 and 48 tiles of halves (94, 96)
    EXPECT(shape(C, 23), BlendWalk::Px, 1, 8, 4u, 259, 0, 1);
    EXPECT(shape(C, 24), BlendWalk::Px, 1, 12, 4u, 259, 0, 1);
    EXPECT(shape(C, 47), BlendWalk::Px, 2, 8, 4u, 259, 0, 2);
    EXPECT(shape(C, 48), BlendWalk::Px, 2, 12, 4u, 259, 0, 2);
    // 12 / 16 waves at 384 units: 191 and 192 tiles of halves (382, 384)
    EXPECT(shape(C, 191), BlendWalk::Px, 2, 12, 4u, 259, 0, 2);
    EXPECT(shape(C, 192), BlendWalk::Px, 2, 16, 4u, 259, 0, 2);
    // the grid: 8 waves, 1 tile -> 4 units -> 1; 6 tiles -> 24 units -> 3 (below the CUs); 7 -> 28 -> 4 (equal, by the
    // division); 9 -> 36 -> 5, clamped to 4
    EXPECT(shape(C, 1), BlendWalk::Px, 1, 8, 1u, 259, 0, 1);
    EXPECT(shape(C, 6), BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    EXPECT(shape(C, 7), BlendWalk::Px, 1, 8, 4u, 259, 0, 1);
    EXPECT(shape(C, 9), BlendWalk::Px, 1, 8, 4u, 259, 0, 1);
    // a waves override: 24 units in workgroups of 8, 12 and 16 waves
    EXPECT(with(shape(C, 6), [](BlendShape& s) { s.waves = 8; }), BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(shape(C, 6), [](BlendShape& s) { s.waves = 12; }), BlendWalk::Px, 1, 12, 2u, 259, 0, 1);
    EXPECT(with(shape(C, 6), [](BlendShape& s) { s.waves = 16; }), BlendWalk::Px, 1, 16, 2u, 259, 0, 1);
    // ... which also overrides a frame that would take 16 (384 units / 8 = 48, / 12 = 32: clamped)
    EXPECT(with(shape(C, 192), [](BlendShape& s) { s.waves = 8; }), BlendWalk::Px, 2, 8, 4u, 259, 0, 2);
    EXPECT(with(shape(C, 192), [](BlendShape& s) { s.waves = 12; }), BlendWalk::Px, 2, 12, 4u, 259, 0, 2);
}

static void shapes_256_cus() {
    const int C = 256;  // P = 1 up to 2048 tiles; 12 waves from 6144 units, 16 from 24576
    NOTHING(shape(C, 0));
    EXPECT(shape(C, 2048), BlendWalk::Px, 1, 12, 256u, 259, 0, 1);  // 8192 units
    EXPECT(shape(C, 2049), BlendWalk::Px, 2, 8, 256u, 259, 0, 2);   // 4098 units
    EXPECT(shape(C, 1535), BlendWalk::Px, 1, 8, 256u, 259, 0, 1);   // 6140 units
    EXPECT(shape(C, 1536), BlendWalk::Px, 1, 12, 256u, 259, 0, 1);  // 6144
    EXPECT(shape(C, 3071), BlendWalk::Px, 2, 8, 256u, 259, 0, 2);   // 6142
    EXPECT(shape(C, 3072), BlendWalk::Px, 2, 12, 256u, 259, 0, 2);  // 6144
    EXPECT(shape(C, 12287), BlendWalk::Px, 2, 12, 256u, 259, 0, 2);  // 24574
    EXPECT(shape(C, 12288), BlendWalk::Px, 2, 16, 256u, 259, 0, 2);  // 24576
    // the grid at 8 waves: 510 tiles -> 2040 units -> 255; 511 -> 2044 -> 256 by the division; 513 -> 2052 -> 257, clamped
    EXPECT(shape(C, 510), BlendWalk::Px, 1, 8, 255u, 259, 0, 1);
    EXPECT(shape(C, 511), BlendWalk::Px, 1, 8, 256u, 259, 0, 1);
    EXPECT(shape(C, 513), BlendWalk::Px, 1, 8, 256u, 259, 0, 1);
    // a waves override: 400 units
    EXPECT(with(shape(C, 100), [](BlendShape& s) { s.waves = 8; }), BlendWalk::Px, 1, 8, 50u, 259, 0, 1);
    EXPECT(with(shape(C, 100), [](BlendShape& s) { s.waves = 12; }), BlendWalk::Px, 1, 12, 34u, 259, 0, 1);
    EXPECT(with(shape(C, 100), [](BlendShape& s) { s.waves = 16; }), BlendWalk::Px, 1, 16, 25u, 259, 0, 1);
    // the pair walk where its rule holds by itself, and its grid: 24576 units / 32 = 768, clamped; with 16 waves
    // asked for, 2049 tiles -> 4098 units / 32 -> 129
    EXPECT(with(shape(C, 12288), [](BlendShape& s) { s.pairs = true; }), BlendWalk::PairSingle, 2, 16, 256u, 2, 1, 3);
    EXPECT(with(shape(C, 2049), [](BlendShape& s) { s.pairs = true, s.waves = 16; }), BlendWalk::PairSingle, 2, 16, 129u,
           2, 1, 3);
    EXPECT(with(shape(C, 12287), [](BlendShape& s) { s.pairs = true; }), BlendWalk::Px, 2, 12, 256u, 259, 0, 2);
}

static void families() {
    const int C = 4;
    const BlendShape small = shape(C, 6);   // quadrants, 8 waves, 3 workgroups
    const BlendShape big = shape(C, 192);   // half tiles, 16 waves, 4 workgroups
    // plain, by kind
    EXPECT(small, BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(small, [](BlendShape& s) { s.kind = FrameKind::Compose; }), BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(small, [](BlendShape& s) { s.kind = FrameKind::Records, s.arrive = true; }), BlendWalk::Px, 1, 8, 3u,
           259 + 4096, 0, 1);
    EXPECT(with(small, [](BlendShape& s) { s.kind = FrameKind::Records; }), BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(small, [](BlendShape& s) { s.kind = FrameKind::Views, s.views = 2; }), BlendWalk::PxViews, 1, 8, 3u, 259,
           0, 1);
    // a batch: bits 1 and 2048 are each view's own (here both would be set: 259 + 2048 without them is 258)
    EXPECT(with(small, [](BlendShape& s) { s.kind = FrameKind::Batch, depth16(s); }), BlendWalk::PxBatch, 1, 8, 3u, 258,
           0, 1);
    EXPECT(with(big, [](BlendShape& s) { s.kind = FrameKind::Batch; }), BlendWalk::PxBatch, 2, 16, 4u, 258, 0, 2);
    // a batch with extras comes first: pick and occluder addresses do not matter, nor their bits
    const Edit extras = [](BlendShape& s) { s.kind = FrameKind::Batch, s.batchExtras = true, s.sortedVals = true, depth16(s); };
    EXPECT(with(small, extras), BlendWalk::BatchOccPick, 1, 8, 3u, 258, 0, 1);
    EXPECT(with(with(small, extras), [](BlendShape& s) { pick8(s), occ8(s), s.pairs = true; }), BlendWalk::BatchOccPick,
           1, 8, 3u, 258, 0, 1);
    EXPECT(with(with(big, extras), [](BlendShape& s) { s.pairs = true; }), BlendWalk::BatchOccPick, 2, 16, 4u, 258, 0, 2);
    NOTHING(with(with(small, extras), [](BlendShape& s) { s.sortedVals = false; }));
    // (extras on a frame that is no batch are not read)
    EXPECT(with(small, [](BlendShape& s) { s.batchExtras = true; }), BlendWalk::Px, 1, 8, 3u, 259, 0, 1);
    // pick + occluder, then pick, then occluder; the occluded walks need the sorted values
    EXPECT(with(small, [](BlendShape& s) { pick8(s), occ8(s); }), BlendWalk::OccPick, 1, 8, 3u, 259 + 8192 + 16384, 0, 1);
    EXPECT(with(small, pick8), BlendWalk::Pick, 1, 8, 3u, 259 + 8192, 0, 1);
    EXPECT(with(small, occ8), BlendWalk::Occ, 1, 8, 3u, 259 + 16384, 0, 1);
    EXPECT(with(with(small, [](BlendShape& s) { s.kind = FrameKind::Compose; }), occ8), BlendWalk::Occ, 1, 8, 3u,
           259 + 16384, 0, 1);
    NOTHING(with(small, [](BlendShape& s) { pick8(s), occ8(s), s.sortedVals = false; }));
    NOTHING(with(small, [](BlendShape& s) { occ8(s), s.sortedVals = false; }));
    EXPECT(with(small, [](BlendShape& s) { pick8(s), s.sortedVals = false; }), BlendWalk::Pick, 1, 8, 3u, 259 + 8192, 0,
           1);
    // ... and each of them before the pair walk
    const Edit pairs = [](BlendShape& s) { s.pairs = true; };
    EXPECT(with(with(big, pairs), pick8), BlendWalk::Pick, 2, 16, 4u, 259 + 8192, 0, 2);
    EXPECT(with(with(big, pairs), occ8), BlendWalk::Occ, 2, 16, 4u, 259 + 16384, 0, 2);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { pick8(s), occ8(s); }), BlendWalk::OccPick, 2, 16, 4u,
           259 + 8192 + 16384, 0, 2);
    // the pair walk by kind: 384 units / 32 = 12 workgroups, clamped; its flags are 2 (+ 4), its target word 1 + format
    EXPECT(with(big, pairs), BlendWalk::PairSingle, 2, 16, 4u, 2, 1, 3);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.kind = FrameKind::Compose; }), BlendWalk::PairSingle, 2, 16, 4u, 2,
           1, 3);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.kind = FrameKind::Views, s.views = 2; }), BlendWalk::PairViews, 2,
           16, 4u, 2, 1, 3);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.kind = FrameKind::Batch, s.colorFormat = 2; }),
           BlendWalk::PairBatch, 2, 16, 4u, 2, 32, 3);  // (bit 1 of the target word is the view's own)
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.costOrder = true, s.colorFormat = 2, s.claim = 2; }),
           BlendWalk::PairSingle, 2, 16, 4u, 2 + 4, 1 + 32, 3);
    // 33 tiles with 16 waves asked for: 66 units / 32 -> 3 workgroups
    EXPECT(with(shape(C, 33), [](BlendShape& s) { s.pairs = true, s.waves = 16; }), BlendWalk::PairSingle, 2, 16, 3u, 2, 1,
           3);
    // refused: pairs off; quadrant units; a gathered frame; any other wave count (asked for, or by the frame's size)
    EXPECT(big, BlendWalk::Px, 2, 16, 4u, 259, 0, 2);
    EXPECT(with(shape(C, 32), [](BlendShape& s) { s.pairs = true, s.waves = 16; }), BlendWalk::Px, 1, 16, 4u, 259, 0, 1);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.kind = FrameKind::Records, s.arrive = true; }), BlendWalk::Px, 2,
           16, 4u, 259 + 4096, 0, 2);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.waves = 12; }), BlendWalk::Px, 2, 12, 4u, 259, 0, 2);
    EXPECT(with(with(big, pairs), [](BlendShape& s) { s.waves = 8; }), BlendWalk::Px, 2, 8, 4u, 259, 0, 2);
    EXPECT(with(shape(C, 191), pairs), BlendWalk::Px, 2, 12, 4u, 259, 0, 2);
    // the pair walk's grid never is 0
    CHECK(gsm::blend_pw_grid(0, 16, C) == 1u);
    CHECK(gsm::blend_pw_grid(1, 16, C) == 1u);
    CHECK(gsm::blend_pw_grid(16, 16, C) == 1u);
    CHECK(gsm::blend_pw_grid(17, 16, C) == 2u);
    CHECK(gsm::blend_pw_grid(1000, 16, C) == 4u);
    CHECK(gsm::blend_px_grid(0, 1, 8, C) == 0u);
}

static void flag_bits() {
    const BlendShape f = shape(4, 6);  // Px, 1, 8, 3 workgroups, kernel 1
#define FLAGS(edit, word) EXPECT(with(f, [](BlendShape& s) { edit; }), BlendWalk::Px, 1, 8, 3u, word, 0, 1)
    // bit 1, colour: pointer and pitch off by 4 and by 8
    FLAGS(s.color = 0x1004, 2 + 256);
    FLAGS(s.color = 0x1008, 2 + 256);
    FLAGS(s.colorPitch = 0x104, 2 + 256);
    FLAGS(s.colorPitch = 0x108, 2 + 256);
    FLAGS(s.colorPitch = 0x110, 1 + 2 + 256);
    // bit 1 and bit 2048, depth: none, 16-byte aligned, then pointer and pitch off by 8 (bit 1 stays) and by 4
    FLAGS(s.depthPitch = 0x44, 1 + 2 + 256);  // (no depth target: its pitch is not read)
    FLAGS(depth16(s), 1 + 2 + 256 + 2048);
    FLAGS((depth16(s), s.depth = 0x2008), 1 + 2 + 256);
    FLAGS((depth16(s), s.depthPitch = 0x48), 1 + 2 + 256);
    FLAGS((depth16(s), s.depth = 0x2004), 2 + 256);
    FLAGS((depth16(s), s.depthPitch = 0x44), 2 + 256);
    // bit 2048 without bit 1
    FLAGS((depth16(s), s.color = 0x1008), 2 + 256 + 2048);
    FLAGS((depth16(s), s.colorPitch = 0x104), 2 + 256 + 2048);
    // the strides of anything but a Views frame of several views are not read
    FLAGS((depth16(s), s.views = 2, s.colorViewStride = 0x1004, s.depthViewStride = 0x804), 1 + 2 + 256 + 2048);
    FLAGS((s.kind = FrameKind::Compose, s.views = 2, s.colorViewStride = 0x1004), 1 + 2 + 256);
#undef FLAGS
#define FLAGS(edit, word)                                                                                          \
    EXPECT(with(f, [](BlendShape& s) { s.kind = FrameKind::Views, s.views = 2, s.colorViewStride = 0x1000, depth16(s), \
                                       s.depthViewStride = 0x800, edit; }),                                            \
           BlendWalk::PxViews, 1, 8, 3u, word, 0, 1)
    FLAGS((void)s, 1 + 2 + 256 + 2048);
    FLAGS(s.colorViewStride = 0x1004, 2 + 256 + 2048);
    FLAGS(s.colorViewStride = 0x1008, 2 + 256 + 2048);
    FLAGS(s.depthViewStride = 0x804, 2 + 256 + 2048);
    FLAGS(s.depthViewStride = 0x808, 1 + 2 + 256 + 2048);  // (bit 2048 does not ask the stride)
    FLAGS((s.depth = 0, s.depthViewStride = 0x804), 1 + 2 + 256);
    FLAGS((s.views = 1, s.colorViewStride = 0x1004, s.depthViewStride = 0x804), 1 + 2 + 256 + 2048);
#undef FLAGS
#define FLAGS(edit, word) EXPECT(with(f, [](BlendShape& s) { edit; }), BlendWalk::Px, 1, 8, 3u, word, 0, 1)
    // the format field, every value (and only its four bits)
    const int byFormat[16] = {259, 275, 291, 307, 323, 339, 355, 371, 387, 403, 419, 435, 451, 467, 483, 499};
    for (int fmt = 0; fmt < 16; ++fmt) {
        BlendShape s = f;
        s.colorFormat = fmt;
        EXPECT(s, BlendWalk::Px, 1, 8, 3u, byFormat[fmt], 0, 1);
    }
    FLAGS(s.colorFormat = 16 + 3, 307);
    // the claim field, cost order, arrive
    FLAGS(s.claim = 0, 1 + 2);
    FLAGS(s.claim = 1, 1 + 2 + 256);
    FLAGS(s.claim = 2, 1 + 2 + 512);
    FLAGS(s.claim = 3, 1 + 2 + 768);
    FLAGS(s.costOrder = true, 1 + 2 + 4 + 256);
    FLAGS((s.kind = FrameKind::Records, s.arrive = true), 1 + 2 + 256 + 4096);
    FLAGS((s.costOrder = true, s.colorFormat = 5, s.claim = 2, s.arrive = true, depth16(s)),
          1 + 2 + 4 + 80 + 512 + 2048 + 4096);
#undef FLAGS
    // bits 8192 and 16384: pointer and pitch off by 4
    EXPECT(with(f, [](BlendShape& s) { pick8(s), s.pick = 0x3004; }), BlendWalk::Pick, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { pick8(s), s.pickPitch = 0x84; }), BlendWalk::Pick, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { occ8(s), s.occluder = 0x4004; }), BlendWalk::Occ, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { occ8(s), s.occluderPitch = 0x84; }), BlendWalk::Occ, 1, 8, 3u, 259, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { pick8(s), occ8(s), s.pick = 0x3004; }), BlendWalk::OccPick, 1, 8, 3u, 259 + 16384,
           0, 1);
    EXPECT(with(f, [](BlendShape& s) { pick8(s), occ8(s), s.occluderPitch = 0x84; }), BlendWalk::OccPick, 1, 8, 3u,
           259 + 8192, 0, 1);
    // the batch kernels' words keep neither bit 1 nor bit 2048 whatever the first view's targets are, and all else
    EXPECT(with(f, [](BlendShape& s) { s.kind = FrameKind::Batch, depth16(s), s.costOrder = true, s.colorFormat = 3; }),
           BlendWalk::PxBatch, 1, 8, 3u, 2 + 4 + 48 + 256, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { s.kind = FrameKind::Batch, s.color = 0x1004; }), BlendWalk::PxBatch, 1, 8, 3u,
           2 + 256, 0, 1);
    EXPECT(with(f, [](BlendShape& s) { s.kind = FrameKind::Batch, s.batchExtras = true, s.sortedVals = true, depth16(s),
                                       s.costOrder = true, s.colorFormat = 3; }),
           BlendWalk::BatchOccPick, 1, 8, 3u, 2 + 4 + 48 + 256, 0, 1);
    // The pair walk's target word asks 4-byte depth alignment where the px walk's bit 1 asks 8: the same targets, wide
    // in one and narrow in the other.
    const BlendShape big = with(shape(4, 192), [](BlendShape& s) { s.pairs = true, depth16(s); });
#define TARGET(edit, word) EXPECT(with(big, [](BlendShape& s) { edit; }), BlendWalk::PairSingle, 2, 16, 4u, 2, word, 3)
    TARGET((void)s, 1);
    TARGET(s.depth = 0x2004, 1);
    TARGET(s.depthPitch = 0x44, 1);
    TARGET(s.depth = 0x2002, 0);
    TARGET(s.depthPitch = 0x42, 0);
    TARGET(s.depth = 0, 1);
    TARGET(s.color = 0x1008, 0);
    TARGET(s.colorPitch = 0x104, 0);
    TARGET((s.views = 2, s.colorViewStride = 0x1004, s.depthViewStride = 0x802), 1);  // (no Views frame)
    TARGET((s.colorFormat = 4, s.depth = 0x2002), 64);
#undef TARGET
    EXPECT(with(big, [](BlendShape& s) { s.pairs = false, s.depth = 0x2004; }), BlendWalk::Px, 2, 16, 4u, 2 + 256, 0, 2);
#define TARGET(edit, word)                                                                                         \
    EXPECT(with(big, [](BlendShape& s) { s.kind = FrameKind::Views, s.views = 2, s.colorViewStride = 0x1000,        \
                                         s.depthViewStride = 0x800, edit; }),                                       \
           BlendWalk::PairViews, 2, 16, 4u, 2, word, 3)
    TARGET((void)s, 1);
    TARGET(s.depthViewStride = 0x804, 1);
    TARGET(s.depthViewStride = 0x802, 0);
    TARGET(s.colorViewStride = 0x1008, 0);
    TARGET((s.views = 1, s.colorViewStride = 0x1008, s.depthViewStride = 0x802), 1);
#undef TARGET
}

// the dispatcher hands the launch the plan's threads and pairs per lane as constants
static void dispatch() {
    const int waves[3] = {8, 12, 16}, threads[3] = {512, 768, 1024};
    for (int i = 0; i < 3; ++i)
        for (int P = 1; P <= 2; ++P) {
            BlendPlan p;
            p.waves = waves[i];
            p.P = P;
            int gotThreads = 0, gotP = 0, calls = 0;
            gsm::dispatch_blend(p, [&](auto NTH, auto PP) {
                gotThreads = decltype(NTH)::value;
                gotP = decltype(PP)::value;
                ++calls;
            });
            CHECK(calls == 1 && gotThreads == threads[i] && gotP == P && p.threads() == threads[i]);
        }
}

int main() {
    shapes_4_cus();
    shapes_256_cus();
    families();
    flag_bits();
    dispatch();
    // the shape rules by themselves (requestKey asks blend_units_per_tile)
    CHECK(gsm::blend_pairs_per_lane(2048, 256) == 1 && gsm::blend_units_per_tile(2048, 256) == 4u);
    CHECK(gsm::blend_pairs_per_lane(2049, 256) == 2 && gsm::blend_units_per_tile(2049, 256) == 2u);
    CHECK(gsm::blend_waves_per_wg(8160 / 2, 256) == 12);   // the 1080p frame: 4080 tiles, 8160 half-tile units
    CHECK(gsm::blend_waves_per_wg(16200, 256) == 16);      // the 4K frame
    if (failures) {
        std::printf("%d of %d checks failed\n", failures, checks);
        return 1;
    }
    std::printf("all checks passed (%d)\n", checks);
    return 0;
}

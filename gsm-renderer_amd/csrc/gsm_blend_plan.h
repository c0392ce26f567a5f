// gsm_blend_plan.h -- which blend kernel a Global frame gets, in what shape and with which flags (host only, plain
// C++17: no HIP; gsm_debug.h for gsm_blend_kernel).  launch_blend (gsm_blend.hip) builds a BlendShape from the frame, asks plan_blend and launches what
// the plan says; tests/host/blend_plan_test.cpp holds the plan to a table written by hand.  DESIGN.md 32.
#pragma once
#include <cstddef>
#include <cstdint>
#include <type_traits>

#include "../../include/gsm_debug.h"
#include "gsm_schedule_key.h"

namespace gsm {

// The `flags` word of the k_blend_px* and k_blend_pw* kernels: the contract between launch_blend and the walks.
constexpr int kBlendWide = 1;         // bit 0: 16-B colour and depth-pair stores are aligned in the targets
constexpr int kBlendAgePrio = 2;      // bit 1: a unit's wave priority rises with the age of its walk
constexpr int kBlendCostSplit = 4;    // bit 2: cost order -- the longest units on one top-priority wave per SIMD
constexpr int kBlendFormatShift = 4;  // bits 4-7: the colour target's gsm_color_format
constexpr int kBlendFormatMask = 15;
constexpr int kBlendClaimShift = 8;   // bits 8-9: when a wave claims its next unit (0 start, 1 end, 2 one batch early)
constexpr int kBlendClaimMask = 3;
constexpr int kBlendDepth16 = 2048;   // bit 11: the depth target and its pitch are 16-byte aligned
constexpr int kBlendArrive = 4096;    // bit 12: a gathered multi-GPU frame -- the L2 write-back and arrival at exit
constexpr int kBlendPick8 = 8192;     // bit 13: 8-byte pick stores are aligned in the pick target
constexpr int kBlendOcc8 = 16384;     // bit 14: 8-byte occluder loads are aligned in the occluder
// what a Batch kernel's word leaves to each view's own line (BatchTarget::vec; BatchExtras::align holds bits 13, 14)
constexpr int kBlendPerView = kBlendWide | kBlendDepth16;
constexpr int kBlendPerViewExtras = kBlendWide | kBlendPick8 | kBlendOcc8;

// The one alignment rule: a pointer, its pitch and (where given) the stride between views are multiples of n, a
// power of two -- every access of n bytes at an n-byte step into any row of any view is then aligned.
constexpr bool blend_aligned(uintptr_t p, size_t pitch, size_t n, size_t stride = 0) {
    return (((size_t)p | pitch | stride) & (n - 1)) == 0;
}
// What that rule grants a frame's targets, for plan_blend and for each view of a batch (gsm_frame_plan.h).  0 stands
// for a target the frame does not have.  The wide stores: 16-B colour, and depth pairs where there is depth.
constexpr bool blend_wide(uintptr_t color, size_t colorPitch, uintptr_t depth, size_t depthPitch, size_t colorStride = 0,
                          size_t depthStride = 0) {
    return blend_aligned(color, colorPitch, 16, colorStride) && (!depth || blend_aligned(depth, depthPitch, 8, depthStride));
}
constexpr int blend_pick8(uintptr_t pick, size_t pitch) { return (pick && blend_aligned(pick, pitch, 8)) ? kBlendPick8 : 0; }
constexpr int blend_occ8(uintptr_t occluder, size_t pitch) {
    return (occluder && blend_aligned(occluder, pitch, 8)) ? kBlendOcc8 : 0;
}

// quadrant units (P = 1) up to this many tiles per CU, half tiles beyond
constexpr uint32_t kBlendP1TilesPerCu = 8;

inline int blend_pairs_per_lane(uint32_t numTiles, int numCUs) {
    // Half tiles (2 pairs per lane) while the tiles outnumber the 8-wave slots; a smaller frame
    // or a slab of a multi-GPU frame has fewer units than slots, its blend time is its longest
    // unit's walk, and quadrant units (1 pair per lane, ~38 instead of ~61 VALU per entry)
    // shorten that (measured on 1/2, 1/4, 1/8 of the 1080p rows: 149/130/118 -> 138/105/96 us)
    return numTiles <= (uint32_t)numCUs * kBlendP1TilesPerCu ? 1 : 2;
}

inline uint32_t blend_units_per_tile(uint32_t numTiles, int numCUs) {
    return 4u / (uint32_t)blend_pairs_per_lane(numTiles, numCUs);
}

inline int blend_waves_per_wg(uint32_t numTiles, int numCUs) {
    // 16 waves per CU hide more latency once every wave slot gets >= 6 units (4K: 16200 tiles);
    // with fewer units per slot the tail weighs more: 12 waves from 2 units per slot (1080p: 8160
    // units, 3213 -> 3268 frames/s; two 1440x1600 views 1046 -> 1086, r02 fused-accumulate blend),
    // 8 below (r03, late queue claim: DESIGN.md 10)
    const uint64_t units = (uint64_t)numTiles * blend_units_per_tile(numTiles, numCUs);
    if (units >= 6ull * (uint64_t)numCUs * 16u) return 16;
    return units >= 2ull * (uint64_t)numCUs * 12u ? 12 : 8;
}

// the k_blend_px* grid: one workgroup per `waves` units, at most one per CU
inline uint32_t blend_px_grid(uint32_t numTiles, int P, int waves, int numCUs) {
    const uint32_t units = numTiles * (4u / (uint32_t)P), grid = (units + (uint32_t)waves - 1) / (uint32_t)waves;
    return grid > (uint32_t)numCUs ? (uint32_t)numCUs : grid;
}
// the k_blend_pw* grid: half-tile units, at most two per wave in the first round; clamped to [1, numCUs]
inline uint32_t blend_pw_grid(uint32_t numTiles, int waves, int numCUs) {
    const uint32_t units = numTiles * 2u, grid = (units + (uint32_t)(2 * waves) - 1u) / (uint32_t)(2 * waves);
    return grid > (uint32_t)numCUs ? (uint32_t)numCUs : grid == 0 ? 1u : grid;
}

// The nine kernel families, and a frame that launches nothing.
enum class BlendWalk : uint32_t {
    None,
    BatchOccPick,  // k_blend_px_batch_occ_pick: a Batch with per-view options
    OccPick,       // k_blend_px_occ_pick
    Pick,          // k_blend_px_pick
    Occ,           // k_blend_px_occ
    PairSingle, PairViews, PairBatch,  // k_blend_pw, _views, _batch: two half-tile units per wave
    Px, PxViews, PxBatch,              // k_blend_px (Single, Records, Compose), _views, _batch
};

// What the choice reads.  Addresses only: nothing is dereferenced.  0 stands for a target the frame does not have
// (the host refuses a pick or an occluder without pixels before any frame is enqueued).
struct BlendShape {
    FrameKind kind = FrameKind::Single;
    uint32_t numTiles = 0, views = 0;  // frame_tiles() (a batch's sum); a Views frame's view count
    uintptr_t color = 0, depth = 0, pick = 0, occluder = 0;
    size_t colorPitch = 0, depthPitch = 0, pickPitch = 0, occluderPitch = 0;
    size_t colorViewStride = 0, depthViewStride = 0;
    bool sortedVals = false;   // the frame kept its sorted values (the occluded walks read them)
    bool batchExtras = false;  // a Batch with per-view options
    bool costOrder = false, pairs = false;
    bool arrive = false;  // a gathered multi-GPU frame
    int colorFormat = 0, claim = 1;
    int waves = 0;  // 8, 12 or 16 (Tuning::blendWaves admits no other), or 0: by frame size
    int numCUs = 0;
};

struct BlendPlan {
    BlendWalk walk = BlendWalk::None;
    int P = 0;      // pixel pairs per lane: 1 quadrant units, 2 half tiles
    int waves = 0;  // per workgroup; the launch has 64 * waves threads
    uint32_t grid = 0;
    int flags = 0;  // the kernel's `flags` argument
    // the pair walk only: its target's word (PwTarget::flags, k_blend_pw_batch's tgFlags) -- kBlendWide and the format
    int targetFlags = 0;
    int kernel = GSM_BLEND_KERNEL_NONE;  // gsm_blend_kernel: what blend_kernel_kind() reports
    int threads() const { return 64 * waves; }
};

// Measured schedule choices: units longest-first by last frame's walk (costOrder;
// 1080p 8 waves 293 -> 248 us, 4K 16 waves 703 -> 660), the longest on one top-priority wave per
// SIMD (kBlendCostSplit), later units' priority rising with the age of their walk (kBlendAgePrio).
inline BlendPlan plan_blend(const BlendShape& s) {
    const BlendPlan nothing;
    if (s.numTiles == 0) return nothing;
    // (a Views frame's later views start view strides after the first: the wide stores need those aligned too)
    const bool strides = s.kind == FrameKind::Views && s.views > 1;
    const size_t colorStride = strides ? s.colorViewStride : 0, depthStride = strides ? s.depthViewStride : 0;
    const bool color16 = blend_aligned(s.color, s.colorPitch, 16, colorStride);
    const bool wide = blend_wide(s.color, s.colorPitch, s.depth, s.depthPitch, colorStride, depthStride);
    const int shared = kBlendAgePrio | (s.costOrder ? kBlendCostSplit : 0);
    const int format = (s.colorFormat & kBlendFormatMask) << kBlendFormatShift;
    const int flags = (wide ? kBlendWide : 0) | shared | format | ((s.claim & kBlendClaimMask) << kBlendClaimShift) |
                      (s.arrive ? kBlendArrive : 0) |
                      ((s.depth && blend_aligned(s.depth, s.depthPitch, 16)) ? kBlendDepth16 : 0);
    const int pick8 = blend_pick8(s.pick, s.pickPitch), occ8 = blend_occ8(s.occluder, s.occluderPitch);
    BlendPlan p;
    p.P = blend_pairs_per_lane(s.numTiles, s.numCUs);
    p.waves = s.waves ? s.waves : blend_waves_per_wg(s.numTiles, s.numCUs);
    p.grid = blend_px_grid(s.numTiles, p.P, p.waves, s.numCUs);
    p.kernel = p.P == 1 ? GSM_BLEND_KERNEL_QUADRANT : GSM_BLEND_KERNEL_HALF_TILE;
    const auto take = [&p](BlendWalk walk, int word) { return p.walk = walk, p.flags = word, p; };
    // The ladder, in this order.  (The walks over the sorted values launch nothing without them: the host keeps them
    // for every such frame.)
    // 1. A batch in which some view has a pick target or an occluder: one union kernel, every option
    // looked up per view.  The alignment bits 13 and 14 are per view (BatchExtras::align), as bits 0 and 11 are.
    if (s.kind == FrameKind::Batch && s.batchExtras)
        return s.sortedVals ? take(BlendWalk::BatchOccPick, flags & ~kBlendPerView) : nothing;
    // 2. A pick target and an occluder: the units and rules of both, the alignment flags of both.
    if (s.pick && s.occluder) return s.sortedVals ? take(BlendWalk::OccPick, flags | pick8 | occ8) : nothing;
    // 3. A pick frame: quadrant or half-tile units by the rule above, no compaction, no pair walk.
    if (s.pick) return take(BlendWalk::Pick, flags | pick8);
    // 4. An occluded frame: the same, over the tiles' whole sorted runs.
    if (s.occluder) return s.sortedVals ? take(BlendWalk::Occ, flags | occ8) : nothing;
    // 5. One GPU's half-tile frame with >= 6 units per wave slot (16 waves per CU: the 4K frame): two units
    // per wave (r05, k_blend_pw).  The pairs cut the VALU work (-10 %) but halve the waves walking: a gain
    // where the walk is VALU-bound (config 3: blend 370 -> 327 us), a loss where it is bound by its
    // longest units and latency (config 2: 121 -> 129-147 us at every split tried).
    if (s.pairs && p.P == 2 && !s.arrive && p.waves == 16) {
        // The pair walk's own kBlendWide asks 4-byte depth alignment (its depth pair is one 4-byte store) where the px
        // walks ask 8: a frame may store wide in one walk and narrow in the other.  The two are not unified.
        const bool pwWide = color16 && (!s.depth || blend_aligned(s.depth, s.depthPitch, 4, depthStride));
        p.grid = blend_pw_grid(s.numTiles, p.waves, s.numCUs);
        // (a batch's store width is each view's own: BatchTarget::vec)
        p.targetFlags = (pwWide && s.kind != FrameKind::Batch ? kBlendWide : 0) | format;
        p.kernel = GSM_BLEND_KERNEL_PAIR_WALK;
        return take(s.kind == FrameKind::Batch   ? BlendWalk::PairBatch
                    : s.kind == FrameKind::Views ? BlendWalk::PairViews
                                                 : BlendWalk::PairSingle,
                    shared);
    }
    // 6. The plain walk by kind; half tiles compact to one pair per lane once <= 16 of their 32 groups are alive.
    // A Batch's store widths are per view (BatchTarget): its flags keep what the batch shares.
    if (s.kind == FrameKind::Batch) return take(BlendWalk::PxBatch, flags & ~kBlendPerView);
    return take(s.kind == FrameKind::Views ? BlendWalk::PxViews : BlendWalk::Px, flags);
}

// plan -> f(std::integral_constant<int, threads>, std::integral_constant<int, P>) for every blend launch of both
// translation units: 16 or 12 waves of 64 lanes, 8 for anything else; quadrant units or half tiles
template <class F>
void dispatch_blend(const BlendPlan& p, F&& f) {
    auto by_waves = [&](auto pp) {
        if (p.waves == 16) f(std::integral_constant<int, 1024>{}, pp);
        else if (p.waves == 12) f(std::integral_constant<int, 768>{}, pp);
        else f(std::integral_constant<int, 512>{}, pp);
    };
    if (p.P == 1) by_waves(std::integral_constant<int, 1>{});
    else by_waves(std::integral_constant<int, 2>{});
}

}  // namespace gsm

// gsm_blend.hip -- the GlobalRenderer's blend stage on gfx950: clear + front-to-back
// alpha blending of every tile's depth-sorted list (globalRender, GlobalShaders.metal:1030-1187;
// clear: :140-154), plus the load-balancing schedule of its work units.
//
// Persistent workgroups: one workgroup per CU holds the 128 KiB fp16 exp table in LDS and its
// waves pull work units (parts of tiles) from a device counter.  Bit-exact with the oracle: the
// per-thread saturation break of the reference (one 4x2 pixel group) is evaluated per group on
// every list entry.  Numeric contract: DESIGN.md.
#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include "../../include/gsm_renderer.h"
#include "gsm_blend_common.h"
#include "gsm_blend_exact.h"
#include "gsm_blend_plan.h"
#include "gsm_internal.h"

namespace gsm {

// entries between the walks' exit / compaction checkpoints (a multiple of 4: the compacted walk's groups;
// 4 and 8 measured no faster)
constexpr uint32_t kBlendExit = 16;
// waves per workgroup that take the schedule's longest units first, at the top priority (waves map
// to SIMDs round-robin: 4 = one per SIMD; 0 and 8 measured slower)
constexpr uint32_t kBlendTopWaves = 4;

// exp table lookup for a packed pair of quadratic forms: the table is indexed by the fp16 bits
// of p and holds fp16(exp(fp16(-0.5 * p))), correctly rounded (gsm_detmath.h)
__device__ __forceinline__ h2 lookup2(const uint16_t* tbl, h2 p) {
    const uint32_t pb = tbl_bits(p);
    const uint32_t lo = tbl[pb & 0xFFFFu];
    const uint32_t hi = tbl[pb >> 16];
    return as_h2(lo | (hi << 16));
}

// max over the 4 lanes of a quad: DPP quad_perm [1,0,3,2] then [2,3,0,1]
__device__ __forceinline__ uint32_t quad_max_u32(uint32_t v) {
    const uint32_t a = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, false);
    v = v > a ? v : a;
    const uint32_t b = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, false);
    return v > b ? v : b;
}

// ---------------------------------------------------------------------------
// k_blend_px: one wave per blend unit, P pixel pairs per lane.
//   P = 1: 16x8 quadrant of a tile (4 units per tile), a 4x2 group spans 4 lanes
//   P = 2: 16x16 half tile (2 units per tile), a group spans 2 lanes (rows)
// More pairs per lane give every list entry's uniform work (5 readlanes, the dy terms of
// the quadratic form) to more pixels and P independent T chains per lane; fewer give
// shorter walks (a unit walks until its slowest group breaks).  The list is walked in
// groups of U = 4/P entries through a three-stage software pipeline (stage 1: next group's
// p and table reads; stage 2: blend this group; stage 3: next group's alphas).
// ---------------------------------------------------------------------------
// The records of the walk's current 64-entry batch are staged in LDS and read back with uniform
// addresses (one ds_read_b128 + one ds_read_b32 broadcast per entry) instead of 5 v_readlane;
// 2-entry pipeline groups at P = 2 (4-entry groups measured no gain).
// the pick walk (k_blend_px_pick): `item` becomes a pixel's pick where its weight w exceeds the heaviest so far.
// Two fp16 compares: the earliest entry wins ties, a weight of zero or NaN never wins.
__device__ __forceinline__ void pick_update(h2& best, uint32_t (&pk)[2], h2 w, uint32_t item) {
    if (w.x > best.x) {
        best.x = w.x;
        pk[0] = item;
    }
    if (w.y > best.y) {
        best.y = w.y;
        pk[1] = item;
    }
}

// the occluded walk (k_blend_px_occ).  A pixel is closed from the first entry on whose fp16 depth
// lies behind its limit Z: H(Z) < H(dep).  The depths the projection keeps are positive (clip.w > near_plane > 0),
// so their fp16 bits order like their values, and the comparison becomes one on 16-bit integers: the pair's limits
// are held as keys k with "open at dep" == bits(dep) < k --
//   Z NaN: 0x7FFF (open at every depth);  Z >= +0 (inf included): bits(Z) + 1;  Z = -0: 1;  Z < 0: 0 (never open).
// (A record of inf or NaN depth sends the unit to the exact rewalk, which compares in fp16: gsm_blend_exact.h.)
__device__ __forceinline__ uint32_t occ_limit_key(uint32_t b) {
    const uint32_t m = b & 0x7FFFu;
    if (m > 0x7C00u) return 0x7FFFu;
    if (b & 0x8000u) return m == 0u ? 1u : 0u;
    return m + 1u;
}
__device__ __forceinline__ uint32_t occ_limit_keys(uint32_t z2) {
    return occ_limit_key(z2 & 0xFFFFu) | (occ_limit_key(z2 >> 16) << 16);
}
// 0xFFFF in the half of every pixel of the pair that is open at the depth of the staged record word `bd`
// (depth in its high half): v_pk_sub_i16 with the depth in both halves, v_pk_ashrrev_i16 by 15.  Both operands
// lie in [0, 0x7FFF]: the difference cannot wrap.
typedef short i16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t occ_open_mask(uint32_t bd, uint32_t keys) {
    const i16x2 d = __builtin_bit_cast(i16x2, bd);
    const i16x2 m = (i16x2{d.y, d.y} - __builtin_bit_cast(i16x2, keys)) >> i16x2{15, 15};
    return __builtin_bit_cast(uint32_t, m);
}

#define GSM_BLEND_OCCLUDE 0
#define GSM_BLEND_PICK 0
#define GSM_BLEND_VIEWS 0
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#undef GSM_BLEND_PICK
#define GSM_BLEND_PICK 1
#define GSM_BLEND_VIEWS 0
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#undef GSM_BLEND_PICK
#define GSM_BLEND_PICK 0
#define GSM_BLEND_VIEWS 1
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#define GSM_BLEND_VIEWS 2
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#undef GSM_BLEND_OCCLUDE
#define GSM_BLEND_OCCLUDE 1
#define GSM_BLEND_VIEWS 0
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#undef GSM_BLEND_PICK
#define GSM_BLEND_PICK 1
#define GSM_BLEND_VIEWS 0
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
// a batch of views with per-view options (gsm_global_render_frames): k_blend_px_batch_occ_pick
#define GSM_BLEND_VIEWS 2
#include "gsm_blend_px_body.h"
#undef GSM_BLEND_VIEWS
#undef GSM_BLEND_OCCLUDE
#undef GSM_BLEND_PICK

// The frame as the plan reads it (gsm_blend_plan.h), the plan, then one launch: every choice is plan_blend's.
int launch_blend(const FrameGeometry& g, const DeviceArena& A, const FrameTargets& t, const BlendOptions& o,
                 hipStream_t s) {
    // local tile ids: tile t = k * tilesX + tx of the renderer's row k (pixel row rowBegin + k * rowStride)
    // (a batch of views: views * tilesPerView tiles, every rule of the plan takes the batch's count)
    const uint32_t numTiles = frame_tiles(g);
    uint8_t *const color = (uint8_t*)t.color, *const depth = (uint8_t*)t.depth;
    const size_t colorPitch = t.colorPitch, depthPitch = t.depthPitch;
    uint8_t* const pick = o.pick ? (uint8_t*)o.pick->pixels : nullptr;
    const uint8_t* const occluder = o.occluder ? (const uint8_t*)o.occluder->pixels : nullptr;
    const size_t pickPitch = o.pick ? o.pick->pitch : 0, occluderPitch = o.occluder ? o.occluder->pitch : 0;
    BlendShape sh;
    sh.kind = g.kind, sh.numTiles = numTiles, sh.views = g.views;
    sh.color = (uintptr_t)color, sh.colorPitch = colorPitch, sh.colorViewStride = g.colorViewStride;
    sh.depth = (uintptr_t)depth, sh.depthPitch = depthPitch, sh.depthViewStride = g.depthViewStride;
    sh.pick = (uintptr_t)pick, sh.pickPitch = pickPitch;
    sh.occluder = (uintptr_t)occluder, sh.occluderPitch = occluderPitch;
    sh.sortedVals = o.sortedVals != nullptr, sh.batchExtras = o.batchExtras != nullptr;
    sh.colorFormat = o.colorFormat, sh.costOrder = o.costOrder, sh.claim = o.claim, sh.waves = o.waves;
    sh.pairs = o.pairs, sh.arrive = o.arrive != nullptr, sh.numCUs = o.numCUs;
    const BlendPlan plan = plan_blend(sh);
    if (plan.walk == BlendWalk::None) return plan.kernel;
    if (plan.kernel == GSM_BLEND_KERNEL_PAIR_WALK) {
        launch_blend_pw(g, A, t, plan, s);
        return plan.kernel;
    }
    // A.tileQueue was zeroed by k_scan_blocks earlier in the frame
    // what the kernels of one frame and those of a batch take after the queue; every px kernel's flags come next
    const auto frame = std::make_tuple(numTiles, g.tilesX, g.width, g.height, color, colorPitch, depth, depthPitch);
    const auto batch = std::make_tuple(numTiles, (const BatchViewArgs*)g.batchArgs, g.batchTileView);
    const auto none = std::make_tuple();
    const auto runs = std::make_tuple(o.sortedVals);
    dispatch_blend(plan, [&](auto NTH, auto PP) {
        constexpr int kNth = decltype(NTH)::value, kP = decltype(PP)::value;
        constexpr bool kCmp = kP == 2;  // half tiles compact to one pair per lane (the plain walks only)
        const auto launch = [&](auto kernel, const auto& mid, const auto& last) {
            launch_blend_walk(kernel, plan, kNth, A, g.tileCount, std::tuple_cat(mid, std::make_tuple(plan.flags)),
                              last, s);
        };
        switch (plan.walk) {
            case BlendWalk::BatchOccPick:
                launch(k_blend_px_batch_occ_pick<kNth, kP, false>,
                       std::tuple_cat(batch, std::make_tuple(o.batchExtras)), runs);
                break;
            case BlendWalk::OccPick:
                launch(k_blend_px_occ_pick<kNth, kP, false>,
                       std::tuple_cat(frame, std::make_tuple(pick, pickPitch, occluder, occluderPitch)), runs);
                break;
            case BlendWalk::Pick:
                launch(k_blend_px_pick<kNth, kP, false>, std::tuple_cat(frame, std::make_tuple(pick, pickPitch)), none);
                break;
            case BlendWalk::Occ:
                launch(k_blend_px_occ<kNth, kP, false>,
                       std::tuple_cat(frame, std::make_tuple(occluder, occluderPitch)), runs);
                break;
            case BlendWalk::PxBatch: launch(k_blend_px_batch<kNth, kP, kCmp>, batch, none); break;
            case BlendWalk::PxViews:
                launch(k_blend_px_views<kNth, kP, kCmp>,
                       std::make_tuple(numTiles, g.tilesX, g.tilesPerView, g.width, g.height, color, colorPitch,
                                       g.colorViewStride, depth, depthPitch, g.depthViewStride),
                       none);
                break;
            default: {  // BlendWalk::Px
                MgArrive ar{};
                if (o.arrive) {
                    ar = *o.arrive;
                    ar.total = plan.grid;  // every workgroup arrives once, at its exit
                }
                launch(k_blend_px<kNth, kP, kCmp>, std::tuple_cat(std::make_tuple(0u), frame),
                       std::make_tuple(g.rowBegin, g.rowStride, ar));
            }
        }
    });
    return plan.kernel;
}

}  // namespace gsm

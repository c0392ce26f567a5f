// gsm_blend.hip -- the GlobalRenderer's blend stage on gfx950: clear + front-to-back
// alpha blending of every tile's depth-sorted list (globalRender, GlobalShaders.metal:1030-1187;
// clear: :140-154), plus the load-balancing schedule of its work units.
//
// Persistent workgroups: one workgroup per CU holds the 128 KiB fp16 exp table in LDS and its
// waves pull work units (parts of tiles) from a device counter.  Bit-exact with the oracle: the
// per-thread saturation break of the reference (one 4x2 pixel group) is evaluated per group on
// every list entry.  Numeric contract: DESIGN.md.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

#include "../../include/gsm_debug.h"
#include "../../include/gsm_renderer.h"
#include "gsm_blend_exact.h"
#include "gsm_detmath.h"
#include "gsm_internal.h"
#include "gsm_types.h"

namespace gsm {

// entries between the walks' exit / compaction checkpoints (a multiple of 4: the compacted walk's groups;
// 4 and 8 measured no faster)
constexpr uint32_t kBlendExit = 16;
// waves per workgroup that take the schedule's longest units first, at the top priority (waves map
// to SIMDs round-robin: 4 = one per SIMD; 0 and 8 measured slower)
constexpr uint32_t kBlendTopWaves = 4;
// quadrant units (P = 1) up to this many tiles per CU, half tiles beyond
constexpr uint32_t kBlendP1TilesPerCu = 8;

typedef _Float16 h1;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
// `color += gColor * w` (GlobalShaders.metal:1137-1145, DepthFirstShaders.metal:1783-1786): one
// fused multiply-add, a single rounding per channel (the numeric contract; the oracle's hfma)
__device__ __forceinline__ h2 blend_acc(h2 acc, h2 c, h2 w) { return __builtin_elementwise_fma(c, w, acc); }
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ h2 as_h2(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ float h_bits_to_f(uint16_t b) { return (float)__builtin_bit_cast(h1, b); }
// linear -> sRGB encode of a [0, 1] value (include/gsm_renderer.h), powr of the numeric contract
__device__ __forceinline__ float srgb_encode(float c) {
    return c <= 0.0031308f ? c * 12.92f : 1.055f * det_powrf(c, 1.0f / 2.4f) - 0.055f;
}
__device__ __forceinline__ uint32_t as_u32(h2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ h2 splat_lo(h2 v) { return h2{v.x, v.x}; }
__device__ __forceinline__ h2 splat_hi(h2 v) { return h2{v.y, v.y}; }

// The table index of a packed pair of quadratic forms: its fp16 bits.  (The far-field clamp and the
// dead-lane columns that cut the gathers' bank conflicts, and the duplicate-read attribution build, are
// kept as tools/exp/rejected_variants.patch: bit-exact, no faster)
__device__ __forceinline__ uint32_t tbl_bits(h2 p) {
    return as_u32(p);
}

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
// Lanes of one wave hand LDS words to each other: the compiler must not forward a lane's own
// store past them (no instruction; the hardware keeps a wave's LDS operations in order).
__device__ __forceinline__ void blend_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

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


int blend_pairs_per_lane(uint32_t numTiles, int numCUs) {
    // Half tiles (2 pairs per lane) while the tiles outnumber the 8-wave slots; a smaller frame
    // or a slab of a multi-GPU frame has fewer units than slots, its blend time is its longest
    // unit's walk, and quadrant units (1 pair per lane, ~38 instead of ~61 VALU per entry)
    // shorten that (measured on 1/2, 1/4, 1/8 of the 1080p rows: 149/130/118 -> 138/105/96 us)
    return numTiles <= (uint32_t)numCUs * kBlendP1TilesPerCu ? 1 : 2;
}

uint32_t blend_units_per_tile(uint32_t numTiles, int numCUs) {
    return 4u / (uint32_t)blend_pairs_per_lane(numTiles, numCUs);
}

static int blend_waves_per_wg(uint32_t numTiles, int numCUs) {
    // 16 waves per CU hide more latency once every wave slot gets >= 6 units (4K: 16200 tiles);
    // with fewer units per slot the tail weighs more: 12 waves from 2 units per slot (1080p: 8160
    // units, 3213 -> 3268 frames/s; two 1440x1600 views 1046 -> 1086, r02 fused-accumulate blend),
    // 8 below (r03, late queue claim: DESIGN.md 10)
    const uint64_t units = (uint64_t)numTiles * blend_units_per_tile(numTiles, numCUs);
    if (units >= 6ull * (uint64_t)numCUs * 16u) return 16;
    return units >= 2ull * (uint64_t)numCUs * 12u ? 12 : 8;
}



// (waves, P) -> f(std::integral_constant<int, NTH>, std::integral_constant<int, PP>, grid) for every k_blend_px*
// launch: 16 or 12 waves of 64 lanes, 8 for anything else; one workgroup per `waves` units, at most one per CU
template <class F>
static void dispatch_blend(int waves, int P, uint32_t numTiles, int numCUs, F&& f) {
    const uint32_t units = numTiles * (4u / (uint32_t)P);
    uint32_t grid = (units + (uint32_t)waves - 1) / (uint32_t)waves;
    if (grid > (uint32_t)numCUs) grid = (uint32_t)numCUs;
    auto by_waves = [&](auto pp) {
        if (waves == 16) f(std::integral_constant<int, 1024>{}, pp, grid);
        else if (waves == 12) f(std::integral_constant<int, 768>{}, pp, grid);
        else f(std::integral_constant<int, 512>{}, pp, grid);
    };
    if (P == 1) by_waves(std::integral_constant<int, 1>{});
    else by_waves(std::integral_constant<int, 2>{});
}

// Measured schedule choices: units longest-first by last frame's walk (costOrder;
// 1080p 8 waves 293 -> 248 us, 4K 16 waves 703 -> 660), the longest on one top-priority wave per
// SIMD (flags bit 2), later units' priority rising with the age of their walk (flags bit 1).
int launch_blend(const FrameGeometry& g, const DeviceArena& A, const FrameTargets& t, const BlendOptions& o,
                 hipStream_t s) {
    // local tile ids: tile t = k * tilesX + tx of the renderer's row k (pixel row rowBegin + k * rowStride)
    // (a batch of views: views * tilesPerView tiles, every rule below takes the batch's count)
    const uint32_t numTiles = frame_tiles(g);
    if (numTiles == 0) return 0;
    uint8_t* const color = (uint8_t*)t.color;
    uint8_t* const depth = (uint8_t*)t.depth;
    const size_t colorPitch = t.colorPitch, depthPitch = t.depthPitch;
    const int numCUs = o.numCUs;
    // (a Views frame's later views start view strides after the first: the wide stores need those aligned too)
    const bool strides = g.kind == FrameKind::Views && g.views > 1;
    const int vec = ((((uintptr_t)color) & 15u) == 0 && (colorPitch & 15u) == 0 &&
                     (!strides || (g.colorViewStride & 15u) == 0) &&
                     (depth == nullptr || ((((uintptr_t)depth) & 7u) == 0 && (depthPitch & 7u) == 0 &&
                                           (!strides || (g.depthViewStride & 7u) == 0))))
                        ? 1
                        : 0;
    const int flags = vec | 2 | (o.costOrder ? 4 : 0) | ((o.colorFormat & 15) << 4) | ((o.claim & 3) << 8) |
                      (o.arrive ? 4096 : 0) |  // (a gathered multi-GPU frame: the L2 write-back at exit)
                      ((depth && (((uintptr_t)depth) & 15u) == 0 && (depthPitch & 15u) == 0) ? 2048 : 0);
    // A.tileQueue was zeroed by k_scan_blocks earlier in the frame
    const int P = blend_pairs_per_lane(numTiles, numCUs);
    const int waves = o.waves ? o.waves : blend_waves_per_wg(numTiles, numCUs);
    const uint32_t* order = o.costOrder ? A.unitOrder : nullptr;
    const int kernel = P == 1 ? GSM_BLEND_KERNEL_QUADRANT : GSM_BLEND_KERNEL_HALF_TILE;
    // One GPU's half-tile frame with >= 6 units per wave slot (16 waves per CU: the 4K frame): two units
    // per wave (r05, k_blend_pw).  The pairs cut the VALU work (-10 %) but halve the waves walking: a gain
    // where the walk is VALU-bound (config 3: blend 370 -> 327 us), a loss where it is bound by its
    // longest units and latency (config 2: 121 -> 129-147 us at every split tried).
    // A pick frame: the single frame's walk that also writes the pick target -- quadrant or
    // half-tile units by the rule above, no compaction, no pair walk.  (Whole frames of one GPU only: the host
    // refuses tile rows, no gathered frame has a pick entry, and a batch with options takes the kernel below.)
    // A frame with a pick target and an occluder (gsm_global_render_frame): the occluded walk over the
    // whole sorted runs that also tracks the pick -- the units and rules of both, the alignment flags of both.
    // A batch in which some view has a pick target or an occluder (gsm_global_render_frames): one
    // union kernel, the occluded pick walk with every option looked up per view.  A view without an occluder
    // walks with a limit of +inf and a view without a pick target stores none, so each view's bytes are those of
    // its own entry; a pick-only batch pays the walk over the whole sorted runs for six instances instead of
    // eighteen.  The alignment bits 13 and 14 are per view (BatchExtras::align), as bits 0 and 11 are.
    if (g.kind == FrameKind::Batch && o.batchExtras) {
        if (!o.sortedVals) return 0;  // (the host keeps them for every such batch)
        dispatch_blend(waves, P, numTiles, numCUs, [&](auto NTH, auto PP, uint32_t grid) {
            hipLaunchKernelGGL((k_blend_px_batch_occ_pick<decltype(NTH)::value, decltype(PP)::value, false>),
                               dim3(grid), dim3(decltype(NTH)::value), 0, s, A.tileStart, A.rec, A.expTable,
                               A.tileQueue, numTiles, (const BatchViewArgs*)g.batchArgs, g.batchTileView,
                               o.batchExtras, flags & ~(1 | 2048), order, A.unitCost, A.blendTrace, A.halfVals[0],
                               A.halfVals[1], A.halfCount, g.tileCount, A.costMax, o.sortedVals);
        });
        return kernel;
    }
    if (o.pick && o.occluder) {
        if (!o.sortedVals) return 0;  // (the host passes them with every occluder)
        uint8_t* const pick = (uint8_t*)o.pick->pixels;
        const size_t pickPitch = o.pick->pitch;
        const uint8_t* const occluder = (const uint8_t*)o.occluder->pixels;
        const size_t occluderPitch = o.occluder->pitch;
        const int pflags = flags | (((((uintptr_t)pick) & 7u) == 0 && (pickPitch & 7u) == 0) ? 8192 : 0) |
                           (((((uintptr_t)occluder) & 7u) == 0 && (occluderPitch & 7u) == 0) ? 16384 : 0);
        dispatch_blend(waves, P, numTiles, numCUs, [&](auto NTH, auto PP, uint32_t grid) {
            hipLaunchKernelGGL((k_blend_px_occ_pick<decltype(NTH)::value, decltype(PP)::value, false>), dim3(grid),
                               dim3(decltype(NTH)::value), 0, s, A.tileStart, A.rec, A.expTable, A.tileQueue, numTiles,
                               g.tilesX, g.width, g.height, color, colorPitch, depth, depthPitch, pick, pickPitch,
                               occluder, occluderPitch, pflags, order, A.unitCost, A.blendTrace, A.halfVals[0],
                               A.halfVals[1], A.halfCount, g.tileCount, A.costMax, o.sortedVals);
        });
        return kernel;
    }
    if (o.pick) {
        uint8_t* const pick = (uint8_t*)o.pick->pixels;
        const size_t pickPitch = o.pick->pitch;
        const int pflags = flags | (((((uintptr_t)pick) & 7u) == 0 && (pickPitch & 7u) == 0) ? 8192 : 0);
        dispatch_blend(waves, P, numTiles, numCUs, [&](auto NTH, auto PP, uint32_t grid) {
            hipLaunchKernelGGL((k_blend_px_pick<decltype(NTH)::value, decltype(PP)::value, false>), dim3(grid),
                               dim3(decltype(NTH)::value), 0, s, A.tileStart, A.rec, A.expTable, A.tileQueue, numTiles,
                               g.tilesX, g.width, g.height, color, colorPitch, depth, depthPitch, pick, pickPitch,
                               pflags, order, A.unitCost, A.blendTrace, A.halfVals[0], A.halfVals[1], A.halfCount,
                               g.tileCount, A.costMax);
        });
        return kernel;
    }
    // An occluded frame: the same units and the same rules, the walk cut at the occluder -- no
    // compaction, no pair walk; whole frames of one GPU only.  It walks the tiles' whole sorted runs (sortedVals,
    // the values with their skip flags), which the host makes the sort keep for such a frame.
    if (o.occluder) {
        if (!o.sortedVals) return 0;  // (the host passes them with every occluder)
        const uint8_t* const occluder = (const uint8_t*)o.occluder->pixels;
        const size_t occluderPitch = o.occluder->pitch;
        const int oflags = flags | (((((uintptr_t)occluder) & 7u) == 0 && (occluderPitch & 7u) == 0) ? 16384 : 0);
        dispatch_blend(waves, P, numTiles, numCUs, [&](auto NTH, auto PP, uint32_t grid) {
            hipLaunchKernelGGL((k_blend_px_occ<decltype(NTH)::value, decltype(PP)::value, false>), dim3(grid),
                               dim3(decltype(NTH)::value), 0, s, A.tileStart, A.rec, A.expTable, A.tileQueue, numTiles,
                               g.tilesX, g.width, g.height, color, colorPitch, depth, depthPitch, occluder,
                               occluderPitch, oflags, order, A.unitCost, A.blendTrace, A.halfVals[0], A.halfVals[1],
                               A.halfCount, g.tileCount, A.costMax, o.sortedVals);
        });
        return kernel;
    }
    if (o.pairs && P == 2 && !o.arrive && waves == 16) {
        BlendOptions po = o;
        po.waves = waves;
        launch_blend_pw(g, A, t, po, s);
        return GSM_BLEND_KERNEL_PAIR_WALK;
    }
    // half tiles (P == 2: CMP) compact to one pair per lane once <= 16 of their 32 groups are alive
    dispatch_blend(waves, P, numTiles, numCUs, [&](auto NTH, auto PP, uint32_t grid) {
        constexpr int kNth = decltype(NTH)::value, kP = decltype(PP)::value;
        constexpr bool kCmp = kP == 2;
        if (g.kind == FrameKind::Batch) {
            //  the targets, sizes and store widths are per view (BatchTarget); the kernel's flags
            // keep what the batch shares
            hipLaunchKernelGGL((k_blend_px_batch<kNth, kP, kCmp>), dim3(grid), dim3(kNth), 0, s, A.tileStart, A.rec,
                               A.expTable, A.tileQueue, numTiles, (const BatchViewArgs*)g.batchArgs, g.batchTileView,
                               flags & ~(1 | 2048), order, A.unitCost, A.blendTrace, A.halfVals[0], A.halfVals[1],
                               A.halfCount, g.tileCount, A.costMax);
        } else if (g.kind == FrameKind::Views) {
            hipLaunchKernelGGL((k_blend_px_views<kNth, kP, kCmp>), dim3(grid), dim3(kNth), 0, s, A.tileStart, A.rec,
                               A.expTable, A.tileQueue, numTiles, g.tilesX, g.tilesPerView, g.width, g.height, color,
                               colorPitch, g.colorViewStride, depth, depthPitch, g.depthViewStride, flags, order,
                               A.unitCost, A.blendTrace, A.halfVals[0], A.halfVals[1], A.halfCount, g.tileCount,
                               A.costMax);
        } else {
            MgArrive ar{};
            if (o.arrive) {
                ar = *o.arrive;
                ar.total = grid;  // every workgroup arrives once, at its exit
            }
            hipLaunchKernelGGL((k_blend_px<kNth, kP, kCmp>), dim3(grid), dim3(kNth), 0, s, A.tileStart, A.rec,
                               A.expTable, A.tileQueue, 0u, numTiles, g.tilesX, g.width, g.height, color, colorPitch,
                               depth, depthPitch, flags, order, A.unitCost, A.blendTrace, A.halfVals[0],
                               A.halfVals[1], A.halfCount, g.tileCount, A.costMax, g.rowBegin, g.rowStride, ar);
        }
    });
    return kernel;
}

}  // namespace gsm

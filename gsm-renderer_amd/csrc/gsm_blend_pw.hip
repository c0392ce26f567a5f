// gsm_blend_pw.hip -- the GlobalRenderer's blend with two half-tile units per wave (r05).
//
// Same per-pixel operations and order as k_blend_px (globalRender, GlobalShaders.metal:1030-1187; the
// numeric contract), so bit-identical output; what changes is which lanes hold which
// pixels.  A wave takes a PAIR of half-tile units (16x16 pixels, 32 groups of the reference's 4x2
// pixels each) -- consecutive positions of the longest-first schedule, so of similar walk -- and walks
// both half-tile lists in lockstep (entry e of unit 0 on lanes 0-31, entry e of unit 1 on lanes 32-63),
// in three lane layouts that follow the live groups:
//   W8: one group per lane (8 pixels, 4 packed pairs): 64 groups, ~78 VALU per entry -- 9.75 per pixel
//       against 10.65 for 4 pixels per lane; the group break needs no cross-lane step;
//   W4: a group on 2 lanes (4 pixels per lane, k_blend_px's half-tile layout), entered once at most
//       32 groups of the pair live;
//   W2: a group on 4 lanes (2 pixels per lane, k_blend_px's compacted layout), entered at <= 16.
// The tails of the two units (their last live groups) share one wave instead of holding one wave
// each -- the per-unit alive curves put this at -14 % wave-instructions at config 2 and -18 % at
// config 3 (tools/blend_pair_model.py).  The schedule's longest units (the top-priority
// first unit of waves 0-3 of each workgroup) still run alone, in W4 from their first entry, so the
// longest job is no longer than before.
#include <hip/hip_runtime.h>

#include <tuple>
#include <type_traits>

#include "../../include/gsm_renderer.h"
#include "gsm_blend_common.h"
#include "gsm_blend_exact.h"
#include "gsm_blend_plan.h"
#include "gsm_internal.h"

namespace gsm {
namespace {

__device__ __forceinline__ uint32_t pw_bperm(uint32_t srcLane, uint32_t v) {
    return (uint32_t)__builtin_amdgcn_ds_bpermute((int)(srcLane * 4u), (int)v);
}
__device__ __forceinline__ h2 pw_bperm(uint32_t srcLane, h2 v) { return as_h2(pw_bperm(srcLane, as_u32(v))); }

struct PwTarget {
    uint8_t* color;
    size_t colorPitch;
    uint8_t* depth;
    size_t depthPitch;
    uint32_t W, H;
    int flags;  // kBlendWide: 16-B colour / 4-B depth stores allowed; the format field: gsm_color_format
};

// one pixel pair (px, py), (px + 1, py) in the target's format (GlobalShaders.metal:1152-1186;
// conversion rules in include/gsm_renderer.h) -- k_blend_px's write_pair without the multi-GPU paths
__device__ __forceinline__ void pw_write_pair(const PwTarget& t, uint32_t px, uint32_t py, h2 Av, h2 Rq, h2 Gq, h2 Bq,
                                              h2 Dq) {
    if (py >= t.H) return;
    uint8_t* crow = t.color + (size_t)py * t.colorPitch;
    const uint32_t ur = as_u32(Rq), ug = as_u32(Gq), ub = as_u32(Bq), ua = as_u32(Av), ud = as_u32(Dq);
    const int fmt = (t.flags >> kBlendFormatShift) & kBlendFormatMask;
    if (fmt == GSM_COLOR_FORMAT_RGBA16F) {
        const uint32_t p0a = (ur & 0xFFFFu) | (ug << 16);
        const uint32_t p0b = (ub & 0xFFFFu) | (ua << 16);
        const uint32_t p1a = (ur >> 16) | (ug & 0xFFFF0000u);
        const uint32_t p1b = (ub >> 16) | (ua & 0xFFFF0000u);
        if ((t.flags & kBlendWide) && px + 1 < t.W) {
            *(uint4*)(crow + (size_t)px * 8) = make_uint4(p0a, p0b, p1a, p1b);
        } else {
            if (px < t.W) {
                *(uint32_t*)(crow + (size_t)px * 8) = p0a;
                *(uint32_t*)(crow + (size_t)px * 8 + 4) = p0b;
            }
            if (px + 1 < t.W) {
                *(uint32_t*)(crow + (size_t)(px + 1) * 8) = p1a;
                *(uint32_t*)(crow + (size_t)(px + 1) * 8 + 4) = p1b;
            }
        }
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 2; ++i) {
            if (px + i >= t.W) break;
            const uint32_t sh = 16u * i;
            float c[4] = {h_bits_to_f((uint16_t)(ur >> sh)), h_bits_to_f((uint16_t)(ug >> sh)), h_bits_to_f((uint16_t)(ub >> sh)),
                          h_bits_to_f((uint16_t)(ua >> sh))};
            if (fmt == GSM_COLOR_FORMAT_RGBA32F) {
                uint8_t* o = crow + (size_t)(px + i) * 16;
                if (t.flags & kBlendWide) {
                    *(uint4*)o = make_uint4(__float_as_uint(c[0]), __float_as_uint(c[1]), __float_as_uint(c[2]),
                                            __float_as_uint(c[3]));
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k) ((uint32_t*)o)[k] = __float_as_uint(c[k]);
                }
                continue;
            }
            const bool srgb = fmt == GSM_COLOR_FORMAT_RGBA8_UNORM_SRGB || fmt == GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB;
            uint32_t u8[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float x = __builtin_fminf(__builtin_fmaxf(c[k], 0.0f), 1.0f);
                if (srgb && k < 3) x = srgb_encode(x);
                u8[k] = (uint32_t)__builtin_rintf(x * 255.0f);
            }
            const bool bgra = fmt >= GSM_COLOR_FORMAT_BGRA8_UNORM;
            *(uint32_t*)(crow + (size_t)(px + i) * 4) =
                (bgra ? u8[2] : u8[0]) | (u8[1] << 8) | ((bgra ? u8[0] : u8[2]) << 16) | (u8[3] << 24);
        }
    }
    if (t.depth) {
        uint8_t* drow = t.depth + (size_t)py * t.depthPitch;
        if ((t.flags & kBlendWide) && px + 1 < t.W) {
            *(uint32_t*)(drow + (size_t)px * 2) = ud;
        } else {
            if (px < t.W) *(uint16_t*)(drow + (size_t)px * 2) = (uint16_t)(ud & 0xFFFFu);
            if (px + 1 < t.W) *(uint16_t*)(drow + (size_t)(px + 1) * 2) = (uint16_t)(ud >> 16);
        }
    }
}

}  // namespace

#define GSM_BLEND_VIEWS 0
#include "gsm_blend_pw_body.h"
#undef GSM_BLEND_VIEWS
#define GSM_BLEND_VIEWS 1
#include "gsm_blend_pw_body.h"
#undef GSM_BLEND_VIEWS
#define GSM_BLEND_VIEWS 2
#include "gsm_blend_pw_body.h"
#undef GSM_BLEND_VIEWS


// the pair walk plan_blend chose (plan.walk: PairSingle, PairViews or PairBatch) for a frame of half-tile units on
// one GPU (no multi-GPU gather): the grid, the waves and both flag words are the plan's
void launch_blend_pw(const FrameGeometry& g, const DeviceArena& A, const FrameTargets& t, const BlendPlan& plan,
                     hipStream_t s) {
    const uint32_t numTiles = frame_tiles(g);
    const PwTarget tg{(uint8_t*)t.color, t.colorPitch, (uint8_t*)t.depth, t.depthPitch, g.width, g.height,
                      plan.targetFlags};
    dispatch_blend(plan, [&](auto NTH, auto) {
        constexpr int kNth = decltype(NTH)::value;
        const auto launch = [&](auto kernel, const auto& mid, const auto& last) {
            launch_blend_walk(kernel, plan, kNth, A, g.tileCount, mid, last, s);
        };
        switch (plan.walk) {
            case BlendWalk::PairBatch:  // (the targets, sizes and store widths are per view, BatchTarget)
                launch(k_blend_pw_batch<kNth>,
                       std::make_tuple(numTiles, (const BatchViewArgs*)g.batchArgs, g.batchTileView, plan.targetFlags),
                       std::make_tuple(plan.flags));
                break;
            case BlendWalk::PairViews:
                launch(k_blend_pw_views<kNth>,
                       std::make_tuple(numTiles, g.tilesX, g.tilesPerView, tg, g.colorViewStride, g.depthViewStride),
                       std::make_tuple(plan.flags));
                break;
            default:  // BlendWalk::PairSingle
                launch(k_blend_pw<kNth>, std::make_tuple(numTiles, g.tilesX, tg),
                       std::make_tuple(g.rowBegin, g.rowStride, plan.flags));
        }
    });
}

}  // namespace gsm

// gsm_blend_exact.h -- the exact re-walk of one blend unit, shared by k_blend_px and k_blend_pw.
//
// The reference skips a list entry for a 4x2 pixel group when the group's eight alphas are all zero
// (GlobalShaders.metal:1133, `if (all(alphaRow0 == 0.0h) && all(alphaRow1 == 0.0h)) continue;`).  The
// fast walks blend such an entry with alpha 0 instead: T * (1 - 0) = T, and c * (0 * T) = 0 leaves
// every colour channel bit for bit (the colours are u8 / 255, finite) -- and the depth channel too,
// unless the record's fp16 depth is inf or NaN (a view depth past 65504 overflows fp16, and the Global
// path has no far-plane cull): inf * 0 = NaN where the reference keeps the depth.  The fast walks test
// every 64-entry batch they stage for such a record (one ballot per batch); a unit that meets one is
// walked again here, after its fast walk, with the group test, and all of its pixels are written again.
// Same fp16 operations in the same order as the fast walks (quadratic form, table word, alpha, group
// break, fused accumulation); entries at a time, records staged per 64-entry batch in the wave's LDS
// stage.  Slow, but only for units that hold such a record.
#pragma once
#include <hip/hip_runtime.h>

#include "gsm_blend_common.h"
#include "gsm_types.h"

namespace gsm {
namespace blend_exact {

template <int CTRL>
__device__ __forceinline__ uint32_t x_dpp_or(uint32_t v) {
    return v | (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
}
template <int CTRL>
__device__ __forceinline__ uint32_t x_dpp_max(uint32_t v) {
    const uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, false);
    return v > o ? v : o;
}

// a staged batch (one record word b | depth << 16 per lane) holds a record of inf / NaN fp16 depth
__device__ __forceinline__ bool batch_depth_nonfinite(uint32_t recB) {
    return __ballot(((recB >> 16) & 0x7C00u) == 0x7C00u) != 0ull;
}

// One unit at (ux, uy) walked exactly.  P = 2: a 16x16 half tile, lane = 2x2 pixels (k_blend_px's
// half-tile layout: a 4x2 group on lanes 2g, 2g + 1); P = 1: a 16x8 quadrant, lane = one pixel pair
// (a group on a lane quad).  stA / stB: the wave's 64-entry LDS record stage.  write(px, py, A, R, G,
// B, D) stores the pixel pair (px, py), (px + 1, py).
// PICK (k_blend_px_pick): the walk also tracks, per pixel, the item (list value) of the heaviest
// weight w = alpha * T among the entries the group blends -- the earliest on ties, never a zero or a NaN -- and
// write takes the pair's two picks after D.  stI: the wave's 64-entry LDS stage of the items.
// OCC (k_blend_px_occ): limits(px, py) gives the fp16 limits of a pixel pair (packed bits).  A pixel
// is closed from the first entry on whose depth lies behind its limit, H(Z) < H(dep) -- fp16 compares, false for
// a NaN on either side: its alpha is +0 from that entry on, and the group break takes its T as +0.  lst is then the
// tile's whole sorted run (an entry a half list drops can still close a pixel), its values masked by idMask.
template <int P, bool PICK = false, bool OCC = false, typename Write, typename Limits = int>
__device__ __forceinline__ void walk_unit_exact(const uint32_t* __restrict__ lst, uint32_t count, const BlendRecord* __restrict__ rec,
                                const uint16_t* tbl, uint4* stA, uint32_t* stB, uint32_t ux, uint32_t uy,
                                uint32_t thrBits, Write&& write, uint32_t* stI = nullptr, Limits limits = 0,
                                uint32_t idMask = 0xFFFFFFFFu) {
    static_assert(P == 1 || P == 2, "quadrant or half-tile units");
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t offX, offY0, offY1;
    if (P == 1) {
        const uint32_t grp = lane >> 2;
        offX = (grp & 3u) * 4u + (lane & 1u) * 2u;
        offY0 = offY1 = (grp >> 2) * 2u + ((lane >> 1) & 1u);
    } else {
        const uint32_t grp = lane >> 1;
        offX = (grp & 3u) * 4u + (lane & 1u) * 2u;
        offY0 = (grp >> 2) * 2u;
        offY1 = offY0 + 1u;
    }
    const h2 ONE = {(h1)1.0f, (h1)1.0f}, ZERO = {(h1)0.0f, (h1)0.0f};
    const h1 c099 = (h1)0.99;
    const h2 C099 = {c099, c099};
    const h2 X = {(h1)(float)(ux + offX), (h1)(float)(ux + offX + 1u)};
    const h2 Yv = {(h1)(float)(uy + offY0), (h1)(float)(uy + offY1)};
    h2 T[P], R[P], G[P], B[P], D[P];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        T[q] = ONE;
        R[q] = G[q] = B[q] = D[q] = ZERO;
    }
    h2 best[P];
    uint32_t pk[P][2];
#pragma unroll
    for (int q = 0; q < P; ++q) {
        best[q] = ZERO;
        pk[q][0] = pk[q][1] = 0xFFFFFFFFu;  // GSM_PICK_NONE
    }
    h2 Z[P];
    uint32_t open[P];  // 0xFFFF in the half of every pixel that is not closed
#pragma unroll
    for (int q = 0; q < P; ++q) {
        Z[q] = ZERO;
        open[q] = 0xFFFFFFFFu;
    }
    if constexpr (OCC) {
        Z[0] = as_h2(limits(ux + offX, uy + offY0));
        if (P == 2) Z[P - 1] = as_h2(limits(ux + offX, uy + offY1));
    }
    bool alive = true;
    const uint32_t last = count - 1u;
    const uint4 pad = make_uint4(as_u32(h2{(h1)(float)ux, (h1)(float)uy}), 0u, 0u, 0u);
    for (uint32_t b0 = 0; b0 < count; b0 += 64u) {
        uint32_t gi = lst[min(b0 + lane, last)];
        if constexpr (OCC) gi &= idMask;
        uint4 a = *(const uint4*)(rec + gi);
        uint32_t b = rec[gi].b;
        if (b0 + lane >= count) {
            a = pad;
            b = 0u;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");  // (earlier reads of the stage are done)
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        stA[lane] = a;
        stB[lane] = b;
        if constexpr (PICK) stI[lane] = gi;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t n = min(64u, count - b0);
        for (uint32_t j = 0; j < n; ++j) {
            // group break before the entry (GlobalShaders.metal:1086-1088): max T of the 4x2 group
            u16x2 tm = __builtin_bit_cast(u16x2, OCC ? (as_u32(T[0]) & open[0]) : as_u32(T[0]));
#pragma unroll
            for (int q = 1; q < P; ++q)
                tm = __builtin_elementwise_max(tm, __builtin_bit_cast(u16x2, OCC ? (as_u32(T[q]) & open[q]) : as_u32(T[q])));
            const uint32_t tb = __builtin_bit_cast(uint32_t, tm);
            uint32_t gm = max(tb & 0xFFFFu, tb >> 16);
            gm = x_dpp_max<0xB1>(gm);
            if (P == 1) gm = x_dpp_max<0x4E>(gm);
            alive = alive && !(gm < thrBits);
            if (__ballot(alive) == 0ull) break;
            const uint4 ra = stA[j];
            const uint32_t bd = stB[j];
            // p = ((dx*dx)*cxx + (dy*dy)*cyy) + (dx*dy)*cxy2 (GlobalShaders.metal:1115-1122)
            const h2 mean = as_h2(ra.x), cc = as_h2(ra.y), oc = as_h2(ra.z);
            const h2 dyv = Yv - splat_hi(mean);
            const h2 dyy = (dyv * dyv) * splat_hi(cc);
            const h2 dx = X - splat_lo(mean);
            h2 pq[P];
            if constexpr (P == 2) {
                const h2 dxx = (dx * dx) * splat_lo(cc);
                pq[0] = (dxx + splat_lo(dyy)) + (dx * splat_lo(dyv)) * splat_lo(oc);
                pq[1] = (dxx + splat_hi(dyy)) + (dx * splat_hi(dyv)) * splat_lo(oc);
            } else {
                pq[0] = ((dx * dx) * splat_lo(cc) + splat_lo(dyy)) + (dx * splat_lo(dyv)) * splat_lo(oc);
            }
            h2 ac[P], om[P];
            uint32_t nz = 0;
#pragma unroll
            for (int q = 0; q < P; ++q) {
                const uint32_t pb = as_u32(pq[q]);
                const h2 ek = as_h2((uint32_t)tbl[pb & 0xFFFFu] | ((uint32_t)tbl[pb >> 16] << 16));
                // a = min(opacity * exp(-0.5h * p), 0.99h) (GlobalShaders.metal:1124-1131)
                ac[q] = __builtin_elementwise_min(splat_hi(oc) * ek, C099);
                if constexpr (OCC) {
                    const h1 dep = as_h2(bd).y;
                    if (Z[q].x < dep) open[q] &= 0xFFFF0000u;
                    if (Z[q].y < dep) open[q] &= 0x0000FFFFu;
                    ac[q] = as_h2(as_u32(ac[q]) & open[q]);
                }
                om[q] = ONE - ac[q];
                nz |= as_u32(ac[q]) & 0x7FFF7FFFu;
            }
            nz = x_dpp_or<0xB1>(nz);
            if (P == 1) nz = x_dpp_or<0x4E>(nz);
            if (alive && nz != 0u) {  // the group's alphas are not all zero (GlobalShaders.metal:1133)
                const h2 rgv = as_h2(ra.w), bdv = as_h2(bd);
#pragma unroll
                for (int q = 0; q < P; ++q) {
                    const h2 w = ac[q] * T[q];  // (GlobalShaders.metal:1137-1149)
                    if constexpr (PICK) {
                        const uint32_t item = stI[j];
                        if (w.x > best[q].x) {
                            best[q].x = w.x;
                            pk[q][0] = item;
                        }
                        if (w.y > best[q].y) {
                            best[q].y = w.y;
                            pk[q][1] = item;
                        }
                    }
                    T[q] = T[q] * om[q];
                    R[q] = __builtin_elementwise_fma(splat_lo(rgv), w, R[q]);
                    G[q] = __builtin_elementwise_fma(splat_hi(rgv), w, G[q]);
                    B[q] = __builtin_elementwise_fma(splat_lo(bdv), w, B[q]);
                    D[q] = __builtin_elementwise_fma(splat_hi(bdv), w, D[q]);
                }
            }
        }
        if (__ballot(alive) == 0ull) break;
    }
    if constexpr (PICK) {
        write(ux + offX, uy + offY0, ONE - T[0], R[0], G[0], B[0], D[0], pk[0][0], pk[0][1]);
        if (P == 2)
            write(ux + offX, uy + offY1, ONE - T[P - 1], R[P - 1], G[P - 1], B[P - 1], D[P - 1], pk[P - 1][0],
                  pk[P - 1][1]);
    } else {
        write(ux + offX, uy + offY0, ONE - T[0], R[0], G[0], B[0], D[0]);
        if (P == 2) write(ux + offX, uy + offY1, ONE - T[P - 1], R[P - 1], G[P - 1], B[P - 1], D[P - 1]);
    }
}

}  // namespace blend_exact
}  // namespace gsm

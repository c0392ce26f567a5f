// gsm_local_kernels.hip -- gfx950 kernels of the LocalRenderer frame (include/gsm_local.h).
//
// Reference: Sources/Renderer/LocalRenderer/LocalShaders.metal, cited per kernel, and the shared
// helpers of Sources/Renderer/Shared/GaussianShared.h (gsm_device.h).  DESIGN.md 13:
//   k_local_clear -> k_local_project -> scan -> k_local_compact -> k_local_scatter -> k_local_sort
//   -> k_local_blend.
// There is no global sort: every 16x16 tile owns 2048 slots, filled with atomics, and is sorted on its
// own in LDS.  Numeric contract as everywhere: no contraction, IEEE division and square
// root, the contract's log2 and exp table, minNum / maxNum, one declared FMA per colour channel.
#include <hip/hip_runtime.h>

#include "gsm_device.h"
#include "gsm_local_internal.h"

namespace gsm {

// ---------------------------------------------------------------------------
// 0. localClear (LocalShaders.metal:10-25): tile counters and the frame's counters
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kLocalBlock) void k_local_clear(uint32_t* __restrict__ tileCounts, uint32_t tileCount,
                                                             LocalStats* __restrict__ stats) {
    const uint32_t i = blockIdx.x * kLocalBlock + threadIdx.x;
    if (i < tileCount) tileCounts[i] = 0u;
    if (i == 0) {
        stats->activeTiles = 0u;
        stats->totalEntries = 0u;
        stats->maxTileCount = 0u;
        stats->pad = 0u;
    }
}

// ---------------------------------------------------------------------------
// 1. localProjectStore (LocalShaders.metal:53-184) + per-block visible counts.
// The culls in the reference's order: scale, clip w against the near plane, the far plane, opacity,
// radius of computeConicAndRadius, total ink on the stabilised covariance, tile rect of the 3 sigma OBB
// extents.  A culled record has maxTile = 0 (:65-76); a visible one has maxTile >= 1 (exclusive).
// ---------------------------------------------------------------------------
template <bool HALF, int DEG>
__global__ __launch_bounds__(kLocalBlock) void k_local_project(const void* __restrict__ world,
                                                               const void* __restrict__ harm, LocalArgs P,
                                                               LocalProjected* __restrict__ temp,
                                                               uint32_t* __restrict__ blockSums) {
    __shared__ uint32_t lds[kLocalBlock / 64];
    const uint32_t gid = blockIdx.x * kLocalBlock + threadIdx.x;
    bool ok = gid < P.count;
    LocalProjected rec;
    rec.a = make_uint4(0u, 0u, 0u, 0u);
    rec.b = make_uint4(0u, 0u, 0u, 0u);
    if (ok) {
        float pos[3], scale[3], rot[4], opacity;
        if constexpr (HALF) {
            const uint4* wq = (const uint4*)((const PackedWorldGaussianHalf*)world + gid);
            const uint4 w0 = wq[0], w1 = wq[1];
            pos[0] = __builtin_bit_cast(float, w0.x);
            pos[1] = __builtin_bit_cast(float, w0.y);
            pos[2] = __builtin_bit_cast(float, w0.z);
            opacity = hbits_to_f((uint16_t)(w0.w & 0xFFFFu));
            scale[0] = hbits_to_f((uint16_t)(w0.w >> 16));
            scale[1] = hbits_to_f((uint16_t)(w1.x & 0xFFFFu));
            scale[2] = hbits_to_f((uint16_t)(w1.x >> 16));
            rot[0] = hbits_to_f((uint16_t)(w1.y & 0xFFFFu));
            rot[1] = hbits_to_f((uint16_t)(w1.y >> 16));
            rot[2] = hbits_to_f((uint16_t)(w1.z & 0xFFFFu));
            rot[3] = hbits_to_f((uint16_t)(w1.z >> 16));
        } else {
            const float4* wq = (const float4*)((const PackedWorldGaussian*)world + gid);
            const float4 w0 = wq[0], w1 = wq[1], w2 = wq[2];
            pos[0] = w0.x; pos[1] = w0.y; pos[2] = w0.z; opacity = w0.w;
            scale[0] = w1.x; scale[1] = w1.y; scale[2] = w1.z;
            rot[0] = w2.x; rot[1] = w2.y; rot[2] = w2.z; rot[3] = w2.w;
        }
        // cullByScale (GaussianShared.h:719-722)
        if (__builtin_fmaxf(scale[0], __builtin_fmaxf(scale[1], scale[2])) < 0.0005f) ok = false;
        float vp[4], clip[4];
        float depth = 0.0f;
        if (ok) {
            const float p4[4] = {pos[0], pos[1], pos[2], 1.0f};
            m4_mul_v(P.view, p4, vp);
            m4_mul_v(P.proj, vp, clip);
            depth = clip[3];
            if (!(clip[3] > P.nearPlane)) ok = false;  // isInFrontOfCameraClipW
            if (depth > P.farPlane) ok = false;        // cullByFarPlane (GaussianShared.h:732-734)
        }
        if (ok && opacity < 0.005f) ok = false;  // params.alphaThreshold (LocalRenderer.swift:165)
        float sx = 0.0f, sy = 0.0f;
        Cov2 cov = {1.0f, 0.0f, 0.0f, 1.0f};
        float conic[3] = {0.0f, 0.0f, 0.0f};
        if (ok) {
            float ndc[2] = {clip[0], clip[1]};
            div_many(ndc, clip[3]);  // clip / w, each correctly rounded (w > near)
            sx = ((ndc[0] + 1.0f) * P.width - 1.0f) * 0.5f;  // ndcToScreenCentered (GaussianShared.h:184-189)
            sy = ((ndc[1] + 1.0f) * P.height - 1.0f) * 0.5f;
            const M3 C3 = build_cov3d(scale, rot);
            cov = project_cov2d(C3, vp, P.view, P.limX, P.limY, P.focalX, P.focalY);
            cov = stabilize_cov2d(cov, P.maxEig);
            // computeConicAndRadius (GaussianShared.h:390-400)
            const float det = cov.a * cov.d - cov.b * cov.c;
            const float invDet = 1.0f / __builtin_fmaxf(det, 1e-8f);
            conic[0] = cov.d * invDet;
            conic[1] = -cov.b * invDet;
            conic[2] = cov.a * invDet;
            const float mid = 0.5f * (cov.a + cov.d);
            const float delta = __builtin_fmaxf(mid * mid - det, 1e-5f);
            const float maxEig = mid + __builtin_sqrtf(delta);
            const float radius = 3.0f * __builtin_ceilf(__builtin_sqrtf(__builtin_fmaxf(maxEig, 1e-5f)));
            if (radius < 0.5f) ok = false;  // cullByRadius
        }
        if (ok) {  // cullByTotalInkFromCov (GaussianShared.h:753-768), threshold 2.0
            const float a = cov.a, b = 0.5f * (cov.b + cov.c), d = cov.d;
            const float ink = opacity * 6.283185f * sqrt_cr(__builtin_fmaxf(a * d - b * b, 1e-12f));
            const float s = clampf((P.adjFar - depth) / P.adjDen, 0.0f, 1.0f);
            const float depthFactor = 1.0f - s * s;
            if (ink < depthFactor * 2.0f) ok = false;
        }
        if (ok) {
            float ex, ey;
            obb_extents(cov, &ex, &ey);
            // computeTileBounds (GaussianShared.h:791-828) on 16x16 tiles (x / 16 = x * 2^-4 exactly)
            const float maxW = P.width - 1.0f, maxH = P.height - 1.0f;
            const float xmin = clampf(sx - ex, 0.0f, maxW), xmax = clampf(sx + ex, 0.0f, maxW);
            const float ymin = clampf(sy - ey, 0.0f, maxH), ymax = clampf(sy + ey, 0.0f, maxH);
            const int minTX = max((int)__builtin_floorf(xmin * (1.0f / 16.0f)), 0);
            const int maxTX = min((int)__builtin_ceilf(xmax * (1.0f / 16.0f)) - 1, (int)P.tilesX - 1);
            const int minTY = max((int)__builtin_floorf(ymin * (1.0f / 16.0f)), 0);
            const int maxTY = min((int)__builtin_ceilf(ymax * (1.0f / 16.0f)) - 1, (int)P.tilesY - 1);
            if (!(minTX <= maxTX && minTY <= maxTY)) ok = false;  // !tb.valid
            if (ok) {
                float col[3];
                sh_color<HALF, DEG>(harm, gid, pos, P.camPos, P.shComponents, col);
                col[0] = __builtin_fmaxf(col[0] + 0.5f, 0.0f);
                col[1] = __builtin_fmaxf(col[1] + 0.5f, 0.0f);
                col[2] = __builtin_fmaxf(col[2] + 0.5f, 0.0f);
                if (P.inputIsSRGB > 0.5f) {
                    col[0] = srgb_to_linear(col[0]);
                    col[1] = srgb_to_linear(col[1]);
                    col[2] = srgb_to_linear(col[2]);
                }
                // ProjectedGaussian (:164-180): every field rounded to fp16, maxTile exclusive
                // (the empty asm keeps the compiler from folding an fp32 product and its conversion into one
                // v_fma_mixlo_f16 with a +0 addend, which turns a product of -0 -- conicB = -b * invDet for
                // an axis-aligned splat -- into +0)
                auto hb = [](float v) {
                    asm volatile("" : "+v"(v));
                    return (uint32_t)f_to_hbits(v);
                };
                auto pk = [&](float lo, float hi) { return hb(lo) | (hb(hi) << 16); };
                rec.a = make_uint4(pk(sx, sy), pk(conic[0], conic[1]), pk(conic[2], depth), pk(col[0], col[1]));
                rec.b = make_uint4(pk(col[2], opacity), (uint32_t)minTX | ((uint32_t)minTY << 16),
                                   (uint32_t)(maxTX + 1) | ((uint32_t)(maxTY + 1) << 16), pk(ex, ey));
            }
        }
    }
    if (gid < P.count) temp[gid] = rec;  // culled: all zero (minTile = maxTile = 0)
    const uint32_t s = block_reduce_add<kLocalBlock>(ok ? 1u : 0u, lds);
    if (threadIdx.x == 0) blockSums[blockIdx.x] = s;
}

// ---------------------------------------------------------------------------
// 2. localCompact (LocalShaders.metal:201-214): the visible records in ascending gaussian order
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kLocalBlock) void k_local_compact(uint32_t count, const LocalProjected* __restrict__ temp,
                                                               const uint32_t* __restrict__ blockOffsets,
                                                               LocalProjected* __restrict__ compacted) {
    __shared__ uint32_t lds[kLocalBlock / 64];
    const uint32_t gid = blockIdx.x * kLocalBlock + threadIdx.x;
    LocalProjected rec;
    rec.a = rec.b = make_uint4(0u, 0u, 0u, 0u);
    if (gid < count) rec = temp[gid];
    const uint32_t v = rec.b.z != 0u ? 1u : 0u;  // maxTile >= 1 marks a visible record
    uint32_t total;
    const uint32_t off = block_exclusive_scan<kLocalBlock>(v, lds, &total);
    if (v) compacted[blockOffsets[blockIdx.x] + off] = rec;  // (< visible <= count <= maxG)
}

// ---------------------------------------------------------------------------
// 3. localScatterSimd16 (LocalShaders.metal:573-667).  16 lanes share one compacted gaussian and stride
// over the tiles of its rect; a tile that passes intersectsTile (GaussianShared.h:647-653, on the fp16
// record widened to fp32) bumps its counter and, while the slot is below 2048, stores
// (depth16, compacted index) there.  Which 2048 of an overflowing tile are kept depends on the
// atomics' order; the count does not.
// ---------------------------------------------------------------------------
constexpr uint32_t kLocalScatterLanes = 16;
__device__ __forceinline__ bool local_intersects_tile(int tx, int ty, float cx, float cy, const Conic& k, float w) {
    const int pminx = tx * (int)kLocalTile, pminy = ty * (int)kLocalTile;
    const int pmaxx = pminx + (int)kLocalTile - 1, pmaxy = pminy + (int)kLocalTile - 1;
    if (cx >= (float)pminx && cx <= (float)pmaxx && cy >= (float)pminy && cy <= (float)pmaxy) return true;
    const float dx = (cx * 2.0f < (float)(pminx + pmaxx)) ? cx - (float)pminx : cx - (float)pmaxx;
    if (seg_ellipse(k.C, -2.0f * k.B * dx, k.A * dx * dx - w, cy, (float)pminy, (float)pmaxy)) return true;
    const float dy = (cy * 2.0f < (float)(pminy + pmaxy)) ? cy - (float)pminy : cy - (float)pmaxy;
    if (seg_ellipse(k.A, -2.0f * k.B * dy, k.C * dy * dy - w, cx, (float)pminx, (float)pmaxx)) return true;
    return false;
}
__global__ __launch_bounds__(kLocalBlock) void k_local_scatter(const TileAssignmentHeader* __restrict__ visHdr,
                                                               const LocalProjected* __restrict__ compacted,
                                                               uint32_t tilesX, uint32_t tilesY,
                                                               uint32_t* __restrict__ tileCounts,
                                                               uint16_t* __restrict__ depthKeys,
                                                               uint32_t* __restrict__ slotIndices) {
    const uint32_t t = blockIdx.x * kLocalBlock + threadIdx.x;
    const uint32_t g = t / kLocalScatterLanes, sub = t % kLocalScatterLanes;
    if (g >= visHdr->totalAssignments) return;
    const LocalProjected r = compacted[g];
    const float cx = hbits_to_f((uint16_t)(r.a.x & 0xFFFFu)), cy = hbits_to_f((uint16_t)(r.a.x >> 16));
    Conic k;
    k.A = hbits_to_f((uint16_t)(r.a.y & 0xFFFFu));
    k.B = hbits_to_f((uint16_t)(r.a.y >> 16));
    k.C = hbits_to_f((uint16_t)(r.a.z & 0xFFFFu));
    const uint16_t depth16 = (uint16_t)((r.a.z >> 16) ^ 0x8000u);
    const float opacity = hbits_to_f((uint16_t)(r.b.x >> 16));
    const float w = 2.0f * compute_power(opacity);  // gaussianComputePower (GaussianShared.h:595-597)
    const int minTX = (int)(r.b.y & 0xFFFFu), minTY = (int)(r.b.y >> 16);
    // the rect was written by k_local_project inside the grid; the clamp keeps a foreign record in bounds
    const int maxTX = min((int)(r.b.z & 0xFFFFu), (int)tilesX), maxTY = min((int)(r.b.z >> 16), (int)tilesY);
    const int rangeX = maxTX - minTX, rangeY = maxTY - minTY;
    if (rangeX <= 0 || rangeY <= 0) return;
    const int total = rangeX * rangeY;
    for (int idx = (int)sub; idx < total; idx += (int)kLocalScatterLanes) {
        const int ly = idx / rangeX, lx = idx - ly * rangeX;
        const int tx = minTX + lx, ty = minTY + ly;
        if (!local_intersects_tile(tx, ty, cx, cy, k, w)) continue;
        const uint32_t tile = (uint32_t)ty * tilesX + (uint32_t)tx;
        const uint32_t slot = atomicAdd(&tileCounts[tile], 1u);
        if (slot < kLocalMaxPerTile) {
            const size_t wp = (size_t)tile * kLocalMaxPerTile + slot;
            depthKeys[wp] = depth16;
            slotIndices[wp] = g;
        }
    }
}

// ---------------------------------------------------------------------------
// 4. localPerTileSort16 (LocalShaders.metal:362-437): one workgroup per tile, a bitonic sort of
// min(count, maxPerTile) entries in LDS.  The reference's key is (depth16 << 16) | slot, and the slot
// of a gaussian is decided by an atomic race; here the key is (depth16, index, slot) in 64 bits, so
// within one depth16 the entries are ordered by their index (in a frame: the compacted index, unique
// per tile) and the order does not depend on scheduling.  16 KB of LDS per tile.  Outputs the sorted
// slots (sortedLocalIdx) and, for a frame, the sorted indices themselves (the blend's list).  Lane 0
// also adds the tile to the frame's counters.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kLocalBlock) void k_local_sort(const uint16_t* __restrict__ keys16,
                                                            const uint32_t* __restrict__ indices,
                                                            const uint32_t* __restrict__ counts, uint32_t maxPerTile,
                                                            uint16_t* __restrict__ sortedLocal,
                                                            uint32_t* __restrict__ lists,
                                                            LocalStats* __restrict__ stats) {
    __shared__ uint64_t sk[kLocalMaxPerTile];
    const uint32_t tile = blockIdx.x, tid = threadIdx.x;
    const uint32_t count = counts[tile];
    const uint32_t n = min(count, maxPerTile);  // (maxPerTile <= 2048: the launcher checks)
    if (n == 0) return;                         // (block-uniform)
    if (stats && tid == 0) {
        atomicAdd(&stats->activeTiles, 1u);
        atomicAdd(&stats->totalEntries, n);
        atomicMax(&stats->maxTileCount, count);
    }
    const size_t start = (size_t)tile * maxPerTile;
    uint32_t padded = 1;
    while (padded < n) padded <<= 1;
    for (uint32_t i = tid; i < padded; i += kLocalBlock)
        sk[i] = i < n ? ((uint64_t)keys16[start + i] << 48) | ((uint64_t)indices[start + i] << 16) | (uint64_t)i
                      : ~0ull;  // (above every real key: a real slot is below 2048)
    __syncthreads();
    for (uint32_t k = 2; k <= padded; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t i = tid; i < padded; i += kLocalBlock) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = sk[i], b = sk[ixj];
                    const bool ascending = (i & k) == 0;
                    if (ascending ? a > b : a < b) {
                        sk[i] = b;
                        sk[ixj] = a;
                    }
                }
            }
            __syncthreads();
        }
    for (uint32_t i = tid; i < n; i += kLocalBlock) {
        const uint64_t v = sk[i];
        sortedLocal[start + i] = (uint16_t)(v & 0xFFFFu);
        if (lists) lists[start + i] = (uint32_t)(v >> 16);
    }
}

// ---------------------------------------------------------------------------
// 5. localClearTextures + localRender16 (LocalShaders.metal:27-39, :440-571) over every tile.
//
// Persistent workgroups: the 128 KiB alpha table (blend_exp_table_entry: exp(-0.5h * p) indexed by the
// bits of p) sits in LDS.  A lane is one reference thread: the 4x2 pixel group (localId.x = lane & 3,
// localId.y = lane >> 2 of its half) held as packed fp16 pairs, so the reference's all-zero skip (:527)
// is the lane's own.  32 lanes are one tile and a wave64 walks two tiles, one per half; the saturation
// break (:549-551) is a vote over the 32 lanes x 8 pixels of ONE tile: the half's 32 bits of the wave's
// ballot.  Lane l of a half stages entry l of its tile's 32-entry batch; every entry is read back as a
// broadcast within the half.  The reference's control flow is applied as data: a half that ended its
// walk, or ran out of entries, keeps its state while the other half goes on.
// A tile without entries leaves the loop at once and writes the clear value: colour (0, 0, 0, 0),
// depth 0 -- what c = 0, T = 1, d = 0 give.  Writes are bounds-checked for ragged sizes.
// ---------------------------------------------------------------------------
constexpr uint32_t kLocalBatch = 32;
__device__ __forceinline__ void lc_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
__device__ __forceinline__ h2 lc_h2(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ uint32_t lc_u32(h2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ h2 lc_lo(h2 v) { return h2{v.x, v.x}; }
__device__ __forceinline__ h2 lc_hi(h2 v) { return h2{v.y, v.y}; }
typedef unsigned short lc_u16x2 __attribute__((ext_vector_type(2)));

template <int NW>
__global__ __launch_bounds__(NW * 64) void k_local_blend(const LocalProjected* __restrict__ compacted,
                                                         const uint32_t* __restrict__ counts,
                                                         const uint32_t* __restrict__ lists,
                                                         const uint16_t* __restrict__ expTable, uint32_t tilesX,
                                                         uint32_t tileCount, uint32_t W, uint32_t H,
                                                         uint8_t* __restrict__ color, size_t pitch, int fmt,
                                                         uint8_t* __restrict__ depthOut, size_t depthPitch) {
    __shared__ __attribute__((aligned(16))) uint16_t tbl[65536];
    __shared__ __attribute__((aligned(16))) uint4 stageA[NW][64];
    __shared__ __attribute__((aligned(16))) uint32_t stageB[NW][64];
    {
        const uint4* src = (const uint4*)expTable;
        uint4* dst = (uint4*)tbl;
        for (int i = threadIdx.x; i < 65536 * 2 / 16; i += NW * 64) dst[i] = src[i];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t half = lane >> 5, hl = lane & 31u;
    const uint32_t bpp = fmt == GSM_COLOR_FORMAT_RGBA16F ? 8u : (fmt == GSM_COLOR_FORMAT_RGBA32F ? 16u : 4u);
    const h2 ONE = {(h1)1.0f, (h1)1.0f};
    const h1 c099 = (h1)0.99, c01 = (h1)0.1, c0004 = (h1)0.004;
    const h2 C099 = {c099, c099};
    uint4* sA = stageA[wave];
    uint32_t* sB = stageB[wave];
    const uint32_t pairs = (tileCount + 1u) / 2u;
    for (uint32_t pair = blockIdx.x * NW + wave; pair < pairs; pair += gridDim.x * NW) {
        const uint32_t t = 2u * pair + half;
        const bool tileValid = t < tileCount;
        const uint32_t cnt = tileValid ? min(counts[t], kLocalMaxPerTile) : 0u;
        const uint32_t tileX = t % tilesX, tileY = t / tilesX;
        const uint32_t bx = tileX * kLocalTile + (hl & 3u) * 4u, by = tileY * kLocalTile + (hl >> 2) * 2u;
        const h2 PX[2] = {{(h1)(float)bx, (h1)(float)(bx + 1u)}, {(h1)(float)(bx + 2u), (h1)(float)(bx + 3u)}};
        const h2 PY = {(h1)(float)by, (h1)(float)(by + 1u)};
        // [row][x pair]: {x, x + 1}, {x + 2, x + 3}
        h2 T[2][2], Cr[2][2], Cg[2][2], Cb[2][2];
        float D[2][4];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                T[r][c] = ONE;
                Cr[r][c] = Cg[r][c] = Cb[r][c] = lc_h2(0u);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) D[r][c] = 0.0f;
        }
        bool done = cnt == 0;  // the half's walk has ended (uniform within a half)
        const uint32_t cnt0 = (uint32_t)__builtin_amdgcn_readlane((int)cnt, 0);
        const uint32_t cnt1 = (uint32_t)__builtin_amdgcn_readlane((int)cnt, 32);
        const uint32_t maxCnt = max(cnt0, cnt1);
        const uint32_t* lst = lists + (size_t)(tileValid ? t : 0u) * kLocalMaxPerTile;
        for (uint32_t b0 = 0; b0 < maxCnt; b0 += kLocalBatch) {
            if (__builtin_amdgcn_ballot_w64(!done) == 0) break;
            const uint32_t n = b0 < cnt ? min(kLocalBatch, cnt - b0) : 0u;
            if (!done && hl < n) {
                const LocalProjected r = compacted[lst[b0 + hl]];
                const h1 cxy2 = (h1)2.0f * __builtin_bit_cast(h1, (uint16_t)(r.a.y >> 16));  // 2.0h * cov.y (:502)
                sA[lane] = make_uint4(r.a.x, (r.a.y & 0xFFFFu) | (r.a.z << 16),
                                      (uint32_t)__builtin_bit_cast(uint16_t, cxy2) | (r.b.x & 0xFFFF0000u), r.a.w);
                sB[lane] = (r.b.x & 0xFFFFu) | (r.a.z & 0xFFFF0000u);  // colorB, depth
            }
            lc_wave_sync();
            const uint32_t nmax = min(kLocalBatch, maxCnt - b0);
            for (uint32_t j = 0; j < nmax; ++j) {
                const bool active = !done && j < n;
                // (an inactive half reads a stale or unwritten stage entry: its values are not used)
                const uint4 ra = sA[half * 32u + j];
                const uint32_t rb = sB[half * 32u + j];
                const h2 mean = lc_h2(ra.x), cc = lc_h2(ra.y);
                const h2 c2 = lc_lo(lc_h2(ra.z)), op = lc_hi(lc_h2(ra.z));
                // p = ((dx*dx)*cxx + (dy*dy)*cyy) + (dx*dy)*cxy2 (:509-516)
                const h2 dy = PY - lc_hi(mean);
                const h2 byy = (dy * dy) * lc_hi(cc);
                h2 a[2][2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    const h2 dx = PX[c] - lc_lo(mean);
                    const h2 ax = (dx * dx) * lc_lo(cc);
#pragma unroll
                    for (int r = 0; r < 2; ++r) {
                        const h2 dyr = r == 0 ? lc_lo(dy) : lc_hi(dy);
                        const h2 p = (ax + (r == 0 ? lc_lo(byy) : lc_hi(byy))) + (dx * dyr) * c2;
                        const uint32_t pw = lc_u32(p);
                        lc_u16x2 e;
                        e.x = tbl[pw & 0xFFFFu];
                        e.y = tbl[pw >> 16];
                        a[r][c] = __builtin_elementwise_min(op * __builtin_bit_cast(h2, e), C099);  // (:518-525)
                    }
                }
                // all eight alphas == 0.0h (:527): +0 or -0 in every half
                const bool anyAlpha =
                    ((lc_u32(a[0][0]) | lc_u32(a[0][1]) | lc_u32(a[1][0]) | lc_u32(a[1][1])) & 0x7FFF7FFFu) != 0u;
                if (active && anyAlpha) {
                    const float gDepth = hbits_to_f((uint16_t)(rb >> 16));
                    const h2 cr = lc_lo(lc_h2(ra.w)), cg = lc_hi(lc_h2(ra.w)), cb = lc_lo(lc_h2(rb));
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int c = 0; c < 2; ++c) {
                            // depth of the first entry with alpha > 0.1h (:530-537)
                            if (D[r][2 * c] == 0.0f && a[r][c].x > c01) D[r][2 * c] = gDepth;
                            if (D[r][2 * c + 1] == 0.0f && a[r][c].y > c01) D[r][2 * c + 1] = gDepth;
                            // c += gColor * (a * t): the declared FMA per channel (:539-542)
                            const h2 w = a[r][c] * T[r][c];
                            Cr[r][c] = __builtin_elementwise_fma(cr, w, Cr[r][c]);
                            Cg[r][c] = __builtin_elementwise_fma(cg, w, Cg[r][c]);
                            Cb[r][c] = __builtin_elementwise_fma(cb, w, Cb[r][c]);
                            T[r][c] = T[r][c] * (ONE - a[r][c]);  // (:544-547)
                        }
                }
                // maxT < 0.004h for every pixel of the tile (:549-551)
                const h2 m = __builtin_elementwise_max(__builtin_elementwise_max(T[0][0], T[0][1]),
                                                       __builtin_elementwise_max(T[1][0], T[1][1]));
                const h1 mt = __builtin_elementwise_max(m.x, m.y);
                const uint64_t sat = __builtin_amdgcn_ballot_w64(mt < c0004);
                const uint32_t satHalf = half ? (uint32_t)(sat >> 32) : (uint32_t)sat;
                if (active && satHalf == 0xFFFFFFFFu) done = true;
                if (__builtin_amdgcn_ballot_w64(!done && j + 1u < n) == 0) break;  // nothing left in this batch
            }
            if (b0 + n >= cnt) done = true;  // the half's list ends with this batch
            lc_wave_sync();  // the stage is rewritten by the next batch
        }
        if (!tileValid) continue;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const uint32_t y = by + (uint32_t)r;
            if (y >= H) continue;
            uint8_t* trow = color + (size_t)y * pitch;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const uint32_t ur = lc_u32(Cr[r][c]), ug = lc_u32(Cg[r][c]), ub = lc_u32(Cb[r][c]);
                const uint32_t ua = lc_u32(ONE - T[r][c]);  // (c, 1 - T) (:563-570)
                const uint32_t x0 = bx + 2u * (uint32_t)c;
                if (x0 < W) {
                    store_color_px(fmt, (char*)(trow + (size_t)x0 * bpp), (ur & 0xFFFFu) | (ug << 16),
                                   (ub & 0xFFFFu) | (ua << 16));
                    if (depthOut)
                        *(uint16_t*)(depthOut + (size_t)y * depthPitch + (size_t)x0 * 2u) = f_to_hbits(D[r][2 * c]);
                }
                if (x0 + 1u < W) {
                    store_color_px(fmt, (char*)(trow + (size_t)(x0 + 1u) * bpp), (ur >> 16) | (ug & 0xFFFF0000u),
                                   (ub >> 16) | (ua & 0xFFFF0000u));
                    if (depthOut)
                        *(uint16_t*)(depthOut + (size_t)y * depthPitch + (size_t)(x0 + 1u) * 2u) =
                            f_to_hbits(D[r][2 * c + 1]);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------
void local_launch_clear(const LocalArgs& a, const LocalArena& A, hipStream_t s) {
    const uint32_t blocks = (a.tileCount + kLocalBlock - 1) / kLocalBlock;
    hipLaunchKernelGGL(k_local_clear, dim3(blocks ? blocks : 1u), dim3(kLocalBlock), 0, s, A.tileCounts, a.tileCount,
                       A.stats);
}

template <bool HALF>
static void local_launch_project_t(uint32_t deg, const void* world, const void* harm, const LocalArgs& a,
                                   const LocalArena& A, hipStream_t s) {
    const uint32_t blocks = (a.count + kLocalBlock - 1) / kLocalBlock;
    if (blocks == 0) return;
#define GSM_LOCAL_PROJ(D) \
    hipLaunchKernelGGL((k_local_project<HALF, D>), dim3(blocks), dim3(kLocalBlock), 0, s, world, harm, a, A.temp, A.blockSums)
    switch (deg) {
        case 0: GSM_LOCAL_PROJ(0); break;
        case 1: GSM_LOCAL_PROJ(1); break;
        case 2: GSM_LOCAL_PROJ(2); break;
        default: GSM_LOCAL_PROJ(3); break;
    }
#undef GSM_LOCAL_PROJ
}

void local_launch_project(bool halfInput, uint32_t deg, const void* world, const void* harm, const LocalArgs& a,
                          const LocalArena& A, hipStream_t s) {
    if (halfInput) local_launch_project_t<true>(deg, world, harm, a, A, s);
    else local_launch_project_t<false>(deg, world, harm, a, A, s);
}

void local_launch_compact(const LocalArgs& a, const LocalArena& A, hipStream_t s) {
    const uint32_t blocks = (a.count + kLocalBlock - 1) / kLocalBlock;
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_local_compact, dim3(blocks), dim3(kLocalBlock), 0, s, a.count, A.temp, A.blockSums,
                       A.compacted);
}

void local_launch_scatter(const LocalArgs& a, const LocalArena& A, hipStream_t s) {
    // capacity-sized: the visible count is read on the device
    const uint64_t threads = (uint64_t)a.count * kLocalScatterLanes;
    const uint32_t blocks = (uint32_t)((threads + kLocalBlock - 1) / kLocalBlock);
    if (blocks == 0) return;
    hipLaunchKernelGGL(k_local_scatter, dim3(blocks), dim3(kLocalBlock), 0, s, A.visHdr, A.compacted, a.tilesX,
                       a.tilesY, A.tileCounts, A.depthKeys, A.slotIndices);
}

void local_launch_sort(const uint16_t* keys16, const uint32_t* indices, const uint32_t* counts, uint32_t tileCount,
                       uint32_t maxPerTile, uint16_t* sortedLocal, uint32_t* lists, LocalStats* stats,
                       hipStream_t s) {
    if (tileCount == 0 || maxPerTile == 0 || maxPerTile > kLocalMaxPerTile) return;
    hipLaunchKernelGGL(k_local_sort, dim3(tileCount), dim3(kLocalBlock), 0, s, keys16, indices, counts, maxPerTile,
                       sortedLocal, lists, stats);
}

constexpr int kLocalBlendWaves = 8;
void local_launch_blend(const LocalArgs& a, const LocalArena& A, void* color, size_t pitch, int colorFormat,
                        void* depth, size_t depthPitch, int numCUs, hipStream_t s) {
    uint32_t grid = (uint32_t)(numCUs > 0 ? numCUs : 256);
    const uint32_t pairs = (a.tileCount + 1u) / 2u;
    const uint32_t need = (pairs + kLocalBlendWaves - 1) / kLocalBlendWaves;
    if (grid > need) grid = need;
    if (grid == 0) return;
    hipLaunchKernelGGL((k_local_blend<kLocalBlendWaves>), dim3(grid), dim3(kLocalBlendWaves * 64), 0, s, A.compacted,
                       A.tileCounts, A.lists, A.expTable, a.tilesX, a.tileCount, (uint32_t)a.width,
                       (uint32_t)a.height, (uint8_t*)color, pitch, colorFormat, (uint8_t*)depth, depthPitch);
}

}  // namespace gsm

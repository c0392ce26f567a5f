// gsm_project_body.h -- the text of k_project, compiled four times (and twice styled) by gsm_kernels.hip: as the single frame's
// kernel (GSM_VIEWS 0: k_project, exactly the kernel it was before batches of views existed; an item is its
// gaussian id), as the projection of a batch of views of one scene (GSM_VIEWS 1: k_project_views), as the
// projection of a batch of views of different scenes and sizes (GSM_VIEWS 2: k_project_batch) and as the
// projection of several posed objects into one frame (GSM_VIEWS 3: k_project_compose).  No include guard.
// With GSM_STYLED defined (GSM_VIEWS 0, 2 and 3 only) the same text gives k_project_styled, k_project_batch_styled
//  and k_project_compose_styled: one more argument, the style table -- for the single
// frame the scene's state bytes and default too, for a batch the per-view options array that holds them -- and
// project_gaussian's kProjStyled mode; nothing else differs.
// With GSM_ORTHO defined (GSM_VIEWS 0, 2 and 3, plain and styled) the text gives the orthographic
// instances: k_project_ortho, k_project_ortho_styled, k_project_compose_ortho and k_project_compose_ortho_styled call
// project_gaussian's ORTHO variant for every gaussian -- the uniforms travel in the fields of ProjectArgs and
// ComposeObjectArgs that carry the perspective terms -- and k_project_batch_ortho, k_project_batch_ortho_styled, the
// projections of a batch in which some view is orthographic, choose the variant by the view's `ortho` word (uniform
// per block: a scalar branch).  The kernels without GSM_ORTHO are the text they were.
#ifdef GSM_ORTHO
#define GSM_PK(plain, ortho) ortho
#else
#define GSM_PK(plain, ortho) plain
#endif
#if defined(GSM_STYLED) && GSM_VIEWS == 2
// The styled projection of a batch with options (gsm_global_render_frames): k_project_batch with the
// style step.  A block reads its view's state pointer, default state and styled flag from the view's options line
// (BatchExtras; the block's view index is uniform: scalar loads).  A view that is not styled takes the identity
// style without a table load -- c * 255 / 255 and o * 255 / 255 in the style rule's integers: the plain bytes.
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project_batch_styled, k_project_batch_ortho_styled)(
    ProjectArgs P, const BatchViewArgs* __restrict__ views, const uint16_t* __restrict__ blockView,
    const BatchExtras* __restrict__ extras, GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds,
    BlendRecord* __restrict__ outRec, uint32_t* __restrict__ counts, uint32_t* __restrict__ masks,
    uint32_t* __restrict__ blockSums, const float2* __restrict__ sincos, const uint16_t* __restrict__ unitCost,
    uint32_t* __restrict__ unitOrder, uint32_t* __restrict__ costMax, const uint2* __restrict__ styleTable) {
    const void* __restrict__ world = nullptr;  // the block's scene: its view's (below)
    const void* __restrict__ harm = nullptr;
    const uint8_t* __restrict__ stateBytes = nullptr;  // the block's state bytes and default: its view's
    uint32_t defaultState = 0, styledView = 0;
#elif defined(GSM_STYLED) && GSM_VIEWS == 3
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project_compose_styled, k_project_compose_ortho_styled)(
    ProjectArgs P, const ComposeObjectArgs* __restrict__ objects, const uint16_t* __restrict__ blockObject,
    GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds, BlendRecord* __restrict__ outRec,
    uint32_t* __restrict__ counts, uint32_t* __restrict__ masks, uint32_t* __restrict__ blockSums,
    const float2* __restrict__ sincos, const uint16_t* __restrict__ unitCost, uint32_t* __restrict__ unitOrder,
    uint32_t* __restrict__ costMax, const uint2* __restrict__ styleTable) {
    const void* __restrict__ world = nullptr;  // the block's scene: its object's (below)
    const void* __restrict__ harm = nullptr;
    const uint8_t* __restrict__ stateBytes = nullptr;  // the block's state bytes and default: its object's
    uint32_t defaultState = 0;
#elif defined(GSM_STYLED)
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project_styled, k_project_ortho_styled)(
    const void* __restrict__ world, const void* __restrict__ harm, ProjectArgs P,
    GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds,
    BlendRecord* __restrict__ outRec, uint32_t* __restrict__ counts,
    uint32_t* __restrict__ masks, uint32_t* __restrict__ blockSums, const float2* __restrict__ sincos,
    const uint16_t* __restrict__ unitCost, uint32_t* __restrict__ unitOrder, uint32_t* __restrict__ costMax,
    const uint2* __restrict__ styleTable, const uint8_t* __restrict__ stateBytes, uint32_t defaultState) {
#elif GSM_VIEWS == 3
// The projection of a composite (gsm_global_render_composite): block b belongs to the object of
// entry blockObject[b] -- uniform per block, one 2-byte load -- and projects gaussians [(b - blockBase) * 256,
// + 256) of that object's scene under that object's camera onto the frame's own tile grid.  The scene, the count
// and the camera terms come from the entry (ComposeObjectArgs) by scalar loads; the grid, the rows and the
// thresholds stay P's, as the single frame's.  The per-gaussian arrays are written at the block's items, b * 256
// + thread; the tile tests and counts are those of k_project for that scene and camera.
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project_compose, k_project_compose_ortho)(
    ProjectArgs P, const ComposeObjectArgs* __restrict__ objects, const uint16_t* __restrict__ blockObject,
    GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds, BlendRecord* __restrict__ outRec,
    uint32_t* __restrict__ counts, uint32_t* __restrict__ masks, uint32_t* __restrict__ blockSums,
    const float2* __restrict__ sincos, const uint16_t* __restrict__ unitCost, uint32_t* __restrict__ unitOrder,
    uint32_t* __restrict__ costMax) {
    const void* __restrict__ world = nullptr;  // the block's scene: its object's (below)
    const void* __restrict__ harm = nullptr;
#elif GSM_VIEWS == 2
// The projection of a batch of different views (gsm_global_render_batch): block b belongs to view
// blockView[b] -- uniform per block, one 2-byte load -- and projects gaussians [(b - blockBase) * 256, + 256) of
// that view's scene under its camera onto its own tile grid; everything the view owns comes from its entry of
// views[] (BatchViewArgs) by scalar loads, P keeps what the batch shares (the thresholds, the schedule).  The
// per-gaussian arrays are written at the block's items, b * 256 + thread; the tile tests and counts are those
// of k_project for that scene, camera and size.
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project_batch, k_project_batch_ortho)(
    ProjectArgs P, const BatchViewArgs* __restrict__ views, const uint16_t* __restrict__ blockView,
    GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds, BlendRecord* __restrict__ outRec,
    uint32_t* __restrict__ counts, uint32_t* __restrict__ masks, uint32_t* __restrict__ blockSums,
    const float2* __restrict__ sincos, const uint16_t* __restrict__ unitCost, uint32_t* __restrict__ unitOrder,
    uint32_t* __restrict__ costMax) {
    const void* __restrict__ world = nullptr;  // the block's scene: its view's (below)
    const void* __restrict__ harm = nullptr;
#elif GSM_VIEWS
// The projection of a batch of views (gsm_global_render_views): block b projects gaussians
// [(b % blocksPerView) * 256, + 256) under view b / blocksPerView -- uniform per block -- whose camera and
// derived constants come from views[] (ViewArgs); P holds what the batch shares (the frame's tile grid,
// the count per view, the thresholds).  The per-gaussian arrays are written at the block's items, v *
// blocksPerView * 256 + id; the tile tests and counts are those of k_project for that camera.
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void k_project_views(
    const void* __restrict__ world, const void* __restrict__ harm, ProjectArgs P, const ViewArgs* __restrict__ views,
    uint32_t blocksPerView, GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds,
    BlendRecord* __restrict__ outRec, uint32_t* __restrict__ counts, uint32_t* __restrict__ masks,
    uint32_t* __restrict__ blockSums, const float2* __restrict__ sincos, const uint16_t* __restrict__ unitCost,
    uint32_t* __restrict__ unitOrder, uint32_t* __restrict__ costMax) {
#else
template <bool HALF, int DEG>
__global__ __launch_bounds__(kProjectBlock) void GSM_PK(k_project, k_project_ortho)(
    const void* __restrict__ world, const void* __restrict__ harm, ProjectArgs P,
    GaussianRenderData* __restrict__ outRD, short4* __restrict__ outBounds,
    BlendRecord* __restrict__ outRec, uint32_t* __restrict__ counts,
    uint32_t* __restrict__ masks, uint32_t* __restrict__ blockSums, const float2* __restrict__ sincos,
    const uint16_t* __restrict__ unitCost, uint32_t* __restrict__ unitOrder, uint32_t* __restrict__ costMax) {
#endif
    __shared__ uint32_t lds[kProjectBlock / 64];
    __shared__ ByteLut lut;
    // block 0 of a scheduled launch orders the blend's units from the previous frame's walks while
    // the other blocks project (no launch, no second stream, no join before the blend)
    if (P.schedUnits) {
        if (blockIdx.x == 0) {
            __shared__ uint32_t uoBase[kUoBuckets], uoMax[kProjectBlock / 64];
            unit_order_block<kProjectBlock>(unitCost, unitOrder, P.schedUnits, uoBase, uoMax, costMax, P.pairBucket);
            return;
        }
    }
    const uint32_t blk = blockIdx.x - (P.schedUnits ? 1u : 0u);
#if GSM_VIEWS == 3
    // the block's object (uniform: scalar loads) and its first gaussian; items are written at blk * 256 + thread
    uint32_t gblk;
    {
        const ComposeObjectArgs& V = objects[__builtin_amdgcn_readfirstlane((uint32_t)blockObject[blk])];
        gblk = blk - V.blockBase;
        world = V.world;
        harm = V.harm;
#ifdef GSM_STYLED
        stateBytes = V.state;
        defaultState = V.defaultState;
#endif
        P.cam = V.cam;
        P.count = V.count;
        P.limX = V.limX;
        P.limY = V.limY;
        P.focalX = V.focalX;
        P.focalY = V.focalY;
        P.maxEig = V.maxEig;
        P.adjFar = V.adjFar;
        P.adjDen = V.adjDen;
    }
#elif GSM_VIEWS == 2
    // the block's view (uniform: scalar loads) and its first gaussian; items are written at blk * 256 + thread
    uint32_t gblk;
#ifdef GSM_ORTHO
    uint32_t orthoView = 0;  // the view's kind (uniform per block)
#endif
    {
        const BatchViewArgs& V = views[__builtin_amdgcn_readfirstlane((uint32_t)blockView[blk])];
        gblk = blk - V.blockBase;
        world = V.world;
        harm = V.harm;
#ifdef GSM_ORTHO
        orthoView = V.ortho;
#endif
#ifdef GSM_STYLED
        {
            const BatchExtras& E = extras[__builtin_amdgcn_readfirstlane((uint32_t)blockView[blk])];
            stateBytes = E.state;
            defaultState = E.defaultState;
            styledView = E.styled;
        }
#endif
        P.cam = V.cam;
        P.bin = V.bin;
        P.rowBegin = 0;
        P.rowEnd = V.bin.tilesY;
        P.rowStride = 1;
        P.count = V.count;
        P.limX = V.limX;
        P.limY = V.limY;
        P.focalX = V.focalX;
        P.focalY = V.focalY;
        P.maxEig = V.maxEig;
        P.adjFar = V.adjFar;
        P.adjDen = V.adjDen;
    }
#elif GSM_VIEWS
    // the block's view (uniform: scalar loads) and its first gaussian; items are written at blk * 256 + thread
    const uint32_t view = blk / blocksPerView, gblk = blk - view * blocksPerView;
    {
        const ViewArgs& V = views[view];
        P.cam = V.cam;
        P.limX = V.limX;
        P.limY = V.limY;
        P.focalX = V.focalX;
        P.focalY = V.focalY;
        P.maxEig = V.maxEig;
        P.adjFar = V.adjFar;
        P.adjDen = V.adjDen;
    }
#else
    const uint32_t gblk = blk;
#endif
    __shared__ float4 sEll[kProjectBlock];   // cmx, cmy, conic A, conic B
    __shared__ float2 sEll2[kProjectBlock];  // conic C, level w
    __shared__ uint32_t sOff[kProjectBlock];  // exclusive candidate offsets
    __shared__ uint32_t sRect[kProjectBlock]; // x0 | rw << 16
    __shared__ int sTy0[kProjectBlock];
    __shared__ uint32_t sMask[kProjectBlock];
    __shared__ uint32_t sMore[kProjectBlock];  // hits among candidates >= 32 (large rects)
    // the block's first kCandCap candidates: owner << 8 | k for rects of <= kCandRect tiles,
    // kSearch for the candidates of larger rects (their owner comes from a binary search).  (r06: 8 waves
    // per SIMD -- 3072 candidates and a 64-VGPR cap -- measured no faster than 7, profiles/r06_proj_ab.txt)
    constexpr uint32_t kCandCap = 4096, kCandRect = 64;
    constexpr uint16_t kSearch = 0xFFFFu;
    __shared__ uint16_t sCand[kCandCap];
    uint4 preW[2];
    preload_world<HALF>(world, gblk * kProjectBlock + threadIdx.x, P.count, preW);
#ifdef GSM_STYLED
    // the gaussian's state byte, loaded with its world record before the byte table's barrier; the style entry
    // (one 8-byte load of the 2 KiB table) follows it
    uint32_t stateByte = defaultState;
    if (stateBytes && gblk * kProjectBlock + threadIdx.x < P.count)
        stateByte = stateBytes[gblk * kProjectBlock + threadIdx.x];
#if GSM_VIEWS == 2
    // (uniform per block: an unstyled view of a styled batch reads neither its state nor the table)
    const uint2 style = styledView ? styleTable[stateByte & (kStyleEntries - 1u)] : make_uint2(0u, kStyleIdentityY);
#else
    const uint2 style = styleTable[stateByte & (kStyleEntries - 1u)];
#endif
#endif
    fill_byte_lut(lut, sincos);
    const uint32_t tid = threadIdx.x;
    const uint32_t gid = gblk * kProjectBlock + tid;
#if GSM_VIEWS
    const uint32_t oid = blk * kProjectBlock + tid;  // the item the gaussian's arrays are written at
#else
#define oid gid
#endif
    ProjOut o;
    o.vis = false;
    o.countable = false;
    o.bounds = make_short4(0, -1, 0, -1);
    uint32_t area = 0;
    int ty0 = 0;
#ifdef GSM_STYLED
#define GSM_PROJ_MODE kProjStyled
#define GSM_PROJ_STYLE style
#else
#define GSM_PROJ_MODE kProjPlain
#define GSM_PROJ_STYLE make_uint2(0u, kStyleIdentityY)
#endif
    if (gid < P.count) {
#if defined(GSM_ORTHO) && GSM_VIEWS == 2
        o = project_gaussian<HALF, DEG, GSM_PROJ_MODE, kOrthoPerView>(world, harm, gid, P, sincos, lut,
                                                                      HALF ? preW : nullptr, GSM_PROJ_STYLE, orthoView);
#elif defined(GSM_ORTHO)
        o = project_gaussian<HALF, DEG, GSM_PROJ_MODE, kOrthoOn>(world, harm, gid, P, sincos, lut, HALF ? preW : nullptr,
                                                                 GSM_PROJ_STYLE);
#elif defined(GSM_STYLED)
        o = project_gaussian<HALF, DEG, kProjStyled>(world, harm, gid, P, sincos, lut, HALF ? preW : nullptr, style);
#else
        o = project_gaussian<HALF, DEG>(world, harm, gid, P, sincos, lut, HALF ? preW : nullptr);
#endif
        outBounds[oid] = o.bounds;
        if (o.vis) {
            // GaussianRenderData: the frame itself only reads it for rects the scatter re-tests
            const int ry0 = max((int)o.bounds.z, (int)P.rowBegin), ry1 = min((int)o.bounds.w, (int)P.rowEnd - 1);
            if (P.keepRenderData || (ry1 - ry0 + 1) * ((int)o.bounds.y - (int)o.bounds.x + 1) > kMaskTiles)
                *(uint4*)(outRD + oid) = o.rd;
            if (o.countable && ry1 >= ry0) {  // rows limited to the slab
                area = (uint32_t)((ry1 - ry0 + 1) * ((int)o.bounds.y - (int)o.bounds.x + 1));
                ty0 = ry0;
            }
        }
    }
    sEll[tid] = make_float4(o.cmx, o.cmy, o.k.A, o.k.B);
    sEll2[tid] = make_float2(o.k.C, o.w);
    sRect[tid] = ((uint32_t)(int)o.bounds.x & 0xFFFFu) | ((uint32_t)((int)o.bounds.y - (int)o.bounds.x + 1) << 16);
    sTy0[tid] = ty0;
    sMask[tid] = 0;
    sMore[tid] = 0;
    uint32_t total;
    const uint32_t coff = block_exclusive_scan<kProjectBlock>(area, lds, &total);
    sOff[tid] = coff;
    const uint32_t nCand = min(total, kCandCap);
    for (uint32_t i = tid; i < nCand; i += kProjectBlock) sCand[i] = kSearch;
    __syncthreads();
    if (area <= kCandRect)
        for (uint32_t k = 0; k < area && coff + k < kCandCap; ++k) sCand[coff + k] = (uint16_t)((tid << 8) | k);
    __syncthreads();
    for (uint32_t c = tid; c < total; c += kProjectBlock) {
        uint32_t lo, k;
        const uint32_t v = c < kCandCap ? (uint32_t)sCand[c] : (uint32_t)kSearch;
        if (v != kSearch) {
            lo = v >> 8;
            k = v & 0xFFu;
        } else {
            lo = 0;
            uint32_t hi = kProjectBlock - 1;  // owner: the largest g with sOff[g] <= c
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (sOff[mid] <= c) lo = mid;
                else hi = mid - 1;
            }
            k = c - sOff[lo];
        }
        const uint32_t rect = sRect[lo], rw = rect >> 16;
        // k / rw from the hardware reciprocal (within one of the quotient), then corrected exactly
        uint32_t row = (uint32_t)((float)k * __builtin_amdgcn_rcpf((float)rw));
        if (row * rw > k) row--;
        else if ((row + 1u) * rw <= k) row++;
        const int ty = sTy0[lo] + (int)row, tx = (int)(rect & 0xFFFFu) + (int)(k - row * rw);
        const float4 e = sEll[lo];
        const float2 e2 = sEll2[lo];
        Conic kk;
        kk.A = e.z;
        kk.B = e.w;
        kk.C = e2.x;
        if (intersects_tile(tx, ty, e.x, e.y, kk, e2.y)) {
            if (k < (uint32_t)kMaskTiles) atomicOr(&sMask[lo], 1u << k);
            else atomicAdd(&sMore[lo], 1u);
        }
    }
    __syncthreads();
    uint32_t ntiles = 0;
    if (gid < P.count && o.vis) {
        const uint32_t mask = sMask[tid];
        ntiles = (uint32_t)__builtin_popcount(mask) + sMore[tid];
        masks[oid] = mask;
        const float2 band = ntiles ? band_of(o.ra, o.bounds, rows_of(P)) : make_float2(0.f, -1.f);
        uint4* rp = (uint4*)(outRec + oid);
        rp[0] = make_uint4(o.ra.x, o.ra.y, o.ra.z, o.ra.w);
        rp[1] = make_uint4(o.rb, __float_as_uint(band.x), __float_as_uint(band.y), 0u);
    }
    if (gid < P.count) counts[oid] = ntiles;
    uint32_t s = block_reduce_add<kProjectBlock>(ntiles, lds);
    if (threadIdx.x == 0) blockSums[blk] = s;
}
#if !GSM_VIEWS
#undef oid
#endif
#undef GSM_PROJ_MODE
#undef GSM_PROJ_STYLE
#undef GSM_PK

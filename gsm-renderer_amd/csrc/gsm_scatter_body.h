// gsm_scatter_body.h -- the text of k_scatter, compiled four times by gsm_kernels.hip: as the single frame's
// kernel (GSM_VIEWS 0: k_scatter, exactly the kernel it was before batches of views existed), as the scatter
// of a batch of views of one scene (GSM_VIEWS 1: k_scatter_views), as the scatter of a batch of views of
// different scenes and sizes (GSM_VIEWS 2: k_scatter_batch) and as the scatter of several posed objects into
// one frame (GSM_VIEWS 3: k_scatter_compose).  No include guard.
#if GSM_VIEWS == 3
// The scatter of a composite (k_project_compose's items): every workgroup holds items of one object
// (blockObject, uniform), the items past that object's count hold no gaussian, and a tile id is the frame's own
// (no base: all objects share one tile space and one target).  Slot order within a tile and depth is ascending
// item = ascending object, then ascending gaussian id.
__global__ __launch_bounds__(kProjectBlock) void k_scatter_compose(
    ProjectArgs P, const ComposeObjectArgs* __restrict__ objects, const uint16_t* __restrict__ blockObject,
    const GaussianRenderData* __restrict__ rd, const short4* __restrict__ bounds,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ masks,
    const uint32_t* __restrict__ blockOffsets, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    const float2* __restrict__ sincos, const BlendRecord* __restrict__ rec, uint32_t fusedScan,
    TileAssignmentHeader* __restrict__ hdr, uint32_t* __restrict__ blendQueue) {
#elif GSM_VIEWS == 2
// The scatter of a batch of different views (k_project_batch's items): every workgroup holds items
// of one view (blockView, uniform), the items past that view's count hold no gaussian, a tile id is the view's
// tileBase + its local tile on the view's own grid, and the rows are [0, tilesY) of that grid.  Slot order within
// a tile is ascending item = ascending gaussian id, as the single frame's.
__global__ __launch_bounds__(kProjectBlock) void k_scatter_batch(
    ProjectArgs P, const BatchViewArgs* __restrict__ views, const uint16_t* __restrict__ blockView,
    const GaussianRenderData* __restrict__ rd, const short4* __restrict__ bounds,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ masks,
    const uint32_t* __restrict__ blockOffsets, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    const float2* __restrict__ sincos, const BlendRecord* __restrict__ rec, uint32_t fusedScan,
    TileAssignmentHeader* __restrict__ hdr, uint32_t* __restrict__ blendQueue) {
#elif GSM_VIEWS
// The scatter of a batch of views (k_project_views' items): every workgroup holds items of one
// view, the items past the view's count hold no gaussian, and a tile id is view * tilesPerView + the view's
// local tile.  Slot order within a tile is ascending item = ascending gaussian id, as the single frame's.
__global__ __launch_bounds__(kProjectBlock) void k_scatter_views(
    ProjectArgs P, uint32_t blocksPerView, uint32_t tilesPerView, const GaussianRenderData* __restrict__ rd,
    const short4* __restrict__ bounds, const uint32_t* __restrict__ counts, const uint32_t* __restrict__ masks,
    const uint32_t* __restrict__ blockOffsets, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    const float2* __restrict__ sincos, const BlendRecord* __restrict__ rec, uint32_t fusedScan,
    TileAssignmentHeader* __restrict__ hdr, uint32_t* __restrict__ blendQueue) {
#else
__global__ __launch_bounds__(kProjectBlock) void k_scatter(
    ProjectArgs P, const GaussianRenderData* __restrict__ rd, const short4* __restrict__ bounds,
    const uint32_t* __restrict__ counts, const uint32_t* __restrict__ masks,
    const uint32_t* __restrict__ blockOffsets, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals,
    const float2* __restrict__ sincos, const BlendRecord* __restrict__ rec, const uint32_t* __restrict__ devCount,
    uint32_t fusedScan, TileAssignmentHeader* __restrict__ hdr, uint32_t* __restrict__ blendQueue) {
#endif
    __shared__ uint32_t lds[kProjectBlock / 64];
    __shared__ unsigned long long lds64[kProjectBlock / 64];
    __shared__ uint32_t sOff[kProjectBlock];
    __shared__ uint32_t sMask[kProjectBlock];  // 0: no cooperative slots (large rect or no tiles)
    __shared__ uint32_t sRect[kProjectBlock];  // x0 | rw << 16 (rw <= 32)
    __shared__ uint32_t sInv[kProjectBlock];   // ceil(2^16 / rw): bit / rw = (bit * inv) >> 16 for bit < 32
    __shared__ int sTy0[kProjectBlock];        // first row index of the rect in the renderer's rows
    __shared__ uint32_t sD[kProjectBlock];     // depth bits of the key
    __shared__ float2 sBand[kProjectBlock];    // skip-flag band of each gaussian: mean x, half width (< 0: none)
    // the block's first kOwnCap slots: owner << 5 | tile bit of each small-rect slot, kNoOwner for the
    // slots of large rects (their own thread writes them); later slots take the binary search
    constexpr uint32_t kOwnCap = 4096;
    constexpr uint16_t kNoOwner = 0xFFFFu;
    __shared__ uint16_t sOwn[kOwnCap];
    const uint32_t gid = blockIdx.x * kProjectBlock + threadIdx.x;
#if GSM_VIEWS == 3
    // every item of the composite (whole blocks per object); the thread's item holds a gaussian below its
    // object's count
    const uint32_t n = gridDim.x * kProjectBlock;
    bool isItem;
    {
        const ComposeObjectArgs& V = objects[__builtin_amdgcn_readfirstlane((uint32_t)blockObject[blockIdx.x])];
        isItem = (blockIdx.x - V.blockBase) * kProjectBlock + threadIdx.x < V.count;
    }
#define GSM_TILE_ID(t) ((uint32_t)(t))
#define GSM_IS_ITEM isItem
#elif GSM_VIEWS == 2
    // every item of the batch (whole blocks per view); the thread's item holds a gaussian below its view's count
    const uint32_t n = gridDim.x * kProjectBlock;
    uint32_t tileBase;
    bool isItem;
    {
        const BatchViewArgs& V = views[__builtin_amdgcn_readfirstlane((uint32_t)blockView[blockIdx.x])];
        isItem = (blockIdx.x - V.blockBase) * kProjectBlock + threadIdx.x < V.count;
        tileBase = V.tg.tileBase;
        P.bin = V.bin;
        P.rowBegin = 0;
        P.rowEnd = V.bin.tilesY;
        P.rowStride = 1;
        P.count = V.count;
    }
#define GSM_TILE_ID(t) (tileBase + (uint32_t)(t))
#define GSM_IS_ITEM isItem
#elif GSM_VIEWS
    // every item of the batch (whole blocks per view); the thread's item holds a gaussian below the view's count
    const uint32_t n = gridDim.x * kProjectBlock;
    const uint32_t view = blockIdx.x / blocksPerView;
    const bool isItem = (blockIdx.x - view * blocksPerView) * kProjectBlock + threadIdx.x < P.count;
    const uint32_t tileBase = view * tilesPerView;
#define GSM_TILE_ID(t) (tileBase + (uint32_t)(t))
#define GSM_IS_ITEM isItem
#else
    // records path: the count lives on the device and the grid covers the capacity
    const uint32_t n = devCount ? min(*devCount, P.count) : P.count;
#define GSM_TILE_ID(t) ((uint32_t)(t))
#define GSM_IS_ITEM (gid < n)
#endif
    if (fusedScan && blockIdx.x == 0) {  // (before any exit: an empty frame still gets its header)
        const uint64_t all = block_sum_prefix(blockOffsets, (n + kProjectBlock - 1u) / kProjectBlock, lds64);
        if (threadIdx.x == 0) {
            uint32_t tot = all > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)all;
            uint32_t ovf = 0;
            if (tot > P.maxAssignments) {
                tot = P.maxAssignments;
                ovf = 1;
            }
            hdr->totalAssignments = tot;
            hdr->maxCapacity = P.maxAssignments;
            hdr->paddedCount = ((tot + 1023u) / 1024u) * 1024u;
            hdr->overflow = ovf;
            for (uint32_t q = 0; q < kQueueStripes; ++q) blendQueue[q * kQueueStride] = 0;
        }
    }
    if (blockIdx.x * kProjectBlock >= n) return;  // (uniform; the scan stopped at the count too)
    // The scatter's once-read inputs (counts, bounds, the records' band half, masks) are streaming loads
    // (nt): they no longer displace the keys and values this kernel writes from the 256 MiB infinity
    // cache, which the first tile pass reads next -- config 3: that pass 64.4-66.1 -> 59.6-61.3 us, nothing
    // else slower (r06, VERDICT r05 item 4: profiles/r06_nt_loads_ab.txt)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
#define GSM_SLD(p) __builtin_nontemporal_load(p)
    // every input of the block in flight at once, while the block counts are added up (r06: the bounds,
    // band and mask no longer wait for the count -- one memory round trip less per workgroup; a gaussian
    // without tiles reads 28 B it does not use)
    uint32_t c = 0u, mw = 0u;
    unsigned long long rb = 0ull;
    u32x4 r1v = {0u, 0u, 0u, 0u};
    if (GSM_IS_ITEM) {
        c = GSM_SLD(counts + gid);
        rb = GSM_SLD((const unsigned long long*)(bounds + gid));
        r1v = GSM_SLD((const u32x4*)(rec + gid) + 1);  // the band k_project left in the padding
        mw = GSM_SLD(masks + gid);
    }
    uint32_t base;
    if (fusedScan) {
        const uint64_t before = blockIdx.x ? block_sum_prefix(blockOffsets, blockIdx.x, lds64) : 0ull;
        base = before > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)before;
    } else {
        base = blockOffsets[blockIdx.x];
    }
    uint32_t total;
    const uint32_t off = block_exclusive_scan<kProjectBlock>(c, lds, &total);
    bool large = false;
    short4 r = make_short4(0, -1, 0, -1);
    uint32_t dbits = 0;
    int ty0 = 0, ty1 = -1;
    uint32_t mask = 0;
    float2 band = make_float2(0.0f, -1.0f);
    if (c != 0) {
        r = __builtin_bit_cast(short4, rb);
        const uint4 r1 = make_uint4(r1v.x, r1v.y, r1v.z, r1v.w);
        band = make_float2(__uint_as_float(r1.y), __uint_as_float(r1.z));
        // the key's depth: the fp16 depth bits of the blend record (b = colB | depth << 16, the same
        // bits as GaussianRenderData.depth), so the scatter reads one 16-B slot per gaussian
        dbits = ((r1.x >> 16) ^ 0x8000u) & 0xFFFFu;
        // row indices of the renderer's rows inside the rect (the keys carry local tile ids,
        // k * tilesX + tx: the sort, the tile starts and the blend count the renderer's rows only)
        rows_within(rows_of(P), (int)r.z, (int)r.w, &ty0, &ty1);
        const int rw = (int)r.y - (int)r.x + 1;
        large = (ty1 - ty0 + 1) * rw > kMaskTiles;
        if (!large) mask = mw;
        sRect[threadIdx.x] = ((uint32_t)(int)r.x & 0xFFFFu) | ((uint32_t)rw << 16);
        // 2^16 / rw is a power of two (v_rcp_f32 exact) or >= 1/rw >= 1/32 away from an integer, and the
        // 1-ulp reciprocal moves it by <= 2^16 * 2^-23 < 0.008: the ceiling is exact.  With inv = ceil(2^16
        // / rw), (bit * inv) >> 16 = bit / rw for every bit < 32 and rw <= 32 (checked exhaustively)
        sInv[threadIdx.x] = (uint32_t)__builtin_ceilf(65536.0f * __builtin_amdgcn_rcpf((float)rw));
    }
    sOff[threadIdx.x] = off;
    sMask[threadIdx.x] = mask;
    sD[threadIdx.x] = dbits;
    sTy0[threadIdx.x] = ty0;
    sBand[threadIdx.x] = band;
    const uint32_t nOwn = min(total, kOwnCap);
    for (uint32_t i = threadIdx.x; i < nOwn; i += kProjectBlock) sOwn[i] = kNoOwner;
    __syncthreads();
    {  // each small rect lists its slots (<= 32, one per set bit of its mask, in bit order)
        uint32_t m = mask;
        for (uint32_t i = off; m != 0 && i < kOwnCap; ++i) {
            sOwn[i] = (uint16_t)((threadIdx.x << 5) | (uint32_t)__builtin_ctz(m));
            m &= m - 1u;
        }
    }
    __syncthreads();
    for (uint32_t sl = threadIdx.x; sl < total; sl += kProjectBlock) {
        uint32_t lo, bit;
        if (sl < kOwnCap) {
            const uint32_t v = sOwn[sl];
            if (v == kNoOwner) continue;  // a large rect: its own thread writes it
            lo = v >> 5;
            bit = v & 31u;
        } else {
            // owner: the largest g with sOff[g] <= sl (zero-count gaussians share the next offset)
            lo = 0;
            uint32_t hi = kProjectBlock - 1;
            while (lo < hi) {
                const uint32_t mid = (lo + hi + 1) >> 1;
                if (sOff[mid] <= sl) lo = mid;
                else hi = mid - 1;
            }
            uint32_t m = sMask[lo];
            if (m == 0) continue;  // a large rect: its own thread writes it
            for (uint32_t k = sl - sOff[lo]; k > 0; --k) m &= m - 1u;
            bit = (uint32_t)__builtin_ctz(m);
        }
        const uint64_t wp = (uint64_t)base + sl;
        if (wp >= P.maxAssignments) continue;
        const uint32_t rect = sRect[lo];
        const uint32_t rwo = rect >> 16;
        const uint32_t row = (bit * sInv[lo]) >> 16;  // bit / rwo (bit < 32)
        const int k = sTy0[lo] + (int)row, tx = (int)(rect & 0xFFFFu) + (int)(bit - row * rwo);
        keys[wp] = (GSM_TILE_ID(k * (int)P.bin.tilesX + tx) << 16) | sD[lo];
        const float2 bd = sBand[lo];
        vals[wp] = (blockIdx.x * kProjectBlock + lo) | (half_skip_flags(bd.x, bd.y, tx) << kHalfSkipShift);
    }
    if (!large) return;
    uint64_t wp = (uint64_t)base + off;
    if (wp >= P.maxAssignments) return;
    // large rects: repeat the tests (tileScatterIndirectKernel, GlobalShaders.metal:623-678)
    uint4 rdw = *(const uint4*)(rd + gid);
    uint16_t hmx = (uint16_t)(rdw.x & 0xFFFFu), hmy = (uint16_t)(rdw.x >> 16);
    uint16_t thq = (uint16_t)(rdw.y & 0xFFFFu), hs1 = (uint16_t)(rdw.y >> 16);
    uint16_t hs2 = (uint16_t)(rdw.z & 0xFFFFu);
    uint32_t opac = rdw.w >> 24;
    float cx = hbits_to_f(hmx), cy = hbits_to_f(hmy);
    Conic k = conic_from_quant(sincos, thq, hbits_to_f(hs1), hbits_to_f(hs2));
    float w = 2.0f * compute_power((float)opac);
    const RowSet R = rows_of(P);
    for (int kr = ty0; kr <= ty1; ++kr)
        for (int tx = (int)r.x, ty = R.b + kr * R.s; tx <= (int)r.y; ++tx)
            if (intersects_tile(tx, ty, cx, cy, k, w)) {
                if (wp < P.maxAssignments) {
                    uint32_t tile = GSM_TILE_ID(kr * (int)P.bin.tilesX + tx);
                    keys[wp] = (tile << 16) | dbits;
                    vals[wp] = gid | (half_skip_flags(band.x, band.y, tx) << kHalfSkipShift);
                    wp++;
                }
            }
}
#undef GSM_TILE_ID
#undef GSM_IS_ITEM

/*
 * local_ref.c -- CPU restatement of the reference's LocalRenderer frame (TEST INFRASTRUCTURE).
 *
 * LocalRenderer.render -> renderView (Sources/Renderer/LocalRenderer/LocalRenderer.swift:83-257), kernels in
 * Sources/Renderer/LocalRenderer/LocalShaders.metal and Sources/Renderer/Shared/GaussianShared.h, cited per
 * function.  Written here from the Metal source line by line, like oracle/gsm_oracle.c and
 * tests/df_mono/df_mono_ref.c; it is the parity checker of gsm_local_render (include/gsm_local.h) and is
 * loaded by tests/ only.
 *
 * Every helper the Global oracle already restates is the oracle's own code: this file includes the
 * oracle's translation unit and calls its static functions (fp16 conversion and arithmetic, hfma, the exp
 * table, the covariance chain, total ink, OBB extents, SH colour, the sRGB decode, intersects_tile and
 * compute_power).  New here: computeConicAndRadius, the fp16 ProjectedGaussian record, the per-tile slot
 * lists and the 4x2 blend.
 *
 * Declared choices of this frame, the same on the GPU:
 *   - a tile's list is ordered by (depth16, compacted index): the reference execution in which every
 *     tile's slots fill in ascending index order;
 *   - a tile with more than 2048 passing gaussians keeps the 2048 of lowest index here (the GPU: some
 *     2048), sorts and walks exactly 2048, and the frame reports overflow = 1;
 *   - the saturation break is a vote over all 256 pixels of the tile, evaluated after every entry;
 *   - c += gColor * (a * T) is one FMA per channel (the contract's declared exception).
 */
#include "../../oracle/gsm_oracle.c"

#define LR_TILE 16
#define LR_MAX_PER_TILE 2048u

/* ProjectedGaussian (BridgingTypes.h:106-114), 32 B, fp16 fields as bits */
typedef struct {
    uint16_t posX, posY;
    uint16_t conicA, conicB, conicC, depth;
    uint16_t colorR, colorG;
    uint16_t colorB, opacity;
    uint16_t minTile[2], maxTile[2]; /* min inclusive, max exclusive */
    uint16_t obbExtentX, obbExtentY;
} lr_projected;

typedef struct {
    uint32_t count, width, height;
    uint32_t tiles_x, tiles_y, tile_count;
    uint32_t visible, active_tiles, total_entries, max_tile_count, max_per_tile, overflow;
    uint8_t *mask;            /* [count] 1 when visible */
    float *pre;               /* [count*5] fp32 screen x, y, conic a, b, c before packing (0 when culled) */
    lr_projected *projected;  /* [visible] compacted, gaussian order */
    int32_t *source;          /* [visible] gaussian id of each compacted record */
    uint32_t *tile_counts;    /* [tile_count] unclamped */
    uint32_t *tile_lists;     /* [tile_count*2048] compacted indices in blend order, up to min(count, 2048) */
    uint32_t *walked;         /* [tile_count] entries the tile's walk consumed */
    uint16_t *color;          /* [height][width][4] rgba16f bits */
    uint16_t *depth;          /* [height][width] r16f bits */
} lr_frame;

/* ---- localProjectStore (LocalShaders.metal:53-184) --------------------------------------- */
typedef struct {
    const og_config *cfg;
    const void *gaussians, *harmonics;
    uint32_t shk;
    const og_camera *cam;
    float W, H;
    int tiles_x, tiles_y;
    lr_frame *f;
    lr_projected *temp; /* [count] tempBuffer */
} lr_ctx;

static void lr_project_range(void *vctx, uint32_t lo, uint32_t hi) {
    lr_ctx *X = (lr_ctx *)vctx;
    lr_frame *f = X->f;
    const og_camera *cam = X->cam;
    const int half_in = X->cfg->precision == 1;
    const float W = X->W, Hh = X->H;
    const float alphaThreshold = 0.005f, totalInkThreshold = 2.0f; /* LocalRenderer.swift:165-166 */
    for (uint32_t gid = lo; gid < hi; ++gid) {
        f3 pos, scale;
        float opacity;
        f4 rot;
        f->mask[gid] = 0; /* :65-76: zero tile bounds, visibilityMarks = 0 */
        if (half_in) {
            const og_world16 *g = (const og_world16 *)X->gaussians + gid;
            pos.x = g->px; pos.y = g->py; pos.z = g->pz;
            scale.x = H(g->sx); scale.y = H(g->sy); scale.z = H(g->sz);
            opacity = H(g->opacity);
            rot.x = H(g->rx); rot.y = H(g->ry); rot.z = H(g->rz); rot.w = H(g->rw);
        } else {
            const og_world32 *g = (const og_world32 *)X->gaussians + gid;
            pos.x = g->px; pos.y = g->py; pos.z = g->pz;
            scale.x = g->sx; scale.y = g->sy; scale.z = g->sz;
            opacity = g->opacity;
            rot.x = g->rot[0]; rot.y = g->rot[1]; rot.z = g->rot[2]; rot.w = g->rot[3];
        }
        /* :70-77 cullByScale (GaussianShared.h:719-722) */
        if (fmaxf(scale.x, fmaxf(scale.y, scale.z)) < 0.0005f) continue;
        /* :79-96 */
        f4 p4 = {pos.x, pos.y, pos.z, 1.0f};
        f4 vp = mat4_mul_vec(cam->view, p4);
        f4 clip = mat4_mul_vec(cam->proj, vp);
        float depth = clip.w;
        if (!(clip.w > cam->near_plane)) continue; /* isInFrontOfCameraClipW */
        if (depth > cam->far_plane) continue;      /* cullByFarPlane (GaussianShared.h:732-734) */
        /* :98-104 */
        if (opacity < alphaThreshold) continue;
        /* :106-109 ndcToScreenCentered (GaussianShared.h:184-189) */
        float ndcx = clip.x / clip.w, ndcy = clip.y / clip.w;
        float sx = ((ndcx + 1.0f) * W - 1.0f) * 0.5f;
        float sy = ((ndcy + 1.0f) * Hh - 1.0f) * 0.5f;
        /* :111-120 */
        f4 quat = normalize_quat(rot);
        m3 cov3d = build_cov3d(scale, quat);
        f3 vp3 = {vp.x, vp.y, vp.z};
        m2 cov2d = project_cov2d(&cov3d, vp3, cam->view, cam->proj, W, Hh);
        cov2d = stabilize_cov2d(cov2d, W, Hh);
        /* :122-132 computeConicAndRadius (GaussianShared.h:390-400), cullByRadius (:727-729) */
        float a = cov2d.c[0].x, b = cov2d.c[0].y, c = cov2d.c[1].x, d = cov2d.c[1].y;
        float det = a * d - b * c;
        float invDet = 1.0f / fmaxf(det, 1e-8f);
        float conicA = d * invDet, conicB = -b * invDet, conicC = a * invDet;
        float mid = 0.5f * (a + d);
        float delta = fmaxf(mid * mid - det, 1e-5f);
        float maxEig = mid + sqrtf(delta);
        float radius = 3.0f * ceilf(sqrtf(fmaxf(maxEig, 1e-5f)));
        if (radius < 0.5f) continue;
        /* :134-140 */
        if (cull_total_ink(opacity, cov2d, depth, cam->near_plane, cam->far_plane, totalInkThreshold)) continue;
        /* :142-157 computeOBBExtents, computeTileBounds (GaussianShared.h:791-828) on 16x16 tiles */
        f2 obb = obb_extents(cov2d, 3.0f);
        float xmin = clampf(sx - obb.x, 0.0f, W - 1.0f), xmax = clampf(sx + obb.x, 0.0f, W - 1.0f);
        float ymin = clampf(sy - obb.y, 0.0f, Hh - 1.0f), ymax = clampf(sy + obb.y, 0.0f, Hh - 1.0f);
        int minTX = (int)floorf(xmin / (float)LR_TILE), maxTX = (int)ceilf(xmax / (float)LR_TILE) - 1;
        int minTY = (int)floorf(ymin / (float)LR_TILE), maxTY = (int)ceilf(ymax / (float)LR_TILE) - 1;
        if (minTX < 0) minTX = 0;
        if (minTY < 0) minTY = 0;
        if (maxTX > X->tiles_x - 1) maxTX = X->tiles_x - 1;
        if (maxTY > X->tiles_y - 1) maxTY = X->tiles_y - 1;
        if (!(minTX <= maxTX && minTY <= maxTY)) continue; /* !tb.valid */
        /* :159-162 */
        f3 camc = {cam->position[0], cam->position[1], cam->position[2]};
        f3 col = compute_sh_color(X->harmonics, half_in, gid, pos, camc, X->shk);
        col.x = fmaxf(col.x + 0.5f, 0.0f);
        col.y = fmaxf(col.y + 0.5f, 0.0f);
        col.z = fmaxf(col.z + 0.5f, 0.0f);
        if (X->cfg->color_space == 1) {
            col.x = srgb_to_linear(col.x);
            col.y = srgb_to_linear(col.y);
            col.z = srgb_to_linear(col.z);
        }
        /* :164-183 */
        lr_projected *p = &X->temp[gid];
        p->posX = og_f2h(sx); p->posY = og_f2h(sy);
        p->conicA = og_f2h(conicA); p->conicB = og_f2h(conicB); p->conicC = og_f2h(conicC);
        p->depth = og_f2h(depth);
        p->colorR = og_f2h(col.x); p->colorG = og_f2h(col.y); p->colorB = og_f2h(col.z);
        p->opacity = og_f2h(opacity);
        p->minTile[0] = (uint16_t)minTX; p->minTile[1] = (uint16_t)minTY;
        p->maxTile[0] = (uint16_t)(maxTX + 1); p->maxTile[1] = (uint16_t)(maxTY + 1);
        p->obbExtentX = og_f2h(obb.x); p->obbExtentY = og_f2h(obb.y);
        float *pre = f->pre + 5 * (size_t)gid;
        pre[0] = sx; pre[1] = sy; pre[2] = conicA; pre[3] = conicB; pre[4] = conicC;
        f->mask[gid] = 1;
    }
}

/* gaussianComputePower (GaussianShared.h:595-597) as the scatter uses it, for the tests' own tile walk */
float lr_compute_power(float opacity) { return compute_power(opacity); }

/* ---- localPerTileSort16 (LocalShaders.metal:362-437), ascending (key16, index, slot) ------- */
typedef struct { uint64_t k; } lr_key;
static int lr_key_cmp(const void *a, const void *b) {
    uint64_t x = ((const lr_key *)a)->k, y = ((const lr_key *)b)->k;
    return x < y ? -1 : (x > y ? 1 : 0);
}
/* tile t owns the slots [t * max_per_tile, (t + 1) * max_per_tile); out_local receives the sorted slots */
int lr_sort_tiles(const uint16_t *keys16, const uint32_t *indices, const uint32_t *counts, uint32_t tile_count,
                  uint32_t max_per_tile, uint16_t *out_local) {
    if (max_per_tile == 0 || max_per_tile > LR_MAX_PER_TILE) return OG_ERR_INVALID_ARGUMENT;
    lr_key *k = (lr_key *)malloc(sizeof(lr_key) * max_per_tile);
    if (!k) return OG_ERR_OUT_OF_MEMORY;
    for (uint32_t t = 0; t < tile_count; ++t) {
        size_t start = (size_t)t * max_per_tile;
        uint32_t n = counts[t] < max_per_tile ? counts[t] : max_per_tile;
        for (uint32_t i = 0; i < n; ++i)
            k[i].k = ((uint64_t)keys16[start + i] << 48) | ((uint64_t)indices[start + i] << 16) | (uint64_t)i;
        qsort(k, n, sizeof(lr_key), lr_key_cmp);
        for (uint32_t i = 0; i < n; ++i) out_local[start + i] = (uint16_t)(k[i].k & 0xFFFFu);
    }
    free(k);
    return OG_OK;
}

/* ---- localRender16 (LocalShaders.metal:440-571) for one tile ------------------------------ */
typedef struct { lr_frame *f; uint32_t *active; } lr_blend_ctx;

static void lr_blend_tiles(void *vctx, uint32_t lo, uint32_t hi) {
    lr_blend_ctx *B = (lr_blend_ctx *)vctx;
    lr_frame *f = B->f;
    const uint16_t ONE = 0x3C00u, TWO = 0x4000u;
    const uint16_t c099 = og_d2h(0.99), c01 = og_d2h(0.1), c0004 = og_d2h(0.004);
    const uint32_t W = f->width, Hh = f->height;
    for (uint32_t ai = lo; ai < hi; ++ai) {
        uint32_t tile = B->active[ai];
        uint32_t cnt = f->tile_counts[tile];
        /* the reference walks `count` entries; declared: min(count, 2048) */
        uint32_t n = cnt < LR_MAX_PER_TILE ? cnt : LR_MAX_PER_TILE;
        const uint32_t *lst = f->tile_lists + (size_t)tile * LR_MAX_PER_TILE;
        uint32_t tileX = tile % f->tiles_x, tileY = tile / f->tiles_x;
        /* 32 threads (4 x 8), 4x2 pixels each: thread th = ly * 4 + lx; pixel q = j * 4 + i */
        static _Thread_local uint16_t T[32][8], C[32][8][3], px[32][4], py[32][2];
        static _Thread_local float D[32][8];
        for (uint32_t th = 0; th < 32; ++th) {
            uint32_t baseX = tileX * LR_TILE + (th & 3u) * 4u, baseY = tileY * LR_TILE + (th >> 2) * 2u;
            for (int i = 0; i < 4; ++i) px[th][i] = og_f2h((float)(baseX + (uint32_t)i));
            for (int j = 0; j < 2; ++j) py[th][j] = og_f2h((float)(baseY + (uint32_t)j));
            for (int q = 0; q < 8; ++q) { T[th][q] = ONE; C[th][q][0] = C[th][q][1] = C[th][q][2] = 0; D[th][q] = 0.0f; }
        }
        uint32_t walked = 0;
        for (uint32_t e = 0; e < n; ++e) {
            const lr_projected *g = &f->projected[lst[e]];
            uint16_t cxx = g->conicA, cyy = g->conicC, cxy2 = hmul(TWO, g->conicB); /* :502 */
            float gDepth = H(g->depth);
            int allSat = 1;
            for (uint32_t th = 0; th < 32; ++th) {
                uint16_t a[8];
                int any = 0;
                for (int j = 0; j < 2; ++j)
                    for (int i = 0; i < 4; ++i) {
                        int q = j * 4 + i;
                        uint16_t dx = hsub(px[th][i], g->posX), dy = hsub(py[th][j], g->posY);
                        uint16_t p = hadd(hadd(hmul(hmul(dx, dx), cxx), hmul(hmul(dy, dy), cyy)),
                                          hmul(hmul(dx, dy), cxy2)); /* :509-516 */
                        a[q] = hmin(hmul(g->opacity, g_exp_h[og_f2h(-0.5f * H(p))]), c099); /* :518-525 */
                        if (H(a[q]) != 0.0f) any = 1; /* NaN != 0: not skipped, like == 0.0h */
                    }
                if (any) { /* :527 */
                    for (int q = 0; q < 8; ++q) {
                        if (D[th][q] == 0.0f && H(a[q]) > H(c01)) D[th][q] = gDepth; /* :530-537 */
                        uint16_t w = hmul(a[q], T[th][q]);
                        C[th][q][0] = hfma(g->colorR, w, C[th][q][0]); /* :539-542, the declared FMA */
                        C[th][q][1] = hfma(g->colorG, w, C[th][q][1]);
                        C[th][q][2] = hfma(g->colorB, w, C[th][q][2]);
                        T[th][q] = hmul(T[th][q], hsub(ONE, a[q])); /* :544-547 */
                    }
                }
                /* :549-551 maxT < 0.004h, voted over the tile */
                uint16_t m0 = hmax(hmax(T[th][0], T[th][1]), hmax(T[th][2], T[th][3]));
                uint16_t m1 = hmax(hmax(T[th][4], T[th][5]), hmax(T[th][6], T[th][7]));
                if (!(H(hmax(m0, m1)) < H(c0004))) allSat = 0;
            }
            walked = e + 1;
            if (allSat) break;
        }
        f->walked[tile] = walked;
        for (uint32_t th = 0; th < 32; ++th) {
            uint32_t baseX = tileX * LR_TILE + (th & 3u) * 4u, baseY = tileY * LR_TILE + (th >> 2) * 2u;
            for (int j = 0; j < 2; ++j)
                for (int i = 0; i < 4; ++i) {
                    uint32_t x = baseX + (uint32_t)i, y = baseY + (uint32_t)j;
                    if (x >= W || y >= Hh) continue;
                    int q = j * 4 + i;
                    uint16_t *o = f->color + 4 * ((size_t)y * W + x);
                    o[0] = C[th][q][0]; o[1] = C[th][q][1]; o[2] = C[th][q][2];
                    o[3] = hsub(ONE, T[th][q]);
                    f->depth[(size_t)y * W + x] = og_f2h(D[th][q]);
                }
        }
    }
}

void lr_frame_free(lr_frame *f) {
    if (!f) return;
    free(f->mask); free(f->pre); free(f->projected); free(f->source); free(f->tile_counts);
    free(f->tile_lists); free(f->walked); free(f->color); free(f->depth);
    free(f);
}

/* LocalRenderer.render -> renderView (LocalRenderer.swift:83-257). */
int lr_render(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count, uint32_t shk,
              const og_camera *cam, uint32_t width, uint32_t height, int nthreads, lr_frame **out) {
    ensure_init();
    *out = NULL;
    if (!cfg || !cam || !gaussians || !harmonics) return OG_ERR_INVALID_ARGUMENT;
    if (cfg->max_gaussians > 30000000u) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxG = cfg->max_gaussians ? cfg->max_gaussians : 1u;
    if (count == 0 || count > maxG) return OG_ERR_INVALID_GAUSSIAN_COUNT; /* guards :139-141 */
    uint32_t maxW = cfg->max_width ? cfg->max_width : 1u, maxH = cfg->max_height ? cfg->max_height : 1u;
    if (width == 0 || height == 0 || width > maxW || height > maxH) return OG_ERR_INVALID_DIMENSIONS;
    if (nthreads <= 0) nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nthreads < 1) nthreads = 1;

    lr_frame *f = (lr_frame *)calloc(1, sizeof(lr_frame));
    if (!f) return OG_ERR_OUT_OF_MEMORY;
    f->count = count;
    f->width = width;
    f->height = height;
    f->tiles_x = (width + LR_TILE - 1) / LR_TILE; /* :143-145 */
    f->tiles_y = (height + LR_TILE - 1) / LR_TILE;
    f->tile_count = f->tiles_x * f->tiles_y;
    f->max_per_tile = LR_MAX_PER_TILE;
    size_t n = count, slots = (size_t)f->tile_count * LR_MAX_PER_TILE;
    f->mask = (uint8_t *)calloc(n, 1);
    f->pre = (float *)calloc(n * 5, sizeof(float));
    f->projected = (lr_projected *)calloc(n, sizeof(lr_projected));
    f->source = (int32_t *)calloc(n, sizeof(int32_t));
    f->tile_counts = (uint32_t *)calloc(f->tile_count, sizeof(uint32_t));
    f->tile_lists = (uint32_t *)calloc(slots, sizeof(uint32_t));
    f->walked = (uint32_t *)calloc(f->tile_count, sizeof(uint32_t));
    f->color = (uint16_t *)calloc((size_t)width * height * 4, sizeof(uint16_t)); /* clear (0,0,0,0) (:27-39) */
    f->depth = (uint16_t *)calloc((size_t)width * height, sizeof(uint16_t));     /* clear 0 */
    lr_projected *temp = (lr_projected *)calloc(n, sizeof(lr_projected));
    uint16_t *keys16 = (uint16_t *)calloc(slots ? slots : 1, sizeof(uint16_t));
    uint16_t *sorted = (uint16_t *)calloc(slots ? slots : 1, sizeof(uint16_t));
    uint32_t *slotidx = (uint32_t *)calloc(slots ? slots : 1, sizeof(uint32_t));
    uint32_t *active = (uint32_t *)calloc(f->tile_count ? f->tile_count : 1, sizeof(uint32_t));
    int rc = OG_ERR_OUT_OF_MEMORY;
    if (!f->mask || !f->pre || !f->projected || !f->source || !f->tile_counts || !f->tile_lists || !f->walked ||
        !f->color || !f->depth || !temp || !keys16 || !sorted || !slotidx || !active)
        goto fail;

    lr_ctx X;
    memset(&X, 0, sizeof(X));
    X.cfg = cfg; X.gaussians = gaussians; X.harmonics = harmonics; X.shk = shk; X.cam = cam;
    X.W = (float)width; X.H = (float)height;
    X.tiles_x = (int)f->tiles_x; X.tiles_y = (int)f->tiles_y;
    X.f = f; X.temp = temp;
    parallel_for(nthreads, count, lr_project_range, &X);

    /* localCompact (:201-214): ascending gaussian order */
    uint32_t V = 0;
    for (uint32_t g = 0; g < count; ++g)
        if (f->mask[g]) { f->projected[V] = temp[g]; f->source[V] = (int32_t)g; V++; }
    f->visible = V;

    /* localScatterSimd16 (:573-667) in ascending compacted index: slot = the tile's count so far */
    for (uint32_t gi = 0; gi < V; ++gi) {
        const lr_projected *g = &f->projected[gi];
        conic3 k = {H(g->conicA), H(g->conicB), H(g->conicC)};
        float cx = H(g->posX), cy = H(g->posY);
        float power = compute_power(H(g->opacity)); /* intersectsTile (GaussianShared.h:647-653) */
        uint16_t depth16 = (uint16_t)(g->depth ^ 0x8000u);
        for (int ty = g->minTile[1]; ty < g->maxTile[1]; ++ty)
            for (int tx = g->minTile[0]; tx < g->maxTile[0]; ++tx) {
                int px0 = tx * LR_TILE, py0 = ty * LR_TILE;
                if (!intersects_tile(px0, py0, px0 + LR_TILE - 1, py0 + LR_TILE - 1, cx, cy, k, power)) continue;
                uint32_t tile = (uint32_t)ty * f->tiles_x + (uint32_t)tx;
                uint32_t slot = f->tile_counts[tile]++;
                if (slot < LR_MAX_PER_TILE) {
                    keys16[(size_t)tile * LR_MAX_PER_TILE + slot] = depth16;
                    slotidx[(size_t)tile * LR_MAX_PER_TILE + slot] = gi;
                }
            }
    }
    /* localPerTileSort16 over min(count, 2048) entries; the list in blend order */
    rc = lr_sort_tiles(keys16, slotidx, f->tile_counts, f->tile_count, LR_MAX_PER_TILE, sorted);
    if (rc != OG_OK) goto fail;
    uint32_t nact = 0;
    for (uint32_t t = 0; t < f->tile_count; ++t) {
        uint32_t c = f->tile_counts[t];
        uint32_t m = c < LR_MAX_PER_TILE ? c : LR_MAX_PER_TILE;
        size_t start = (size_t)t * LR_MAX_PER_TILE;
        for (uint32_t i = 0; i < m; ++i) f->tile_lists[start + i] = slotidx[start + sorted[start + i]];
        if (c > 0) active[nact++] = t; /* localFinalizeScanAndZero (:308-338) */
        f->total_entries += m;
        if (c > f->max_tile_count) f->max_tile_count = c;
    }
    f->active_tiles = nact;
    f->overflow = f->max_tile_count > LR_MAX_PER_TILE ? 1u : 0u;

    lr_blend_ctx B = {f, active};
    parallel_for_interleaved(nthreads, nact, lr_blend_tiles, &B);
    free(temp); free(keys16); free(sorted); free(slotidx); free(active);
    *out = f;
    return OG_OK;
fail:
    free(temp); free(keys16); free(sorted); free(slotidx); free(active);
    lr_frame_free(f);
    return rc;
}

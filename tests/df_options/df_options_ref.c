/*
 * df_options_ref.c -- CPU restatement of the DepthFirst frames under the two other constructor
 * arguments of DepthFirstRenderer.init (DepthFirstRenderer.swift:45-50): depthSortKeyPrecision
 * (.bits16 / .bits32) and tileIdPrecision (.bits16 / .bits32).  TEST INFRASTRUCTURE: the parity
 * checker of gsm_depthfirst_create_with_options (include/gsm_depthfirst.h), loaded by tests/ only.
 *
 * The projection and the blend of both frames are the existing checkers' own code: this file
 * includes tests/df_mono/df_mono_ref.c, which in turn includes oracle/gsm_oracle.c, and calls their
 * static ranges (df_project_range / df_blend_tiles, dfm_project_range / dfm_blend_tiles).  Only the
 * orchestration from the compaction onward is restated here, from og_df_render_stereo and dfm_render,
 * with the two parameters:
 *   depth_key_bits 16: visibilityScatterCompactKernel's DF_DEPTH_KEY_16 branch
 *     (DepthFirstShaders.metal:606-611), line for line in dfo_compact_key;
 *   tile_id_bits 32: the `& 0xFFFF` of the instance kernels is dropped (createInstancesKernel /
 *     createInstancesStereoKernel with 32-bit tile ids).
 * With (32, 16) both functions compute what og_df_render_stereo and dfm_render compute.
 */
#include "../df_mono/df_mono_ref.c" /* (includes ../../oracle/gsm_oracle.c) */

/* sortable_uint_to_float (DepthFirstShaders.metal:39-43) */
static inline float dfo_sortable_to_float(uint32_t v) {
    uint32_t bits = (v & 0x80000000u) ? (v ^ 0x80000000u) : ~v;
    float f;
    memcpy(&f, &bits, 4);
    return f;
}

/* visibilityScatterCompactKernel (:604-613): the key a visible gaussian is compacted with */
static inline uint32_t dfo_compact_key(uint32_t key, int depth_key_bits) {
    if (depth_key_bits == 16) {
        float depth = dfo_sortable_to_float(key);
        uint16_t depthHalf = og_f2h(depth);                  /* half(depth): round to nearest even */
        uint16_t depthBits = (uint16_t)(depthHalf ^ 0x8000u); /* as_type<ushort>(depthHalf) ^ 0x8000u */
        key = (uint32_t)depthBits;
    }
    return key;
}

/* compaction in ascending id + DepthRadixSortEncoder (a stable LSD sort; with 16-bit keys the upper
 * passes see zeros, so the order is the stable order of the 16 bits).  keys_out: [count] scratch that
 * holds the sorted keys of the V visible gaussians on return. */
static uint32_t dfo_depth_order(uint32_t count, const uint32_t *touched, const uint32_t *pre_keys,
                                int depth_key_bits, uint32_t *keys_out, int32_t *order) {
    uint32_t V = 0;
    for (uint32_t g = 0; g < count; ++g)
        if (touched[g] > 0) { keys_out[V] = dfo_compact_key(pre_keys[g], depth_key_bits); order[V] = (int32_t)g; V++; }
    og_radix_sort_pairs(keys_out, order, V);
    return V;
}

/* TileSortEncoder (a stable sort of the instances by tile id) + extractTileRangesKernel
 * (DepthFirstShaders.metal:1258-1313); cnt: [max(tile_count, 65536) + 1] zeros */
static uint32_t dfo_tile_sort_ranges(const uint32_t *tiles, const int32_t *gids, uint32_t tot, uint32_t tile_count,
                                     uint32_t *cnt, size_t ncnt, uint32_t *inst_tiles, int32_t *inst_gids,
                                     uint32_t *headers, uint32_t *active) {
    for (uint32_t i = 0; i < tot; ++i) cnt[tiles[i] + 1]++;
    for (size_t t = 0; t + 1 < ncnt; ++t) cnt[t + 1] += cnt[t];
    for (uint32_t i = 0; i < tot; ++i) {
        uint32_t p = cnt[tiles[i]]++;
        inst_tiles[p] = tiles[i];
        inst_gids[p] = gids[i];
    }
    uint32_t nact = 0;
    for (uint32_t tile = 0; tile < tile_count; ++tile) {
        if (tot == 0) { headers[2 * tile] = 0; headers[2 * tile + 1] = 0; continue; }
        uint32_t l = 0, r = tot;
        while (l < r) { uint32_t m = (l + r) >> 1; if (inst_tiles[m] < tile) l = m + 1; else r = m; }
        uint32_t s = l;
        l = s; r = tot;
        while (l < r) { uint32_t m = (l + r) >> 1; if (inst_tiles[m] <= tile) l = m + 1; else r = m; }
        headers[2 * tile] = s;
        headers[2 * tile + 1] = l > s ? l - s : 0u;
        if (l > s) active[nact++] = tile;
    }
    return nact;
}

static int dfo_bits_ok(int depth_key_bits, int tile_id_bits) {
    return (depth_key_bits == 16 || depth_key_bits == 32) && (tile_id_bits == 16 || tile_id_bits == 32);
}

void dfo_free_keys(uint32_t *keys) { free(keys); }

/* encodeStereoPipeline (DepthFirstRenderer.swift:595-831) as og_df_render_stereo, with the two options.
 * *sorted_keys: [visible] the compacted keys after the depth sort (dfo_free_keys). */
int dfo_render_stereo(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count,
                      uint32_t shk, const og_camera *left, const og_camera *right, const float *scene_transform,
                      uint32_t width, uint32_t height, int nthreads, int depth_key_bits, int tile_id_bits,
                      og_df_frame **out, uint32_t **sorted_keys) {
    ensure_init();
    *out = NULL;
    *sorted_keys = NULL;
    if (!cfg || !left || !right || (count > 0 && (!gaussians || !harmonics))) return OG_ERR_INVALID_ARGUMENT;
    if (!dfo_bits_ok(depth_key_bits, tile_id_bits)) return OG_ERR_INVALID_ARGUMENT;
    if (cfg->max_gaussians > 30000000u) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxG = cfg->max_gaussians ? cfg->max_gaussians : 1u;
    if (count > maxG) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxW = cfg->max_width ? cfg->max_width : 1u, maxH = cfg->max_height ? cfg->max_height : 1u;
    if (width == 0 || height == 0 || width > maxW || height > maxH) return OG_ERR_INVALID_DIMENSIONS;
    if (nthreads <= 0) nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nthreads < 1) nthreads = 1;
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float *scene = scene_transform ? scene_transform : identity;
    const uint32_t tile_mask = tile_id_bits == 16 ? 0xFFFFu : 0xFFFFFFFFu;

    og_df_frame *f = (og_df_frame *)calloc(1, sizeof(og_df_frame));
    if (!f) return OG_ERR_OUT_OF_MEMORY;
    f->count = count;
    f->width = width;
    f->height = height;
    f->tiles_x = (width + 15u) / 16u;
    f->tiles_y = (height + 15u) / 16u;
    f->tile_count = f->tiles_x * f->tiles_y;
    f->max_instances = 4u * maxG;
    size_t n = count ? count : 1;
    size_t ncnt = (size_t)(f->tile_count > 65536u ? f->tile_count : 65536u) + 1;
    f->render_data = (og_stereo_render_data *)calloc(n, sizeof(og_stereo_render_data));
    f->bounds = (int32_t *)calloc(n * 4, sizeof(int32_t));
    f->touched = (uint32_t *)calloc(n, sizeof(uint32_t));
    f->depth_keys = (uint32_t *)calloc(n, sizeof(uint32_t));
    f->depth_order = (int32_t *)calloc(n, sizeof(int32_t));
    f->headers = (uint32_t *)calloc((size_t)f->tile_count * 2, sizeof(uint32_t));
    f->eye_color = (uint16_t *)calloc((size_t)2 * width * height * 4, sizeof(uint16_t));
    f->color = (uint16_t *)calloc((size_t)2 * width * height * 4, sizeof(uint16_t));
    uint32_t *keys = (uint32_t *)malloc(sizeof(uint32_t) * n);
    uint32_t *cnt = (uint32_t *)calloc(ncnt, sizeof(uint32_t));
    uint32_t *active = (uint32_t *)calloc(f->tile_count ? f->tile_count : 1, sizeof(uint32_t));
    uint32_t *tiles = NULL;
    int32_t *gids = NULL;
    if (!f->render_data || !f->bounds || !f->touched || !f->depth_keys || !f->depth_order || !f->headers ||
        !f->eye_color || !f->color || !keys || !cnt || !active)
        goto fail;
    df_ctx X;
    memset(&X, 0, sizeof(X));
    X.cfg = cfg; X.gaussians = gaussians; X.harmonics = harmonics; X.shk = shk;
    X.left = left; X.right = right; X.scene = scene;
    {
        float d = scene[0] * scene[0] + scene[1] * scene[1];
        d = d + scene[2] * scene[2];
        X.scene_scale = sqrtf(d);
    }
    X.W = (float)width; X.H = (float)height;
    X.tiles_x = (int)f->tiles_x; X.tiles_y = (int)f->tiles_y;
    X.f = f;
    parallel_for(nthreads, count, df_project_range, &X);
    /* visibilityScatterCompactKernel (:589-621) + DepthRadixSortEncoder */
    uint32_t V = dfo_depth_order(count, f->touched, f->depth_keys, depth_key_bits, keys, f->depth_order);
    f->visible = V;
    /* applyDepthOrderingKernel + prefix sum + createInstancesStereoKernel (:623-640, :790-826) */
    uint64_t total = 0;
    for (uint32_t i = 0; i < V; ++i) total += f->touched[f->depth_order[i]];
    f->overflow = total > f->max_instances ? 1u : 0u;
    uint32_t tot = (uint32_t)(total > f->max_instances ? f->max_instances : total);
    f->total_instances = tot;
    size_t na = tot ? tot : 1;
    tiles = (uint32_t *)malloc(sizeof(uint32_t) * na);
    gids = (int32_t *)malloc(sizeof(int32_t) * na);
    f->inst_tiles = (uint32_t *)calloc(na, sizeof(uint32_t));
    f->inst_gids = (int32_t *)calloc(na, sizeof(int32_t));
    if (!tiles || !gids || !f->inst_tiles || !f->inst_gids) goto fail;
    uint64_t off = 0;
    for (uint32_t i = 0; i < V; ++i) {
        int32_t g = f->depth_order[i];
        const int32_t *b = f->bounds + 4 * (size_t)g;
        for (int ty = b[2]; ty <= b[3]; ++ty)
            for (int tx = b[0]; tx <= b[1]; ++tx) {
                if (off < f->max_instances) {
                    tiles[off] = (uint32_t)(ty * (int)f->tiles_x + tx) & tile_mask;
                    gids[off] = g;
                }
                off++;
            }
    }
    uint32_t nact = dfo_tile_sort_ranges(tiles, gids, tot, f->tile_count, cnt, ncnt, f->inst_tiles, f->inst_gids,
                                         f->headers, active);
    f->active_tiles = nact;
    /* clearStereoRenderTextureKernel (:1813-1823) */
    for (size_t i = 0; i < (size_t)2 * width * height; ++i) {
        f->eye_color[4 * i] = 0; f->eye_color[4 * i + 1] = 0; f->eye_color[4 * i + 2] = 0;
        f->eye_color[4 * i + 3] = 0x3C00u;
    }
    df_blend_ctx B = {f, active};
    parallel_for_interleaved(nthreads, nact, df_blend_tiles, &B);
    /* DepthFirstStereoCopyEncoder: target row y of eye e is slice e's row height-1-y */
    for (uint32_t e = 0; e < 2; ++e)
        for (uint32_t y = 0; y < height; ++y)
            memcpy(f->color + 4 * ((size_t)y * 2 * width + (size_t)e * width),
                   f->eye_color + 4 * ((size_t)e * width * height + (size_t)(height - 1 - y) * width),
                   (size_t)width * 8);
    free(cnt); free(active); free(tiles); free(gids);
    *sorted_keys = keys;
    *out = f;
    return OG_OK;
fail:
    free(keys); free(cnt); free(active); free(tiles); free(gids);
    og_df_frame_free(f);
    return OG_ERR_OUT_OF_MEMORY;
}

/* encodeRender (DepthFirstRenderer.swift:237-465) as dfm_render, with the two options. */
int dfo_render_mono(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count,
                    uint32_t shk, const og_camera *cam, uint32_t width, uint32_t height, int nthreads,
                    int depth_key_bits, int tile_id_bits, dfm_frame **out, uint32_t **sorted_keys) {
    ensure_init();
    *out = NULL;
    *sorted_keys = NULL;
    if (!cfg || !cam || !gaussians || !harmonics) return OG_ERR_INVALID_ARGUMENT;
    if (!dfo_bits_ok(depth_key_bits, tile_id_bits)) return OG_ERR_INVALID_ARGUMENT;
    if (cfg->max_gaussians > 30000000u) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxG = cfg->max_gaussians ? cfg->max_gaussians : 1u;
    if (count == 0 || count > maxG) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxW = cfg->max_width ? cfg->max_width : 1u, maxH = cfg->max_height ? cfg->max_height : 1u;
    if (width == 0 || height == 0 || width > maxW || height > maxH) return OG_ERR_INVALID_DIMENSIONS;
    if (nthreads <= 0) nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nthreads < 1) nthreads = 1;
    const uint32_t tile_mask = tile_id_bits == 16 ? 0xFFFFu : 0xFFFFFFFFu;

    dfm_frame *f = (dfm_frame *)calloc(1, sizeof(dfm_frame));
    if (!f) return OG_ERR_OUT_OF_MEMORY;
    f->count = count;
    f->width = width;
    f->height = height;
    f->tiles_x = (width + 15u) / 16u;
    f->tiles_y = (height + 15u) / 16u;
    f->tile_count = f->tiles_x * f->tiles_y;
    f->max_instances = 4u * maxG;
    size_t n = count;
    size_t ncnt = (size_t)(f->tile_count > 65536u ? f->tile_count : 65536u) + 1;
    f->render_data = (og_render_data *)calloc(n, sizeof(og_render_data));
    f->bounds = (int32_t *)calloc(n * 4, sizeof(int32_t));
    f->touched = (uint32_t *)calloc(n, sizeof(uint32_t));
    f->depth_keys = (uint32_t *)calloc(n, sizeof(uint32_t));
    f->depth_order = (int32_t *)calloc(n, sizeof(int32_t));
    f->headers = (uint32_t *)calloc((size_t)f->tile_count * 2, sizeof(uint32_t));
    f->color = (uint16_t *)calloc((size_t)width * height * 4, sizeof(uint16_t));
    f->depth = (uint16_t *)calloc((size_t)width * height, sizeof(uint16_t));
    uint32_t *keys = (uint32_t *)malloc(sizeof(uint32_t) * n);
    blend_rec *rec = (blend_rec *)calloc(n, sizeof(blend_rec));
    uint32_t *active = (uint32_t *)calloc(f->tile_count ? f->tile_count : 1, sizeof(uint32_t));
    uint32_t *cnt = (uint32_t *)calloc(ncnt, sizeof(uint32_t));
    uint32_t *tiles = NULL;
    int32_t *gids = NULL;
    if (!f->render_data || !f->bounds || !f->touched || !f->depth_keys || !f->depth_order || !f->headers ||
        !f->color || !f->depth || !keys || !rec || !active || !cnt)
        goto fail;

    dfm_ctx X;
    memset(&X, 0, sizeof(X));
    X.cfg = cfg; X.gaussians = gaussians; X.harmonics = harmonics; X.shk = shk; X.cam = cam;
    X.W = (float)width; X.H = (float)height;
    X.tiles_x = (int)f->tiles_x; X.tiles_y = (int)f->tiles_y;
    X.f = f;
    parallel_for(nthreads, count, dfm_project_range, &X);

    /* visibilityScatterCompactKernel (:589-621) + DepthRadixSortEncoder */
    uint32_t V = dfo_depth_order(count, f->touched, f->depth_keys, depth_key_bits, keys, f->depth_order);
    f->visible = V;
    /* applyDepthOrderingKernel (:623-640) + prefix sum; clamp of prepareDepthFirstDispatchKernel (:2191-2194) */
    uint64_t total = 0;
    for (uint32_t i = 0; i < V; ++i) total += f->touched[f->depth_order[i]];
    f->overflow = total > f->max_instances ? 1u : 0u;
    uint32_t tot = (uint32_t)(total > f->max_instances ? f->max_instances : total);
    f->total_instances = tot;
    size_t na = tot ? tot : 1;
    tiles = (uint32_t *)malloc(sizeof(uint32_t) * na);
    gids = (int32_t *)malloc(sizeof(int32_t) * na);
    f->inst_tiles = (uint32_t *)calloc(na, sizeof(uint32_t));
    f->inst_gids = (int32_t *)calloc(na, sizeof(int32_t));
    if (!tiles || !gids || !f->inst_tiles || !f->inst_gids) goto fail;
    /* createInstancesKernel (:642-716) */
    uint64_t off = 0;
    for (uint32_t i = 0; i < V; ++i) {
        int32_t g = f->depth_order[i];
        const int32_t *b = f->bounds + 4 * (size_t)g;
        if (b[0] > b[1] || b[2] > b[3]) continue;
        dfm_tile_test T = dfm_tile_setup(&f->render_data[g], 0.005f);
        uint64_t writeOffset = off;
        if (T.d2 >= 0.0f)
            for (int ty = b[2]; ty <= b[3]; ++ty)
                for (int tx = b[0]; tx <= b[1]; ++tx)
                    if (dfm_tile_pass(&T, tx, ty) && writeOffset < f->max_instances) {
                        tiles[writeOffset] = (uint32_t)(ty * (int)f->tiles_x + tx) & tile_mask;
                        gids[writeOffset] = g;
                        writeOffset++;
                    }
        off += f->touched[g];
    }
    uint32_t nact = dfo_tile_sort_ranges(tiles, gids, tot, f->tile_count, cnt, ncnt, f->inst_tiles, f->inst_gids,
                                         f->headers, active);
    f->active_tiles = nact;
    /* clear (:2020-2034): colour (0,0,0,1), depth 0 */
    for (size_t i = 0; i < (size_t)width * height; ++i) {
        f->color[4 * i] = 0; f->color[4 * i + 1] = 0; f->color[4 * i + 2] = 0;
        f->color[4 * i + 3] = 0x3C00u;
        f->depth[i] = 0;
    }
    /* per-entry values of depthFirstRender (:1753-1764), as dfm_render */
    for (uint32_t gid = 0; gid < count; ++gid) {
        if (f->touched[gid] == 0) continue;
        const og_render_data *g = &f->render_data[gid];
        conic3 k = conic_from_quant(g->theta, H(g->sigma1), H(g->sigma2));
        blend_rec *r = &rec[gid];
        r->mx = g->meanX;
        r->my = g->meanY;
        r->cxx = og_f2h(k.A);
        r->cyy = og_f2h(k.C);
        r->cxy2 = og_f2h(2.0f * k.B);
        r->op = og_f2h(H(og_f2h((float)g->opacity)) / 255.0f);
        r->cr = og_f2h(H(og_f2h((float)g->colorR)) / 255.0f);
        r->cg = og_f2h(H(og_f2h((float)g->colorG)) / 255.0f);
        r->cb = og_f2h(H(og_f2h((float)g->colorB)) / 255.0f);
        r->dep = g->depth;
    }
    dfm_blend_ctx B = {f, rec, active};
    parallel_for_interleaved(nthreads, nact, dfm_blend_tiles, &B);
    free(rec); free(active); free(cnt); free(tiles); free(gids);
    *sorted_keys = keys;
    *out = f;
    return OG_OK;
fail:
    free(keys); free(rec); free(active); free(cnt); free(tiles); free(gids);
    dfm_frame_free(f);
    return OG_ERR_OUT_OF_MEMORY;
}

/*
 * style_ref.c -- CPU checker of the styled frames (TEST INFRASTRUCTURE; include/gsm_renderer.h).
 *
 * It includes the pick target's checker, and through it the composite's and the oracle's translation unit.
 * sr_render restates og_render's stage sequence (as cr_render does: the projection per object, under that
 * object's camera) with ONE more stage between project_range and count_range, the style pass:
 *
 *   for a gaussian the projection left visible (mask 1), s = its state byte, S = styles[s] when s < style_count,
 *   otherwise the identity;  S.hidden: mark_culled (bounds (0,-1,0,-1), mask 0 -- count_range gives it no tile,
 *   rec_range no record);  otherwise c' = (c (255 - k) + t k + 127) / 255 on the three colour bytes and
 *   o' = (o scale + 127) / 255 on the opacity byte of its render data, in unsigned integers.
 *
 * count_range, scatter_range, rec_range, the sort, the headers and the blend are the oracle's own code and read
 * the styled bytes.  The result is an og_frame (cr_frame_free); pr_pick gives its pick.  States arrive resolved:
 * one byte per concatenated gaussian (the binding expands a NULL array's default).  Loaded by tests/ only.
 */
#include "../pick/pick_ref.c"

typedef struct {
    uint8_t tint_r, tint_g, tint_b, tint_amount, opacity_scale, hidden, pad[2];
} sr_style;

/* the two integer formulas of the rule */
uint32_t sr_tint(uint32_t c, uint32_t t, uint32_t k) { return (c * (255u - k) + t * k + 127u) / 255u; }
uint32_t sr_fade(uint32_t o, uint32_t scale) { return (o * scale + 127u) / 255u; }

typedef struct {
    og_frame *f;
    const uint8_t *states;
    const sr_style *styles;
    uint32_t style_count;
} sr_style_ctx;

static void sr_style_range(void *vctx, uint32_t lo, uint32_t hi) {
    sr_style_ctx *S = (sr_style_ctx *)vctx;
    og_frame *f = S->f;
    for (uint32_t gid = lo; gid < hi; ++gid) {
        if (!f->mask[gid]) continue;
        uint32_t s = S->states[gid];
        if (s >= S->style_count) continue; /* the identity */
        const sr_style *st = &S->styles[s];
        if (st->hidden) { mark_culled(f, gid); continue; }
        og_render_data *rd = &f->render_data[gid];
        rd->colorR = (uint8_t)sr_tint(rd->colorR, st->tint_r, st->tint_amount);
        rd->colorG = (uint8_t)sr_tint(rd->colorG, st->tint_g, st->tint_amount);
        rd->colorB = (uint8_t)sr_tint(rd->colorB, st->tint_b, st->tint_amount);
        rd->opacity = (uint8_t)sr_fade(rd->opacity, st->opacity_scale);
    }
}

/* cr_render (tests/compose/compose_ref.c) with the style pass; states: `count` bytes, styles: style_count entries */
int sr_render(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count, uint32_t shk,
              const cr_object *objects, uint32_t object_count, uint32_t width, uint32_t height,
              const uint8_t *states, const sr_style *styles, uint32_t style_count, int nthreads, og_frame **out) {
    ensure_init();
    *out = NULL;
    if (!cfg || !objects || object_count == 0 || (count > 0 && (!gaussians || !harmonics || !states)) || !styles ||
        style_count == 0 || style_count > 256)
        return OG_ERR_INVALID_ARGUMENT;
    if (cfg->max_gaussians > 30000000u) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxG = cfg->max_gaussians ? cfg->max_gaussians : 1u;
    if (count > maxG) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint64_t covered = 0; /* the objects tile [0, count) in order */
    for (uint32_t o = 0; o < object_count; ++o) {
        if (objects[o].first != covered) return OG_ERR_INVALID_ARGUMENT;
        covered += objects[o].count;
    }
    if (covered != count) return OG_ERR_INVALID_ARGUMENT;
    uint32_t maxW = cfg->max_width ? cfg->max_width : 1u;
    uint32_t maxH = cfg->max_height ? cfg->max_height : 1u;
    if (width == 0 || height == 0 || width > maxW || height > maxH) return OG_ERR_INVALID_DIMENSIONS;
    if (nthreads <= 0) nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nthreads < 1) nthreads = 1;

    og_frame *f = (og_frame *)calloc(1, sizeof(og_frame));
    if (!f) return OG_ERR_OUT_OF_MEMORY;
    f->count = count;
    f->width = width;
    f->height = height;
    f->tiles_x = (maxW + 31u) / 32u;
    f->tiles_y = (maxH + 15u) / 16u;
    f->tile_count = f->tiles_x * f->tiles_y;
    f->max_assignments = 4u * maxG;
    size_t n = count ? count : 1;
    f->render_data = (og_render_data *)calloc(n, sizeof(og_render_data));
    f->bounds = (int32_t *)calloc(n * 4, sizeof(int32_t));
    f->mask = (uint8_t *)calloc(n, 1);
    f->tile_counts = (uint32_t *)calloc(n, sizeof(uint32_t));
    f->headers = (uint32_t *)calloc((size_t)f->tile_count * 2, sizeof(uint32_t));
    f->color = (uint16_t *)calloc((size_t)width * height * 4, sizeof(uint16_t));
    f->depth = (uint16_t *)calloc((size_t)width * height, sizeof(uint16_t));
    f->group_iters = (uint32_t *)calloc((size_t)f->tile_count * 64, sizeof(uint32_t));
    uint32_t *offsets = (uint32_t *)calloc(n, sizeof(uint32_t));
    conic3 *conic = (conic3 *)calloc(n, sizeof(conic3));
    float *power = (float *)calloc(n, sizeof(float));
    if (!f->render_data || !f->bounds || !f->mask || !f->tile_counts || !f->headers || !f->color ||
        !f->depth || !f->group_iters || !offsets || !conic || !power) {
        free(offsets); free(conic); free(power);
        og_frame_free(f);
        return OG_ERR_OUT_OF_MEMORY;
    }

    frame_ctx X;
    memset(&X, 0, sizeof(X));
    X.cfg = cfg; X.gaussians = gaussians; X.harmonics = harmonics;
    X.count = count; X.shk = shk; X.cam = &objects[0].camera;
    X.width = (float)width; X.height = (float)height;
    X.tiles_x = f->tiles_x; X.tiles_y = f->tiles_y;
    X.f = f; X.offsets = offsets; X.conic = conic; X.power = power;

    for (uint32_t o = 0; o < object_count; ++o) { /* the projection per object, as cr_render */
        frame_ctx Xo = X;
        Xo.cam = &objects[o].camera;
        cr_range_ctx R = {&Xo, objects[o].first};
        parallel_for(nthreads, objects[o].count, cr_project_range, &R);
    }
    /* the style pass: the one stage this file adds */
    sr_style_ctx SC = {f, states, styles, style_count};
    parallel_for(nthreads, count, sr_style_range, &SC);
    parallel_for(nthreads, count, count_range, &X);
    uint64_t total = 0;
    uint32_t visible = 0;
    for (uint32_t i = 0; i < count; ++i) {
        offsets[i] = (uint32_t)(total > 0xFFFFFFFFull ? 0xFFFFFFFFu : total);
        total += f->tile_counts[i];
        visible += f->mask[i];
    }
    f->visible = visible;
    uint32_t tot = (uint32_t)(total > f->max_assignments ? f->max_assignments : total);
    f->overflow = total > f->max_assignments ? 1u : 0u;
    f->total_assignments = tot;
    size_t na = tot ? tot : 1;
    f->keys = (uint32_t *)calloc(na, sizeof(uint32_t));
    f->values = (int32_t *)calloc(na, sizeof(int32_t));
    f->sorted_keys = (uint32_t *)calloc(na, sizeof(uint32_t));
    f->sorted_values = (int32_t *)calloc(na, sizeof(int32_t));
    uint32_t *active = (uint32_t *)calloc(f->tile_count ? f->tile_count : 1, sizeof(uint32_t));
    blend_rec *rec = (blend_rec *)calloc(n, sizeof(blend_rec));
    if (!f->keys || !f->values || !f->sorted_keys || !f->sorted_values || !active || !rec) {
        free(offsets); free(conic); free(power); free(active); free(rec);
        og_frame_free(f);
        return OG_ERR_OUT_OF_MEMORY;
    }
    parallel_for(nthreads, count, scatter_range, &X);
    memcpy(f->sorted_keys, f->keys, sizeof(uint32_t) * tot);
    memcpy(f->sorted_values, f->values, sizeof(int32_t) * tot);
    og_radix_sort_pairs(f->sorted_keys, f->sorted_values, tot);
    uint32_t nact = 0; /* buildHeadersFromSortedKernel, as og_render */
    for (uint32_t tile = 0; tile < f->tile_count; ++tile) {
        if (tot == 0) { f->headers[2 * tile] = 0; f->headers[2 * tile + 1] = 0; continue; }
        uint32_t l = 0, r = tot;
        while (l < r) {
            uint32_t mid = (l + r) >> 1;
            if ((f->sorted_keys[mid] >> 16) < tile) l = mid + 1; else r = mid;
        }
        uint32_t s = l;
        l = s; r = tot;
        while (l < r) {
            uint32_t mid = (l + r) >> 1;
            if ((f->sorted_keys[mid] >> 16) <= tile) l = mid + 1; else r = mid;
        }
        uint32_t e = l;
        f->headers[2 * tile] = s;
        f->headers[2 * tile + 1] = e > s ? e - s : 0u;
        if (e > s) active[nact++] = tile;
    }
    f->active_tiles = nact;
    for (size_t i = 0; i < (size_t)width * height; ++i) { /* the clear value: colour (0, 0, 0, 1), depth 0 */
        f->color[4 * i + 0] = 0; f->color[4 * i + 1] = 0; f->color[4 * i + 2] = 0;
        f->color[4 * i + 3] = 0x3C00u;
        f->depth[i] = 0;
    }
    rec_ctx RC = {f, rec};
    parallel_for(nthreads, count, rec_range, &RC);
    blend_ctx B = {f, rec, active};
    parallel_for_interleaved(nthreads, nact, blend_tiles, &B);
    free(rec); free(active); free(offsets); free(conic); free(power);
    *out = f;
    return OG_OK;
}

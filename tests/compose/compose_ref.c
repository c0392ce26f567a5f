/*
 * compose_ref.c -- CPU restatement of gsm_global_render_composite (TEST INFRASTRUCTURE).
 *
 * A composite (include/gsm_renderer.h) is the Global frame of the concatenated objects, except
 * that every object is projected under its own camera.  This file includes the oracle's translation unit and
 * restates og_render (oracle/gsm_oracle.c) with that one difference: project_range runs once per object, over
 * that object's id range, with that object's camera.  In the oracle only project_range reads the camera;
 * count_range, scatter_range, rec_range, the sort, the headers and the blend are the oracle's own code, called
 * here as og_render calls them.  The gaussians arrive as one concatenated host buffer plus (first, count,
 * camera) per object; the result is an og_frame (free it with cr_frame_free), ids = concatenated ids, so ties
 * of (tile, depth16) are broken by object, then by gaussian id, as the stable sort leaves them.
 *
 * It is the parity checker of the composite and is loaded by tests/ only.
 */
#include "../../oracle/gsm_oracle.c"

typedef struct {
    uint32_t first, count; /* ids [first, first + count) of the concatenated buffers */
    og_camera camera;      /* the frame's camera seen from this object's space */
} cr_object;

typedef struct {
    frame_ctx *X;
    uint32_t first;
} cr_range_ctx;

static void cr_project_range(void *vctx, uint32_t lo, uint32_t hi) {
    cr_range_ctx *R = (cr_range_ctx *)vctx;
    project_range(R->X, R->first + lo, R->first + hi);
}

void cr_frame_free(og_frame *f) { og_frame_free(f); }

/* og_render (oracle/gsm_oracle.c) over `count` concatenated gaussians, the projection per object. */
int cr_render(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count, uint32_t shk,
              const cr_object *objects, uint32_t object_count, uint32_t width, uint32_t height, int nthreads,
              og_frame **out) {
    ensure_init();
    *out = NULL;
    if (!cfg || !objects || object_count == 0 || (count > 0 && (!gaussians || !harmonics)))
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

    /* the one difference from og_render: the projection per object, under that object's camera */
    for (uint32_t o = 0; o < object_count; ++o) {
        frame_ctx Xo = X;
        Xo.cam = &objects[o].camera;
        cr_range_ctx R = {&Xo, objects[o].first};
        parallel_for(nthreads, objects[o].count, cr_project_range, &R);
    }
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
    /* buildHeadersFromSortedKernel, as og_render */
    uint32_t nact = 0;
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
    /* the clear value: colour (0, 0, 0, 1), depth 0 */
    for (size_t i = 0; i < (size_t)width * height; ++i) {
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

/*
 * ortho_ref.c -- CPU checker of the orthographic frames (TEST INFRASTRUCTURE; include/gsm_renderer.h).
 *
 * It includes gsm_global_render_frame's checker, and through it the styled frames', the pick target's, the
 * composite's and the oracle's translation unit, so it calls their static functions.  xr_render restates sr_render's
 * stage sequence (tests/style/style_ref.c: the projection per object under that object's camera, the style pass,
 * then the oracle's own count_range, scatter_range, sort, headers, rec_range and blend) with ONE difference: the
 * projection is xr_project_range, project_range (oracle/gsm_oracle.c) restated with the orthographic rule at the four
 * places where it differs from the perspective one --
 *
 *   depth   d = sigma * vp.z, sigma = +1 when proj[10] >= 0 and -1 otherwise; the near cull is !(d > near) and d
 *           replaces clip.w in cull_total_ink's depth and in rd.depth = f2h(d) (the sort key, the depth target);
 *   screen  ndcx = clip.x, ndcy = clip.y: no division;
 *   cov     J = diag(W * proj[0] * 0.5f, H * proj[5] * 0.5f), every other entry 0; T = J * W3, T * C3 * T^T and
 *           + 0.3f on the diagonal by project_cov2d's own mat3_mul sequence;
 *   colour  compute_sh_color's d0 = cam - pos becomes the uniform d0 = -sigma * (view[2], view[6], view[10]),
 *           normalised by the same normalize3; cam.position is not read.
 *
 * With orthographic == 0 the same restated text takes the perspective branch at those four places, and the frame
 * must be og_render's byte for byte: that guards the restatement (tests/test_ortho_ref.py).  The result is an
 * og_frame (cr_frame_free); pr_pick gives its pick and fr_walk the occluded walk with its pick.  Loaded by tests/ only.
 */
#include "../frame/frame_ref.c"

/* project_cov2d (oracle/gsm_oracle.c) with the orthographic J */
static m2 xr_project_cov2d_ortho(const m3 *cov3d, const float *view, const float *proj, float sw, float sh) {
    m3 W;
    for (int c = 0; c < 3; ++c) {
        W.c[c].x = view[c * 4 + 0];
        W.c[c].y = view[c * 4 + 1];
        W.c[c].z = view[c * 4 + 2];
    }
    m3 J;
    J.c[0].x = sw * proj[0] * 0.5f; J.c[0].y = 0.0f; J.c[0].z = 0.0f;
    J.c[1].x = 0.0f; J.c[1].y = sh * proj[5] * 0.5f; J.c[1].z = 0.0f;
    J.c[2].x = 0.0f; J.c[2].y = 0.0f; J.c[2].z = 0.0f;
    m3 T = mat3_mul(&J, &W);
    m3 M1 = mat3_mul(&T, cov3d);
    m3 Tt = mat3_transpose(&T);
    m3 F = mat3_mul(&M1, &Tt);
    m2 c2;
    c2.c[0].x = F.c[0].x; c2.c[0].y = F.c[0].y;
    c2.c[1].x = F.c[1].x; c2.c[1].y = F.c[1].y;
    c2.c[0].x = c2.c[0].x + 0.3f;
    c2.c[1].y = c2.c[1].y + 0.3f;
    return c2;
}

typedef struct {
    frame_ctx *X;
    uint32_t first;
    int orthographic;
} xr_range_ctx;

/* project_range restated; `orthographic` chooses the rule at the four marked places */
static void xr_project_range(void *vctx, uint32_t lo0, uint32_t hi0) {
    xr_range_ctx *R = (xr_range_ctx *)vctx;
    frame_ctx *X = R->X;
    const int ortho = R->orthographic;
    const uint32_t lo = R->first + lo0, hi = R->first + hi0;
    og_frame *f = X->f;
    const og_camera *cam = X->cam;
    const int half_in = X->cfg->precision == 1;
    const float W = X->width, Hh = X->height;
    const float alphaThreshold = 0.005f, totalInkThreshold = 2.0f;
    const int tileW = 32, tileH = 16;
    const float sigma = cam->proj[10] >= 0.0f ? 1.0f : -1.0f;
    for (uint32_t gid = lo; gid < hi; ++gid) {
        f3 pos, scale;
        float opacity;
        f4 rot;
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
        if (fmaxf(scale.x, fmaxf(scale.y, scale.z)) < 0.0005f) { mark_culled(f, gid); continue; }
        f4 p4 = {pos.x, pos.y, pos.z, 1.0f};
        f4 vp = mat4_mul_vec(cam->view, p4);
        f4 clip = mat4_mul_vec(cam->proj, vp);
        float depth = ortho ? sigma * vp.z : clip.w;                      /* (1) depth */
        if (!(depth > cam->near_plane)) { mark_culled(f, gid); continue; }
        float ndcx = ortho ? clip.x : clip.x / clip.w;                    /* (2) screen position */
        float ndcy = ortho ? clip.y : clip.y / clip.w;
        float sx = ((ndcx + 1.0f) * W - 1.0f) * 0.5f;
        float sy = ((ndcy + 1.0f) * Hh - 1.0f) * 0.5f;
        if (opacity < alphaThreshold) { mark_culled(f, gid); continue; }
        f4 quat = normalize_quat(rot);
        m3 cov3d = build_cov3d(scale, quat);
        f3 vp3 = {vp.x, vp.y, vp.z};
        m2 cov2d = ortho ? xr_project_cov2d_ortho(&cov3d, cam->view, cam->proj, W, Hh) /* (3) covariance */
                         : project_cov2d(&cov3d, vp3, cam->view, cam->proj, W, Hh);
        cov2d = stabilize_cov2d(cov2d, W, Hh);
        float theta, s1, s2;
        if (!cov_to_theta_sigmas(cov2d, &theta, &s1, &s2)) { mark_culled(f, gid); continue; }
        float radius = 3.0f * fmaxf(s1, s2);
        if (radius < 0.5f) { mark_culled(f, gid); continue; }
        if (cull_total_ink(opacity, cov2d, depth, cam->near_plane, cam->far_plane, totalInkThreshold)) {
            mark_culled(f, gid);
            continue;
        }
        f2 obb = obb_extents(cov2d, 3.0f);
        if (sx + obb.x < 0.0f || sx - obb.x > W || sy + obb.y < 0.0f || sy - obb.y > Hh) {
            mark_culled(f, gid);
            continue;
        }
        f3 col;
        if (ortho) {                                                      /* (4) colour: a parallel ray */
            /* compute_sh_color forms d0 = cam - pos and normalises it: with pos = 0 and cam = the uniform d0 the
             * difference is d0 itself (x - 0 is exact), so the oracle's own function evaluates the rule */
            f3 d0 = {-sigma * cam->view[2], -sigma * cam->view[6], -sigma * cam->view[10]};
            f3 zero = {0.0f, 0.0f, 0.0f};
            col = compute_sh_color(X->harmonics, half_in, gid, zero, d0, X->shk);
        } else {
            f3 camc = {cam->position[0], cam->position[1], cam->position[2]};
            col = compute_sh_color(X->harmonics, half_in, gid, pos, camc, X->shk);
        }
        col.x = fmaxf(col.x + 0.5f, 0.0f);
        col.y = fmaxf(col.y + 0.5f, 0.0f);
        col.z = fmaxf(col.z + 0.5f, 0.0f);
        if (X->cfg->color_space == 1) {
            col.x = srgb_to_linear(col.x);
            col.y = srgb_to_linear(col.y);
            col.z = srgb_to_linear(col.z);
        }
        og_render_data rd;
        rd.meanX = og_f2h(sx);
        rd.meanY = og_f2h(sy);
        rd.theta = pack_theta_pi(theta);
        rd.sigma1 = og_f2h(s1);
        rd.sigma2 = og_f2h(s2);
        rd.depth = og_f2h(depth);
        rd.colorR = (uint8_t)clampf(col.x * 255.0f, 0.0f, 255.0f);
        rd.colorG = (uint8_t)clampf(col.y * 255.0f, 0.0f, 255.0f);
        rd.colorB = (uint8_t)clampf(col.z * 255.0f, 0.0f, 255.0f);
        rd.opacity = (uint8_t)clampf(opacity * 255.0f, 0.0f, 255.0f);
        f->render_data[gid] = rd;
        float xmin = sx - obb.x, xmax = sx + obb.x, ymin = sy - obb.y, ymax = sy + obb.y;
        float maxW = W - 1.0f, maxH = Hh - 1.0f;
        xmin = clampf(xmin, 0.0f, maxW);
        xmax = clampf(xmax, 0.0f, maxW);
        ymin = clampf(ymin, 0.0f, maxH);
        ymax = clampf(ymax, 0.0f, maxH);
        int minTX = (int)floorf(xmin / (float)tileW);
        int maxTX = (int)ceilf(xmax / (float)tileW) - 1;
        int minTY = (int)floorf(ymin / (float)tileH);
        int maxTY = (int)ceilf(ymax / (float)tileH) - 1;
        if (minTX < 0) minTX = 0;
        if (minTY < 0) minTY = 0;
        if (maxTX > (int)X->tiles_x - 1) maxTX = (int)X->tiles_x - 1;
        if (maxTY > (int)X->tiles_y - 1) maxTY = (int)X->tiles_y - 1;
        int32_t *b = f->bounds + 4 * (size_t)gid;
        b[0] = minTX; b[1] = maxTX; b[2] = minTY; b[3] = maxTY;
        f->mask[gid] = 1;
    }
}

/* sr_render (tests/style/style_ref.c) with xr_project_range; orthographic: the frame's flag, for every object */
int xr_render(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count, uint32_t shk,
              const cr_object *objects, uint32_t object_count, uint32_t width, uint32_t height,
              const uint8_t *states, const sr_style *styles, uint32_t style_count, int orthographic, int nthreads,
              og_frame **out) {
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

    for (uint32_t o = 0; o < object_count; ++o) { /* the projection per object: sigma, J and d0 are the object's */
        frame_ctx Xo = X;
        Xo.cam = &objects[o].camera;
        xr_range_ctx R = {&Xo, objects[o].first, orthographic};
        parallel_for(nthreads, objects[o].count, xr_project_range, &R);
    }
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

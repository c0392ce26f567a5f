/*
 * df_mono_ref.c -- CPU restatement of the reference's DepthFirst MONO frame (TEST INFRASTRUCTURE).
 *
 * DepthFirstRenderer.render(commandBuffer:colorTexture:depthTexture:input:camera:width:height:)
 * (Sources/Renderer/DepthFirstRenderer/DepthFirstRenderer.swift:166-203 -> encodeRender :237-465),
 * kernels in Sources/Renderer/DepthFirstRenderer/DepthFirstShaders.metal and
 * Sources/Renderer/Shared/GaussianShared.h, cited per function.  Written here from the Metal
 * source line by line, like oracle/gsm_oracle.c; it is the parity checker of
 * gsm_depthfirst_render (include/gsm_depthfirst.h) and is loaded by tests/ only.
 *
 * Every helper the Global oracle already restates is the oracle's own code: this file includes
 * the oracle's translation unit and calls its static functions (fp16 conversion and arithmetic,
 * hfma, the exp table, the covariance chain, theta / sigmas, total ink, OBB extents, SH colour,
 * the sRGB decode, the quantised-angle conic, the radix sort).  The oracle has no callable
 * computeTileBounds (it is written out inside its projection loops), so those few lines are
 * written out here as well, on 16x16 tiles.
 *
 * New numeric choices of this frame ("DepthFirst mono"), the same on the GPU
 * (gsm_device.h mono_tile_setup / mono_tile_pass):
 *   - log(x) := ln2 * log2(x) with the contract's log2 (ogm_log2f), ln2 = 0.693147180559945f;
 *   - sin / cos of the quantised theta: the contract's 65536-entry table (g_sin_t / g_cos_t);
 *   - min, max, clamp: fminf / fmaxf (a NaN operand yields the other operand);
 *     clamp(v, lo, hi) = fminf(fmaxf(v, lo), hi).
 */
#include "../../oracle/gsm_oracle.c"

typedef struct {
    uint32_t count, width, height;
    uint32_t tiles_x, tiles_y, tile_count, max_instances;
    uint32_t visible, total_instances, overflow, active_tiles;
    og_render_data *render_data; /* [count]; culled entries zero-filled */
    int32_t *bounds;      /* [count*4] tile rect, (0,-1,0,-1) when no tile passes */
    uint32_t *touched;    /* [count] tiles of the rect that pass the per-tile test */
    uint32_t *depth_keys; /* [count] float_to_sortable_uint(clip w), 0xFFFFFFFF when culled */
    int32_t *depth_order; /* [visible] */
    uint32_t *inst_tiles; /* [total_instances] after the stable tile sort */
    int32_t *inst_gids;   /* [total_instances] */
    uint32_t *headers;    /* [tile_count*2] {offset, count} */
    uint16_t *color;      /* [height][width][4] rgba16f bits */
    uint16_t *depth;      /* [height][width] r16f bits */
} dfm_frame;

/* ---- the per-tile test on the quantised record ------------------------------------------- */
typedef struct {
    float mx, my, a, b, c, d2;
} dfm_tile_test;

/* evalQuad (GaussianShared.h:518-520) */
static inline float dfm_eval_quad(float x, float y, float a, float b, float c) {
    return a * x * x + 2.0f * b * x * y + c * y * y;
}

/* minQuadRect (GaussianShared.h:525-564) */
static float dfm_min_quad_rect(float xmin, float xmax, float ymin, float ymax, float a, float b, float c) {
    if (xmin <= 0.0f && 0.0f <= xmax && ymin <= 0.0f && 0.0f <= ymax) return 0.0f;
    float invA = 1.0f / fmaxf(a, 1e-20f);
    float invC = 1.0f / fmaxf(c, 1e-20f);
    float qmin = INFINITY;
    {
        float x = xmin;
        float y = clampf(-(b * invC) * x, ymin, ymax);
        qmin = fminf(qmin, dfm_eval_quad(x, y, a, b, c));
    }
    {
        float x = xmax;
        float y = clampf(-(b * invC) * x, ymin, ymax);
        qmin = fminf(qmin, dfm_eval_quad(x, y, a, b, c));
    }
    {
        float y = ymin;
        float x = clampf(-(b * invA) * y, xmin, xmax);
        qmin = fminf(qmin, dfm_eval_quad(x, y, a, b, c));
    }
    {
        float y = ymax;
        float x = clampf(-(b * invA) * y, xmin, xmax);
        qmin = fminf(qmin, dfm_eval_quad(x, y, a, b, c));
    }
    return qmin;
}

/* computeD2Cutoff (GaussianShared.h:590-593); log := ln2 * log2 (numeric contract) */
static float dfm_d2_cutoff(float opacity, float tau) {
    if (opacity < tau) return -1.0f;
    const float LN2 = 0.693147180559945f;
    return -2.0f * (LN2 * ogm_log2f(tau / opacity));
}

/* the quantised values both kernels rebuild from GaussianRenderData
 * (DepthFirstShaders.metal:166-179 and :668-684) + conicFromSigmaTheta (GaussianShared.h:569-585) */
static dfm_tile_test dfm_tile_setup(const og_render_data *g, float alphaThreshold) {
    dfm_tile_test T;
    T.mx = H(g->meanX);
    T.my = H(g->meanY);
    float sigma1 = H(g->sigma1), sigma2 = H(g->sigma2);
    float opacity = (float)g->opacity * (1.0f / 255.0f);
    float s = g_sin_t[g->theta], c = g_cos_t[g->theta]; /* unpackThetaPi + fast::sincos */
    float invS1sq = 1.0f / fmaxf(sigma1 * sigma1, 1e-12f);
    float invS2sq = 1.0f / fmaxf(sigma2 * sigma2, 1e-12f);
    float cc = c * c, ss = s * s, cs = c * s;
    T.a = cc * invS1sq + ss * invS2sq;
    T.c = ss * invS1sq + cc * invS2sq;
    T.b = cs * (invS1sq - invS2sq);
    float tau = fmaxf(alphaThreshold, 1e-12f);
    T.d2 = dfm_d2_cutoff(opacity, tau);
    return T;
}

/* one iteration of the tile loops (DepthFirstShaders.metal:186-204, :693-713) */
static inline int dfm_tile_pass(const dfm_tile_test *T, int tx, int ty) {
    if (!(T->d2 >= 0.0f)) return 0;
    float tileMinY = (float)ty * 16.0f, tileMaxY = tileMinY + 16.0f;
    float tile_ymin = tileMinY - T->my, tile_ymax = tileMaxY - T->my;
    float tileMinX = (float)tx * 16.0f, tileMaxX = tileMinX + 16.0f;
    float tile_xmin = tileMinX - T->mx, tile_xmax = tileMaxX - T->mx;
    float d2min = dfm_min_quad_rect(tile_xmin, tile_xmax, tile_ymin, tile_ymax, T->a, T->b, T->c);
    return d2min <= T->d2;
}

/* ---- depthFirstProjectCullKernel (DepthFirstShaders.metal:46-219) ------------------------- */
typedef struct {
    const og_config *cfg;
    const void *gaussians, *harmonics;
    uint32_t shk;
    const og_camera *cam;
    float W, H;
    int tiles_x, tiles_y;
    dfm_frame *f;
} dfm_ctx;

static void dfm_mark_culled(dfm_frame *f, uint32_t gid) {
    int32_t *b = f->bounds + 4 * (size_t)gid;
    b[0] = 0; b[1] = -1; b[2] = 0; b[3] = -1;
    f->touched[gid] = 0;
    /* the reference leaves preDepthKeys unwritten on the returns of :111-122 and :133-137;
     * defined as 0xFFFFFFFF (include/gsm_depthfirst.h) */
    f->depth_keys[gid] = 0xFFFFFFFFu;
}

static void dfm_project_range(void *vctx, uint32_t lo, uint32_t hi) {
    dfm_ctx *X = (dfm_ctx *)vctx;
    dfm_frame *f = X->f;
    const og_camera *cam = X->cam;
    const int half_in = X->cfg->precision == 1;
    const float W = X->W, Hh = X->H;
    const float alphaThreshold = 0.005f, totalInkThreshold = 2.0f; /* GlobalRenderer.swift:54-69 */
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
        /* :63-69 cullByScale (GaussianShared.h:719-722) */
        if (fmaxf(scale.x, fmaxf(scale.y, scale.z)) < 0.0005f) { dfm_mark_culled(f, gid); continue; }
        /* :71-87 */
        f4 p4 = {pos.x, pos.y, pos.z, 1.0f};
        f4 vp = mat4_mul_vec(cam->view, p4);
        f4 clip = mat4_mul_vec(cam->proj, vp);
        float depth = clip.w;
        if (!(clip.w > cam->near_plane)) { dfm_mark_culled(f, gid); continue; } /* isInFrontOfCameraClipW */
        if (depth > cam->far_plane) { dfm_mark_culled(f, gid); continue; }      /* cullByFarPlane (:732-734) */
        /* :89-91 ndcToScreen (GaussianShared.h:150-155): no pixel-centre shift */
        float ndcx = clip.x / clip.w, ndcy = clip.y / clip.w;
        float sx = (ndcx + 1.0f) * 0.5f * W;
        float sy = (ndcy + 1.0f) * 0.5f * Hh;
        /* :93-99 */
        if (opacity < alphaThreshold) { dfm_mark_culled(f, gid); continue; }
        /* :101-122 */
        f4 quat = normalize_quat(rot);
        m3 cov3d = build_cov3d(scale, quat);
        f3 vp3 = {vp.x, vp.y, vp.z};
        m2 cov2d = project_cov2d(&cov3d, vp3, cam->view, cam->proj, W, Hh);
        cov2d = stabilize_cov2d(cov2d, W, Hh);
        float theta, s1, s2;
        if (!cov_to_theta_sigmas(cov2d, &theta, &s1, &s2)) { dfm_mark_culled(f, gid); continue; }
        float radius = 3.0f * fmaxf(s1, s2);
        if (radius < 0.5f) { dfm_mark_culled(f, gid); continue; } /* cullByRadius */
        /* :124-129 */
        if (cull_total_ink(opacity, cov2d, depth, cam->near_plane, cam->far_plane, totalInkThreshold)) {
            dfm_mark_culled(f, gid);
            continue;
        }
        /* :131-137 */
        f2 obb = obb_extents(cov2d, 3.0f);
        if (sx + obb.x < 0.0f || sx - obb.x > W || sy + obb.y < 0.0f || sy - obb.y > Hh) {
            dfm_mark_culled(f, gid);
            continue;
        }
        /* :139-154 */
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
        /* :157-164 computeTileBounds (GaussianShared.h:791-828), 16x16 tiles */
        float xmin = clampf(sx - obb.x, 0.0f, W - 1.0f), xmax = clampf(sx + obb.x, 0.0f, W - 1.0f);
        float ymin = clampf(sy - obb.y, 0.0f, Hh - 1.0f), ymax = clampf(sy + obb.y, 0.0f, Hh - 1.0f);
        int minTX = (int)floorf(xmin / 16.0f), maxTX = (int)ceilf(xmax / 16.0f) - 1;
        int minTY = (int)floorf(ymin / 16.0f), maxTY = (int)ceilf(ymax / 16.0f) - 1;
        if (minTX < 0) minTX = 0;
        if (minTY < 0) minTY = 0;
        if (maxTX > X->tiles_x - 1) maxTX = X->tiles_x - 1;
        if (maxTY > X->tiles_y - 1) maxTY = X->tiles_y - 1;
        /* :166-205 */
        dfm_tile_test T = dfm_tile_setup(&rd, alphaThreshold);
        uint32_t touchedCount = 0;
        if (T.d2 >= 0.0f)
            for (int ty = minTY; ty <= maxTY; ++ty)
                for (int tx = minTX; tx <= maxTX; ++tx)
                    if (dfm_tile_pass(&T, tx, ty)) touchedCount++;
        /* :207-216 */
        if (touchedCount == 0) { dfm_mark_culled(f, gid); continue; }
        int32_t *b = f->bounds + 4 * (size_t)gid;
        b[0] = minTX; b[1] = maxTX; b[2] = minTY; b[3] = maxTY;
        f->depth_keys[gid] = df_sortable(depth);
        f->touched[gid] = touchedCount;
    }
}

/* ---- depthFirstRender (DepthFirstShaders.metal:1703-1811) for one active tile -------------- */
typedef struct { dfm_frame *f; blend_rec *rec; uint32_t *active; } dfm_blend_ctx;

static void dfm_blend_tiles(void *vctx, uint32_t lo, uint32_t hi) {
    dfm_blend_ctx *B = (dfm_blend_ctx *)vctx;
    dfm_frame *f = B->f;
    const uint16_t ONE = 0x3C00u;
    const uint16_t thr = og_f2h(1.0f / 255.0f); /* half(1.0h/255.0h) */
    const uint16_t c099 = og_d2h(0.99);
    const uint32_t W = f->width, Hh = f->height;
    for (uint32_t ai = lo; ai < hi; ++ai) {
        uint32_t tile = B->active[ai];
        uint32_t start = f->headers[2 * tile], count = f->headers[2 * tile + 1];
        uint32_t tileX = tile % f->tiles_x, tileY = tile / f->tiles_x;
        for (uint32_t ly = 0; ly < 8; ++ly)
            for (uint32_t lx = 0; lx < 8; ++lx) {
                uint32_t baseX = tileX * 16 + lx * 2, baseY = tileY * 16 + ly * 2;
                /* pixel q = (q & 1, q >> 1): 00, 10, 01, 11 */
                uint16_t px[4], py[4];
                for (int q = 0; q < 4; ++q) {
                    px[q] = og_f2h((float)(baseX + (uint32_t)(q & 1)));
                    py[q] = og_f2h((float)(baseY + (uint32_t)(q >> 1)));
                }
                uint16_t T[4], C[4][3], D[4];
                for (int q = 0; q < 4; ++q) { T[q] = ONE; C[q][0] = C[q][1] = C[q][2] = 0; D[q] = 0; }
                for (uint32_t i = 0; i < count; ++i) {
                    uint16_t mt = hmax(hmax(T[0], T[1]), hmax(T[2], T[3]));
                    if (H(mt) < H(thr)) break;
                    int32_t gi = f->inst_gids[start + i];
                    if (gi < 0) continue;
                    const blend_rec *g = &B->rec[gi];
                    uint16_t a[4];
                    int any = 0;
                    for (int q = 0; q < 4; ++q) {
                        uint16_t dx = hsub(px[q], g->mx), dy = hsub(py[q], g->my);
                        uint16_t p = hadd(hadd(hmul(hmul(dx, dx), g->cxx), hmul(hmul(dy, dy), g->cyy)),
                                          hmul(hmul(dx, dy), g->cxy2));
                        a[q] = hmin(hmul(g->op, g_exp_h[og_f2h(-0.5f * H(p))]), c099);
                        if (H(a[q]) != 0.0f) any = 1;
                    }
                    if (!any) continue;
                    for (int q = 0; q < 4; ++q) {
                        uint16_t w = hmul(a[q], T[q]);
                        C[q][0] = hfma(g->cr, w, C[q][0]);
                        C[q][1] = hfma(g->cg, w, C[q][1]);
                        C[q][2] = hfma(g->cb, w, C[q][2]);
                        D[q] = hfma(g->dep, w, D[q]);
                        T[q] = hmul(T[q], hsub(ONE, a[q]));
                    }
                }
                for (int q = 0; q < 4; ++q) {
                    uint32_t x = baseX + (uint32_t)(q & 1), y = baseY + (uint32_t)(q >> 1);
                    if (x >= W || y >= Hh) continue;
                    uint16_t *o = f->color + 4 * ((size_t)y * W + x);
                    o[0] = C[q][0]; o[1] = C[q][1]; o[2] = C[q][2];
                    o[3] = hsub(ONE, T[q]);
                    f->depth[(size_t)y * W + x] = D[q];
                }
            }
    }
}

void dfm_frame_free(dfm_frame *f) {
    if (!f) return;
    free(f->render_data); free(f->bounds); free(f->touched); free(f->depth_keys);
    free(f->depth_order); free(f->inst_tiles); free(f->inst_gids); free(f->headers);
    free(f->color); free(f->depth);
    free(f);
}

/* DepthFirstRenderer.render -> encodeRender (DepthFirstRenderer.swift:166-203, 237-465). */
int dfm_render(const og_config *cfg, const void *gaussians, const void *harmonics, uint32_t count,
               uint32_t shk, const og_camera *cam, uint32_t width, uint32_t height, int nthreads,
               dfm_frame **out) {
    ensure_init();
    *out = NULL;
    if (!cfg || !cam || !gaussians || !harmonics) return OG_ERR_INVALID_ARGUMENT;
    if (cfg->max_gaussians > 30000000u) return OG_ERR_INVALID_GAUSSIAN_COUNT;
    uint32_t maxG = cfg->max_gaussians ? cfg->max_gaussians : 1u;
    if (count == 0 || count > maxG) return OG_ERR_INVALID_GAUSSIAN_COUNT; /* encodeRender guard :249 */
    uint32_t maxW = cfg->max_width ? cfg->max_width : 1u, maxH = cfg->max_height ? cfg->max_height : 1u;
    if (width == 0 || height == 0 || width > maxW || height > maxH) return OG_ERR_INVALID_DIMENSIONS;
    if (nthreads <= 0) nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    if (nthreads < 1) nthreads = 1;

    dfm_frame *f = (dfm_frame *)calloc(1, sizeof(dfm_frame));
    if (!f) return OG_ERR_OUT_OF_MEMORY;
    f->count = count;
    f->width = width;
    f->height = height;
    f->tiles_x = (width + 15u) / 16u; /* :251-253 */
    f->tiles_y = (height + 15u) / 16u;
    f->tile_count = f->tiles_x * f->tiles_y;
    f->max_instances = 4u * maxG; /* DepthFirstResources.swift:399 */
    size_t n = count;
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
    uint32_t *cnt = (uint32_t *)calloc((size_t)f->tile_count + 1, sizeof(uint32_t));
    uint32_t *tiles = NULL;
    int32_t *gids = NULL;
    int rc = OG_ERR_OUT_OF_MEMORY;
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

    /* visibilityScatterCompactKernel (DepthFirstShaders.metal:589-621): ascending gid */
    uint32_t V = 0;
    for (uint32_t g = 0; g < count; ++g)
        if (f->touched[g] > 0) { keys[V] = f->depth_keys[g]; f->depth_order[V] = (int32_t)g; V++; }
    f->visible = V;
    /* DepthRadixSortEncoder, 32-bit keys: stable LSD */
    og_radix_sort_pairs(keys, f->depth_order, V);
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
                        tiles[writeOffset] = (uint32_t)(ty * (int)f->tiles_x + tx) & 0xFFFFu; /* ushort */
                        gids[writeOffset] = g;
                        writeOffset++;
                    }
        off += f->touched[g]; /* instanceOffsets: the prefix sum of nTouchedTiles in depth order */
    }
    /* TileSortEncoder: stable sort of the instances by tile id */
    for (uint32_t i = 0; i < tot; ++i) cnt[tiles[i] + 1]++;
    for (uint32_t t = 0; t < f->tile_count; ++t) cnt[t + 1] += cnt[t];
    for (uint32_t i = 0; i < tot; ++i) {
        uint32_t p = cnt[tiles[i]]++;
        f->inst_tiles[p] = tiles[i];
        f->inst_gids[p] = gids[i];
    }
    /* extractTileRangesKernel (:1258-1313) */
    uint32_t nact = 0;
    for (uint32_t tile = 0; tile < f->tile_count; ++tile) {
        if (tot == 0) { f->headers[2 * tile] = 0; f->headers[2 * tile + 1] = 0; continue; }
        uint32_t l = 0, r = tot;
        while (l < r) { uint32_t m = (l + r) >> 1; if (f->inst_tiles[m] < tile) l = m + 1; else r = m; }
        uint32_t s = l;
        l = s; r = tot;
        while (l < r) { uint32_t m = (l + r) >> 1; if (f->inst_tiles[m] <= tile) l = m + 1; else r = m; }
        f->headers[2 * tile] = s;
        f->headers[2 * tile + 1] = l > s ? l - s : 0u;
        if (l > s) active[nact++] = tile;
    }
    f->active_tiles = nact;
    /* clear (:2020-2034): colour (0,0,0,1), depth 0 */
    for (size_t i = 0; i < (size_t)width * height; ++i) {
        f->color[4 * i] = 0; f->color[4 * i + 1] = 0; f->color[4 * i + 2] = 0;
        f->color[4 * i + 3] = 0x3C00u;
        f->depth[i] = 0;
    }
    /* per-entry values of depthFirstRender (:1753-1764; getColor / getOpacity): the Global
     * blend's, so the oracle's conic_from_quant and blend_rec */
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
    free(keys); free(rec); free(active); free(cnt); free(tiles); free(gids);
    *out = f;
    return OG_OK;
fail:
    free(keys); free(rec); free(active); free(cnt); free(tiles); free(gids);
    dfm_frame_free(f);
    return rc;
}

/*
 * frame_ref.c -- CPU checker of gsm_global_render_frame (TEST INFRASTRUCTURE; include/gsm_renderer.h).
 *
 * It includes the styled frames' checker, and through it the pick target's, the composite's and the oracle's
 * translation unit: sr_render makes the frame from styled bytes (an identity table: cr_render's frame).  fr_walk
 * takes a finished og_frame and an optional occluder and walks every active tile ONCE with the loop of blend_tiles
 * (oracle/gsm_oracle.c) restated, plus the two rules the entry composes:
 *
 *   the occluded walk of tests/occlude/occlude_ref.c -- per pixel q of a 4x2 group, Z[q] = og_f2h(occluder[y][x])
 *   (+inf without an occluder and outside width x height), closed[q] = false; the break test takes a closed pixel's
 *   T as +0; for an evaluated entry, if H(Z[q]) < H(g->dep) then closed[q] = true, and while closed[q] holds
 *   a[q] = +0, before the `any` test;
 *
 *   the pick rule of tests/pick/pick_ref.c on that walk -- for every entry the group blends, w = hmul(a[q], T[q])
 *   with T before the entry's update, the same w the colour takes; if H(w) > H(best[q]): best = w, pick = the id.
 *   A closed pixel's w is 0 and never wins.
 *
 * It writes colour, depth, pick (ids of the frame: a composite's concatenated ids) and, per pixel, whether it was
 * closed when its group's walk ended.  Loaded by tests/ only.
 */
#include "../style/style_ref.c"

typedef struct {
    og_frame *f;
    blend_rec *rec;
    const float *occ; /* nullable */
    size_t occ_stride;
    uint16_t *color, *depth;
    uint32_t *pick;
    uint8_t *closed; /* nullable */
} fr_ctx;

static void fr_tiles(void *vctx, uint32_t lo, uint32_t hi) {
    fr_ctx *P = (fr_ctx *)vctx;
    og_frame *f = P->f;
    const blend_rec *rec = P->rec;
    const uint16_t H_ONE = 0x3C00u, H_ZERO = 0, H_INF = 0x7C00u;
    const uint16_t thr = og_f2h(1.0f / 255.0f);
    const uint16_t c099 = og_d2h(0.99);
    const uint32_t W = f->width, Hh = f->height;
    for (uint32_t tile = lo; tile < hi; ++tile) {
        uint32_t start = f->headers[2 * tile], count = f->headers[2 * tile + 1];
        if (count == 0) continue; /* (an inactive tile keeps the clear value and PR_PICK_NONE) */
        uint32_t tileX = tile % f->tiles_x, tileY = tile / f->tiles_x;
        for (uint32_t ly = 0; ly < 8; ++ly)
            for (uint32_t lx = 0; lx < 8; ++lx) {
                uint32_t baseX = tileX * 32 + lx * 4, baseY = tileY * 16 + ly * 2;
                uint16_t posx[4], posy[2];
                for (int i = 0; i < 4; ++i) posx[i] = og_f2h((float)(baseX + (uint32_t)i));
                for (int j = 0; j < 2; ++j) posy[j] = og_f2h((float)(baseY + (uint32_t)j));
                uint16_t T[8], C[8][3], D[8], Z[8], best[8];
                uint32_t pk[8];
                int closed[8], inside[8];
                for (int q = 0; q < 8; ++q) {
                    T[q] = H_ONE; C[q][0] = C[q][1] = C[q][2] = H_ZERO; D[q] = H_ZERO;
                    best[q] = H_ZERO; pk[q] = PR_PICK_NONE;
                    uint32_t x = baseX + (uint32_t)(q & 3), y = baseY + (uint32_t)(q >> 2);
                    inside[q] = x < W && y < Hh;
                    Z[q] = (inside[q] && P->occ) ? og_f2h(P->occ[(size_t)y * P->occ_stride + x]) : H_INF;
                    closed[q] = 0;
                }
                for (uint32_t i = 0; i < count; ++i) {
                    uint16_t Tb[8];
                    for (int q = 0; q < 8; ++q) Tb[q] = closed[q] ? H_ZERO : T[q];
                    uint16_t m0 = hmax(hmax(Tb[0], Tb[1]), hmax(Tb[2], Tb[3]));
                    uint16_t m1 = hmax(hmax(Tb[4], Tb[5]), hmax(Tb[6], Tb[7]));
                    if (H(hmax(m0, m1)) < H(thr)) break;
                    int32_t gi = f->sorted_values[start + i];
                    if (gi < 0) continue;
                    const blend_rec *g = &rec[gi];
                    uint16_t a[8];
                    int any = 0;
                    for (int j = 0; j < 2; ++j)
                        for (int ii = 0; ii < 4; ++ii) {
                            int q = j * 4 + ii;
                            uint16_t dx = hsub(posx[ii], g->mx), dy = hsub(posy[j], g->my);
                            uint16_t t2 = hmul(hmul(dx, dx), g->cxx);
                            uint16_t t4 = hmul(hmul(dy, dy), g->cyy);
                            uint16_t t7 = hmul(hmul(dx, dy), g->cxy2);
                            uint16_t p = hadd(hadd(t2, t4), t7);
                            uint16_t arg = og_f2h(-0.5f * H(p));
                            uint16_t e = g_exp_h[arg];
                            a[q] = hmin(hmul(g->op, e), c099);
                            if (H(Z[q]) < H(g->dep)) closed[q] = 1; /* the occlusion rule */
                            if (closed[q]) a[q] = H_ZERO;
                            if (H(a[q]) != 0.0f) any = 1;
                        }
                    if (!any) continue;
                    for (int q = 0; q < 8; ++q) {
                        uint16_t w = hmul(a[q], T[q]);
                        if (H(w) > H(best[q])) { /* the pick rule, on the colour's own w */
                            best[q] = w;
                            pk[q] = (uint32_t)gi;
                        }
                        C[q][0] = hfma(g->cr, w, C[q][0]);
                        C[q][1] = hfma(g->cg, w, C[q][1]);
                        C[q][2] = hfma(g->cb, w, C[q][2]);
                        D[q] = hfma(g->dep, w, D[q]);
                        T[q] = hmul(T[q], hsub(H_ONE, a[q]));
                    }
                }
                for (int q = 0; q < 8; ++q) {
                    if (!inside[q]) continue;
                    uint32_t x = baseX + (uint32_t)(q & 3), y = baseY + (uint32_t)(q >> 2);
                    size_t at = (size_t)y * W + x;
                    uint16_t *px = P->color + 4 * at;
                    px[0] = C[q][0]; px[1] = C[q][1]; px[2] = C[q][2];
                    px[3] = hsub(H_ONE, T[q]);
                    P->depth[at] = D[q];
                    P->pick[at] = pk[q];
                    if (P->closed) P->closed[at] = (uint8_t)closed[q];
                }
            }
    }
}

/* occluder (nullable: nothing is occluded): height rows of occ_stride floats.  color: width * height * 4 fp16 words,
 * depth, pick: width * height, closed (nullable): width * height bytes.  records (nullable): count * 10 fp16 words
 * (mx, my, cxx, cyy, cxy2, op, cr, cg, cb, dep).  Inactive tiles: the frame's own clear values, PR_PICK_NONE, not
 * closed.  < 0: out of memory or a NULL argument. */
long fr_walk(og_frame *f, const float *occluder, size_t occ_stride, uint16_t *color, uint16_t *depth, uint32_t *pick,
             uint8_t *closed, uint16_t *records) {
    ensure_init();
    if (!f || !color || !depth || !pick) return -1;
    size_t n = f->count ? f->count : 1;
    blend_rec *rec = (blend_rec *)calloc(n, sizeof(blend_rec));
    if (!rec) return -1;
    rec_ctx RC = {f, rec};
    rec_range(&RC, 0, f->count);
    if (records)
        for (uint32_t g = 0; g < f->count; ++g) {
            const blend_rec *r = &rec[g];
            uint16_t v[10] = {r->mx, r->my, r->cxx, r->cyy, r->cxy2, r->op, r->cr, r->cg, r->cb, r->dep};
            memcpy(records + (size_t)g * 10, v, sizeof(v));
        }
    const size_t px = (size_t)f->width * f->height;
    memcpy(color, f->color, px * 4 * sizeof(uint16_t));
    memcpy(depth, f->depth, px * sizeof(uint16_t));
    for (size_t i = 0; i < px; ++i) pick[i] = PR_PICK_NONE;
    if (closed) memset(closed, 0, px);
    fr_ctx P = {f, rec, occluder, occ_stride, color, depth, pick, closed};
    int nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    parallel_for(nthreads < 1 ? 1 : nthreads > 16 ? 16 : nthreads, f->tile_count, fr_tiles, &P);
    free(rec);
    return 0;
}

/*
 * occlude_ref.c -- CPU checker of the occluded frames (TEST INFRASTRUCTURE; include/gsm_renderer.h).
 *
 * It includes the composite's checker, and with it the oracle's translation unit: og_render and cr_render make
 * the frame.  or_occlude takes a finished og_frame and an occluder (one float per pixel) and walks every active
 * tile again with the loop of blend_tiles (oracle/gsm_oracle.c) restated, plus the occlusion rule:
 *
 *   per pixel q of a 4x2 group: Z[q] = og_f2h(occluder[y][x]) (+inf outside width x height, not read there),
 *   closed[q] = false.  The break test before entry i takes Tb[q] = closed[q] ? +0 : T[q] in place of T[q].  For
 *   an evaluated entry (not gi < 0), after a[q] is computed and before the `any` test: if H(Z[q]) < H(g->dep),
 *   closed[q] = true; while closed[q] holds, a[q] = +0.  The `any` test, w, colour, depth and T go on unchanged.
 *
 * The frame's sorted_values, headers, render_data and mask are all it reads; rec_range gives the records.  It
 * writes colour, depth and group_iters of the occluded frame (inactive tiles: the frame's own clear values) and
 * three counts, and returns the number of colour, depth and group_iters values that differ from the frame's
 * own -- 0 under an occluder of all +inf, or the restatement has drifted from the oracle.
 *
 * half_model != 0 walks a wrong model on purpose, the one a blend over half-tile lists would compute: an entry
 * whose alpha is +0 on every pixel of the group's 16-column half of the tile is left out of the walk altogether,
 * so it closes no pixel either.  The contract lets such an entry close pixels, and the break before the next
 * entries sees them closed.  Where the two frames differ, the scene reaches the one place where the lists
 * matter; the tests assert that theirs do.  It is loaded by tests/ only.
 */
#include "../compose/compose_ref.c"

typedef struct {
    og_frame *f;
    blend_rec *rec;
    const float *occ;
    size_t occ_stride; /* floats per row */
    uint16_t *color, *depth;
    uint32_t *iters;
    int half_model;
    long differ, closed_pixels, closure_breaks, mixed_groups;
} or_ctx;

/* tiles [lo, hi): blend_tiles restated, plus the occlusion rule, the counts and the comparison */
static void or_tiles(void *vctx, uint32_t lo, uint32_t hi) {
    or_ctx *P = (or_ctx *)vctx;
    og_frame *f = P->f;
    const blend_rec *rec = P->rec;
    const uint16_t H_ONE = 0x3C00u, H_ZERO = 0, H_INF = 0x7C00u;
    const uint16_t thr = og_f2h(1.0f / 255.0f);
    const uint16_t c099 = og_d2h(0.99);
    const uint32_t W = f->width, Hh = f->height;
    long differ = 0, closed_pixels = 0, closure_breaks = 0, mixed_groups = 0;
    for (uint32_t tile = lo; tile < hi; ++tile) {
        uint32_t start = f->headers[2 * tile], count = f->headers[2 * tile + 1];
        if (count == 0) { /* (an inactive tile keeps the clear value; the oracle leaves its group_iters alone) */
            for (int g = 0; g < 64; ++g) P->iters[(size_t)tile * 64 + g] = f->group_iters[(size_t)tile * 64 + g];
            continue;
        }
        uint32_t tileX = tile % f->tiles_x, tileY = tile / f->tiles_x;
        uint8_t *kept = NULL; /* half_model: kept[h * count + i], entry i has a nonzero alpha on half h */
        if (P->half_model) {
            kept = (uint8_t *)calloc((size_t)2 * count, 1);
            if (!kept) { __sync_fetch_and_add(&P->differ, 1L << 40); return; }
            uint16_t hx[32], hy[16];
            for (int i = 0; i < 32; ++i) hx[i] = og_f2h((float)(tileX * 32 + (uint32_t)i));
            for (int j = 0; j < 16; ++j) hy[j] = og_f2h((float)(tileY * 16 + (uint32_t)j));
            for (uint32_t i = 0; i < count; ++i) {
                int32_t gi = f->sorted_values[start + i];
                if (gi < 0) continue;
                const blend_rec *g = &rec[gi];
                for (int xx = 0; xx < 32; ++xx) {
                    if (kept[(size_t)(xx >> 4) * count + i]) { xx |= 15; continue; }
                    for (int yy = 0; yy < 16; ++yy) {
                        uint16_t dx = hsub(hx[xx], g->mx), dy = hsub(hy[yy], g->my);
                        uint16_t p = hadd(hadd(hmul(hmul(dx, dx), g->cxx), hmul(hmul(dy, dy), g->cyy)),
                                          hmul(hmul(dx, dy), g->cxy2));
                        uint16_t a = hmin(hmul(g->op, g_exp_h[og_f2h(-0.5f * H(p))]), c099);
                        if (H(a) != 0.0f) { kept[(size_t)(xx >> 4) * count + i] = 1; break; }
                    }
                }
            }
        }
        for (uint32_t ly = 0; ly < 8; ++ly)
            for (uint32_t lx = 0; lx < 8; ++lx) {
                uint32_t baseX = tileX * 32 + lx * 4, baseY = tileY * 16 + ly * 2;
                uint16_t posx[4], posy[2];
                for (int i = 0; i < 4; ++i) posx[i] = og_f2h((float)(baseX + (uint32_t)i));
                for (int j = 0; j < 2; ++j) posy[j] = og_f2h((float)(baseY + (uint32_t)j));
                uint16_t T[8], C[8][3], D[8], Z[8];
                int closed[8], inside[8];
                for (int q = 0; q < 8; ++q) {
                    T[q] = H_ONE; C[q][0] = C[q][1] = C[q][2] = H_ZERO; D[q] = H_ZERO;
                    uint32_t x = baseX + (uint32_t)(q & 3), y = baseY + (uint32_t)(q >> 2);
                    inside[q] = x < W && y < Hh;
                    Z[q] = inside[q] ? og_f2h(P->occ[(size_t)y * P->occ_stride + x]) : H_INF;
                    closed[q] = 0;
                }
                int mixed = 0;
                uint32_t i = 0;
                for (; i < count; ++i) {
                    uint16_t Tb[8];
                    for (int q = 0; q < 8; ++q) Tb[q] = closed[q] ? H_ZERO : T[q];
                    uint16_t m0 = hmax(hmax(Tb[0], Tb[1]), hmax(Tb[2], Tb[3]));
                    uint16_t m1 = hmax(hmax(Tb[4], Tb[5]), hmax(Tb[6], Tb[7]));
                    if (H(hmax(m0, m1)) < H(thr)) {
                        uint16_t u0 = hmax(hmax(T[0], T[1]), hmax(T[2], T[3]));
                        uint16_t u1 = hmax(hmax(T[4], T[5]), hmax(T[6], T[7]));
                        if (!(H(hmax(u0, u1)) < H(thr))) closure_breaks++;
                        break;
                    }
                    int32_t gi = f->sorted_values[start + i];
                    if (gi < 0) continue;
                    if (kept && !kept[(size_t)(lx >> 2) * count + i]) continue; /* (the wrong model's only line) */
                    const blend_rec *g = &rec[gi];
                    uint16_t a[8];
                    int any = 0, has_closed = 0, has_open = 0;
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
                            if (closed[q]) has_closed = 1;
                            else if (!(H(T[q]) < H(thr))) has_open = 1;
                        }
                    if (has_closed && has_open) mixed = 1;
                    if (!any) continue;
                    for (int q = 0; q < 8; ++q) {
                        uint16_t w = hmul(a[q], T[q]);
                        C[q][0] = hfma(g->cr, w, C[q][0]);
                        C[q][1] = hfma(g->cg, w, C[q][1]);
                        C[q][2] = hfma(g->cb, w, C[q][2]);
                        D[q] = hfma(g->dep, w, D[q]);
                        T[q] = hmul(T[q], hsub(H_ONE, a[q]));
                    }
                }
                mixed_groups += mixed;
                P->iters[(size_t)tile * 64 + ly * 8 + lx] = i;
                if (f->group_iters[(size_t)tile * 64 + ly * 8 + lx] != i) differ++;
                for (int q = 0; q < 8; ++q) {
                    if (!inside[q]) continue;
                    uint32_t x = baseX + (uint32_t)(q & 3), y = baseY + (uint32_t)(q >> 2);
                    size_t at = (size_t)y * W + x;
                    uint16_t *px = P->color + 4 * at;
                    px[0] = C[q][0]; px[1] = C[q][1]; px[2] = C[q][2];
                    px[3] = hsub(H_ONE, T[q]);
                    P->depth[at] = D[q];
                    const uint16_t *own = f->color + 4 * at;
                    differ += (px[0] != own[0]) + (px[1] != own[1]) + (px[2] != own[2]) + (px[3] != own[3]);
                    differ += f->depth[at] != D[q];
                    closed_pixels += closed[q];
                }
            }
        free(kept);
    }
    __sync_fetch_and_add(&P->differ, differ);
    __sync_fetch_and_add(&P->closed_pixels, closed_pixels);
    __sync_fetch_and_add(&P->closure_breaks, closure_breaks);
    __sync_fetch_and_add(&P->mixed_groups, mixed_groups);
}

/* occluder: height rows of occ_stride floats.  color: width * height * 4 fp16 words, depth: width * height,
 * group_iters: tile_count * 64.  counts: closed_pixels (pixels of the frame closed when their group's walk
 * ended), closure_breaks (groups that broke at an entry where the unmasked maximum of T was still at or above
 * the threshold), mixed_groups (groups that, at some evaluated entry, held both a closed pixel and an open pixel
 * with T at or above the threshold).  records: count * 10 fp16 words (mx, my, cxx, cyy, cxy2, op, cr, cg, cb,
 * dep), the oracle's blend records (nullable; rows of masked-out gaussians are zero).  < 0: out of memory. */
long or_occlude(og_frame *f, const float *occluder, size_t occ_stride, uint16_t *color, uint16_t *depth,
                uint32_t *group_iters, long *counts, uint16_t *records, int half_model) {
    ensure_init();
    if (!f || !occluder || !color || !depth || !group_iters || !counts) return -1;
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
    or_ctx P = {f, rec, occluder, occ_stride, color, depth, group_iters, half_model, 0, 0, 0, 0};
    int nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    parallel_for(nthreads < 1 ? 1 : nthreads > 16 ? 16 : nthreads, f->tile_count, or_tiles, &P);
    free(rec);
    counts[0] = P.closed_pixels;
    counts[1] = P.closure_breaks;
    counts[2] = P.mixed_groups;
    return P.differ;
}

/*
 * pick_ref.c -- CPU checker of the pick target (TEST INFRASTRUCTURE; include/gsm_renderer.h).
 *
 * It includes the composite's checker, and with it the oracle's translation unit: og_render and cr_render make
 * the frame.  pr_pick takes a finished og_frame and walks every active tile again with the loop of blend_tiles
 * (oracle/gsm_oracle.c) restated, plus the pick rule:
 *
 *   per pixel q: best = +0 (fp16), pick = PR_PICK_NONE; for every list entry the pixel's 4x2 group blends, in
 *   list order, w = hmul(a[q], T[q]) with T before that entry's update; if H(w) > H(best): best = w, pick = the
 *   entry's id.  (The earliest entry wins ties; a weight of zero or NaN never wins.)
 *
 * The frame's sorted_values, headers, render_data and mask are all it reads; rec_range gives the records.  It
 * returns the number of colour and depth values that differ from the frame's own -- 0, or the restatement has
 * drifted from the oracle and the pick it gives means nothing.  Ids are the frame's ids (a composite:
 * concatenated ids).  It is loaded by tests/ only.
 */
#include "../compose/compose_ref.c"

#define PR_PICK_NONE 0xFFFFFFFFu

typedef struct {
    og_frame *f;
    blend_rec *rec;
    uint32_t *pick, *pick_pos;
    long differ;
} pr_ctx;

/* tiles [lo, hi): blend_tiles restated, plus the pick rule and the comparison with the frame's own pixels */
static void pr_tiles(void *vctx, uint32_t lo, uint32_t hi) {
    pr_ctx *P = (pr_ctx *)vctx;
    og_frame *f = P->f;
    const blend_rec *rec = P->rec;
    uint32_t *pick = P->pick, *pick_pos = P->pick_pos;
    const uint16_t H_ONE = 0x3C00u, H_ZERO = 0;
    const uint16_t thr = og_f2h(1.0f / 255.0f);
    const uint16_t c099 = og_d2h(0.99);
    const uint32_t W = f->width, Hh = f->height;
    long differ = 0;
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
                uint16_t T[8], C[8][3], D[8], best[8];
                uint32_t pk[8], pp[8];
                for (int q = 0; q < 8; ++q) {
                    T[q] = H_ONE; C[q][0] = C[q][1] = C[q][2] = H_ZERO; D[q] = H_ZERO;
                    best[q] = H_ZERO; pk[q] = PR_PICK_NONE; pp[q] = PR_PICK_NONE;
                }
                uint32_t i = 0;
                for (; i < count; ++i) {
                    uint16_t m0 = hmax(hmax(T[0], T[1]), hmax(T[2], T[3]));
                    uint16_t m1 = hmax(hmax(T[4], T[5]), hmax(T[6], T[7]));
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
                            if (H(a[q]) != 0.0f) any = 1;
                        }
                    if (!any) continue;
                    for (int q = 0; q < 8; ++q) {
                        uint16_t w = hmul(a[q], T[q]);
                        if (H(w) > H(best[q])) { /* the pick rule */
                            best[q] = w;
                            pk[q] = (uint32_t)gi;
                            pp[q] = i;
                        }
                        C[q][0] = hfma(g->cr, w, C[q][0]);
                        C[q][1] = hfma(g->cg, w, C[q][1]);
                        C[q][2] = hfma(g->cb, w, C[q][2]);
                        D[q] = hfma(g->dep, w, D[q]);
                        T[q] = hmul(T[q], hsub(H_ONE, a[q]));
                    }
                }
                if (f->group_iters[(size_t)tile * 64 + ly * 8 + lx] != i) differ++;
                for (int j = 0; j < 2; ++j)
                    for (int ii = 0; ii < 4; ++ii) {
                        uint32_t x = baseX + (uint32_t)ii, y = baseY + (uint32_t)j;
                        if (x >= W || y >= Hh) continue;
                        int q = j * 4 + ii;
                        const uint16_t *px = f->color + 4 * ((size_t)y * W + x);
                        differ += px[0] != C[q][0];
                        differ += px[1] != C[q][1];
                        differ += px[2] != C[q][2];
                        differ += px[3] != hsub(H_ONE, T[q]);
                        differ += f->depth[(size_t)y * W + x] != D[q];
                        pick[(size_t)y * W + x] = pk[q];
                        if (pick_pos) pick_pos[(size_t)y * W + x] = pp[q];
                    }
            }
    }
    __sync_fetch_and_add(&P->differ, differ);
}

/* pick, pick_pos: width * height words each (pick_pos: the list position of the winning entry, PR_PICK_NONE
 * where pick is; nullable).  records: count * 10 fp16 words (mx, my, cxx, cyy, cxy2, op, cr, cg, cb, dep), the
 * oracle's blend records (nullable; rows of masked-out gaussians are zero).  < 0: out of memory. */
long pr_pick(og_frame *f, uint32_t *pick, uint32_t *pick_pos, uint16_t *records) {
    ensure_init();
    if (!f || !pick) return -1;
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
    const uint32_t W = f->width, Hh = f->height;
    for (size_t i = 0; i < (size_t)W * Hh; ++i) {
        pick[i] = PR_PICK_NONE;
        if (pick_pos) pick_pos[i] = PR_PICK_NONE;
    }
    pr_ctx P = {f, rec, pick, pick_pos, 0};
    int nthreads = (int)sysconf(_SC_NPROCESSORS_ONLN);
    parallel_for(nthreads < 1 ? 1 : nthreads > 16 ? 16 : nthreads, f->tile_count, pr_tiles, &P);
    free(rec);
    return P.differ;
}

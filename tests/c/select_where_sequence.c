/* A world-space editing loop through the C ABI alone, in C: select the gaussians inside a box that
 * are opaque enough (gsm_global_select_where sets bit 0 of their state bytes) -> the selection's extent
 * (gsm_global_state_bounds) -> separate it into a scene of its own (gsm_global_keep_masked, gsm_global_extract) ->
 * the extent of that scene with a full keep set, which must equal the first word for word -> render it
 * (gsm_global_render).  Test infrastructure: run by tests/test_select_where.py, which writes the scene and the box
 * and compares the state bytes and the bounds with numpy and the frame with the oracle.
 *
 * usage: select_where_sequence world.bin harm.bin count sh width height cam.bin box.bin opacity_min out
 * box.bin: the twelve floats of to_shape.  writes out.state (count bytes), out.bounds (two gsm_global_bounds),
 * out.ids (kept words) and out.color */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gsm_renderer.h"

static void* slurp(const char* path, size_t* n) {
    FILE* f = fopen(path, "rb");
    if (!f) return NULL;
    fseek(f, 0, SEEK_END);
    *n = (size_t)ftell(f);
    fseek(f, 0, SEEK_SET);
    void* p = malloc(*n ? *n : 1);
    if (fread(p, 1, *n, f) != *n) {
        fclose(f);
        free(p);
        return NULL;
    }
    fclose(f);
    return p;
}

#define CHECK(cond, msg)                       \
    do {                                       \
        if (!(cond)) {                         \
            fprintf(stderr, "FAIL: %s\n", msg); \
            return 1;                          \
        }                                      \
    } while (0)

/* `bytes` bytes of device memory into the file base.suffix */
static int dump(const char* base, const char* suffix, const void* dev, size_t bytes) {
    char path[4096];
    snprintf(path, sizeof(path), "%s.%s", base, suffix);
    void* host = malloc(bytes ? bytes : 1);
    if (bytes && hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) return 1;
    FILE* f = fopen(path, "wb");
    if (!f || fwrite(host, 1, bytes, f) != bytes) return 1;
    fclose(f);
    free(host);
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 11) {
        fprintf(stderr, "usage: %s world harm count sh width height cam box opacity_min out\n", argv[0]);
        return 2;
    }
    size_t wn = 0, hn = 0, cn = 0, bn = 0;
    void* world = slurp(argv[1], &wn);
    void* harm = slurp(argv[2], &hn);
    float* camf = (float*)slurp(argv[7], &cn); /* view[16] proj[16] pos[3] fx fy near far */
    float* box = (float*)slurp(argv[8], &bn);
    const uint32_t count = (uint32_t)atoi(argv[3]), sh = (uint32_t)atoi(argv[4]);
    const uint32_t W = (uint32_t)atoi(argv[5]), H = (uint32_t)atoi(argv[6]);
    const char* out_base = argv[10];
    CHECK(world && harm && camf && box && cn == 39 * sizeof(float) && bn == 12 * sizeof(float) && count > 0, "inputs");
    const size_t rec = wn / count, row = hn / count; /* bytes of a record and of a harmonics row */
    CHECK(rec * count == wn && row * count == hn && (rec == 32 || rec == 48), "row sizes");

    gsm_renderer_config cfg;
    gsm_renderer_config_default(&cfg);
    cfg.max_gaussians = count;
    cfg.max_width = W;
    cfg.max_height = H;
    cfg.precision = rec == 32 ? GSM_PRECISION_FLOAT16 : GSM_PRECISION_FLOAT32;
    cfg.color_format = GSM_COLOR_FORMAT_RGBA16F;
    cfg.gaussian_color_space = GSM_COLOR_SPACE_LINEAR;
    gsm_renderer* r = NULL;
    CHECK(gsm_global_create(&cfg, 0, &r) == GSM_OK && r, "gsm_global_create");

    void *dw = NULL, *dh = NULL, *dc = NULL, *dd = NULL, *dstate = NULL, *ow = NULL, *oh = NULL, *oids = NULL;
    void* dwords = NULL; /* matched, kept, then two gsm_global_bounds */
    CHECK(hipMalloc(&dw, wn) == hipSuccess && hipMalloc(&dh, hn) == hipSuccess &&
              hipMalloc(&dc, (size_t)W * H * 8) == hipSuccess && hipMalloc(&dd, (size_t)W * H * 2) == hipSuccess &&
              hipMalloc(&dstate, count) == hipSuccess && hipMalloc(&ow, wn) == hipSuccess &&
              hipMalloc(&oh, hn) == hipSuccess && hipMalloc(&oids, (size_t)count * 4) == hipSuccess &&
              hipMalloc(&dwords, 18 * 4) == hipSuccess,
          "hipMalloc");
    CHECK(hipMemcpy(dw, world, wn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dh, harm, hn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(dstate, 0x40, count) == hipSuccess && hipMemset(dwords, 0xEE, 18 * 4) == hipSuccess,
          "upload");
    gsm_camera_params cam;
    gsm_camera_params_init(&cam, camf, camf + 16, camf + 32, camf[35], camf[36]);
    cam.near_plane = camf[37];
    cam.far_plane = camf[38];
    gsm_gaussian_input in = {dw, dh, count, sh};
    hipStream_t stream = NULL;
    CHECK(hipStreamCreate(&stream) == hipSuccess, "stream");
    uint32_t* matched = (uint32_t*)dwords;
    uint32_t* kept = matched + 1;
    gsm_global_bounds* bounds = (gsm_global_bounds*)(matched + 2);

    /* select: set bit 0 inside the box, opaque gaussians only; every state byte starts as 0x40 */
    gsm_global_select_query q;
    gsm_global_select_query_default(&q);
    CHECK(q.shape == GSM_SELECT_ALL && q.flags == 0 && q.to_shape[0] == 1.0f && q.to_shape[3] == 0.0f &&
              q.test_mask == 0 && q.test_value == 0, "select_query_default");
    q.shape = GSM_SELECT_BOX;
    memcpy(q.to_shape, box, sizeof(q.to_shape));
    q.opacity_min = (float)atof(argv[9]);
    CHECK(gsm_global_select_where(r, stream, &in, &q, (uint8_t*)dstate, NULL, 0, ~1u, 1u, matched) == GSM_OK,
          "select_where");
    /* refused before anything is enqueued */
    q.flags = 2u;
    CHECK(gsm_global_select_where(r, stream, &in, &q, (uint8_t*)dstate, NULL, 0, 0u, 0u, matched) ==
              GSM_ERR_INVALID_ARGUMENT, "a flags bit other than bit 0");
    CHECK(gsm_global_select_where(NULL, stream, &in, &q, (uint8_t*)dstate, NULL, 0, 0u, 0u, matched) ==
              GSM_ERR_INVALID_ARGUMENT, "NULL handle");
    /* the selection's extent */
    uint32_t keep[8];
    gsm_global_keep_masked(1u, 1u, keep);
    const gsm_global_state st = {(const uint8_t*)dstate, 0, 0};
    CHECK(gsm_global_state_bounds(r, stream, &in, &st, keep, &bounds[0]) == GSM_OK, "state_bounds");
    CHECK(gsm_global_state_bounds(NULL, stream, &in, &st, keep, &bounds[0]) == GSM_ERR_INVALID_ARGUMENT, "NULL handle 2");
    /* separate the selection, and its extent as a scene of its own */
    const gsm_global_extract_out out = {ow, oh, NULL, (uint32_t*)oids, count, 0};
    CHECK(gsm_global_extract(r, stream, &in, &st, keep, &out, kept) == GSM_OK, "extract");
    uint32_t words[18];
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync");
    CHECK(hipMemcpy(words, dwords, sizeof(words), hipMemcpyDeviceToHost) == hipSuccess, "read counts");
    const uint32_t K = words[1];
    CHECK(K <= count && K == words[0], "kept == matched");
    gsm_gaussian_input sel = {ow, oh, K, sh};
    const gsm_global_state whole = {NULL, 0, 0};
    uint32_t all[8];
    gsm_global_keep_masked(0u, 0u, all);
    CHECK(gsm_global_state_bounds(r, stream, &sel, &whole, all, &bounds[1]) == GSM_OK, "state_bounds of the extract");
    CHECK(gsm_global_render(r, stream, &sel, &cam, W, H, dc, (size_t)W * 8, dd, (size_t)W * 2) == GSM_OK, "render");
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync 2");
    CHECK(hipMemcpy(words, dwords, sizeof(words), hipMemcpyDeviceToHost) == hipSuccess, "read bounds");
    CHECK(memcmp(&words[2], &words[10], sizeof(gsm_global_bounds)) == 0, "the two bounds agree word for word");
    CHECK(words[8] + words[9] == K, "count + skipped == kept");
    CHECK(dump(out_base, "state", dstate, count) == 0 && dump(out_base, "bounds", bounds, 2 * sizeof(gsm_global_bounds)) == 0 &&
              dump(out_base, "ids", oids, (size_t)K * 4) == 0 && dump(out_base, "color", dc, (size_t)W * H * 8) == 0,
          "write");
    hipStreamDestroy(stream);
    hipFree(dw); hipFree(dh); hipFree(dc); hipFree(dd); hipFree(dstate);
    hipFree(ow); hipFree(oh); hipFree(oids); hipFree(dwords);
    gsm_global_destroy(r);
    printf("matched %u kept %u count %u skipped %u abi %d\n", words[0], K, words[8], words[9], gsm_abi_version());
    return 0;
}

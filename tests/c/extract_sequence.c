/* An editing session through the C ABI alone, in C: select the gaussians whose centres lie on the
 * left half of the frame (gsm_global_select_mask sets bit 0 of their state bytes) -> count them
 * (gsm_global_state_histogram) -> separate them into a scene of their own (gsm_global_keep_masked,
 * gsm_global_extract) -> render that scene (gsm_global_render).  kept must equal the select's matched count and the
 * histogram's.  Test infrastructure: run by tests/test_extract.py, which writes the scene and compares the rows with
 * numpy and the frame with the oracle.
 *
 * usage: extract_sequence world.bin harm.bin count sh width height cam.bin out
 * writes out.ids, out.gaussians, out.harmonics (kept rows each) and out.color */
#define __HIP_PLATFORM_AMD__ 1
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "gsm_debug.h"
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
    if (argc != 9) {
        fprintf(stderr, "usage: %s world harm count sh width height cam out\n", argv[0]);
        return 2;
    }
    size_t wn = 0, hn = 0, cn = 0;
    void* world = slurp(argv[1], &wn);
    void* harm = slurp(argv[2], &hn);
    float* camf = (float*)slurp(argv[7], &cn); /* view[16] proj[16] pos[3] fx fy near far */
    const uint32_t count = (uint32_t)atoi(argv[3]), sh = (uint32_t)atoi(argv[4]);
    const uint32_t W = (uint32_t)atoi(argv[5]), H = (uint32_t)atoi(argv[6]);
    CHECK(world && harm && camf && cn == 39 * sizeof(float) && count > 0, "inputs");
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

    void *dw = NULL, *dh = NULL, *dc = NULL, *dd = NULL, *dmask = NULL, *dstate = NULL, *ow = NULL, *oh = NULL;
    void *ostate = NULL, *oids = NULL, *dwords = NULL; /* dwords: matched, kept, then the 256 histogram words */
    CHECK(hipMalloc(&dw, wn) == hipSuccess && hipMalloc(&dh, hn) == hipSuccess &&
              hipMalloc(&dc, (size_t)W * H * 8) == hipSuccess && hipMalloc(&dd, (size_t)W * H * 2) == hipSuccess &&
              hipMalloc(&dmask, (size_t)W * H) == hipSuccess && hipMalloc(&dstate, count) == hipSuccess &&
              hipMalloc(&ow, wn) == hipSuccess && hipMalloc(&oh, hn) == hipSuccess &&
              hipMalloc(&ostate, count) == hipSuccess && hipMalloc(&oids, (size_t)count * 4) == hipSuccess &&
              hipMalloc(&dwords, 258 * 4) == hipSuccess,
          "hipMalloc");
    uint8_t* mask = (uint8_t*)calloc((size_t)W * H, 1);
    for (uint32_t y = 0; y < H; ++y) memset(mask + (size_t)y * W, 1, W / 2);
    CHECK(hipMemcpy(dw, world, wn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dh, harm, hn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dmask, mask, (size_t)W * H, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemset(dstate, 0x40, count) == hipSuccess && hipMemset(dwords, 0xEE, 258 * 4) == hipSuccess,
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
    uint32_t* hist = matched + 2;

    /* select: set bit 0 under the mask; every state byte starts as 0x40 */
    CHECK(gsm_global_select_mask(r, stream, &in, &cam, W, H, dmask, W, (uint8_t*)dstate, NULL, 0, ~1u, 1u, matched) ==
              GSM_OK, "select_mask");
    CHECK(gsm_global_state_histogram(r, stream, (const uint8_t*)dstate, count, hist) == GSM_OK, "state_histogram");
    /* separate the selection */
    uint32_t keep[8];
    gsm_global_keep_masked(1u, 1u, keep);
    CHECK(keep[0] == 0xAAAAAAAAu && keep[7] == 0xAAAAAAAAu, "keep_masked");
    const gsm_global_state st = {(const uint8_t*)dstate, 0, 0};
    const gsm_global_extract_out out = {ow, oh, (uint8_t*)ostate, (uint32_t*)oids, count, 0};
    CHECK(gsm_global_extract(r, stream, &in, &st, keep, &out, kept) == GSM_OK, "extract");
    /* in place is refused, and refused before anything is enqueued */
    const gsm_global_extract_out same = {dw, oh, NULL, NULL, count, 0};
    CHECK(gsm_global_extract(r, stream, &in, &st, keep, &same, kept) == GSM_ERR_INVALID_ARGUMENT, "in place");
    CHECK(gsm_global_extract(NULL, stream, &in, &st, keep, &out, kept) == GSM_ERR_INVALID_ARGUMENT, "NULL handle");
    uint32_t words[258];
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync");
    CHECK(hipMemcpy(words, dwords, sizeof(words), hipMemcpyDeviceToHost) == hipSuccess, "read counts");
    const uint32_t K = words[1];
    CHECK(K <= count && words[2 + 0x41] + words[2 + 0x40] == count, "histogram: two states only");

    /* the extracted scene is a scene: render it */
    gsm_gaussian_input sel = {ow, oh, K, sh};
    CHECK(gsm_global_render(r, stream, &sel, &cam, W, H, dc, (size_t)W * 8, dd, (size_t)W * 2) == GSM_OK, "render");
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync 2");
    uint8_t* hs = (uint8_t*)malloc(K ? K : 1);
    CHECK(hipMemcpy(hs, ostate, K, hipMemcpyDeviceToHost) == hipSuccess, "read states");
    for (uint32_t j = 0; j < K; ++j) CHECK(hs[j] == 0x41, "a kept gaussian's state byte");
    CHECK(dump(argv[8], "ids", oids, (size_t)K * 4) == 0 && dump(argv[8], "gaussians", ow, (size_t)K * rec) == 0 &&
              dump(argv[8], "harmonics", oh, (size_t)K * row) == 0 && dump(argv[8], "color", dc, (size_t)W * H * 8) == 0,
          "write");
    hipStreamDestroy(stream);
    hipFree(dw); hipFree(dh); hipFree(dc); hipFree(dd); hipFree(dmask); hipFree(dstate);
    hipFree(ow); hipFree(oh); hipFree(ostate); hipFree(oids); hipFree(dwords);
    gsm_global_destroy(r);
    printf("matched %u kept %u histogram %u abi %d\n", words[0], K, words[2 + 0x41], gsm_abi_version());
    return 0;
}

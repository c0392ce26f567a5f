/* One orthographic frame and one select through the C ABI alone, in C: gsm_global_render_frame with
 * GSM_FRAME_ORTHOGRAPHIC and a pick target, then gsm_global_select_mask_ortho under a full mask into a zeroed state
 * array.  Test infrastructure: run by tests/test_ortho_sequence.py, which writes the scene and compares colour, pick,
 * the state bytes and the count with the orthographic checker.
 *
 * usage: ortho_sequence world.bin harm.bin count sh width height cam.bin out.bin
 * out.bin: colour (W*H*8 bytes), pick (W*H*4), state (count), matched (4) */
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
    CHECK(world && harm && camf && cn == 39 * sizeof(float), "inputs");

    gsm_renderer_config cfg;
    gsm_renderer_config_default(&cfg);
    cfg.max_gaussians = count;
    cfg.max_width = W;
    cfg.max_height = H;
    cfg.precision = GSM_PRECISION_FLOAT32;
    cfg.color_format = GSM_COLOR_FORMAT_RGBA16F;
    cfg.gaussian_color_space = GSM_COLOR_SPACE_LINEAR;
    gsm_renderer* r = NULL;
    CHECK(gsm_global_create(&cfg, 0, &r) == GSM_OK && r, "gsm_global_create");

    const size_t px = (size_t)W * H;
    void *dw = NULL, *dh = NULL, *dc = NULL, *dd = NULL, *dp = NULL, *dk = NULL, *ds = NULL, *dm = NULL;
    CHECK(hipMalloc(&dw, wn) == hipSuccess && hipMalloc(&dh, hn) == hipSuccess && hipMalloc(&dc, px * 8) == hipSuccess &&
              hipMalloc(&dd, px * 2) == hipSuccess && hipMalloc(&dp, px * 4) == hipSuccess &&
              hipMalloc(&dk, px) == hipSuccess && hipMalloc(&ds, count ? count : 1) == hipSuccess &&
              hipMalloc(&dm, 4) == hipSuccess,
          "hipMalloc");
    CHECK(hipMemcpy(dw, world, wn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dh, harm, hn, hipMemcpyHostToDevice) == hipSuccess && hipMemset(dk, 1, px) == hipSuccess &&
              hipMemset(ds, 0, count ? count : 1) == hipSuccess,
          "upload");
    hipStream_t stream = NULL;
    CHECK(hipStreamCreate(&stream) == hipSuccess, "stream");

    gsm_global_object obj;
    memset(&obj, 0, sizeof(obj));
    obj.input.gaussians = dw;
    obj.input.harmonics = dh;
    obj.input.gaussian_count = count;
    obj.input.sh_components = sh;
    gsm_camera_params_init(&obj.camera, camf, camf + 16, camf + 32, camf[35], camf[36]);
    obj.camera.near_plane = camf[37];
    obj.camera.far_plane = camf[38];

    gsm_global_frame fr;
    memset(&fr, 0, sizeof(fr));
    fr.objects = &obj;
    fr.object_count = 1;
    fr.width = W;
    fr.height = H;
    fr.color = dc;
    fr.color_pitch_bytes = (size_t)W * 8;
    fr.depth_r16f = dd;
    fr.depth_pitch_bytes = (size_t)W * 2;
    fr.pick_r32u = dp;
    fr.pick_pitch_bytes = (size_t)W * 4;
    fr.flags = 1; /* bit 0 stays reserved, alone and beside the flag */
    CHECK(gsm_global_render_frame(r, stream, &fr) == GSM_ERR_INVALID_ARGUMENT, "flags == 1");
    fr.flags = 1 | GSM_FRAME_ORTHOGRAPHIC;
    CHECK(gsm_global_render_frame(r, stream, &fr) == GSM_ERR_INVALID_ARGUMENT, "flags == 3");
    CHECK(gsm_global_render_frames(r, stream, &fr, 1) == GSM_ERR_INVALID_ARGUMENT, "frames: flags == 3");
    fr.flags = GSM_FRAME_ORTHOGRAPHIC;
    CHECK(gsm_global_render_frame(r, stream, &fr) == GSM_OK, "orthographic render_frame");
    CHECK(gsm_global_select_mask_ortho(r, stream, &obj.input, &obj.camera, W, H, dk, W - 1, (uint8_t*)ds, NULL, 0, 0xFF,
                                       4, (uint32_t*)dm) == GSM_ERR_INVALID_BUFFER_SIZE, "mask pitch below the width");
    CHECK(gsm_global_select_mask_ortho(r, stream, &obj.input, &obj.camera, W, H, dk, W, (uint8_t*)ds, NULL, 0, 0xFF, 4,
                                       (uint32_t*)dm) == GSM_OK, "select_mask_ortho");
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync");

    const size_t total = px * 8 + px * 4 + count + 4;
    char* host = (char*)malloc(total);
    CHECK(hipMemcpy(host, dc, px * 8, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(host + px * 8, dp, px * 4, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(host + px * 12, ds, count, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(host + px * 12 + count, dm, 4, hipMemcpyDeviceToHost) == hipSuccess,
          "download");
    FILE* f = fopen(argv[8], "wb");
    CHECK(f && fwrite(host, 1, total, f) == total, "write");
    fclose(f);
    hipStreamDestroy(stream);
    hipFree(dw); hipFree(dh); hipFree(dc); hipFree(dd); hipFree(dp); hipFree(dk); hipFree(ds); hipFree(dm);
    gsm_global_destroy(r);
    uint32_t matched;
    memcpy(&matched, host + px * 12 + count, 4);
    printf("matched %u abi %d\n", matched, gsm_abi_version());
    return 0;
}

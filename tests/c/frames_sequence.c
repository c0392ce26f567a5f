/* gsm_global_render_frames and gsm_global_select_pick_ids through the C ABI alone, in C: two frames of one scene in
 * one batch -- frame 0 under a constant-depth occluder with a pick target and a depth target, frame 1 with a pick
 * target only (no occluder, no depth) -- then "select what frame 1 shows" (NULL mask) into a zeroed state array.
 * Test infrastructure: run by tests/test_render_frames.py, which writes the scene and compares every output with the
 * Python path.
 *
 * usage: frames_sequence world.bin harm.bin count sh width height cam.bin occluder_depth out.bin
 * out.bin: colour 0 (W*H*8 bytes), pick 0 (W*H*4), colour 1 (W*H*8), pick 1 (W*H*4), state (count), matched (4) */
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
    if (argc != 10) {
        fprintf(stderr, "usage: %s world harm count sh width height cam occluder_depth out\n", argv[0]);
        return 2;
    }
    size_t wn = 0, hn = 0, cn = 0;
    void* world = slurp(argv[1], &wn);
    void* harm = slurp(argv[2], &hn);
    float* camf = (float*)slurp(argv[7], &cn); /* view[16] proj[16] pos[3] fx fy near far */
    const uint32_t count = (uint32_t)atoi(argv[3]), sh = (uint32_t)atoi(argv[4]);
    const uint32_t W = (uint32_t)atoi(argv[5]), H = (uint32_t)atoi(argv[6]);
    const float Z = (float)atof(argv[8]);
    CHECK(world && harm && camf && cn == 39 * sizeof(float), "inputs");

    /* a handle that holds both frames: two scenes' items, two frames' tiles side by side */
    gsm_renderer_config cfg;
    gsm_renderer_config_default(&cfg);
    cfg.max_gaussians = 2u * ((count + 255u) / 256u * 256u);
    cfg.max_width = 2u * W + 32u;
    cfg.max_height = H;
    cfg.precision = GSM_PRECISION_FLOAT32;
    cfg.color_format = GSM_COLOR_FORMAT_RGBA16F;
    cfg.gaussian_color_space = GSM_COLOR_SPACE_LINEAR;
    gsm_renderer* r = NULL;
    CHECK(gsm_global_create(&cfg, 0, &r) == GSM_OK && r, "gsm_global_create");

    const size_t px = (size_t)W * H;
    void *dw = NULL, *dh = NULL, *dc = NULL, *dd = NULL, *dp = NULL, *dz = NULL, *ds = NULL, *dm = NULL;
    CHECK(hipMalloc(&dw, wn) == hipSuccess && hipMalloc(&dh, hn) == hipSuccess &&
              hipMalloc(&dc, 2 * px * 8) == hipSuccess && hipMalloc(&dd, px * 2) == hipSuccess &&
              hipMalloc(&dp, 2 * px * 4) == hipSuccess && hipMalloc(&dz, px * 4) == hipSuccess &&
              hipMalloc(&ds, count ? count : 1) == hipSuccess && hipMalloc(&dm, 4) == hipSuccess,
          "hipMalloc");
    float* occ = (float*)malloc(px * 4);
    for (size_t i = 0; i < px; ++i) occ[i] = Z;
    CHECK(hipMemcpy(dw, world, wn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dh, harm, hn, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(dz, occ, px * 4, hipMemcpyHostToDevice) == hipSuccess &&
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

    gsm_global_frame fr[2];
    memset(fr, 0, sizeof(fr));
    for (int v = 0; v < 2; ++v) {
        fr[v].objects = &obj;
        fr[v].object_count = 1;
        fr[v].width = W;
        fr[v].height = H;
        fr[v].color = (char*)dc + (size_t)v * px * 8;
        fr[v].color_pitch_bytes = (size_t)W * 8;
        fr[v].pick_r32u = (char*)dp + (size_t)v * px * 4;
        fr[v].pick_pitch_bytes = (size_t)W * 4;
    }
    fr[0].depth_r16f = dd;
    fr[0].depth_pitch_bytes = (size_t)W * 2;
    fr[0].occluder_r32f = dz;
    fr[0].occluder_pitch_bytes = (size_t)W * 4;

    CHECK(gsm_global_render_frames(r, stream, NULL, 2) == GSM_ERR_MISSING_REQUIRED_BUFFER, "NULL frames");
    CHECK(gsm_global_render_frames(r, stream, fr, 0) == GSM_ERR_INVALID_GAUSSIAN_COUNT, "no frames");
    fr[1].flags = 1;
    CHECK(gsm_global_render_frames(r, stream, fr, 2) == GSM_ERR_INVALID_ARGUMENT, "flags != 0");
    fr[1].flags = 0;
    fr[1].object_count = 2;
    CHECK(gsm_global_render_frames(r, stream, fr, 2) == GSM_ERR_UNSUPPORTED, "a composite inside a batch");
    fr[1].object_count = 1;
    CHECK(gsm_global_render_frames(r, stream, fr, 2) == GSM_OK, "render_frames");
    /* the batch leaves no pick frame behind: the stateful select refuses, the stateless one selects */
    CHECK(gsm_global_select_pick(r, stream, fr[1].pick_r32u, (size_t)W * 4, W, H, NULL, 0, 0, (uint8_t*)ds, count, 0xFF,
                                 1, (uint32_t*)dm) == GSM_ERR_RENDER_FAILED, "select_pick after render_frames");
    CHECK(gsm_global_select_pick_ids(r, stream, fr[1].pick_r32u, (size_t)W * 4, W, H, NULL, 0, (uint8_t*)ds, count,
                                     0xFF, 1, (uint32_t*)dm) == GSM_OK, "select_pick_ids");
    CHECK(hipStreamSynchronize(stream) == hipSuccess, "sync");

    const size_t total = 2 * px * 12 + count + 4;
    char* host = (char*)malloc(total);
    char* at = host;
    for (int v = 0; v < 2; ++v) {
        CHECK(hipMemcpy(at, fr[v].color, px * 8, hipMemcpyDeviceToHost) == hipSuccess &&
                  hipMemcpy(at + px * 8, fr[v].pick_r32u, px * 4, hipMemcpyDeviceToHost) == hipSuccess,
              "download");
        at += px * 12;
    }
    CHECK(hipMemcpy(at, ds, count, hipMemcpyDeviceToHost) == hipSuccess &&
              hipMemcpy(at + count, dm, 4, hipMemcpyDeviceToHost) == hipSuccess,
          "download");
    FILE* f = fopen(argv[9], "wb");
    CHECK(f && fwrite(host, 1, total, f) == total, "write");
    fclose(f);
    hipStreamDestroy(stream);
    hipFree(dw); hipFree(dh); hipFree(dc); hipFree(dd); hipFree(dp); hipFree(dz); hipFree(ds); hipFree(dm);
    gsm_global_destroy(r);
    uint32_t matched;
    memcpy(&matched, at + count, 4);
    printf("matched %u abi %d\n", matched, gsm_abi_version());
    return 0;
}

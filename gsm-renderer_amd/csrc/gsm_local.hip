// gsm_local.hip -- host orchestration and C ABI (include/gsm_local.h) of the LocalRenderer frame.
//
// The C++ analogue of LocalRenderer.render -> renderView (LocalRenderer.swift:83-257) over the
// LocalViewResources scratch set.  One HIP stream replaces the command buffer; grids are capacity-sized
// and the visible count is read on the device, so a frame is enqueue-only.  DESIGN.md 13.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/gsm_local.h"
#include "gsm_detmath.h"
#include "gsm_host.h"
#include "gsm_internal.h"
#include "gsm_local_internal.h"

namespace gsm {

static_assert(sizeof(gsm_local_projected) == sizeof(LocalProjected), "ProjectedGaussian layout");
static_assert(GSM_LOCAL_MAX_PER_TILE == kLocalMaxPerTile && GSM_LOCAL_TILE == kLocalTile, "header constants");

class LocalRenderer {
   public:
    static gsm_status create(const gsm_renderer_config& cfg, int hipDevice, LocalRenderer** out);
    ~LocalRenderer() { hipSetDevice(dev_.id); }  // (the events and buffers are released on their device)
    gsm_status render(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& cam, uint32_t width,
                      uint32_t height, void* color, size_t pitch, void* depth, size_t depthPitch);
    gsm_status counters(gsm_local_counters* out);
    gsm_status debugCopy(int which, void* dst, size_t bytes, size_t* needed);
    // any nonzero flag: every stage bracketed by events
    gsm_status setProfiling(int flags) {
        hipSetDevice(dev_.id);
        return timer_.setProfiling(flags ? 1 : 0);
    }
    gsm_status stageTimes(float* ms, int n) {
        hipSetDevice(dev_.id);
        return timer_.stageTimes(ms, n, GSM_LOCAL_STAGE_BLEND);
    }
    gsm_status lastGpuTime(double* seconds) {
        hipSetDevice(dev_.id);
        return timer_.lastGpuTime(seconds);
    }

   private:
    LocalRenderer() = default;
    Device dev_;
    gsm_renderer_config config_{};
    uint32_t maxGaussians_ = 1, maxWidth_ = 1, maxHeight_ = 1, maxTiles_ = 1;
    LocalArena A_;
    DeviceAllocations allocs_;
    // last frame
    uint32_t lastCount_ = 0, lastTilesX_ = 0, lastTilesY_ = 0;
    StageTimer timer_{GSM_LOCAL_STAGE_COUNT, 64};  // the last 64 profiled frames are averaged
};

gsm_status LocalRenderer::create(const gsm_renderer_config& cfg, int hipDevice, LocalRenderer** out) {
    *out = nullptr;
    gsm_status st = check_config(cfg);
    if (st != GSM_OK) return st;
    const uint32_t maxW = cfg.max_width ? cfg.max_width : 1u, maxH = cfg.max_height ? cfg.max_height : 1u;
    // LocalRenderer.swift:67-70: maxTileCount and maxAssignments = maxTileCount * 2048
    const uint64_t tiles = (uint64_t)((maxW + kLocalTile - 1) / kLocalTile) * ((maxH + kLocalTile - 1) / kLocalTile);
    if (tiles > 65535u) return GSM_ERR_INVALID_TILE_COUNT;  // 16-bit tile coordinates, 512 MiB of slots
    Device dev;
    if ((st = pick_device(hipDevice, &dev)) != GSM_OK) return st;
    LocalRenderer* r = new (std::nothrow) LocalRenderer();
    if (!r) return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    r->dev_ = dev;
    r->allocs_.setDevice(dev.id);
    r->config_ = cfg;
    r->maxGaussians_ = cfg.max_gaussians ? cfg.max_gaussians : 1u;
    r->maxWidth_ = maxW;
    r->maxHeight_ = maxH;
    r->maxTiles_ = (uint32_t)tiles;
    const size_t G = r->maxGaussians_, slots = (size_t)r->maxTiles_ * kLocalMaxPerTile;
    const size_t nb = (G + kLocalBlock - 1) / kLocalBlock;
    LocalArena& A = r->A_;
    r->allocs_.alloc(st, A.temp, G * sizeof(LocalProjected));
    r->allocs_.alloc(st, A.compacted, G * sizeof(LocalProjected));
    r->allocs_.alloc(st, A.blockSums, (nb + 1) * 4);
    r->allocs_.alloc(st, A.visHdr, sizeof(TileAssignmentHeader));
    r->allocs_.alloc(st, A.queue, kQueueStripes * kQueueStride * sizeof(uint32_t));
    r->allocs_.alloc(st, A.tileCounts, (size_t)r->maxTiles_ * 4);
    r->allocs_.alloc(st, A.depthKeys, slots * sizeof(uint16_t));
    r->allocs_.alloc(st, A.slotIndices, slots * sizeof(uint32_t));
    r->allocs_.alloc(st, A.sortedLocal, slots * sizeof(uint16_t));
    r->allocs_.alloc(st, A.lists, slots * sizeof(uint32_t));
    r->allocs_.alloc(st, A.stats, sizeof(LocalStats));
    r->allocs_.alloc(st, A.expTable, 65536 * 2);
    if (st != GSM_OK) {
        delete r;
        return st;
    }
    if (upload_table(A.expTable, [](uint32_t i) { return blend_exp_table_entry((uint16_t)i); }) != GSM_OK ||
        hipMemset(A.visHdr, 0, sizeof(TileAssignmentHeader)) != hipSuccess ||
        hipMemset(A.stats, 0, sizeof(LocalStats)) != hipSuccess ||
        hipMemset(A.tileCounts, 0, (size_t)r->maxTiles_ * 4) != hipSuccess ||
        hipMemset(A.lists, 0, slots * sizeof(uint32_t)) != hipSuccess) {
        delete r;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    *out = r;
    return GSM_OK;
}

gsm_status LocalRenderer::render(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& cam,
                                 uint32_t width, uint32_t height, void* color, size_t pitch, void* depth,
                                 size_t depthPitch) {
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    // renderView's guards (LocalRenderer.swift:139-141) and the texture sizes -- errors, not a silent return
    const gsm_status vst = validate_frame(config_, maxGaussians_, maxWidth_, maxHeight_, in.gaussian_count, false,
                                          !in.gaussians || !in.harmonics, width, height, color, pitch, 1, depth,
                                          depthPitch);
    if (vst != GSM_OK) return vst;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    const int fmt = (int)config_.color_format;

    LocalArgs a;
    std::memset(&a, 0, sizeof(a));
    const float W = (float)width, H = (float)height;
    // CameraUniforms(from: camera, ...) (KernelTypes.swift:107-123) and the per-frame terms of
    // projectCovariance2D (GaussianShared.h:340-355), the same fp32 operations the reference repeats
    std::memcpy(a.view, cam.view, sizeof(a.view));
    std::memcpy(a.proj, cam.proj, sizeof(a.proj));
    const ProjectionUniforms u = projection_uniforms(cam.proj, W, H, cam.near_plane, cam.far_plane);
    a.limX = u.limX;
    a.limY = u.limY;
    a.focalX = u.focalX;
    a.focalY = u.focalY;
    a.width = W;
    a.height = H;
    a.nearPlane = cam.near_plane;
    a.farPlane = cam.far_plane;
    a.maxEig = u.maxEig;
    a.adjFar = u.adjFar;
    a.adjDen = u.adjDen;
    for (int i = 0; i < 3; ++i) a.camPos[i] = cam.position[i];
    a.inputIsSRGB = config_.gaussian_color_space == GSM_COLOR_SPACE_SRGB ? 1.0f : 0.0f;
    a.shComponents = in.sh_components;
    a.count = in.gaussian_count;
    a.tilesX = (width + kLocalTile - 1) / kLocalTile;  // LocalRenderer.swift:143-145
    a.tilesY = (height + kLocalTile - 1) / kLocalTile;
    a.tileCount = a.tilesX * a.tilesY;
    const uint32_t deg = sh_degree(in.sh_components);
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    const uint32_t nb = (a.count + kLocalBlock - 1) / kLocalBlock;

    timer_.beginFrame();
    timer_.record(0, s);
    local_launch_clear(a, A_, s);
    local_launch_project(half, deg, in.gaussians, in.harmonics, a, A_, s);
    launch_scan_sums(A_.blockSums, nb, maxGaussians_, A_.visHdr, A_.queue, s);
    local_launch_compact(a, A_, s);
    timer_.record(1, s);
    local_launch_scatter(a, A_, s);
    timer_.record(2, s);
    local_launch_sort(A_.depthKeys, A_.slotIndices, A_.tileCounts, a.tileCount, kLocalMaxPerTile, A_.sortedLocal,
                      A_.lists, A_.stats, s);
    timer_.record(3, s);
    local_launch_blend(a, A_, color, pitch, fmt, depth, depthPitch, dev_.numCUs, s);
    timer_.record(4, s);
    timer_.frameDone();
    lastCount_ = a.count;
    lastTilesX_ = a.tilesX;
    lastTilesY_ = a.tilesY;
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status LocalRenderer::counters(gsm_local_counters* out) {
    hipSetDevice(dev_.id);
    TileAssignmentHeader v;
    LocalStats st;
    if (hipMemcpy(&v, A_.visHdr, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&st, A_.stats, sizeof(st), hipMemcpyDeviceToHost) != hipSuccess)
        return GSM_ERR_RENDER_FAILED;
    out->gaussian_count = lastCount_;
    out->visible = v.totalAssignments;
    out->tiles_x = lastTilesX_;
    out->tiles_y = lastTilesY_;
    out->tile_count = lastTilesX_ * lastTilesY_;
    out->active_tiles = st.activeTiles;
    out->total_entries = st.totalEntries;
    out->max_tile_count = st.maxTileCount;
    out->max_per_tile = kLocalMaxPerTile;
    out->overflow = st.maxTileCount > kLocalMaxPerTile ? 1u : 0u;
    return GSM_OK;
}

gsm_status LocalRenderer::debugCopy(int which, void* dst, size_t bytes, size_t* needed) {
    gsm_local_counters c;
    gsm_status st = counters(&c);
    if (st != GSM_OK) return st;
    const void* src = nullptr;
    size_t full = 0;
    switch (which) {
        case GSM_LOCAL_BUF_PROJECTED: src = A_.compacted; full = (size_t)c.visible * sizeof(LocalProjected); break;
        case GSM_LOCAL_BUF_TILE_COUNTS: src = A_.tileCounts; full = (size_t)c.tile_count * 4; break;
        case GSM_LOCAL_BUF_TILE_LISTS: src = A_.lists; full = (size_t)c.tile_count * kLocalMaxPerTile * 4; break;
        default: return GSM_ERR_INVALID_ARGUMENT;
    }
    if (needed) *needed = full;
    if (!dst || bytes == 0 || full == 0) return GSM_OK;
    const size_t cpy = bytes < full ? bytes : full;
    if (hipMemcpy(dst, src, cpy, hipMemcpyDeviceToHost) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

}  // namespace gsm

struct gsm_local : gsm::Handle<gsm::LocalRenderer> {};

extern "C" {

gsm_status gsm_local_create(const gsm_renderer_config* config, int hip_device, gsm_local** out) {
    if (!config || !out) return GSM_ERR_INVALID_ARGUMENT;
    return gsm_local::create(out, *config, hip_device);
}

void gsm_local_destroy(gsm_local* r) { gsm_local::destroy(r); }

gsm_status gsm_local_render(gsm_local* r, void* stream, const gsm_gaussian_input* input,
                            const gsm_camera_params* camera, uint32_t width, uint32_t height, void* color,
                            size_t color_pitch_bytes, void* depth_r16f, size_t depth_pitch_bytes) {
    if (!r || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->render((hipStream_t)stream, *input, *camera, width, height, color, color_pitch_bytes, depth_r16f,
                           depth_pitch_bytes);
}

gsm_status gsm_local_debug_counters(gsm_local* r, gsm_local_counters* out) {
    if (!r || !out) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->counters(out);
}

gsm_status gsm_local_debug_copy(gsm_local* r, int which, void* host_dst, size_t bytes, size_t* needed) {
    if (!r) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->debugCopy(which, host_dst, bytes, needed);
}

gsm_status gsm_local_debug_sort_tiles(void* stream, const void* keys16, const void* indices, const void* counts,
                                      uint32_t tile_count, uint32_t max_per_tile, void* out_local_idx) {
    if (!keys16 || !indices || !counts || !out_local_idx) return GSM_ERR_INVALID_ARGUMENT;
    if (max_per_tile == 0 || max_per_tile > gsm::kLocalMaxPerTile) return GSM_ERR_INVALID_ARGUMENT;
    if (tile_count == 0) return GSM_OK;
    (void)hipGetLastError();
    gsm::local_launch_sort((const uint16_t*)keys16, (const uint32_t*)indices, (const uint32_t*)counts, tile_count,
                           max_per_tile, (uint16_t*)out_local_idx, nullptr, nullptr, (hipStream_t)stream);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status gsm_local_set_profiling(gsm_local* r, int enable) {
    if (!r) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->setProfiling(enable);
}

gsm_status gsm_local_stage_times(gsm_local* r, float* ms, int n) {
    if (!r || !ms) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->stageTimes(ms, n);
}

gsm_status gsm_local_last_gpu_time(gsm_local* r, double* seconds) {
    if (!r || !seconds) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->lastGpuTime(seconds);
}

}  // extern "C"

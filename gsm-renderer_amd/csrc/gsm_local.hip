// gsm_local.hip -- host orchestration and C ABI (include/gsm_local.h) of the LocalRenderer frame.
//
// The C++ analogue of LocalRenderer.render -> renderView (LocalRenderer.swift:83-257) over the
// LocalViewResources scratch set.  One HIP stream replaces the command buffer; grids are capacity-sized
// and the visible count is read on the device, so a frame is enqueue-only.  DESIGN.md 13.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/gsm_local.h"
#include "gsm_detmath.h"
#include "gsm_internal.h"
#include "gsm_local_internal.h"

namespace gsm {

static_assert(sizeof(gsm_local_projected) == sizeof(LocalProjected), "ProjectedGaussian layout");
static_assert(GSM_LOCAL_MAX_PER_TILE == kLocalMaxPerTile && GSM_LOCAL_TILE == kLocalTile, "header constants");

class LocalRenderer {
   public:
    static gsm_status create(const gsm_renderer_config& cfg, int hipDevice, LocalRenderer** out);
    ~LocalRenderer() { release(); }
    gsm_status render(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& cam, uint32_t width,
                      uint32_t height, void* color, size_t pitch, void* depth, size_t depthPitch);
    gsm_status counters(gsm_local_counters* out);
    gsm_status debugCopy(int which, void* dst, size_t bytes, size_t* needed);
    gsm_status setProfiling(int flags);
    gsm_status stageTimes(float* ms, int n);
    gsm_status lastGpuTime(double* seconds);

   private:
    LocalRenderer() = default;
    gsm_status alloc(void** p, size_t bytes);
    void release();
    int device_ = -1;
    int numCUs_ = 256;
    gsm_renderer_config config_{};
    uint32_t maxGaussians_ = 1, maxWidth_ = 1, maxHeight_ = 1, maxTiles_ = 1;
    LocalArena A_;
    std::vector<void*> allocations_;
    // last frame
    uint32_t lastCount_ = 0, lastTilesX_ = 0, lastTilesY_ = 0;
    // profiling: a ring of per-stage events
    static constexpr int kRing = 64;
    std::vector<hipEvent_t> events_;  // [kRing][GSM_LOCAL_STAGE_COUNT + 1]
    uint32_t profFrames_ = 0;
    int profiling_ = 0;
    hipEvent_t* frameEvents(uint32_t f) { return &events_[(f % kRing) * (GSM_LOCAL_STAGE_COUNT + 1)]; }
};

static size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

void LocalRenderer::release() {
    if (device_ >= 0) hipSetDevice(device_);
    for (void* p : allocations_) hipFree(p);
    allocations_.clear();
    for (auto& e : events_)
        if (e) hipEventDestroy(e);
    events_.clear();
}

gsm_status LocalRenderer::alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(p, align_up(bytes, 256)) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    allocations_.push_back(*p);
    return GSM_OK;
}

gsm_status LocalRenderer::create(const gsm_renderer_config& cfg, int hipDevice, LocalRenderer** out) {
    *out = nullptr;
    if (cfg.max_gaussians > kMaxSupportedGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (cfg.precision != GSM_PRECISION_FLOAT32 && cfg.precision != GSM_PRECISION_FLOAT16)
        return GSM_ERR_INVALID_ARGUMENT;
    if (cfg.color_format > GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB) return GSM_ERR_INVALID_ARGUMENT;
    const uint32_t maxW = cfg.max_width ? cfg.max_width : 1u, maxH = cfg.max_height ? cfg.max_height : 1u;
    // LocalRenderer.swift:67-70: maxTileCount and maxAssignments = maxTileCount * 2048
    const uint64_t tiles = (uint64_t)((maxW + kLocalTile - 1) / kLocalTile) * ((maxH + kLocalTile - 1) / kLocalTile);
    if (tiles > 65535u) return GSM_ERR_INVALID_TILE_COUNT;  // 16-bit tile coordinates, 512 MiB of slots
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return GSM_ERR_DEVICE_NOT_AVAILABLE;
    }
    int dev = hipDevice;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    LocalRenderer* r = new (std::nothrow) LocalRenderer();
    if (!r) return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    r->device_ = dev;
    r->config_ = cfg;
    r->maxGaussians_ = cfg.max_gaussians ? cfg.max_gaussians : 1u;
    r->maxWidth_ = maxW;
    r->maxHeight_ = maxH;
    r->maxTiles_ = (uint32_t)tiles;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        delete r;
        return GSM_ERR_DEVICE_NOT_AVAILABLE;
    }
    r->numCUs_ = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    const size_t G = r->maxGaussians_, slots = (size_t)r->maxTiles_ * kLocalMaxPerTile;
    const size_t nb = (G + kLocalBlock - 1) / kLocalBlock;
    LocalArena& A = r->A_;
    gsm_status st = GSM_OK;
#define GSM_LOCAL_ALLOC(ptr, bytes) \
    do {                            \
        if (st == GSM_OK) st = r->alloc((void**)&(ptr), (bytes)); \
    } while (0)
    GSM_LOCAL_ALLOC(A.temp, G * sizeof(LocalProjected));
    GSM_LOCAL_ALLOC(A.compacted, G * sizeof(LocalProjected));
    GSM_LOCAL_ALLOC(A.blockSums, (nb + 1) * 4);
    GSM_LOCAL_ALLOC(A.visHdr, sizeof(TileAssignmentHeader));
    GSM_LOCAL_ALLOC(A.queue, kQueueStripes * kQueueStride * sizeof(uint32_t));
    GSM_LOCAL_ALLOC(A.tileCounts, (size_t)r->maxTiles_ * 4);
    GSM_LOCAL_ALLOC(A.depthKeys, slots * sizeof(uint16_t));
    GSM_LOCAL_ALLOC(A.slotIndices, slots * sizeof(uint32_t));
    GSM_LOCAL_ALLOC(A.sortedLocal, slots * sizeof(uint16_t));
    GSM_LOCAL_ALLOC(A.lists, slots * sizeof(uint32_t));
    GSM_LOCAL_ALLOC(A.stats, sizeof(LocalStats));
    GSM_LOCAL_ALLOC(A.expTable, 65536 * 2);
#undef GSM_LOCAL_ALLOC
    if (st != GSM_OK) {
        delete r;
        return st;
    }
    std::vector<uint16_t> expt(65536);
    for (uint32_t i = 0; i < 65536; ++i) expt[i] = blend_exp_table_entry((uint16_t)i);
    if (hipMemcpy(A.expTable, expt.data(), 65536 * 2, hipMemcpyHostToDevice) != hipSuccess ||
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
    if (in.gaussian_count == 0 || in.gaussian_count > maxGaussians_) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (width == 0 || height == 0 || width > maxWidth_ || height > maxHeight_) return GSM_ERR_INVALID_DIMENSIONS;
    if (!color || !in.gaussians || !in.harmonics) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    const int fmt = (int)config_.color_format;
    const size_t bpp = fmt == GSM_COLOR_FORMAT_RGBA16F ? 8 : (fmt == GSM_COLOR_FORMAT_RGBA32F ? 16 : 4);
    if (pitch < (size_t)width * bpp) return GSM_ERR_INVALID_BUFFER_SIZE;
    if ((((uintptr_t)color) & 3u) || (pitch & 3u)) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (depth && (depthPitch < (size_t)width * 2 || (depthPitch & 1u) || (((uintptr_t)depth) & 1u)))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    if (hipSetDevice(device_) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;

    LocalArgs a;
    std::memset(&a, 0, sizeof(a));
    const float W = (float)width, H = (float)height;
    // CameraUniforms(from: camera, ...) (KernelTypes.swift:107-123) and the per-frame terms of
    // projectCovariance2D (GaussianShared.h:340-355), the same fp32 operations the reference repeats
    std::memcpy(a.view, cam.view, sizeof(a.view));
    std::memcpy(a.proj, cam.proj, sizeof(a.proj));
    const float p00 = cam.proj[0], p11 = cam.proj[5];
    a.limX = 1.3f * (1.0f / std::fmax(std::fabs(p00), 1e-4f));
    a.limY = 1.3f * (1.0f / std::fmax(std::fabs(p11), 1e-4f));
    a.focalX = W * std::fabs(p00) * 0.5f;
    a.focalY = H * std::fabs(p11) * 0.5f;
    a.width = W;
    a.height = H;
    a.nearPlane = cam.near_plane;
    a.farPlane = cam.far_plane;
    const float maxDim = std::fmax(W, H);
    const float maxEig = (maxDim * 2.0f) / 3.0f;
    a.maxEig = maxEig * maxEig;
    a.adjFar = a.farPlane * 0.02f;
    a.adjDen = a.adjFar - a.nearPlane;
    for (int i = 0; i < 3; ++i) a.camPos[i] = cam.position[i];
    a.inputIsSRGB = config_.gaussian_color_space == GSM_COLOR_SPACE_SRGB ? 1.0f : 0.0f;
    a.shComponents = in.sh_components;
    a.count = in.gaussian_count;
    a.tilesX = (width + kLocalTile - 1) / kLocalTile;  // LocalRenderer.swift:143-145
    a.tilesY = (height + kLocalTile - 1) / kLocalTile;
    a.tileCount = a.tilesX * a.tilesY;
    const uint32_t k = in.sh_components;
    const uint32_t deg = k <= 1 ? 0u : (k <= 4 ? 1u : (k <= 9 ? 2u : 3u));
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    const uint32_t nb = (a.count + kLocalBlock - 1) / kLocalBlock;

    const bool prof = profiling_ != 0;
    hipEvent_t* ev = prof ? frameEvents(profFrames_) : nullptr;
    if (prof) hipEventRecord(ev[0], s);
    local_launch_clear(a, A_, s);
    local_launch_project(half, deg, in.gaussians, in.harmonics, a, A_, s);
    launch_scan_sums(A_.blockSums, nb, maxGaussians_, A_.visHdr, A_.queue, s);
    local_launch_compact(a, A_, s);
    if (prof) hipEventRecord(ev[1], s);
    local_launch_scatter(a, A_, s);
    if (prof) hipEventRecord(ev[2], s);
    local_launch_sort(A_.depthKeys, A_.slotIndices, A_.tileCounts, a.tileCount, kLocalMaxPerTile, A_.sortedLocal,
                      A_.lists, A_.stats, s);
    if (prof) hipEventRecord(ev[3], s);
    local_launch_blend(a, A_, color, pitch, fmt, depth, depthPitch, numCUs_, s);
    if (prof) {
        hipEventRecord(ev[4], s);
        profFrames_++;
    }
    lastCount_ = a.count;
    lastTilesX_ = a.tilesX;
    lastTilesY_ = a.tilesY;
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status LocalRenderer::counters(gsm_local_counters* out) {
    hipSetDevice(device_);
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

gsm_status LocalRenderer::setProfiling(int flags) {
    hipSetDevice(device_);
    if (flags && events_.empty()) {
        events_.assign((size_t)kRing * (GSM_LOCAL_STAGE_COUNT + 1), nullptr);
        for (auto& e : events_)
            if (hipEventCreate(&e) != hipSuccess) return GSM_ERR_ENCODER_CREATION_FAILED;
    }
    profiling_ = flags;
    profFrames_ = 0;
    return GSM_OK;
}

gsm_status LocalRenderer::stageTimes(float* ms, int n) {
    if (profFrames_ == 0 || events_.empty()) return GSM_ERR_RENDER_FAILED;
    hipSetDevice(device_);
    if (hipEventSynchronize(frameEvents(profFrames_ - 1)[GSM_LOCAL_STAGE_COUNT]) != hipSuccess)
        return GSM_ERR_RENDER_FAILED;
    const uint32_t frames = profFrames_ < (uint32_t)kRing ? profFrames_ : (uint32_t)kRing;
    for (int i = 0; i < n && i < GSM_LOCAL_STAGE_COUNT; ++i) {
        double acc = 0.0;
        for (uint32_t f = profFrames_ - frames; f < profFrames_; ++f) {
            float t = 0.f;
            if (hipEventElapsedTime(&t, frameEvents(f)[i], frameEvents(f)[i + 1]) != hipSuccess)
                return GSM_ERR_RENDER_FAILED;
            acc += t;
        }
        ms[i] = (float)(acc / frames);
    }
    return GSM_OK;
}

gsm_status LocalRenderer::lastGpuTime(double* seconds) {
    if (profFrames_ == 0 || events_.empty()) return GSM_ERR_RENDER_FAILED;
    hipSetDevice(device_);
    hipEvent_t* ev = frameEvents(profFrames_ - 1);
    if (hipEventSynchronize(ev[GSM_LOCAL_STAGE_COUNT]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    float t = 0.f;
    if (hipEventElapsedTime(&t, ev[0], ev[GSM_LOCAL_STAGE_COUNT]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    *seconds = (double)t * 1e-3;
    return GSM_OK;
}

}  // namespace gsm

struct gsm_local {
    gsm::LocalRenderer* impl;
};

extern "C" {

gsm_status gsm_local_create(const gsm_renderer_config* config, int hip_device, gsm_local** out) {
    if (!config || !out) return GSM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    gsm::LocalRenderer* impl = nullptr;
    gsm_status st = gsm::LocalRenderer::create(*config, hip_device, &impl);
    if (st != GSM_OK) return st;
    gsm_local* h = new (std::nothrow) gsm_local;
    if (!h) {
        delete impl;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    h->impl = impl;
    *out = h;
    return GSM_OK;
}

void gsm_local_destroy(gsm_local* r) {
    if (!r) return;
    delete r->impl;
    delete r;
}

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

// gsm_host.hip -- the shared host layer (gsm_host.h), out of line.  No kernels.
#include "gsm_host.h"

#include <cmath>
#include <cstring>

#include "gsm_types.h"

namespace gsm {

gsm_status check_config(const gsm_renderer_config& cfg) {
    if (cfg.max_gaussians > kMaxSupportedGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (cfg.precision != GSM_PRECISION_FLOAT32 && cfg.precision != GSM_PRECISION_FLOAT16)
        return GSM_ERR_INVALID_ARGUMENT;
    if (cfg.color_format > GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

gsm_status pick_device(int requested, Device* out) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        (void)hipGetLastError();
        return GSM_ERR_DEVICE_NOT_AVAILABLE;
    }
    int dev = requested;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (dev >= ndev || hipSetDevice(dev) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    out->id = dev;
    out->numCUs = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    return GSM_OK;
}

DeviceAllocations::~DeviceAllocations() {
    if (device_ >= 0) hipSetDevice(device_);
    for (void* p : allocations_) hipFree(p);
}

gsm_status DeviceAllocations::alloc(void** p, size_t bytes) {
    *p = nullptr;
    if (bytes == 0) bytes = 16;
    if (hipMalloc(p, (bytes + 255) / 256 * 256) != hipSuccess) {
        (void)hipGetLastError();
        *p = nullptr;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    allocations_.push_back(*p);
    return GSM_OK;
}

StageTimer::~StageTimer() {
    for (auto& e : events_)
        if (e) hipEventDestroy(e);
}

gsm_status StageTimer::setProfiling(int flags) {
    if ((flags & 9) && events_.empty()) {  // bit 0 (every stage) or bit 3 (blend only)
        events_.assign((size_t)ring_ * (stages_ + 1), nullptr);
        for (auto& e : events_)
            if (hipEventCreate(&e) != hipSuccess) return GSM_ERR_ENCODER_CREATION_FAILED;
    }
    flags_ = flags;
    frames_ = 0;
    sample_ = 0;
    return GSM_OK;
}

gsm_status StageTimer::stageTimes(float* ms, int n, int blendStage) {
    if (frames_ == 0) return GSM_ERR_RENDER_FAILED;
    if (hipEventSynchronize(frameEvents(frames_ - 1)[stages_]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    const uint32_t frames = frames_ < (uint32_t)ring_ ? frames_ : (uint32_t)ring_;
    const bool blendOnly = (flags_ & 1) == 0;  // bit 3: only the blend's pair of events exists
    for (int i = 0; i < n && i < stages_; ++i) {
        if (blendOnly && i != blendStage) {
            ms[i] = 0.0f;
            continue;
        }
        double acc = 0.0;
        for (uint32_t f = frames_ - frames; f < frames_; ++f) {
            float t = 0.f;
            hipEvent_t* ev = frameEvents(f);
            if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
            acc += t;
        }
        ms[i] = (float)(acc / frames);
    }
    return GSM_OK;
}

gsm_status StageTimer::lastGpuTime(double* seconds) {
    // the whole-frame span needs event 0, which only the every-stage mode records
    if (frames_ == 0 || (flags_ & 1) == 0) return GSM_ERR_RENDER_FAILED;
    float ms[1];
    hipEvent_t* ev = frameEvents(frames_ - 1);
    if (hipEventSynchronize(ev[stages_]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    if (hipEventElapsedTime(ms, ev[0], ev[stages_]) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    *seconds = (double)ms[0] * 1e-3;
    return GSM_OK;
}

ProjectionUniforms projection_uniforms(const float proj[16], float width, float height, float nearPlane,
                                       float farPlane) {
    ProjectionUniforms u;
    const float p00 = proj[0], p11 = proj[5];
    u.limX = 1.3f * (1.0f / std::fmax(std::fabs(p00), 1e-4f));
    u.limY = 1.3f * (1.0f / std::fmax(std::fabs(p11), 1e-4f));
    u.focalX = width * std::fabs(p00) * 0.5f;
    u.focalY = height * std::fabs(p11) * 0.5f;
    const float maxDim = std::fmax(width, height);
    const float maxEig = (maxDim * 2.0f) / 3.0f;
    u.maxEig = maxEig * maxEig;
    u.adjFar = farPlane * 0.02f;
    u.adjDen = u.adjFar - nearPlane;
    return u;
}

gsm_status copy_bounds_int4(const short4* bounds, size_t n, void* dst, size_t bytes) {
    std::vector<short4> b(n);
    if (n && hipMemcpy(b.data(), bounds, n * sizeof(short4), hipMemcpyDeviceToHost) != hipSuccess)
        return GSM_ERR_RENDER_FAILED;
    std::vector<int32_t> w(n * 4);
    for (size_t i = 0; i < n; ++i) {
        w[4 * i + 0] = b[i].x;
        w[4 * i + 1] = b[i].y;
        w[4 * i + 2] = b[i].z;
        w[4 * i + 3] = b[i].w;
    }
    if (n) std::memcpy(dst, w.data(), bytes < n * 16 ? bytes : n * 16);
    return GSM_OK;
}

gsm_status copy_headers(const uint32_t* starts, size_t tiles, void* dst, size_t bytes) {
    std::vector<uint32_t> ts(tiles + 1);
    if (hipMemcpy(ts.data(), starts, ts.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    std::vector<uint32_t> h(tiles * 2);
    for (size_t t = 0; t < tiles; ++t) {
        h[2 * t] = ts[t];
        h[2 * t + 1] = ts[t + 1] >= ts[t] ? ts[t + 1] - ts[t] : 0u;
    }
    if (tiles) std::memcpy(dst, h.data(), bytes < tiles * 8 ? bytes : tiles * 8);
    return GSM_OK;
}

}  // namespace gsm

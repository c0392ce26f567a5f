// gsm_host.h -- the host layer the Global, DepthFirst and Local renderers share (no kernels):
// device pick, device allocations, the stage-event ring, frame validation, the uniform terms of
// the projection, table uploads, readback conversions and the C handle.  DESIGN.md 15.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <new>
#include <utility>
#include <vector>

#include "../../include/gsm_renderer.h"
#include "gsm_frame_plan.h"

namespace gsm {

// ---- config ----
// the guards every renderer's init shares (GlobalRenderer.swift:111-113)
gsm_status check_config(const gsm_renderer_config& cfg);
// SH_DEGREE selection (GlobalProjectCullEncoder.swift:19-26)
inline uint32_t sh_degree(uint32_t components) {
    return components <= 1 ? 0u : (components <= 4 ? 1u : (components <= 9 ? 2u : 3u));
}

// ---- device ----
struct Device {
    int id = -1;
    int numCUs = 256;
};
// requested < 0: the current device.  Makes the device current.  GSM_ERR_DEVICE_NOT_AVAILABLE for
// no device, an id past the count, or a failed set / properties query.
gsm_status pick_device(int requested, Device* out);

// ---- allocations ----
// Owner of a renderer's device buffers: freed together, on the renderer's device.
class DeviceAllocations {
   public:
    DeviceAllocations() = default;
    DeviceAllocations(const DeviceAllocations&) = delete;
    DeviceAllocations& operator=(const DeviceAllocations&) = delete;
    ~DeviceAllocations();
    void setDevice(int device) { device_ = device; }
    // 0 bytes become 16, sizes round up to 256; a failure clears HIP's last error
    gsm_status alloc(void** p, size_t bytes);
    // the same, skipped once `st` is bad
    template <class T>
    void alloc(gsm_status& st, T*& p, size_t bytes) {
        if (st == GSM_OK) st = alloc((void**)&p, bytes);
    }

   private:
    int device_ = -1;
    std::vector<void*> allocations_;
};

// ---- stage timer ----
// A ring of per-frame HIP events, stages + 1 a frame: stage i runs between events i and i + 1.
// Profiling flags: bit 0 brackets every stage; bit 3 (without bit 0) only the blend, on every
// frame or, with a period in bits 8-15, on every period-th.  The events are created by the first
// setProfiling that needs them, on the device current then.
class StageTimer {
   public:
    enum Events { kNone, kBlendPair, kEveryStage };
    StageTimer(int stages, int ring) : stages_(stages), ring_(ring) {}
    StageTimer(const StageTimer&) = delete;
    StageTimer& operator=(const StageTimer&) = delete;
    ~StageTimer();
    gsm_status setProfiling(int flags);  // restarts the averaging window
    int flags() const { return flags_; }
    // which events the frame about to be enqueued records
    Events beginFrame() {
        const bool every = (flags_ & 1) != 0;
        const uint32_t period = ((uint32_t)flags_ >> 8) & 0xFFu;
        const bool blend = !every && (flags_ & 8) != 0 && (period <= 1 || (sample_++ % period) == 0);
        return now_ = every ? kEveryStage : (blend ? kBlendPair : kNone);
    }
    // event `boundary` of the frame; blendPair: one of the two events around the blend
    void record(int boundary, hipStream_t s, bool blendPair = false) {
        if (now_ == kEveryStage || (now_ == kBlendPair && blendPair)) hipEventRecord(frameEvents(frames_)[boundary], s);
    }
    void frameDone() {
        if (now_ != kNone) frames_++;
    }
    // the average over the profiled frames still in the ring; blend-only mode: 0 for the other stages
    gsm_status stageTimes(float* ms, int n, int blendStage);
    gsm_status lastGpuTime(double* seconds);  // the last profiled frame's whole span (needs bit 0)

   private:
    hipEvent_t* frameEvents(uint32_t f) { return &events_[(size_t)(f % (uint32_t)ring_) * (stages_ + 1)]; }
    const int stages_, ring_;
    std::vector<hipEvent_t> events_;  // [ring][stages + 1]
    int flags_ = 0;
    uint32_t frames_ = 0;  // profiled frames since setProfiling
    uint32_t sample_ = 0;  // frames since setProfiling that took part in the blend-event sampling
    Events now_ = kNone;
};

// ---- frame ----
// validate_frame, PickTarget, OccluderSource and color_bytes_per_pixel: gsm_frame_plan.h (plain C++, tested on the CPU)

// The per-frame terms of projectCovariance2D (GaussianShared.h:340-355), the same fp32 operations
// in the same order as the reference repeats per gaussian: part of the numeric contract.
struct ProjectionUniforms {
    float limX, limY, focalX, focalY, maxEig, adjFar, adjDen;
};
ProjectionUniforms projection_uniforms(const float proj[16], float width, float height, float nearPlane,
                                       float farPlane);

// ---- tables and readback ----
constexpr uint32_t kTableEntries = 65536;
// entry(i) for every i < 65,536 (or `entries`, for a table with a tail) into the device table `dst`
template <class T, class Entry>
gsm_status upload_table(T* dst, Entry&& entry, uint32_t entries = kTableEntries) {
    std::vector<T> t(entries);
    for (uint32_t i = 0; i < entries; ++i) t[i] = entry(i);
    return hipMemcpy(dst, t.data(), entries * sizeof(T), hipMemcpyHostToDevice) == hipSuccess
               ? GSM_OK
               : GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
}
// n device short4 tile rects as the reference's int4, the first `bytes` of them into dst
gsm_status copy_bounds_int4(const short4* bounds, size_t n, void* dst, size_t bytes);
// tile run starts [tiles + 1] as the reference's {offset, count} headers, the first `bytes` into dst
gsm_status copy_headers(const uint32_t* starts, size_t tiles, void* dst, size_t bytes);

// ---- C handle ----
// What an opaque C handle points to: `struct gsm_x : gsm::Handle<X> {}`.
template <class Impl>
struct Handle {
    Impl* impl = nullptr;
    // Impl::create(args..., &impl) wrapped in a new H
    template <class H, class... Args>
    static gsm_status create(H** out, Args&&... args) {
        *out = nullptr;
        Impl* impl = nullptr;
        gsm_status st = Impl::create(std::forward<Args>(args)..., &impl);
        if (st != GSM_OK) return st;
        H* h = new (std::nothrow) H;
        if (!h) {
            delete impl;
            return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
        }
        h->impl = impl;
        *out = h;
        return GSM_OK;
    }
    template <class H>
    static void destroy(H* h) {
        if (!h) return;
        delete h->impl;
        delete h;
    }
};

}  // namespace gsm

// gsm_renderer_impl.h -- C++ GlobalRenderer behind the C ABI (include/gsm_renderer.h).
// Mirrors the reference class GlobalRenderer (GlobalRenderer.swift:72-572).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/gsm_debug.h"
#include "../../include/gsm_renderer.h"
#include "gsm_extract_check.h"
#include "gsm_host.h"
#include "gsm_internal.h"
#include "gsm_schedule_key.h"
#include "gsm_select_check.h"
#include "gsm_transform_check.h"

namespace gsm {

// (FrameExtras, StyleSource, PickTarget, OccluderSource, BatchViewOptions: gsm_frame_plan.h, with the entries' checks)
class GlobalRenderer {
   public:
    // GlobalRenderer.init(device:config:) (GlobalRenderer.swift:110-193)
    static gsm_status create(const gsm_renderer_config& cfg, int hipDevice, GlobalRenderer** out);
    ~GlobalRenderer() { hipSetDevice(dev_.id); }  // (the events and buffers are released on their device)

    // GlobalRenderer.render (GlobalRenderer.swift:201-238): gsm_global_render and its pick / occluded / styled
    // entries
    gsm_status renderFrame(hipStream_t stream, const gsm_gaussian_input& input, const gsm_camera_params& camera,
                           uint32_t width, uint32_t height, const FrameTargets& targets,
                           const FrameExtras& extras = {});
    // several posed objects in one frame over one tile space and one target: gsm_global_render_composite and its
    // pick / occluded / styled entries
    gsm_status composeFrame(hipStream_t stream, const gsm_global_object* objects, uint32_t objectCount,
                            uint32_t width, uint32_t height, const FrameTargets& targets,
                            const FrameExtras& extras = {});

    // several views of one scene in one frame over a combined tile space (gsm_global_render_views)
    gsm_status renderViews(hipStream_t stream, const gsm_gaussian_input& input, const gsm_camera_params* cameras,
                           uint32_t viewCount, uint32_t width, uint32_t height, void* color, size_t colorPitch,
                           size_t colorStride, void* depth, size_t depthPitch, size_t depthStride);

    // views of different scenes and sizes in one frame (gsm_global_render_batch)
    gsm_status renderBatch(hipStream_t stream, const gsm_global_view* views, uint32_t viewCount);
    // the same batch from frame descriptors, each with its own nullable pick target, occluder and styles
    // (gsm_global_render_frames)
    gsm_status renderFrames(hipStream_t stream, const gsm_global_frame* frames, uint32_t frameCount);

    // state bytes of the gaussians whose projected centre lies on a nonzero mask byte (gsm_global_select_mask;
    // orthographic: gsm_global_select_mask_ortho)
    gsm_status selectMask(hipStream_t stream, const gsm_gaussian_input* input, const gsm_camera_params* camera,
                          uint32_t width, uint32_t height, const void* mask, size_t maskPitch, uint8_t* state,
                          const gsm_global_style* styles, uint32_t styleCount, uint32_t andMask, uint32_t xorMask,
                          uint32_t* matched, bool orthographic = false);
    // state bytes of the gaussians of `object` that the last pick frame's image shows under the mask
    // (gsm_global_select_pick)
    gsm_status selectPick(hipStream_t stream, const void* pick, size_t pickPitch, uint32_t width, uint32_t height,
                          const void* mask, size_t maskPitch, uint32_t object, uint8_t* state, uint32_t gaussianCount,
                          uint32_t andMask, uint32_t xorMask, uint32_t* matched);
    // the stateless form for pick images that hold gaussian ids (gsm_global_select_pick_ids)
    gsm_status selectPickIds(hipStream_t stream, const void* pick, size_t pickPitch, uint32_t width, uint32_t height,
                             const void* mask, size_t maskPitch, uint8_t* state, uint32_t gaussianCount,
                             uint32_t andMask, uint32_t xorMask, uint32_t* matched);
    // the rows of the gaussians whose state byte is in the keep set, in ascending id order (gsm_global_extract,
    // DESIGN.md 28); the handle's last-frame state is neither read nor changed
    gsm_status extract(hipStream_t stream, const gsm_gaussian_input* input, const gsm_global_state* state,
                       const uint32_t* keep, const gsm_global_extract_out* out, uint32_t* kept);
    // the number of gaussians of every state value (gsm_global_state_histogram)
    gsm_status stateHistogram(hipStream_t stream, const uint8_t* state, uint32_t gaussianCount, uint32_t* histogram);
    // the state bytes of the gaussians whose records match the query become (old & andMask) ^ xorMask
    // (gsm_global_select_where): no camera, no frame state
    gsm_status selectWhere(hipStream_t stream, const gsm_gaussian_input* input, const gsm_global_select_query* query,
                           uint8_t* state, const gsm_global_style* styles, uint32_t styleCount, uint32_t andMask,
                           uint32_t xorMask, uint32_t* matched);
    // the axis-aligned box and the count of the gaussians whose state byte is in the keep set (gsm_global_state_bounds)
    gsm_status stateBounds(hipStream_t stream, const gsm_gaussian_input* input, const gsm_global_state* state,
                           const uint32_t* keep, gsm_global_bounds* bounds);
    // the pose of `desc` baked into the records and harmonics of the gaussians whose state byte is in the keep set,
    // in place (gsm_global_transform): no frame state, nothing allocated
    gsm_status transform(hipStream_t stream, const gsm_global_scene* scene, const gsm_global_state* state,
                         const uint32_t* keep, const gsm_global_transform_desc* desc);
    // items of the last enqueued pick frame -> (object of the call, gaussian id within it); host only, no sync
    gsm_status pickOwner(const uint32_t* items, uint32_t n, uint32_t* object, uint32_t* gaussian) const;

    // multi-GPU partition: project ids [first, first+count) and pack the splat
    // records of every tile-row slab they meet; render a slab from the records it received
    gsm_status projectPartition(hipStream_t stream, const gsm_gaussian_input& input,
                                const gsm_camera_params& camera, uint32_t width, uint32_t height,
                                uint32_t first, uint32_t count, const uint32_t* slabRows, uint32_t numSlabs,
                                void* send, uint64_t capacity, uint32_t* sendCounts, bool interleave = false);
    // the same projection for the direct exchange: per-slab counts first, then the records written
    // into every slab owner's receive buffer once the count matrix is on the device (gsm_multigpu.hip)
    // orderUnits: the launch also orders the blend units of the renderer's own rows (set_tile_rows) for a
    // later renderRecords(..., preOrdered = true) of the same frame
    // publish (multi-GPU frame): the per-slab totals also go into every rank's count matrix and the
    // scan's workgroups arrive at barrier 0 (gsm_multigpu.hip); null: counts only
    gsm_status partitionCounts(hipStream_t stream, const gsm_gaussian_input& input, const gsm_camera_params& camera,
                               uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                               const uint32_t* slabRows, uint32_t numSlabs, uint32_t* sendCounts,
                               bool orderUnits = false, bool interleave = false, const CountPublish* publish = nullptr);
    // the push's workgroups arrive at `arrive`'s barrier after their record stores
    gsm_status partitionPush(hipStream_t stream, uint32_t world, uint32_t rank, const uint32_t* counts,
                             const SlabPeers& peers, uint32_t* recvCount, const MgArrive& arrive);
    // blendArrive (nullable): the blend's waves arrive at that barrier after their pixel stores
    gsm_status renderRecords(hipStream_t stream, const void* records, uint32_t count, uint32_t width,
                             uint32_t height, void* color, size_t colorPitch, void* depth, size_t depthPitch,
                             const uint32_t* devCount = nullptr, bool preOrdered = false,
                             const MgArrive* blendArrive = nullptr);
    // what renderRecords / the multi-GPU frame would refuse, checked before anything is enqueued
    gsm_status validateFrame(uint32_t count, bool inputMissing, uint32_t width, uint32_t height,
                             const void* color, size_t colorPitch, const void* depth, size_t depthPitch) const;
    // the partition buffers (allocated lazily by the first partition frame; the multi-GPU frame
    // allocates them at prepare so that no frame can fail on an allocation)
    gsm_status ensurePartitionBuffers(uint32_t numSlabs);
    // The multi-GPU frame's two sets of blend-schedule buffers (unit costs, order, longest walk):
    // frame f uses set f & 1 in its projection (ordering) and in its blend, so with frame f + 1's
    // projection running beside frame f's blend (gsm_multigpu pipelined) neither reads what the other
    // writes; the ordering then follows the walks of frame f - 2.  Set 1 is allocated by
    // ensurePartitionBuffers.
    void selectSchedule(uint32_t parity);
    uint32_t maxGaussians() const { return maxGaussians_; }
    uint32_t tilesY() const { return tilesY_; }
    uint32_t maxWidth() const { return maxWidth_; }
    uint32_t maxHeight() const { return maxHeight_; }
    uint32_t colorBytesPerPixel() const { return color_bytes_per_pixel(config_.color_format); }
    bool halfPrecision() const { return config_.precision == GSM_PRECISION_FLOAT16; }

    gsm_status counters(gsm_debug_counters* out);
    int lastBlendKernel() const { return lastBlendKernel_; }
    gsm_status debugCopy(int which, void* dst, size_t bytes, size_t* needed);
    gsm_status setProfiling(int flags);  // bit0: stage events, bit1: keep unsorted keys
    gsm_status stageTimes(float* ms, int n) {
        hipSetDevice(dev_.id);
        return timer_.stageTimes(ms, n, GSM_STAGE_BLEND);
    }
    gsm_status lastGpuTime(double* seconds) {
        hipSetDevice(dev_.id);
        return timer_.lastGpuTime(seconds);
    }
    // the renderer's tile rows: begin, begin + stride, ... < end (0, 0: the whole frame)
    gsm_status setTileRows(uint32_t begin, uint32_t end, uint32_t stride = 1);
    uint32_t rowCount() const { return rowEnd_ > rowBegin_ ? (rowEnd_ - rowBegin_ + rowStride_ - 1) / rowStride_ : 0u; }
    int device() const { return dev_.id; }

   private:
    GlobalRenderer() = default;
    // the handle's style table: allocated by its first use, filled from the caller's styles (identity past them)
    gsm_status fillStyleTable(hipStream_t s, const gsm_global_style* styles, uint32_t styleCount);
    // orthographic: the uniforms of the orthographic rule in place of the perspective terms (ProjectArgs)
    ProjectArgs frameArgs(const gsm_camera_params& camera, uint32_t width, uint32_t height, uint32_t count,
                          uint32_t shComponents, bool orthographic = false) const;
    // One description of a frame: everything runFrame enqueues, the projection (or records) launch in front.
    // (Views: args holds what the views share, the targets are view 0's.  Batch: args holds what the views share,
    // nothing per view.  Compose: args is the frame's, as a single frame's; only the items differ.)
    struct FrameRequest {
        ProjectArgs args;
        uint32_t width = 0, height = 0;
        FrameTargets targets;
        FramePayload payload;  // the kind and its payload
        // what the front launch reads: a Single or Views frame's scene (a Batch's and a Compose's travel in their
        // entries), the SH degree of the frame's scenes, a Records frame's received records
        const void* world = nullptr;
        const void* harm = nullptr;
        uint32_t shDegree = 0;
        const void* records = nullptr;
        const PickTarget* pick = nullptr;
        const OccluderSource* occluder = nullptr;
        // table non-null: the projection applies styles (state / defaultState: a Single frame's), and the walks are
        // the frame's own (schedule key)
        StyleArgs style;
        // the projection follows the orthographic rule (a Batch: some view's does): the footprints, and with them
        // the walks, are the frame's own (schedule key)
        bool orthographic = false;
        // a Batch with options (renderFrames): some view has a pick target / an occluder.  The targets themselves
        // are per view (BatchFrame::extras); these are the union the schedule key and the blend's kernel follow.
        bool anyPick = false, anyOccluder = false;
        // the records path: the count on the device, the units ordered by an earlier partitionCounts, the barrier
        // the blend's waves arrive at
        const uint32_t* devCount = nullptr;
        bool preOrdered = false;
        const MgArrive* blendArrive = nullptr;
    };
    FrameRequest request(FrameKind kind, const ProjectArgs& args, uint32_t width, uint32_t height,
                         const FrameTargets& targets) const;
    // the projection (or records) launch, then scan, scatter, sort, headers and blend
    gsm_status runFrame(hipStream_t s, const FrameRequest& rq);
    // the request's schedule key in key_ (reserved: no allocation) and the tiles its blend units cover
    const ScheduleKey& requestKey(const FrameRequest& rq, uint32_t* tiles);
    // the blend schedule's unit count for a frame of that key over `tiles` tiles (0 when cost order is off), the
    // cost arrays cleared when the key is not the one they belong to
    uint32_t scheduleUnits(hipStream_t s, const ScheduleKey& key, uint32_t tiles);
    // what the handle contributes to the entries' checks (gsm_frame_plan.h)
    FrameLimits limits() const {
        FrameLimits L;
        L.colorFormat = config_.color_format;
        L.maxGaussians = maxGaussians_;
        L.maxWidth = maxWidth_;
        L.maxHeight = maxHeight_;
        L.tileCount = tileCount_;
        L.tilesY = tilesY_;
        L.rowsRestricted = tileRowsRestricted();
        L.rowStride = rowStride_;
        return L;
    }
    bool tileRowsRestricted() const { return rowBegin_ != 0 || rowEnd_ != tilesY_ || rowStride_ != 1; }
    // the ProjectArgs of what renderViews and a batch share: view 0's, on that view's own grid
    ProjectArgs batchSharedArgs(const gsm_camera_params& camera0, uint32_t width0, uint32_t height0, uint32_t count,
                                uint32_t shComponents) const;
    // renderBatch and renderFrames after check_batch: the lazy allocations, the per-view entries and tables from the
    // layout, the request, the frame.  options (nullable, [viewCount]): null is the plain batch, device code and all.
    gsm_status enqueueBatch(hipStream_t s, const gsm_global_view* views, uint32_t viewCount,
                            const BatchViewOptions* options);
    // the tail selectPick and selectPickIds share: the bitmap (allocated by the first call) and the two launches
    gsm_status enqueueSelectPick(hipStream_t s, const void* pick, size_t pickPitch, uint32_t width, uint32_t height,
                                 const void* mask, size_t maskPitch, uint32_t base, uint32_t n, uint8_t* state,
                                 uint32_t andMask, uint32_t xorMask, uint32_t* matched);
    PartitionBuffers part_;
    uint32_t partCount_ = 0;  // ids of the last partitionCounts
    SlabTable partSlabs_{};
    struct ScheduleSet {
        uint16_t* unitCost = nullptr;
        uint32_t* unitOrder = nullptr;
        uint32_t* costMax = nullptr;
    } sched_[2];   // its slab table (partitionPush cuts each record's tile answers by it)
    struct PartitionFrame {
        ProjectArgs a;
        SlabTable slabs;
        const void* world;
        const void* harm;
        uint32_t deg;
        bool half;
    };
    gsm_status preparePartition(const gsm_gaussian_input& in, const gsm_camera_params& camera, uint32_t width,
                                uint32_t height, uint32_t first, uint32_t count, const uint32_t* slabRows,
                                uint32_t numSlabs, bool needSend, const void* send, const uint32_t* sendCounts,
                                PartitionFrame* f, bool interleave = false);
    int sortPassCount() const;

    Device dev_;
    gsm_renderer_config config_{};
    Tuning tuning_{};  // A/B switches, read once at create
    uint32_t maxGaussians_ = 1, maxWidth_ = 1, maxHeight_ = 1;
    uint32_t tilesX_ = 1, tilesY_ = 1, tileCount_ = 1;
    uint32_t rowBegin_ = 0, rowEnd_ = 1, rowStride_ = 1;
    uint32_t maxAssignments_ = 4;
    DeviceArena arena_;
    DeviceAllocations allocs_;
    StageTimer timer_{GSM_STAGE_COUNT, 128};  // the last 128 profiled frames are averaged
    int lastBlendKernel_ = 0;  // gsm_blend_kernel of the last enqueued frame (gsm_global_debug_blend_kernel)
    bool keptRenderData_ = false;  // the last frame wrote GaussianRenderData for readback
    uint32_t lastCount_ = 0, lastWidth_ = 0, lastHeight_ = 0;
    uint32_t lastItems_ = 0;  // entries of the last frame's per-gaussian arrays (a composite: 256 per block)
    const uint32_t* sortedKeys_ = nullptr;
    const uint32_t* sortedVals_ = nullptr;
    const uint32_t* unsortedKeys_ = nullptr;
    const uint32_t* unsortedVals_ = nullptr;
    unsigned long long* traceBuf_ = nullptr;  // blend unit trace (profiling bit 2)
    ScheduleKey key_;                         // this call's schedule key
    ScheduleState schedState_;                // the key the unit costs belong to
    std::vector<ViewArgs> viewHost_;          // the last batch's per-view terms (render_views)
    uint32_t maxViews_ = 0;                   // entries of arena_.viewArgs
    std::vector<BatchViewArgs> batchHost_;    // the last batch's per-view entries (render_batch)
    uint32_t maxBatchViews_ = 0;              // entries of arena_.batchArgs
    std::vector<BatchExtras> extrasHost_;     // the last batch's per-view options (render_frames)
    std::vector<gsm_global_view> framesViews_;      // render_frames: the call's frames as batch views ...
    std::vector<BatchViewOptions> framesOptions_;   // ... and what each adds
    std::vector<ComposeObjectArgs> composeHost_;  // the last composite's per-object entries (render_composite)
    std::vector<uint32_t> composeObject_;     // the call's object index of every entry of composeHost_
    bool lastPick_ = false;                   // the last enqueued frame was a pick frame (pickOwner)
    bool lastPickComposite_ = false;          // ... of a composite: its owners are composeHost_ / composeObject_
    uint32_t lastPickObjects_ = 0;            // ... and the objects of that call (1 for a single frame)
};

}  // namespace gsm

struct gsm_renderer : gsm::Handle<gsm::GlobalRenderer> {};

// gsm_depthfirst.hip -- host orchestration and C ABI (include/gsm_depthfirst.h) of the
// DepthFirst stereo side-by-side path on MI355X.
//
// The C++ analogue of DepthFirstRenderer.renderStereo(target: .sideBySide) ->
// renderStereoSideBySideRaster -> encodeStereoPipeline (DepthFirstRenderer.swift:205-223,
// 469-512, 595-831) over the DepthFirstResources scratch set (DepthFirstResources.swift:380-470).
// One HIP stream replaces the command buffer; grids are capacity-sized and data-dependent
// counts are read on the device, so a frame is enqueue-only.
// The mono frame, DepthFirstRenderer.render -> encodeRender (:166-203, 237-465), runs on the same
// handle and arena (renderMono).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/gsm_depthfirst.h"
#include "gsm_detmath.h"
#include "gsm_df_internal.h"
#include "gsm_host.h"
#include "gsm_internal.h"

namespace gsm {

class DepthFirstRenderer {
   public:
    static gsm_status create(const gsm_renderer_config& cfg, int hipDevice, const gsm_depthfirst_options& opt,
                             DepthFirstRenderer** out);
    const gsm_depthfirst_options& options() const { return options_; }
    ~DepthFirstRenderer() { hipSetDevice(dev_.id); }  // (the events and buffers are released on their device)
    gsm_status renderStereoSbs(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& left,
                               const gsm_camera_params& right, const float* scene, uint32_t width, uint32_t height,
                               void* color, size_t pitch);
    gsm_status renderMono(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& cam, uint32_t width,
                          uint32_t height, void* color, size_t pitch, void* depth, size_t depthPitch);
    gsm_status counters(gsm_depthfirst_counters* out);
    gsm_status debugCopy(int which, void* dst, size_t bytes, size_t* needed);
    gsm_status setProfiling(int flags);
    gsm_status stageTimes(float* ms, int n) {
        hipSetDevice(dev_.id);
        return timer_.stageTimes(ms, n, GSM_DF_STAGE_BLEND);
    }
    gsm_status lastGpuTime(double* seconds) {
        hipSetDevice(dev_.id);
        return timer_.lastGpuTime(seconds);
    }

   private:
    DepthFirstRenderer() = default;
    // the arguments both frames share; `cam` (the left eye, or the mono camera) gives eye[0], near and far
    DfArgs frameArgs(const gsm_gaussian_input& in, const gsm_camera_params& cam, uint32_t width, uint32_t height) const;
    // One frame after validation.  project(), expand(depth order), blend(sorted gaussian ids) are the mode's
    // launches and beforeBlend() what it enqueues between the tile sort and the blend's events; the scans,
    // the compaction, both sorts and the instance counts between them are common.
    template <class Project, class Expand, class BeforeBlend, class Blend>
    gsm_status runFrame(hipStream_t s, const DfArgs& a, bool mono, Project&& project, Expand&& expand,
                        BeforeBlend&& beforeBlend, Blend&& blend);
    Device dev_;
    gsm_renderer_config config_{};
    Tuning tuning_{};  // A/B switches, read once at create
    uint32_t maxGaussians_ = 1, maxWidth_ = 1, maxHeight_ = 1, maxInstances_ = 4;
    uint32_t maxTiles_ = 1;
    gsm_depthfirst_options options_{};  // fixed at create
    bool key16_ = false, tile32_ = false;
    const uint32_t* sortedDepthKeys_ = nullptr;
    int sortDepth(hipStream_t s);
    int sortTiles(const DfArgs& a, hipStream_t s);
    DfArena A_;
    DeviceAllocations allocs_;
    // last frame
    uint32_t lastCount_ = 0, lastTilesX_ = 0, lastTilesY_ = 0;
    bool lastMono_ = false;  // the last frame was a mono frame (16-byte records)
    uint64_t schedKey_ = ~0ull;  // geometry the unit costs belong to
    unsigned long long* statsBuf_ = nullptr;  // blend walk statistics (profiling bit 1)
    const uint32_t* depthOrder_ = nullptr;
    const uint32_t* instTiles_ = nullptr;
    const uint32_t* instGids_ = nullptr;
    StageTimer timer_{GSM_DF_STAGE_COUNT, 64};  // the last 64 profiled frames are averaged
};

gsm_status DepthFirstRenderer::create(const gsm_renderer_config& cfg, int hipDevice,
                                      const gsm_depthfirst_options& opt, DepthFirstRenderer** out) {
    *out = nullptr;
    // DepthFirstRenderer.init guard (DepthFirstRenderer.swift:51-56)
    gsm_status st = check_config(cfg);
    if (st != GSM_OK) return st;
    const uint32_t maxW = cfg.max_width ? cfg.max_width : 1u, maxH = cfg.max_height ? cfg.max_height : 1u;
    const uint64_t tiles = (uint64_t)((maxW + kDfTile - 1) / kDfTile) * ((maxH + kDfTile - 1) / kDfTile);
    const bool tile32 = opt.tile_id_bits == 32u;
    // 16-bit tile ids (DepthFirstResources.swift); 32-bit: the tile sort's two passes (plan_sort_tiles_wide)
    static_assert((1u << kTilesWideMaxBits) == GSM_DF_MAX_TILES_32, "the header's limit is the tile sort's");
    if (tiles > (tile32 ? (uint64_t)GSM_DF_MAX_TILES_32 : 65535u)) return GSM_ERR_INVALID_TILE_COUNT;
    // tile rects are short4 (DfArena::bounds): a 32-bit grid may not exceed GSM_DF_MAX_TILES_AXIS per axis
    // (with 16-bit ids the grid check is the reference's, unchanged)
    if (tile32 && ((maxW + kDfTile - 1) / kDfTile > GSM_DF_MAX_TILES_AXIS ||
                   (maxH + kDfTile - 1) / kDfTile > GSM_DF_MAX_TILES_AXIS))
        return GSM_ERR_INVALID_TILE_COUNT;
    Device dev;
    if ((st = pick_device(hipDevice, &dev)) != GSM_OK) return st;
    DepthFirstRenderer* r = new (std::nothrow) DepthFirstRenderer();
    if (!r) return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    r->dev_ = dev;
    r->allocs_.setDevice(dev.id);
    r->config_ = cfg;
    r->maxGaussians_ = cfg.max_gaussians ? cfg.max_gaussians : 1u;
    r->maxWidth_ = maxW;
    r->maxHeight_ = maxH;
    r->maxTiles_ = (uint32_t)tiles;
    r->options_ = opt;
    r->key16_ = opt.depth_key_bits == 16u;
    r->tile32_ = tile32;
    const uint64_t cap64 = 4ull * r->maxGaussians_;  // DepthFirstResources.swift:399
    r->maxInstances_ = (uint32_t)(cap64 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : cap64);
    r->tuning_ = tuning_from_env(dev.id);
    const size_t G = r->maxGaussians_, cap = r->maxInstances_;
    const size_t nb = (G + kDfBlock - 1) / kDfBlock;
    DfArena& A = r->A_;
    DeviceAllocations& M = r->allocs_;
    M.alloc(st, A.renderData, G * sizeof(StereoTiledRenderData));
    M.alloc(st, A.bounds, G * sizeof(short4));
    M.alloc(st, A.touched, G * 4);
    M.alloc(st, A.depthKeys, G * 4);
    M.alloc(st, A.blockSums, (nb + 1) * 4);
    M.alloc(st, A.instSums, (nb + 1) * 4);
    M.alloc(st, A.visHdr, sizeof(TileAssignmentHeader));
    M.alloc(st, A.instHdr, sizeof(TileAssignmentHeader));
    for (int i = 0; i < 2; ++i) {
        M.alloc(st, A.dkeys[i], G * 4);
        M.alloc(st, A.dvals[i], G * 4);
        M.alloc(st, A.ikeys[i], cap * 4);
        M.alloc(st, A.ivals[i], cap * 4);
    }
    A.radixHistBytes = sort_workspace_bytes(r->maxInstances_ > r->maxGaussians_ ? r->maxInstances_ : r->maxGaussians_);
    M.alloc(st, A.radixHist, A.radixHistBytes);
    if (st == GSM_OK && hipMemset(A.radixHist, 0, A.radixHistBytes) != hipSuccess) st = GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    M.alloc(st, A.radixBinTotals, kSortTotalsWords * 4);  // radix_sort_tiles: totals + block table
    M.alloc(st, A.starts, ((size_t)r->maxTiles_ + 1) * sizeof(uint32_t));
    M.alloc(st, A.queue, kQueueStripes * kQueueStride * sizeof(uint32_t));
    M.alloc(st, A.expTable, 65536 * 2);
    M.alloc(st, A.unitCost, (size_t)r->maxTiles_ * 2 * sizeof(uint16_t));
    M.alloc(st, A.unitOrder, (size_t)r->maxTiles_ * 2 * sizeof(uint32_t));
    M.alloc(st, A.costMax, kCostMaxSlots * sizeof(uint32_t));
    M.alloc(st, A.sincos, 65536 * sizeof(float2));
    M.alloc(st, A.expTableMono, 65536 * 2);
    if (tiles > 65536u) M.alloc(st, A.tileBuckets, ((size_t)kWideBins + 1) * sizeof(uint32_t));
    // the sort plans the options add must fit the workspace now, not at the first frame
    if (st == GSM_OK && r->key16_ && !sort_bits_plan_fits(r->maxGaussians_, 16, r->tuning_.wideSort, sort_space(A)))
        st = GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
    if (st == GSM_OK && tiles > 65536u && !sort_tiles_wide_fits(r->maxInstances_, (uint32_t)tiles, sort_space(A)))
        st = GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
    if (st != GSM_OK) {
        delete r;
        return st;
    }
    // the stereo alpha table; the mono frame's tables: the Global blend's alpha table and the sin/cos of
    // the quantised angles
    if (upload_table(A.expTableMono, [](uint32_t i) { return blend_exp_table_entry((uint16_t)i); }) != GSM_OK ||
        upload_table(A.sincos, [](uint32_t i) {
            float2 v;
            det_sincos_table_entry(i, &v.x, &v.y);
            return v;
        }) != GSM_OK ||
        upload_table(A.expTable, [](uint32_t i) { return stereo_exp_table_entry((uint16_t)i); }) != GSM_OK ||
        hipMemset(A.visHdr, 0, sizeof(TileAssignmentHeader)) != hipSuccess ||
        hipMemset(A.instHdr, 0, sizeof(TileAssignmentHeader)) != hipSuccess ||
        hipMemset(A.costMax, 0, kCostMaxSlots * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(A.starts, 0, ((size_t)r->maxTiles_ + 1) * sizeof(uint32_t)) != hipSuccess) {
        delete r;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    *out = r;
    return GSM_OK;
}

// DepthRadixSortEncoder (DepthFirstRenderer.swift:664-681): stable LSD over the compacted keys, all 32
// bits or (depth_key_bits 16, DepthRadixSortEncoder.swift:13-24) the low 16.  The passes: plan_sort_bits
// (gsm_sort_plan.h) -- the same stable order with either switch.  Returns the ping-pong index of the
// result (or kSortNoSpace: nothing launched).
int DepthFirstRenderer::sortDepth(hipStream_t s) {
    return radix_sort_bits(A_.dkeys, A_.dvals, &A_.visHdr->totalAssignments, maxGaussians_, 0, key16_ ? 16u : 32u,
                           sort_space(A_), s, tuning_.ballotRank, tuning_.wideSort, tuning_.sortScanless);
}

// TileSortEncoder (DepthFirstRenderer.swift:683-768): stable sort by the tile id; the last pass also
// writes the tile ranges' starts (no pass over the instances).  A frame of more than 65,536 tiles (only
// with tile_id_bits 32) takes plan_sort_tiles_wide; every other frame, in either mode, plan_sort_tiles
// (gsm_sort_plan.h).
int DepthFirstRenderer::sortTiles(const DfArgs& a, hipStream_t s) {
    if (a.tileCount > 65536u)
        return radix_sort_tiles_wide(A_.ikeys, A_.ivals, &A_.instHdr->totalAssignments, maxInstances_, sort_space(A_),
                                     A_.starts, A_.tileBuckets, a.tileCount, s, tuning_.ballotRank);
    return radix_sort_tiles(A_.ikeys, A_.ivals, &A_.instHdr->totalAssignments, maxInstances_, 0, sort_space(A_),
                            A_.starts, 0u, a.tileCount, a.tileCount, s, tuning_.ballotRank, tuning_.wideSort,
                            tuning_.sortScanless);
}

// one eye's matrices and its projectCovariance2D terms (GaussianShared.h:340-355)
static void set_eye(const gsm_camera_params& c, const ProjectionUniforms& u, DfEyeConst* e) {
    std::memcpy(e->view, c.view, sizeof(e->view));
    std::memcpy(e->proj, c.proj, sizeof(e->proj));
    e->limX = u.limX;
    e->limY = u.limY;
    e->focalX = u.focalX;
    e->focalY = u.focalY;
}

DfArgs DepthFirstRenderer::frameArgs(const gsm_gaussian_input& in, const gsm_camera_params& cam, uint32_t width,
                                     uint32_t height) const {
    DfArgs a;
    std::memset(&a, 0, sizeof(a));
    a.width = (float)width;
    a.height = (float)height;
    // makeStereoCameraUniforms: near/far of the left camera (DepthFirstRenderer.swift:583-584)
    a.nearPlane = cam.near_plane;
    a.farPlane = cam.far_plane;
    const ProjectionUniforms u = projection_uniforms(cam.proj, a.width, a.height, a.nearPlane, a.farPlane);
    set_eye(cam, u, &a.eye[0]);
    a.maxEig = u.maxEig;
    a.adjFar = u.adjFar;
    a.adjDen = u.adjDen;
    a.inputIsSRGB = config_.gaussian_color_space == GSM_COLOR_SPACE_SRGB ? 1.0f : 0.0f;
    a.shComponents = in.sh_components;
    a.count = in.gaussian_count;
    // buildBinningParams(gaussianCount:width:height:) on 16x16 tiles (GlobalRenderer.swift:54-70)
    a.tilesX = (width + kDfTile - 1) / kDfTile;
    a.tilesY = (height + kDfTile - 1) / kDfTile;
    a.tileCount = a.tilesX * a.tilesY;
    a.maxInstances = maxInstances_;
    return a;
}

template <class Project, class Expand, class BeforeBlend, class Blend>
gsm_status DepthFirstRenderer::runFrame(hipStream_t s, const DfArgs& a, bool mono, Project&& project, Expand&& expand,
                                        BeforeBlend&& beforeBlend, Blend&& blend) {
    const uint32_t nb = (a.count + kDfBlock - 1) / kDfBlock;
    timer_.beginFrame();
    timer_.record(0, s);
    project();
    launch_scan_sums(A_.blockSums, nb, maxGaussians_, A_.visHdr, A_.queue, s);
    df_launch_compact(a, A_, s, key16_);
    timer_.record(1, s);
    const int dc = sortDepth(s);
    if (dc == kSortNoSpace) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;  // (nothing of the sort launched)
    timer_.record(2, s);
    df_launch_instance_counts(A_.dvals[dc], a, A_, s);
    launch_scan_sums(A_.instSums, nb, maxInstances_, A_.instHdr, A_.queue, s);
    expand(A_.dvals[dc]);
    timer_.record(3, s);
    const int ic = sortTiles(a, s);
    if (ic == kSortNoSpace) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
    beforeBlend();
    timer_.record(4, s, true);
    blend(A_.ivals[ic]);
    timer_.record(5, s, true);
    timer_.frameDone();
    lastCount_ = a.count;
    lastTilesX_ = a.tilesX;
    lastTilesY_ = a.tilesY;
    lastMono_ = mono;
    depthOrder_ = A_.dvals[dc];
    sortedDepthKeys_ = A_.dkeys[dc];
    instTiles_ = A_.ikeys[ic];
    instGids_ = A_.ivals[ic];
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status DepthFirstRenderer::renderStereoSbs(hipStream_t s, const gsm_gaussian_input& in,
                                               const gsm_camera_params& left, const gsm_camera_params& right,
                                               const float* scene, uint32_t width, uint32_t height, void* color,
                                               size_t pitch) {
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's: the launches below are checked)
    // encodeStereoPipeline guards (DepthFirstRenderer.swift:478, 607) -- errors, not a silent skip
    const gsm_status st = validate_frame(config_, maxGaussians_, maxWidth_, maxHeight_, in.gaussian_count, true,
                                         !in.gaussians || !in.harmonics, width, height, color, pitch, 2, nullptr, 0);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;

    DfArgs a = frameArgs(in, left, width, height);
    set_eye(right, projection_uniforms(right.proj, a.width, a.height, a.nearPlane, a.farPlane), &a.eye[1]);
    static const float kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(a.scene, scene ? scene : kIdentity, sizeof(a.scene));
    {  // length(sceneTransform[0].xyz) (DepthFirstShaders.metal:293)
        float d = a.scene[0] * a.scene[0] + a.scene[1] * a.scene[1];
        d = d + a.scene[2] * a.scene[2];
        a.sceneScale = std::sqrt(d);
    }
    for (int i = 0; i < 3; ++i) a.mid[i] = (left.position[i] + right.position[i]) * 0.5f;
    // Blend schedule: (tile, eye) units handed out longest first by the walk lengths the previous
    // frame of the same geometry measured (the image does not depend on the order, only the load
    // balance does).  Tuning::costOrder false (GSM_BLEND_SCHED=0 at create): index order.
    // The schedule only needs the previous frame's walk lengths: one extra workgroup of the
    // projection launch orders the units while the others project (no side stream, no join).
    const bool costOrder = tuning_.costOrder;
    a.schedUnits = costOrder ? 2u * a.tileCount : 0u;
    const uint64_t key = ((uint64_t)a.tilesX << 32) | a.tilesY;
    if (key != schedKey_) {  // costs of another geometry: start from index order
        hipMemsetAsync(A_.unitCost, 0, (size_t)a.tileCount * 2 * sizeof(uint16_t), s);
        hipMemsetAsync(A_.costMax, 0, kCostMaxSlots * sizeof(uint32_t), s);
        schedKey_ = key;
    }
    const uint32_t deg = sh_degree(in.sh_components);
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    const int fmt = (int)config_.color_format;
    return runFrame(
        s, a, false, [&] { df_launch_project(half, deg, in.gaussians, in.harmonics, a, A_, s); },
        [&](const uint32_t* order) { df_launch_instances(order, a, A_, s, tile32_); },  // with the blend's skip flags
        [&] {
            A_.blendStats = (timer_.flags() & 2) ? statsBuf_ : nullptr;
            if (A_.blendStats) hipMemsetAsync(statsBuf_, 0, 4 * sizeof(unsigned long long), s);
        },
        [&](const uint32_t* gids) { df_launch_blend(gids, a, A_, color, pitch, fmt, dev_.numCUs, costOrder, s); });
}

// DepthFirstRenderer.render -> encodeRender (DepthFirstRenderer.swift:166-203, 237-465) on the same
// arena as the stereo frame: the 16-byte GaussianRenderData records alias the stereo renderData, the
// compaction, both sorts and the scans are the stereo frame's, and the stage events map onto the same
// GSM_DF_STAGE_* slots.  Nothing of a frame outlives it except the stereo blend's unit costs, which
// this path neither reads nor writes.
gsm_status DepthFirstRenderer::renderMono(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& cam,
                                          uint32_t width, uint32_t height, void* color, size_t pitch, void* depth,
                                          size_t depthPitch) {
    (void)hipGetLastError();
    // encodeRender's guard (:249) and the texture sizes -- errors, not a silent return
    const gsm_status st = validate_frame(config_, maxGaussians_, maxWidth_, maxHeight_, in.gaussian_count, false,
                                         !in.gaussians || !in.harmonics, width, height, color, pitch, 1, depth,
                                         depthPitch);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;

    // CameraUniforms(from: camera, ...) (KernelTypes.swift:107-123)
    DfArgs a = frameArgs(in, cam, width, height);
    for (int i = 0; i < 3; ++i) a.mid[i] = cam.position[i];
    const uint32_t deg = sh_degree(in.sh_components);
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    const int fmt = (int)config_.color_format;
    return runFrame(
        s, a, true, [&] { df_launch_project_mono(half, deg, in.gaussians, in.harmonics, a, A_, s); },
        [&](const uint32_t* order) { df_launch_instances_mono(order, a, A_, s, tile32_); }, [] {},
        [&](const uint32_t* gids) {
            df_launch_blend_mono(gids, a, A_, color, pitch, fmt, depth, depthPitch, dev_.numCUs, s);
        });
}

gsm_status DepthFirstRenderer::counters(gsm_depthfirst_counters* out) {
    hipSetDevice(dev_.id);
    TileAssignmentHeader v, i;
    if (hipMemcpy(&v, A_.visHdr, sizeof(v), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&i, A_.instHdr, sizeof(i), hipMemcpyDeviceToHost) != hipSuccess)
        return GSM_ERR_RENDER_FAILED;
    out->gaussian_count = lastCount_;
    out->visible = v.totalAssignments;
    out->total_instances = i.totalAssignments;
    out->max_instances = maxInstances_;
    out->overflow = i.overflow;
    out->tiles_x = lastTilesX_;
    out->tiles_y = lastTilesY_;
    out->tile_count = lastTilesX_ * lastTilesY_;
    return GSM_OK;
}

gsm_status DepthFirstRenderer::debugCopy(int which, void* dst, size_t bytes, size_t* needed) {
    gsm_depthfirst_counters c;
    gsm_status st = counters(&c);
    if (st != GSM_OK) return st;
    const size_t n = lastCount_;
    const void* src = nullptr;
    size_t full = 0;
    switch (which) {
        case GSM_DF_BUF_RENDER_DATA: src = A_.renderData; full = n * (lastMono_ ? 16 : 32); break;
        case GSM_DF_BUF_BOUNDS: full = n * 16; break;
        case GSM_DF_BUF_TOUCHED: src = A_.touched; full = n * 4; break;
        case GSM_DF_BUF_DEPTH_KEYS: src = A_.depthKeys; full = n * 4; break;
        case GSM_DF_BUF_DEPTH_ORDER: src = depthOrder_; full = (size_t)c.visible * 4; break;
        case GSM_DF_BUF_SORTED_DEPTH_KEYS: src = sortedDepthKeys_; full = (size_t)c.visible * 4; break;
        case GSM_DF_BUF_INSTANCE_TILES: src = instTiles_; full = (size_t)c.total_instances * 4; break;
        case GSM_DF_BUF_INSTANCE_GAUSSIANS: src = instGids_; full = (size_t)c.total_instances * 4; break;
        case GSM_DF_BUF_HEADERS: full = (size_t)c.tile_count * 8; break;
        case GSM_DF_BUF_BLEND_STATS: src = (timer_.flags() & 2) ? statsBuf_ : nullptr; full = 32; break;
        default: return GSM_ERR_INVALID_ARGUMENT;
    }
    if (needed) *needed = full;
    if (!dst || bytes == 0 || full == 0) return GSM_OK;
    const size_t cpy = bytes < full ? bytes : full;
    // short4 on the device, int4 in the reference buffer; GaussianHeader {offset, count} from the run starts
    if (which == GSM_DF_BUF_BOUNDS) return copy_bounds_int4(A_.bounds, n, dst, bytes);
    if (which == GSM_DF_BUF_HEADERS) return copy_headers(A_.starts, c.tile_count, dst, bytes);
    if (!src) return GSM_ERR_RENDER_FAILED;
    if (hipMemcpy(dst, src, cpy, hipMemcpyDeviceToHost) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    if (which == GSM_DF_BUF_INSTANCE_GAUSSIANS) {  // drop the blend's skip flags (kDfSkipShift)
        uint32_t* v = (uint32_t*)dst;
        for (size_t i = 0; i < cpy / 4; ++i) v[i] &= kDfGidMask;
    }
    return GSM_OK;
}

gsm_status DepthFirstRenderer::setProfiling(int flags) {
    hipSetDevice(dev_.id);
    if ((flags & 2) && !statsBuf_) {
        gsm_status st = allocs_.alloc((void**)&statsBuf_, 4 * sizeof(unsigned long long));
        if (st != GSM_OK) return st;
    }
    return timer_.setProfiling(flags);  // bit 0: every stage, bit 3: the blend only
}

}  // namespace gsm

struct gsm_depthfirst : gsm::Handle<gsm::DepthFirstRenderer> {};

extern "C" {

void gsm_depthfirst_default_options(gsm_depthfirst_options* out) {
    if (!out) return;
    out->struct_bytes = (uint32_t)sizeof(gsm_depthfirst_options);
    out->depth_key_bits = 32;
    out->tile_id_bits = 16;
    out->reserved = 0;
}

gsm_status gsm_depthfirst_create(const gsm_renderer_config* config, int hip_device, gsm_depthfirst** out) {
    return gsm_depthfirst_create_with_options(config, hip_device, nullptr, out);
}

gsm_status gsm_depthfirst_get_options(gsm_depthfirst* r, gsm_depthfirst_options* out) {
    if (!r || !out) return GSM_ERR_INVALID_ARGUMENT;
    *out = r->impl->options();
    return GSM_OK;
}

gsm_status gsm_depthfirst_create_with_options(const gsm_renderer_config* config, int hip_device,
                                              const gsm_depthfirst_options* options, gsm_depthfirst** out) {
    if (!config || !out) return GSM_ERR_INVALID_ARGUMENT;
    *out = nullptr;
    gsm_depthfirst_options opt;
    gsm_depthfirst_default_options(&opt);
    if (options) {
        if (options->struct_bytes != sizeof(gsm_depthfirst_options) || options->reserved != 0 ||
            (options->depth_key_bits != 16u && options->depth_key_bits != 32u) ||
            (options->tile_id_bits != 16u && options->tile_id_bits != 32u))
            return GSM_ERR_INVALID_ARGUMENT;
        opt = *options;
    }
    return gsm_depthfirst::create(out, *config, hip_device, opt);
}

void gsm_depthfirst_destroy(gsm_depthfirst* r) { gsm_depthfirst::destroy(r); }

gsm_status gsm_depthfirst_render_stereo_sbs(gsm_depthfirst* r, void* stream, const gsm_gaussian_input* input,
                                            const gsm_camera_params* left, const gsm_camera_params* right,
                                            const float* scene_transform, uint32_t width, uint32_t height,
                                            void* color, size_t color_pitch_bytes) {
    if (!r || !input || !left || !right) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderStereoSbs((hipStream_t)stream, *input, *left, *right, scene_transform, width, height,
                                    color, color_pitch_bytes);
}

gsm_status gsm_depthfirst_render(gsm_depthfirst* r, void* stream, const gsm_gaussian_input* input,
                                 const gsm_camera_params* camera, uint32_t width, uint32_t height, void* color,
                                 size_t color_pitch_bytes, void* depth_r16f, size_t depth_pitch_bytes) {
    if (!r || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderMono((hipStream_t)stream, *input, *camera, width, height, color, color_pitch_bytes,
                               depth_r16f, depth_pitch_bytes);
}

gsm_status gsm_depthfirst_debug_counters(gsm_depthfirst* r, gsm_depthfirst_counters* out) {
    if (!r || !out) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->counters(out);
}

gsm_status gsm_depthfirst_debug_copy(gsm_depthfirst* r, int which, void* host_dst, size_t bytes, size_t* needed) {
    if (!r) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->debugCopy(which, host_dst, bytes, needed);
}

gsm_status gsm_depthfirst_set_profiling(gsm_depthfirst* r, int enable) {
    if (!r) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->setProfiling(enable);
}

gsm_status gsm_depthfirst_stage_times(gsm_depthfirst* r, float* ms, int n) {
    if (!r || !ms) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->stageTimes(ms, n);
}

gsm_status gsm_depthfirst_last_gpu_time(gsm_depthfirst* r, double* seconds) {
    if (!r || !seconds) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->lastGpuTime(seconds);
}

}  // extern "C"

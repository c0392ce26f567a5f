// gsm_renderer.hip -- host orchestration of one GlobalRenderer frame on MI355X.
//
// The C++ analogue of GlobalRenderer.swift (frame orchestration, :110-572) and
// GlobalResources.swift (up-front scratch arena, :58-361).  One HIP stream replaces
// the Metal command buffer; every grid size is a host constant (capacity-sized) and
// data-dependent counts are read on the device, so a frame is enqueue-only and can
// be captured into a hipGraph.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/gsm_debug.h"
#include "../../include/gsm_renderer.h"
#include "gsm_detmath.h"
#include "gsm_internal.h"
#include "gsm_renderer_impl.h"

namespace gsm {

gsm_status GlobalRenderer::create(const gsm_renderer_config& cfg, int hipDevice, GlobalRenderer** out) {
    *out = nullptr;
    // GlobalRenderer.init guard (GlobalRenderer.swift:111-113)
    gsm_status st = check_config(cfg);
    if (st != GSM_OK) return st;
    Device dev;
    if ((st = pick_device(hipDevice, &dev)) != GSM_OK) return st;

    GlobalRenderer* r = new (std::nothrow) GlobalRenderer();
    if (!r) return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    r->dev_ = dev;
    r->allocs_.setDevice(dev.id);
    r->config_ = cfg;
    // RendererLimits (GlobalRenderer.swift:6-23)
    r->maxGaussians_ = cfg.max_gaussians ? cfg.max_gaussians : 1u;
    r->maxWidth_ = cfg.max_width ? cfg.max_width : 1u;
    r->maxHeight_ = cfg.max_height ? cfg.max_height : 1u;
    r->tilesX_ = tiles_x(r->maxWidth_);
    r->tilesY_ = tiles_y(r->maxHeight_);
    r->tileCount_ = r->tilesX_ * r->tilesY_;
    if (r->tileCount_ > 65536u) {  // 16-bit tile field of the sort key (GlobalShaders.metal:288)
        delete r;
        return GSM_ERR_INVALID_TILE_COUNT;
    }
    r->rowBegin_ = 0;
    r->rowEnd_ = r->tilesY_;
    const uint64_t cap64 = 4ull * r->maxGaussians_;  // GlobalResources.swift:79
    r->maxAssignments_ = (uint32_t)(cap64 > 0xFFFFFFF0ull ? 0xFFFFFFF0ull : cap64);
    r->tuning_ = tuning_from_env(dev.id);

    const size_t G = r->maxGaussians_;
    const size_t cap = r->maxAssignments_;
    const size_t nb = blocks_of(r->maxGaussians_);
    DeviceArena& A = r->arena_;
    DeviceAllocations& M = r->allocs_;
    M.alloc(st, A.renderData, G * sizeof(GaussianRenderData));
    M.alloc(st, A.bounds, G * sizeof(short4));
    M.alloc(st, A.rec, G * sizeof(BlendRecord));
    M.alloc(st, A.tileCounts, G * sizeof(uint32_t));
    M.alloc(st, A.tileMasks, G * sizeof(uint32_t));
    M.alloc(st, A.blockSums, (nb + 1) * sizeof(uint32_t));
    M.alloc(st, A.header, sizeof(TileAssignmentHeader));
    M.alloc(st, A.keys[0], cap * sizeof(uint32_t));
    M.alloc(st, A.keys[1], cap * sizeof(uint32_t));
    M.alloc(st, A.vals[0], cap * sizeof(uint32_t));
    M.alloc(st, A.vals[1], cap * sizeof(uint32_t));
    A.radixHistBytes = sort_workspace_bytes(r->maxAssignments_);
    M.alloc(st, A.radixHist, A.radixHistBytes);
    if (st == GSM_OK && hipMemset(A.radixHist, 0, A.radixHistBytes) != hipSuccess) st = GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    M.alloc(st, A.radixBinTotals, kSortTotalsWords * sizeof(uint32_t));  // radix_sort_tiles: totals + block table
    M.alloc(st, A.tileStart, ((size_t)r->tileCount_ + 1) * sizeof(uint32_t));
    M.alloc(st, A.tileQueue, kQueueStripes * kQueueStride * sizeof(uint32_t));
    M.alloc(st, A.unitCost, (size_t)r->tileCount_ * 4 * sizeof(uint16_t));
    M.alloc(st, A.unitOrder, (size_t)r->tileCount_ * 4 * sizeof(uint32_t));
    M.alloc(st, A.costMax, (kCostMaxSlots + 2) * sizeof(uint32_t));
    M.alloc(st, A.halfVals[0], cap * sizeof(uint32_t));
    M.alloc(st, A.halfVals[1], cap * sizeof(uint32_t));
    M.alloc(st, A.halfCount, (size_t)r->tileCount_ * 2 * sizeof(uint32_t));
    M.alloc(st, A.expTable, 65536 * sizeof(uint16_t));
    M.alloc(st, A.sincosTable, (kSincosEntries + 256) * sizeof(float2));
    if (st != GSM_OK) {
        delete r;
        return st;
    }
    r->sched_[0] = {A.unitCost, A.unitOrder, A.costMax};
    // numeric-contract tables (gsm_detmath.h): alpha, sin/cos, and the byte table after the sin/cos entries
    if (upload_table(A.expTable, [](uint32_t i) { return blend_exp_table_entry((uint16_t)i); }) != GSM_OK ||
        upload_table(A.sincosTable, [](uint32_t i) {
            float2 v;
            if (i < kSincosEntries) {
                det_sincos_table_entry(i, &v.x, &v.y);
            } else {
                uint32_t d;
                det_byte_lut_entry(i - kSincosEntries, &v.x, &d);
                std::memcpy(&v.y, &d, 4);  // (bits, not a value)
            }
            return v;
        }, kSincosEntries + 256) != GSM_OK ||
        hipMemset(A.header, 0, sizeof(TileAssignmentHeader)) != hipSuccess ||
        hipMemset(A.tileStart, 0, ((size_t)r->tileCount_ + 1) * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(A.unitCost, 0, (size_t)r->tileCount_ * 4 * sizeof(uint16_t)) != hipSuccess ||
        hipMemset(A.costMax, 0, (kCostMaxSlots + 2) * sizeof(uint32_t)) != hipSuccess ||
        // every entry of the value buffers is a valid gaussian id at all times (the blend's
        // clamped, unpredicated gathers may read entry 0 of an empty frame)
        hipMemset(A.vals[0], 0, cap * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(A.vals[1], 0, cap * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(A.halfVals[0], 0, cap * sizeof(uint32_t)) != hipSuccess ||
        hipMemset(A.halfVals[1], 0, cap * sizeof(uint32_t)) != hipSuccess) {
        delete r;
        return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    *out = r;
    return GSM_OK;
}

int GlobalRenderer::sortPassCount() const {
    // RadixSortEncoder.swift:52-63: depth bytes (2) + bytes of (tileCount-1), max 4.
    int tileBytes = 1;
    uint32_t remaining = tileCount_ > 0 ? tileCount_ - 1 : 0;
    while (remaining >= 256) {
        tileBytes++;
        remaining >>= 8;
    }
    int p = 2 + tileBytes;
    return p > 4 ? 4 : p;
}

ProjectArgs GlobalRenderer::frameArgs(const gsm_camera_params& camp, uint32_t width, uint32_t height,
                                      uint32_t count, uint32_t shComponents, bool orthographic) const {
    ProjectArgs a;
    std::memset(&a, 0, sizeof(a));
    // CameraUniforms(from: camera, ...) (KernelTypes.swift:107-123)
    std::memcpy(a.cam.view, camp.view, sizeof(a.cam.view));
    std::memcpy(a.cam.proj, camp.proj, sizeof(a.cam.proj));
    std::memcpy(a.cam.cameraCenter, camp.position, sizeof(a.cam.cameraCenter));
    a.cam.pixelFactor = 1.0f;
    a.cam.focalX = camp.focal_x;
    a.cam.focalY = camp.focal_y;
    a.cam.width = (float)width;
    a.cam.height = (float)height;
    a.cam.nearPlane = camp.near_plane;
    a.cam.farPlane = camp.far_plane;
    a.cam.shComponents = shComponents;
    a.cam.gaussianCount = count;
    a.cam.inputIsSRGB = config_.gaussian_color_space == GSM_COLOR_SPACE_SRGB ? 1.0f : 0.0f;
    // buildBinningParams (GlobalRenderer.swift:38-51)
    a.bin.gaussianCount = count;
    a.bin.tilesX = tilesX_;
    a.bin.tilesY = tilesY_;
    a.bin.tileWidth = kTileWidth;
    a.bin.tileHeight = kTileHeight;
    a.bin.surfaceWidth = maxWidth_;
    a.bin.surfaceHeight = maxHeight_;
    a.bin.maxCapacity = count;
    a.bin.alphaThreshold = 0.005f;
    a.bin.totalInkThreshold = 2.0f;
    a.rowBegin = rowBegin_;
    a.rowEnd = rowEnd_;
    a.rowStride = rowStride_;
    a.count = count;
    a.maxAssignments = maxAssignments_;
    // uniform terms of the projection (a.cam.focalX / focalY above are the caller's, these the computed ones)
    const ProjectionUniforms u =
        projection_uniforms(a.cam.proj, a.cam.width, a.cam.height, a.cam.nearPlane, a.cam.farPlane);
    a.limX = u.limX;
    a.limY = u.limY;
    a.focalX = u.focalX;
    a.focalY = u.focalY;
    a.maxEig = u.maxEig;
    a.adjFar = u.adjFar;
    a.adjDen = u.adjDen;
    if (orthographic) {
        // The orthographic rule's uniforms, in the fields that carry the perspective terms, each formed
        // once with the fp32 operations the checker repeats per gaussian: sigma, the two signed entries of the
        // diagonal J, and the uniform SH direction -- minus the view's +z axis in world space, times sigma,
        // normalised by normalize3's sequence (x x + y y, + z z, sqrt, three divisions).  camp.position is ignored.
        const float sigma = a.cam.proj[10] >= 0.0f ? 1.0f : -1.0f;
        a.limX = sigma;
        a.limY = 0.0f;
        a.focalX = a.cam.width * a.cam.proj[0] * 0.5f;
        a.focalY = a.cam.height * a.cam.proj[5] * 0.5f;
        const float d0 = -sigma * a.cam.view[2], d1 = -sigma * a.cam.view[6], d2 = -sigma * a.cam.view[10];
        float dd = d0 * d0 + d1 * d1;
        dd = dd + d2 * d2;
        const float n = sqrtf(dd);
        a.cam.cameraCenter[0] = d0 / n;
        a.cam.cameraCenter[1] = d1 / n;
        a.cam.cameraCenter[2] = d2 / n;
    }
    return a;
}

gsm_status GlobalRenderer::validateFrame(uint32_t count, bool inputMissing, uint32_t width, uint32_t height,
                                         const void* color, size_t colorPitch, const void* depth,
                                         size_t depthPitch) const {
    const gsm_status st = validate_frame(config_, maxGaussians_, maxWidth_, maxHeight_, count, true, inputMissing,
                                         width, height, color, colorPitch, 1, depth, depthPitch);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    return GSM_OK;
}

gsm_status GlobalRenderer::pickOwner(const uint32_t* items, uint32_t n, uint32_t* object, uint32_t* gaussian) const {
    if (!lastPick_) return GSM_ERR_RENDER_FAILED;  // (the handle's last enqueued frame wrote no pick target)
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t item = items[i];
        uint32_t obj = GSM_PICK_NONE, id = GSM_PICK_NONE;
        if (item != GSM_PICK_NONE && item < lastItems_) {
            if (!lastPickComposite_) {  // (lastItems_ = the input's count)
                obj = 0;
                id = item;
            } else {
                // the entry whose blocks hold the item (DESIGN.md 19's layout: entries ascend in blockBase)
                const uint32_t block = item / (uint32_t)kProjectBlock;
                size_t lo = 0, hi = composeHost_.size();
                while (hi - lo > 1) {
                    const size_t mid = (lo + hi) / 2;
                    if (composeHost_[mid].blockBase <= block) lo = mid;
                    else hi = mid;
                }
                const uint32_t local = item - composeHost_[lo].blockBase * (uint32_t)kProjectBlock;
                if (local < composeHost_[lo].count) {
                    obj = composeObject_[lo];
                    id = local;
                }
            }
        }
        object[i] = obj;
        gaussian[i] = id;
    }
    return GSM_OK;
}

gsm_status GlobalRenderer::selectPick(hipStream_t s, const void* pick, size_t pickPitch, uint32_t width,
                                      uint32_t height, const void* mask, size_t maskPitch, uint32_t object,
                                      uint8_t* state, uint32_t gaussianCount, uint32_t andMask, uint32_t xorMask,
                                      uint32_t* matched) {
    if (!lastPick_) return GSM_ERR_RENDER_FAILED;  // (the handle's last enqueued frame wrote no pick target)
    if (object >= lastPickObjects_) return GSM_ERR_INVALID_ARGUMENT;
    const gsm_status st = check_select_pick(limits(), gaussianCount, width, height, lastWidth_, lastHeight_, pick,
                                            pickPitch, mask, maskPitch, state, matched);
    if (st != GSM_OK) return st;
    // the object's items of the pick frame's layout: [256 * B_o, 256 * B_o + count_o); an object
    // without gaussians has no entry and no item
    uint32_t base = 0, count = 0;
    if (!lastPickComposite_) {
        count = lastCount_;
    } else {
        for (size_t e = 0; e < composeObject_.size(); ++e) {
            if (composeObject_[e] != object) continue;
            base = composeHost_[e].blockBase * (uint32_t)kProjectBlock;
            count = composeHost_[e].count;
        }
    }
    return enqueueSelectPick(s, pick, pickPitch, width, height, mask, maskPitch, base, std::min(count, gaussianCount),
                             state, andMask, xorMask, matched);
}

gsm_status GlobalRenderer::selectPickIds(hipStream_t s, const void* pick, size_t pickPitch, uint32_t width,
                                         uint32_t height, const void* mask, size_t maskPitch, uint8_t* state,
                                         uint32_t gaussianCount, uint32_t andMask, uint32_t xorMask,
                                         uint32_t* matched) {
    // selectPick's rows in its order, without those that read the last pick frame: the image holds gaussian ids
    // (a frame of renderFrames), so the items are [0, gaussianCount) and the handle's pick state is not consulted
    const gsm_status st = check_select_pick(limits(), gaussianCount, width, height, width, height, pick, pickPitch, mask,
                                            maskPitch, state, matched);
    if (st != GSM_OK) return st;
    return enqueueSelectPick(s, pick, pickPitch, width, height, mask, maskPitch, 0u, gaussianCount, state, andMask,
                             xorMask, matched);
}

gsm_status GlobalRenderer::enqueueSelectPick(hipStream_t s, const void* pick, size_t pickPitch, uint32_t width,
                                             uint32_t height, const void* mask, size_t maskPitch, uint32_t base,
                                             uint32_t n, uint8_t* state, uint32_t andMask, uint32_t xorMask,
                                             uint32_t* matched) {
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (!arena_.selectBitmap) {  // (the handle's first select_pick: one bit per gaussian the handle can hold)
        const gsm_status st =
            allocs_.alloc((void**)&arena_.selectBitmap, (((size_t)maxGaussians_ + 31) / 32) * sizeof(uint32_t));
        if (st != GSM_OK) return st;
    }
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    launch_select_pick((const uint8_t*)pick, pickPitch, width, height, (const uint8_t*)mask, maskPitch, base, n,
                       arena_.selectBitmap, state, andMask, xorMask, matched, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::extract(hipStream_t s, const gsm_gaussian_input* in, const gsm_global_state* state,
                                   const uint32_t* keep, const gsm_global_extract_out* out, uint32_t* kept) {
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    gsm_status st = extract_check(maxGaussians_, half, in, state, keep, out, kept);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (!arena_.extractBlocks) {  // (the handle's first extract: one word per block of 256 gaussians it can hold)
        st = allocs_.alloc((void**)&arena_.extractBlocks,
                           (size_t)blocks_of(maxGaussians_) * sizeof(uint32_t));
        if (st != GSM_OK) return st;
    }
    ExtractArgs a{};
    a.records = (const uint8_t*)in->gaussians;
    a.harmonics = (const uint8_t*)in->harmonics;
    a.state = state->state;
    a.defaultState = state->default_state;
    a.count = in->gaussian_count;
    for (int k = 0; k < 8; ++k) a.keep.w[k] = keep[k];
    a.blockBase = arena_.extractBlocks;
    a.outRecords = (uint8_t*)out->gaussians;
    a.outHarmonics = (uint8_t*)out->harmonics;
    a.outState = out->state;
    a.outIds = out->ids;
    a.capacity = out->capacity;
    a.recordBytes = extract_record_bytes(half);
    a.harmonicsBytes = extract_harmonics_row_bytes(half, in->sh_components);
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    launch_extract(a, kept, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::stateHistogram(hipStream_t s, const uint8_t* state, uint32_t gaussianCount,
                                          uint32_t* histogram) {
    const gsm_status st = state_histogram_check(maxGaussians_, state, gaussianCount, histogram);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    launch_state_histogram(state, gaussianCount, histogram, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::selectWhere(hipStream_t s, const gsm_gaussian_input* in, const gsm_global_select_query* q,
                                       uint8_t* state, const gsm_global_style* styles, uint32_t styleCount,
                                       uint32_t andMask, uint32_t xorMask, uint32_t* matched) {
    const gsm_status st = select_where_check(maxGaussians_, in, q, state, styles, styleCount, matched);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    if (styles && in->gaussian_count > 0) {
        const gsm_status fs = fillStyleTable(s, styles, styleCount);
        if (fs != GSM_OK) return fs;
    }
    SelectWhereArgs a{};
    a.shape = q->shape;
    if (q->shape != GSM_SELECT_ALL)  // (GSM_SELECT_ALL never reads to_shape)
        for (int i = 0; i < 12; ++i) a.A[i] = q->to_shape[i];
    a.outside = q->flags & GSM_SELECT_OUTSIDE;
    a.opacityMin = q->opacity_min;
    a.opacityMax = q->opacity_max;
    a.scaleMin = q->scale_min;
    a.scaleMax = q->scale_max;
    a.opacityOn = select_range_applied(q->opacity_min, q->opacity_max) ? 1u : 0u;
    a.scaleOn = select_range_applied(q->scale_min, q->scale_max) ? 1u : 0u;
    a.testMask = q->test_mask & 0xFFu;
    a.testValue = q->test_value & 0xFFu;
    a.andMask = andMask;
    a.xorMask = xorMask;
    a.count = in->gaussian_count;
    launch_select_where(config_.precision == GSM_PRECISION_FLOAT16, in->gaussians, a, state,
                        styles ? arena_.styleTable : nullptr, matched, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::stateBounds(hipStream_t s, const gsm_gaussian_input* in, const gsm_global_state* state,
                                       const uint32_t* keep, gsm_global_bounds* bounds) {
    gsm_status st = state_bounds_check(maxGaussians_, in, state, keep, bounds);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (!arena_.boundsPartials) {  // (the handle's first state_bounds: 32 bytes per block of 256 gaussians it can hold)
        st = allocs_.alloc((void**)&arena_.boundsPartials,
                           std::max<size_t>(blocks_of(maxGaussians_), 1) *
                               kBoundsPartialBytes);
        if (st != GSM_OK) return st;
    }
    KeepSet k;
    for (int i = 0; i < 8; ++i) k.w[i] = keep[i];
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    launch_state_bounds(config_.precision == GSM_PRECISION_FLOAT16, in->gaussians, state->state, state->default_state,
                        in->gaussian_count, k, arena_.boundsPartials, (uint32_t*)bounds, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::transform(hipStream_t s, const gsm_global_scene* scene, const gsm_global_state* state,
                                     const uint32_t* keep, const gsm_global_transform_desc* desc) {
    const bool half = config_.precision == GSM_PRECISION_FLOAT16;
    const gsm_status st = transform_check(maxGaussians_, half, scene, state, keep, desc);
    if (st != GSM_OK) return st;
    if (scene->gaussian_count == 0) return GSM_OK;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    KeepSet k;
    for (int i = 0; i < 8; ++i) k.w[i] = keep[i];
    const uint32_t degree = (uint32_t)transform_degree(scene->sh_components);
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    launch_transform(half, degree, scene->gaussians, degree ? scene->harmonics : nullptr, state->state,
                     state->default_state, scene->gaussian_count, k, *desc,
                     degree && transform_wide_rows(half, scene->sh_components, scene->harmonics), s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

GlobalRenderer::FrameRequest GlobalRenderer::request(FrameKind kind, const ProjectArgs& args, uint32_t width,
                                                     uint32_t height, const FrameTargets& targets) const {
    FrameRequest rq;
    rq.args = args;
    rq.width = width;
    rq.height = height;
    rq.targets = targets;
    rq.payload.kind = kind;
    return rq;
}

gsm_status GlobalRenderer::renderFrame(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& camp,
                                       uint32_t width, uint32_t height, const FrameTargets& t,
                                       const FrameExtras& extras) {
    const StyleSource* style = extras.style;
    gsm_status st = check_frame(limits(), in, width, height, t, extras);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    const bool ortho = extras.orthographic;
    FrameRequest rq = request(FrameKind::Single,
                              frameArgs(camp, width, height, in.gaussian_count, in.sh_components, ortho), width,
                              height, t);
    rq.pick = extras.pick;
    rq.occluder = extras.occluder;
    rq.orthographic = ortho;
    rq.world = in.gaussians;
    rq.harm = in.harmonics;
    rq.shDegree = sh_degree(in.sh_components);
    if (style) {
        if ((st = fillStyleTable(s, style->styles, style->styleCount)) != GSM_OK) return st;
        rq.style = StyleArgs{arena_.styleTable, style->states[0].state, style->states[0].default_state};
    }
    return runFrame(s, rq);
}

gsm_status GlobalRenderer::fillStyleTable(hipStream_t s, const gsm_global_style* styles, uint32_t styleCount) {
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    if (!arena_.styleTable) {  // (the handle's first styled frame or select with styles)
        const gsm_status st = allocs_.alloc((void**)&arena_.styleTable, sizeof(StyleChunk));
        if (st != GSM_OK) return st;
    }
    StyleChunk c;
    for (uint32_t i = 0; i < kStyleEntries; ++i) {
        c.v[i] = make_uint2(0u, kStyleIdentityY);
        if (i < styleCount) {
            const gsm_global_style& S = styles[i];
            c.v[i].x = (uint32_t)S.tint_r | ((uint32_t)S.tint_g << 8) | ((uint32_t)S.tint_b << 16) |
                       ((uint32_t)S.tint_amount << 24);
            c.v[i].y = (uint32_t)S.opacity_scale | (S.hidden ? 1u << 8 : 0u);
        }
    }
    launch_fill_styles(c, arena_.styleTable, s);
    return GSM_OK;
}

gsm_status GlobalRenderer::selectMask(hipStream_t s, const gsm_gaussian_input* in, const gsm_camera_params* camp,
                                      uint32_t width, uint32_t height, const void* mask, size_t maskPitch,
                                      uint8_t* state, const gsm_global_style* styles, uint32_t styleCount,
                                      uint32_t andMask, uint32_t xorMask, uint32_t* matched, bool orthographic) {
    const gsm_status cst =
        check_select_mask(limits(), in, camp, width, height, mask, maskPitch, state, styles, styleCount, matched);
    if (cst != GSM_OK) return cst;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    if (styles && in->gaussian_count > 0) {
        const gsm_status st = fillStyleTable(s, styles, styleCount);
        if (st != GSM_OK) return st;
    }
    const ProjectArgs a = frameArgs(*camp, width, height, in->gaussian_count, 0, orthographic);
    launch_select_mask(config_.precision == GSM_PRECISION_FLOAT16, in->gaussians, a, (const uint8_t*)mask, maskPitch,
                       width, height, state, styles ? arena_.styleTable : nullptr, andMask, xorMask, matched, arena_, s,
                       orthographic);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

// What the two batch entries below share on the host.
// the per-view terms of an entry (ViewArgs, BatchViewArgs): the camera and what projection_uniforms derives from it
template <class Entry>
static void set_view_terms(Entry& d, const ProjectArgs& pv) {
    d.cam = pv.cam;
    d.limX = pv.limX;
    d.limY = pv.limY;
    d.focalX = pv.focalX;
    d.focalY = pv.focalY;
    d.maxEig = pv.maxEig;
    d.adjFar = pv.adjFar;
    d.adjDen = pv.adjDen;
}

// the first `count` entries of a host copy to their device array, a kernel-argument chunk at a time: launch(chunk,
// first, n) writes entries [first, first + n)
template <class Chunk, class Entry, class Launch>
static void fill_chunks(const std::vector<Entry>& host, uint32_t count, Launch&& launch) {
    constexpr uint32_t kPer = sizeof(Chunk::v) / sizeof(Entry);
    for (uint32_t e0 = 0; e0 < count; e0 += kPer) {
        Chunk c;
        const uint32_t n = std::min(kPer, count - e0);
        std::memset(&c, 0, sizeof(c));
        std::memcpy(c.v, host.data() + e0, (size_t)n * sizeof(Entry));
        launch(c, e0, n);
    }
}

ProjectArgs GlobalRenderer::batchSharedArgs(const gsm_camera_params& camera0, uint32_t width0, uint32_t height0,
                                            uint32_t count, uint32_t shComponents) const {
    // what a batch shares: view 0's arguments on that view's own tile grid, rows [0, tilesY)
    ProjectArgs a = frameArgs(camera0, width0, height0, count, shComponents);
    a.bin.tilesX = tiles_x(width0);
    a.bin.tilesY = tiles_y(height0);
    a.rowBegin = 0;
    a.rowEnd = a.bin.tilesY;
    a.rowStride = 1;
    return a;
}

gsm_status GlobalRenderer::renderViews(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params* cameras,
                                       uint32_t viewCount, uint32_t width, uint32_t height, void* color,
                                       size_t colorPitch, size_t colorStride, void* depth, size_t depthPitch,
                                       size_t depthStride) {
    const FrameTargets t{color, colorPitch, depth, depthPitch};
    gsm_status st = check_views(limits(), in, cameras, viewCount, width, height, t, colorStride, depthStride);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    // the per-view array: allocated by the first batch, for the most views the handle's tile space holds
    if (!arena_.viewArgs) {
        maxViews_ = max_batch_views(tileCount_);
        st = allocs_.alloc((void**)&arena_.viewArgs, (size_t)maxViews_ * sizeof(ViewArgs));
        if (st != GSM_OK) return st;
    }
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    const ProjectArgs a = batchSharedArgs(cameras[0], width, height, in.gaussian_count, in.sh_components);
    // the host copy of the per-view terms (the cameras are consumed before the call returns), to the device
    // array in kernel-argument chunks
    viewHost_.resize(viewCount);
    for (uint32_t v = 0; v < viewCount; ++v) {
        const ProjectArgs pv = frameArgs(cameras[v], width, height, in.gaussian_count, in.sh_components);
        ViewArgs& d = viewHost_[v];
        std::memset(&d, 0, sizeof(d));
        set_view_terms(d, pv);
    }
    fill_chunks<ViewChunk>(viewHost_, viewCount, [&](const ViewChunk& c, uint32_t v0, uint32_t n) {
        launch_fill_views(c, v0, n, arena_.viewArgs, s);
    });
    FrameRequest rq = request(FrameKind::Views, a, width, height, t);
    const ViewsLayout layout = views_layout(in.gaussian_count, width, height);
    ViewBatch& vb = rq.payload.viewBatch;
    vb.views = viewCount;
    vb.blocksPerView = layout.blocksPerView;
    vb.tilesPerView = layout.tilesPerView;
    vb.args = arena_.viewArgs;
    rq.payload.colorViewStride = colorStride;
    rq.payload.depthViewStride = depthStride;
    rq.world = in.gaussians;
    rq.harm = in.harmonics;
    rq.shDegree = sh_degree(in.sh_components);
    return runFrame(s, rq);
}

gsm_status GlobalRenderer::renderBatch(hipStream_t s, const gsm_global_view* views, uint32_t viewCount) {
    const gsm_status st = check_batch(limits(), BatchViewArray{views, nullptr}, viewCount);
    return st != GSM_OK ? st : enqueueBatch(s, views, viewCount, nullptr);
}

gsm_status GlobalRenderer::renderFrames(hipStream_t s, const gsm_global_frame* frames, uint32_t frameCount) {
    gsm_status st = check_frames_front(frames, frameCount);
    if (st != GSM_OK) return st;
    // the frames as batch views plus what each adds: host copies only (reserved by the handle's first such call
    // for the most views it can hold, so no later call allocates)
    if (framesViews_.capacity() == 0) {
        const uint32_t mv = max_batch_views(tileCount_);
        framesViews_.reserve(mv);
        framesOptions_.reserve(mv);
    }
    // the batch's rows, read from the frames themselves (more frames than the copies hold do not pass the tile row:
    // every view takes a tile)
    const BatchFrameArray batch{frames};
    if ((st = check_batch(limits(), batch, frameCount)) != GSM_OK) return st;
    framesViews_.resize(frameCount);
    framesOptions_.resize(frameCount);
    bool any = false;
    for (uint32_t v = 0; v < frameCount; ++v) {
        const gsm_global_frame& F = frames[v];
        gsm_global_view& V = framesViews_[v];
        V.input = F.objects[0].input;
        V.camera = F.objects[0].camera;
        V.width = F.width;
        V.height = F.height;
        V.color = F.color;
        V.color_pitch_bytes = F.color_pitch_bytes;
        V.depth = F.depth_r16f;
        V.depth_pitch_bytes = F.depth_pitch_bytes;
        const BatchViewOptions& O = framesOptions_[v] = batch.optionsAt(v);
        any = any || O.pick.pixels || O.occluder.pixels || O.styled || O.orthographic;
    }
    // every option NULL and no flag in every frame: the plain batch, its path and its device code
    return enqueueBatch(s, framesViews_.data(), frameCount, any ? framesOptions_.data() : nullptr);
}

gsm_status GlobalRenderer::enqueueBatch(hipStream_t s, const gsm_global_view* views, uint32_t viewCount,
                                        const BatchViewOptions* options) {
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    // the per-view array and the two lookup tables: allocated by the handle's first batch, for the most views
    // its tile space and its item space hold (every view takes at least one tile; the host copies are reserved
    // with them, so no later batch allocates)
    const uint32_t maxBlocks = blocks_of(maxGaussians_);
    if (!arena_.batchArgs) {
        const uint32_t mv = max_batch_views(tileCount_);
        BatchViewArgs* args = nullptr;
        uint16_t *bv = nullptr, *tv = nullptr;
        gsm_status st = allocs_.alloc((void**)&args, (size_t)mv * sizeof(BatchViewArgs));
        if (st == GSM_OK) st = allocs_.alloc((void**)&bv, (size_t)maxBlocks * sizeof(uint16_t));
        if (st == GSM_OK) st = allocs_.alloc((void**)&tv, (size_t)tileCount_ * sizeof(uint16_t));
        if (st != GSM_OK) return st;
        batchHost_.reserve(mv);
        key_.reserve(ScheduleKey::kFixedWords + 3 * (size_t)mv + 1);  // (the largest signature the handle can hold)
        schedState_.reserve(ScheduleKey::kFixedWords + 3 * (size_t)mv + 1);
        arena_.batchArgs = args;
        arena_.batchBlockView = bv;
        arena_.batchTileView = tv;
        maxBatchViews_ = mv;
    }
    // the per-view options array: allocated by the handle's first batch with options, one line per view it can hold
    if (options && !arena_.batchExtras) {
        const gsm_status st = allocs_.alloc((void**)&arena_.batchExtras, (size_t)maxBatchViews_ * sizeof(BatchExtras));
        if (st != GSM_OK) return st;
        extrasHost_.reserve(maxBatchViews_);
    }
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    // the host copies of the per-view entries and, with options, of the per-view options lines (`views` is consumed
    // before the call returns): each view's own frameArgs -- the camera terms depend on its width and height -- on
    // its own tile grid, rows [0, tilesY), placed by the layout
    const BatchViewArray batch{views, options};
    const uint32_t sh = views[0].input.sh_components;
    batchHost_.resize(viewCount);
    if (options) extrasHost_.resize(viewCount);
    BatchLayout layout;
    for (uint32_t v = 0; v < viewCount; ++v) {
        const gsm_global_view& V = views[v];
        const BatchViewDesc desc = batch.at(v);
        const BatchViewOptions& O = desc.options;
        const BatchViewLayout l = layout.place(desc);
        const uint32_t n = V.input.gaussian_count;
        // (the kind is per view: a quad view mixes them)
        const ProjectArgs pv = frameArgs(V.camera, V.width, V.height, n, sh, O.orthographic);
        BatchViewArgs& d = batchHost_[v];
        std::memset(&d, 0, sizeof(d));
        set_view_terms(d, pv);
        d.ortho = O.orthographic ? 1u : 0u;
        d.count = n;
        d.bin = pv.bin;
        d.bin.tilesX = l.tilesX;
        d.bin.tilesY = l.tilesY;
        d.blockBase = l.blockBase;
        d.world = V.input.gaussians;
        d.harm = V.input.harmonics;
        d.tg.color = (uint8_t*)V.color;
        d.tg.depth = (uint8_t*)V.depth;
        d.tg.colorPitch = V.color_pitch_bytes;
        d.tg.depthPitch = V.depth ? V.depth_pitch_bytes : 0;
        d.tg.tileBase = l.tileBase;
        d.tg.tilesX = l.tilesX;
        d.tg.tilesY = l.tilesY;
        d.tg.width = V.width;
        d.tg.height = V.height;
        d.tg.vec = l.vec;  // (the wide stores where this view's targets are aligned for them)
        if (!options) continue;
        BatchExtras& e = extrasHost_[v];
        std::memset(&e, 0, sizeof(e));
        e.pick = (uint8_t*)O.pick.pixels;
        e.pickPitch = O.pick.pixels ? O.pick.pitch : 0;
        e.occluder = (const uint8_t*)O.occluder.pixels;
        e.occluderPitch = O.occluder.pixels ? O.occluder.pitch : 0;
        if (O.styled) {  // (one object per frame: states[0], as renderFrame)
            e.styled = 1u;
            e.state = O.style.states[0].state;
            e.defaultState = O.style.states[0].default_state;
        }
        e.align = l.align;
        e.itemBase = l.itemBase;
    }
    fill_chunks<BatchChunk>(batchHost_, viewCount, [&](const BatchChunk& c, uint32_t v0, uint32_t n) {
        launch_fill_batch(c, v0, n, arena_.batchArgs, arena_.batchBlockView, maxBlocks, arena_.batchTileView, tileCount_,
                          s);
    });
    // what the batch shares: the thresholds, the capacity and the schedule; count = the batch's gaussians (counters)
    const ProjectArgs a = batchSharedArgs(views[0].camera, views[0].width, views[0].height, layout.countSum, sh);
    FrameRequest rq = request(FrameKind::Batch, a, views[0].width, views[0].height, batch.at(0).targets);
    BatchFrame& bf = rq.payload.batchFrame;
    bf.views = viewCount;
    bf.blocks = layout.blocks;
    bf.tiles = layout.tiles;
    bf.args = arena_.batchArgs;
    bf.blockView = arena_.batchBlockView;
    bf.tileView = arena_.batchTileView;
    rq.shDegree = sh_degree(sh);
    if (options) {  // the options lines to the device array in kernel-argument chunks, as the entries above
        fill_chunks<ExtrasChunk>(extrasHost_, viewCount, [&](const ExtrasChunk& c, uint32_t v0, uint32_t n) {
            launch_fill_batch_extras(c, v0, n, arena_.batchExtras, s);
        });
        bf.extras = arena_.batchExtras;
        rq.anyPick = layout.anyPick;
        rq.anyOccluder = layout.anyOccluder;
        rq.orthographic = layout.anyOrtho;
        if (layout.tableView != BatchLayout::kNoTable) {
            const StyleSource& table = options[layout.tableView].style;
            const gsm_status st = fillStyleTable(s, table.styles, table.styleCount);
            if (st != GSM_OK) return st;
            rq.style.table = arena_.styleTable;  // (the views' state bytes travel in their options lines)
        }
    }
    // (a batch without an orthographic view launches the kernels it launched before the flag existed)
    return runFrame(s, rq);
}

gsm_status GlobalRenderer::composeFrame(hipStream_t s, const gsm_global_object* objects, uint32_t objectCount,
                                        uint32_t width, uint32_t height, const FrameTargets& t,
                                        const FrameExtras& extras) {
    const StyleSource* style = extras.style;
    const bool ortho = extras.orthographic;  // (the flag holds for every object; sigma, J and d0 are per object)
    gsm_status st = check_compose(limits(), objects, objectCount, width, height, t, extras);
    if (st != GSM_OK) return st;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    // the per-object array and the block table: allocated by the handle's first composite, for the most objects
    // with gaussians its item space holds (each takes at least one block; the host copies are reserved with
    // them, so no later composite allocates)
    const uint32_t maxBlocks = blocks_of(maxGaussians_);
    const uint32_t maxEntries = max_compose_entries(maxBlocks);
    if (!arena_.composeArgs) {
        ComposeObjectArgs* args = nullptr;
        uint16_t* bo = nullptr;
        st = allocs_.alloc((void**)&args, (size_t)maxEntries * sizeof(ComposeObjectArgs));
        if (st == GSM_OK) st = allocs_.alloc((void**)&bo, (size_t)maxBlocks * sizeof(uint16_t));
        if (st != GSM_OK) return st;
        composeHost_.reserve(maxEntries);
        composeObject_.reserve(maxEntries);
        key_.reserve(ScheduleKey::kFixedWords + kBatchIndexMax + 1u);  // (the largest signature: a count per object)
        schedState_.reserve(ScheduleKey::kFixedWords + kBatchIndexMax + 1u);
        arena_.composeArgs = args;
        arena_.composeBlockObject = bo;
    }
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
    // the host copy of the entries (`objects` is consumed before the call returns): each object's own frameArgs
    // -- its camera on the frame's size -- for the objects that have gaussians
    const uint32_t sh = objects[0].input.sh_components;
    composeHost_.clear();
    composeObject_.clear();
    ComposeLayout layout;
    for (uint32_t o = 0; o < objectCount; ++o) {
        const gsm_global_object& O = objects[o];
        const uint32_t n = O.input.gaussian_count;
        ComposeEntry entry;
        if (!layout.place(n, &entry)) continue;  // (no gaussians: no block, no entry)
        const ProjectArgs po = frameArgs(O.camera, width, height, n, sh, ortho);
        ComposeObjectArgs d;
        std::memset(&d, 0, sizeof(d));
        set_view_terms(d, po);
        d.count = n;
        d.world = O.input.gaussians;
        d.harm = O.input.harmonics;
        d.blockBase = entry.blockBase;
        if (style) {  // (a styled composite: the object's state bytes and default travel with its entry)
            d.state = style->states[o].state;
            d.defaultState = style->states[o].default_state;
        }
        composeHost_.push_back(d);
        composeObject_.push_back(entry.object);  // (pickOwner: the entry's object index of the call)
    }
    fill_chunks<ComposeChunk>(composeHost_, layout.entries, [&](const ComposeChunk& c, uint32_t e0, uint32_t n) {
        launch_fill_compose(c, e0, n, arena_.composeArgs, arena_.composeBlockObject, maxBlocks, s);
    });
    // the frame's arguments are the single frame's: the handle's tile grid and rows, the thresholds, the capacity
    // and the schedule; count = the composite's gaussians (counters).  (Not batchSharedArgs: that puts a batch on
    // view 0's own grid, and a composite stays on the handle's, as gsm_global_render does.)
    const ProjectArgs a = frameArgs(objects[0].camera, width, height, layout.countSum, sh, ortho);
    FrameRequest rq = request(FrameKind::Compose, a, width, height, t);
    rq.orthographic = ortho;
    ComposeFrame& cf = rq.payload.composeFrame;
    cf.objects = objectCount;
    cf.entries = layout.entries;
    cf.blocks = layout.blocks;
    cf.args = arena_.composeArgs;
    cf.blockObject = arena_.composeBlockObject;
    rq.pick = extras.pick;
    rq.occluder = extras.occluder;
    rq.shDegree = sh_degree(sh);
    if (style) {
        if ((st = fillStyleTable(s, style->styles, style->styleCount)) != GSM_OK) return st;
        rq.style.table = arena_.styleTable;  // (the objects' state bytes travel in their entries)
    }
    return runFrame(s, rq);
}

gsm_status GlobalRenderer::renderRecords(hipStream_t s, const void* records, uint32_t count, uint32_t width,
                                         uint32_t height, void* color, size_t colorPitch, void* depth,
                                         size_t depthPitch, const uint32_t* devCount, bool preOrdered,
                                         const MgArrive* blendArrive) {
    // devCount: the count lives on the device (multi-GPU exchange, gsm_multigpu_render); `count` is
    // then the capacity the grids cover
    gsm_status st = validateFrame(count, !records, width, height, color, colorPitch, depth, depthPitch);
    if (st != GSM_OK) return st;
    gsm_camera_params cam;
    std::memset(&cam, 0, sizeof(cam));
    FrameRequest rq = request(FrameKind::Records, frameArgs(cam, width, height, count, 1), width, height,
                              FrameTargets{color, colorPitch, depth, depthPitch});
    rq.records = records;
    rq.devCount = devCount;
    rq.preOrdered = preOrdered;
    rq.blendArrive = blendArrive;
    return runFrame(s, rq);
}

gsm_status GlobalRenderer::preparePartition(const gsm_gaussian_input& in, const gsm_camera_params& camp,
                                            uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                                            const uint32_t* slabRows, uint32_t numSlabs, bool needSend,
                                            const void* send, const uint32_t* sendCounts, PartitionFrame* f,
                                            bool interleave) {
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's: the launches below are checked)
    gsm_status st = check_partition(limits(), in, width, height, first, count, slabRows, numSlabs, needSend, send,
                                    sendCounts, interleave);
    if (st != GSM_OK) return st;
    std::memset(&f->slabs, 0, sizeof(f->slabs));
    f->slabs.n = numSlabs;
    f->slabs.interleave = interleave ? 1u : 0u;  // slab s = rows s, s + n, ... < slabRows[n]
    for (uint32_t i = 0; i <= numSlabs; ++i) f->slabs.rows[i] = slabRows[i];
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    st = ensurePartitionBuffers(numSlabs);
    if (st != GSM_OK) return st;
    f->half = config_.precision == GSM_PRECISION_FLOAT16;
    f->a = frameArgs(camp, width, height, count, in.sh_components);
    f->a.rowBegin = 0;  // the rank's ids are projected against the whole frame
    f->a.rowEnd = tilesY_;
    f->a.rowStride = 1;
    const size_t ws = f->half ? sizeof(PackedWorldGaussianHalf) : sizeof(PackedWorldGaussian);
    const size_t hs = (size_t)in.sh_components * 3 * (f->half ? 2 : 4);
    f->world = (const char*)in.gaussians + (size_t)first * ws;
    f->harm = (const char*)in.harmonics + (size_t)first * hs;
    f->deg = sh_degree(in.sh_components);
    return GSM_OK;
}

gsm_status GlobalRenderer::ensurePartitionBuffers(uint32_t numSlabs) {
    // lazily: only ranks of a partitioned frame need these (the multi-GPU frame: at prepare)
    if (part_.runs && part_.runSlabs >= numSlabs) return GSM_OK;
    if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
    const size_t blocks = blocks_of(maxGaussians_);
    PartitionBuffers b = part_;
    b.runStride = (uint32_t)(blocks * kProjectBlock);
    b.runSlabs = numSlabs;
    // (a buffer for fewer slabs stays allocated until the renderer is destroyed)
    gsm_status st = allocs_.alloc((void**)&b.runs, (size_t)numSlabs * b.runStride * sizeof(SplatRecord));
    if (st == GSM_OK && !b.blockSlabCounts) st = allocs_.alloc((void**)&b.blockSlabCounts, kMaxSlabs * (blocks + 1) * 4);
    if (st == GSM_OK) part_ = b;
    if (st == GSM_OK && !sched_[1].unitOrder) {
        ScheduleSet t;
        st = allocs_.alloc((void**)&t.unitCost, (size_t)tileCount_ * 4 * sizeof(uint16_t));
        if (st == GSM_OK) st = allocs_.alloc((void**)&t.unitOrder, (size_t)tileCount_ * 4 * sizeof(uint32_t));
        if (st == GSM_OK) st = allocs_.alloc((void**)&t.costMax, (kCostMaxSlots + 2) * sizeof(uint32_t));
        if (st == GSM_OK && (hipMemset(t.unitCost, 0, (size_t)tileCount_ * 4 * sizeof(uint16_t)) != hipSuccess ||
                             hipMemset(t.costMax, 0, (kCostMaxSlots + 2) * sizeof(uint32_t)) != hipSuccess ||
                             hipDeviceSynchronize() != hipSuccess))
            st = GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
        if (st == GSM_OK) sched_[1] = t;
    }
    return st;
}

void GlobalRenderer::selectSchedule(uint32_t parity) {
    const ScheduleSet& t = sched_[(parity & 1u) && sched_[1].unitOrder ? 1 : 0];
    arena_.unitCost = t.unitCost;
    arena_.unitOrder = t.unitOrder;
    arena_.costMax = t.costMax;
}

gsm_status GlobalRenderer::projectPartition(hipStream_t s, const gsm_gaussian_input& in,
                                            const gsm_camera_params& camp, uint32_t width, uint32_t height,
                                            uint32_t first, uint32_t count, const uint32_t* slabRows,
                                            uint32_t numSlabs, void* send, uint64_t capacity,
                                            uint32_t* sendCounts, bool interleave) {
    PartitionFrame f;
    gsm_status st = preparePartition(in, camp, width, height, first, count, slabRows, numSlabs, true, send,
                                     sendCounts, &f, interleave);
    if (st != GSM_OK) return st;
    launch_partition(f.half, f.deg, f.world, f.harm, f.a, f.slabs, part_, arena_.sincosTable, send, capacity,
                     sendCounts, s);
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::partitionCounts(hipStream_t s, const gsm_gaussian_input& in, const gsm_camera_params& camp,
                                           uint32_t width, uint32_t height, uint32_t first, uint32_t count,
                                           const uint32_t* slabRows, uint32_t numSlabs, uint32_t* sendCounts,
                                           bool orderUnits, bool interleave, const CountPublish* publish) {
    PartitionFrame f;
    gsm_status st = preparePartition(in, camp, width, height, first, count, slabRows, numSlabs, false, nullptr,
                                     sendCounts, &f, interleave);
    if (st != GSM_OK) return st;
    // the blend units of this renderer's rows (its slab), ordered by one extra workgroup of the launch
    if (orderUnits) {
        uint32_t tiles = 0;
        const ScheduleKey& key = requestKey(request(FrameKind::Single, f.a, width, height, FrameTargets{}), &tiles);
        f.a.schedUnits = scheduleUnits(s, key, tiles);
    }
    f.a.pairBucket = tuning_.blendPairs ? (uint32_t)std::max(1, tuning_.pairBucket) : kUoBuckets;
    launch_partition_counts(f.half, f.deg, f.world, f.harm, f.a, f.slabs, part_, arena_.sincosTable, sendCounts,
                            arena_, publish ? *publish : CountPublish{}, s);
    partCount_ = count;
    partSlabs_ = f.slabs;
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::partitionPush(hipStream_t s, uint32_t world, uint32_t rank, const uint32_t* counts,
                                         const SlabPeers& peers, uint32_t* recvCount, const MgArrive& arrive) {
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's: the launches below are checked)
    ProjectArgs a;
    std::memset(&a, 0, sizeof(a));
    a.count = partCount_;
    if (world != partSlabs_.n) return GSM_ERR_INVALID_ARGUMENT;  // one slab per rank, as partitionCounts split
    launch_partition_push(a, world, rank, part_, counts, peers, recvCount, partSlabs_, arrive, s,
                          (uint32_t)(4 * dev_.numCUs));  // 4 workgroups per CU looping over the runs
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

const ScheduleKey& GlobalRenderer::requestKey(const FrameRequest& rq, uint32_t* tiles) {
    const FramePayload& p = rq.payload;
    // (the records path walks the single frame's units of the handle's rows: it shares the Single key, so a slab
    // ordered by partitionCounts and one ordered by renderRecords itself keep one set of costs)
    key_.reset(p.kind == FrameKind::Records ? FrameKind::Single : p.kind);
    *tiles = rowCount() * tilesX_;  // (a composite: the single frame's units)
    if (const ViewBatch* vb = p.views()) {
        *tiles = vb->views * tiles_of(rq.width, rq.height);
        key_[ScheduleKey::kViewCount] = vb->views;
    } else if (const BatchFrame* bf = p.batch()) {  // (every view's width, height and count: batchHost_)
        *tiles = bf->tiles;
        key_[ScheduleKey::kViewCount] = bf->views;
        for (uint32_t v = 0; v < bf->views; ++v) {
            key_.push(batchHost_[v].tg.width);
            key_.push(batchHost_[v].tg.height);
            key_.push(batchHost_[v].count);
        }
    } else if (const ComposeFrame* cf = p.compose()) {  // (every object's count: composeHost_, 0 without an entry)
        key_[ScheduleKey::kViewCount] = cf->objects;
        for (uint32_t o = 0, e = 0; o < cf->objects; ++o) {
            const bool has = e < cf->entries && composeObject_[e] == o;
            key_.push(has ? composeHost_[e].count : 0u);
            e += has ? 1u : 0u;
        }
    }
    // (a pick frame walks without compaction or pairs, an occluded frame's walks end at the occluder, a styled
    // frame hides and fades gaussians: their costs are their own, either way round)
    // (a batch with options: the union over its views, so such batches keep unit costs of their own)
    key_[ScheduleKey::kPick] = (rq.pick || rq.anyPick) ? 1u : 0u;
    key_[ScheduleKey::kOccluded] = (rq.occluder || rq.anyOccluder) ? 1u : 0u;
    key_[ScheduleKey::kStyled] = rq.style.table ? 1u : 0u;
    key_[ScheduleKey::kUnitsPerTile] = blend_units_per_tile(*tiles, dev_.numCUs);
    key_[ScheduleKey::kWidth] = rq.width;
    key_[ScheduleKey::kHeight] = rq.height;
    key_[ScheduleKey::kRowBegin] = rowBegin_;
    key_[ScheduleKey::kRowEnd] = rowEnd_;
    key_[ScheduleKey::kRowStride] = rowStride_;
    // (an orthographic frame's footprints are another camera model's: its costs are its own, either way round; a
    // batch: whether any view is orthographic)
    if (rq.orthographic) key_.markOrthographic();
    return key_;
}

uint32_t GlobalRenderer::scheduleUnits(hipStream_t s, const ScheduleKey& key, uint32_t tiles) {
    const uint32_t units = tiles * key[ScheduleKey::kUnitsPerTile];
    if (schedState_.update(key)) {  // another frame: no walks to order by yet (either schedule set)
        for (const ScheduleSet& t : sched_) {
            if (!t.unitCost) continue;
            hipMemsetAsync(t.unitCost, 0, (size_t)units * sizeof(uint16_t), s);
            hipMemsetAsync(t.costMax, 0, (kCostMaxSlots + 2) * sizeof(uint32_t), s);
        }
    }
    return tuning_.costOrder ? units : 0u;
}

gsm_status GlobalRenderer::runFrame(hipStream_t s, const FrameRequest& rq) {
    (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's: the launches below are checked)
    const ProjectArgs& a = rq.args;
    const FrameTargets& tg = rq.targets;
    const int profiling = timer_.flags();
    const bool keep = (profiling & 2) != 0;
    // captured frame: the reference's intermediates (render data, sorted keys / values) are kept
    // for readback; the product path writes neither (the blend reads its records and half lists)
    const bool capture = (profiling & (2 | 16)) != 0;
    // (Views: a.count gaussians per view, every view's items padded to whole blocks.  Batch: the same per view.
    // Compose: the objects' items padded to whole blocks, everything from the scan on the single frame's)
    const ViewBatch* views = rq.payload.views();
    const BatchFrame* batch = rq.payload.batch();
    const ComposeFrame* comp = rq.payload.compose();
    const uint32_t nb = comp ? comp->blocks : batch ? batch->blocks : views ? views->views * views->blocksPerView
                                                                            : blocks_of(a.count);
    // GaussianRenderData for readback only when profiling (bits 0, 1), gsm_debug.h
    ProjectArgs fa = a;
    fa.keepRenderData = capture ? 1u : 0u;
    keptRenderData_ = fa.keepRenderData != 0;
    lastCount_ = a.count;
    lastItems_ = comp ? comp->blocks * (uint32_t)kProjectBlock : a.count;
    lastWidth_ = rq.width;
    lastHeight_ = rq.height;
    lastPick_ = rq.pick != nullptr;
    lastPickComposite_ = rq.pick && comp;
    lastPickObjects_ = !rq.pick ? 0u : comp ? comp->objects : 1u;
    // Blend schedule: the units ordered by the walk lengths the previous frame of the same
    // key measured (the image does not depend on the order, only the load balance does).
    // The ordering only needs those costs: one extra workgroup of the projection launch does it
    // (unit_order_block) while the others project (k_project, or k_records_in on the records path;
    // the multi-GPU frame orders them earlier, in its partition projection: preOrdered).
    uint32_t units = 0;
    if (!rq.preOrdered) {
        uint32_t tiles = 0;
        const ScheduleKey& key = requestKey(rq, &tiles);
        units = scheduleUnits(s, key, tiles);
    }
    const bool costOrder = rq.preOrdered ? tuning_.costOrder : units > 0;
    fa.schedUnits = units;
    // (written on every scheduled frame: the blend's remaining-walk priorities read the longest walk too)
    fa.pairBucket = tuning_.blendPairs ? (uint32_t)std::max(1, tuning_.pairBucket) : kUoBuckets;

    timer_.beginFrame();  // every stage bracketed by events, only the blend, or none
    timer_.record(0, s);
    // the projection (or records) launch; its block 0 orders the blend units (fa.schedUnits)
    if (rq.payload.kind == FrameKind::Records)
        launch_records_in(rq.records, fa, arena_, s, rq.devCount);
    else
        launch_project(config_.precision == GSM_PRECISION_FLOAT16, rq.shDegree, rq.payload, rq.world, rq.harm, fa,
                       rq.style.table ? &rq.style : nullptr, rq.orthographic, arena_, s);
    timer_.record(1, s);
    // (a frame of few blocks: the scatter's workgroups add up the block counts themselves).  The records path
    // (devCount: a multi-GPU slab) sizes its grids for the receive capacity but adds up only the blocks of
    // the records received -- at 8 ranks ~1/8 of a frame's gaussians -- so it takes the fused scan up to 4x
    // the block count (a slab that receives more than 2M records pays a longer prefix instead of the launch)
    const bool fusedScan = tuning_.fusedScan && nb > 0 && nb <= (rq.devCount ? 4u : 1u) * kFusedScanMaxBlocks;
    if (!fusedScan) launch_scan_blocks(nb, a, arena_, s, rq.devCount);
    timer_.record(2, s);
    launch_scatter(a, arena_, s, rq.payload, rq.devCount, fusedScan);
    if (keep) {  // preserve the unsorted assignment arrays for readback
        hipMemcpyAsync(arena_.keysKeep, arena_.keys[0], (size_t)maxAssignments_ * 4, hipMemcpyDeviceToDevice, s);
        hipMemcpyAsync(arena_.valsKeep, arena_.vals[0], (size_t)maxAssignments_ * 4, hipMemcpyDeviceToDevice, s);
    }
    timer_.record(3, s);
    uint32_t* kb[2] = {arena_.keys[0], arena_.keys[1]};
    uint32_t* vb[2] = {arena_.vals[0], arena_.vals[1]};
    FrameGeometry g;
    g.kind = rq.payload.kind;
    g.tilesX = tilesX_;
    g.tilesY = tilesY_;
    g.tileCount = tileCount_;
    g.rowBegin = rowBegin_;
    g.rowEnd = rowEnd_;
    g.rowStride = rowStride_;
    g.rowCount = rowCount();
    g.width = rq.width;
    g.height = rq.height;
    g.maxAssignments = maxAssignments_;
    if (batch) {  // every view on its own grid, one after another in the handle's tile space
        g.rowBegin = 0;
        g.rowStride = 1;
        g.views = batch->views;
        g.batchTiles = batch->tiles;
        g.batchArgs = batch->args;
        g.batchTileView = batch->tileView;
    } else if (views) {  // the frame's own tile grid, one after another in the handle's tile space
        g.tilesX = a.bin.tilesX;
        g.tilesY = a.bin.tilesY;
        g.rowBegin = 0;
        g.rowEnd = g.rowCount = g.tilesY;
        g.rowStride = 1;
        g.views = views->views;
        g.tilesPerView = views->tilesPerView;
        g.colorViewStride = rq.payload.colorViewStride;
        g.depthViewStride = rq.payload.depthViewStride;
    }
    // Frame sort.  Default: a stable LSD sort by the tile field only
    // (ceil(tileBits / 8) passes, the last one writing the tile starts), then each tile's run sorted
    // stably by depth by one wave in LDS -- the same order as the reference's 4-pass sort of
    // (tile << 16 | depth) keys.  Tuning::fullRadix keeps the 4 full 8-bit passes (A/B).
    const bool fullRadix = tuning_.fullRadix;
    // an occluded frame's blend walks the tiles' whole sorted runs: the tile sort writes them out
    // as it does for a captured frame
    // (a batch in which some view has a pick target or an occluder walks them too: its one union kernel is the
    // occluded pick walk)
    const bool unionWalk = batch && batch->extras && (rq.anyPick || rq.anyOccluder);
    const bool keepRuns = rq.occluder || unionWalk;
    const uint32_t* blendRun = nullptr;
    const bool ballot = tuning_.ballotRank;
    if (!fullRadix) {
        // the last tile pass also writes the tile starts (radix_sort_tiles: no pass over the keys); the
        // keys hold local tile ids of the renderer's rows (k_scatter): a slab of <= 2048 tiles
        // (multi-GPU) takes one wide pass
        const uint32_t localTiles = frame_tiles(g);  // (a batch: the pass plan follows views * tiles)
        const int res = radix_sort_tiles(kb, vb, &arena_.header->totalAssignments, maxAssignments_, 16,
                                         sort_space(arena_), arena_.tileStart, 0u, localTiles,
                                         tileCount_, s, ballot, tuning_.wideSort, tuning_.sortScanless);
        if (res == kSortNoSpace) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;  // (nothing of the sort launched)
        tile_depth_sort(kb[res], vb[res], kb[res ^ 1], vb[res ^ 1], arena_.tileStart, 0u, localTiles, s, ballot,
                        arena_.halfVals[0], arena_.halfVals[1],
                        arena_.halfCount, tileCount_, capture || keepRuns, dev_.numCUs);
        sortedKeys_ = capture ? kb[res ^ 1] : nullptr;
        sortedVals_ = capture ? vb[res ^ 1] : nullptr;
        blendRun = keepRuns ? vb[res ^ 1] : nullptr;
    } else {
        const int res = radix_sort_pairs(kb, vb, &arena_.header->totalAssignments, maxAssignments_, 0,
                                         sortPassCount(), sort_space(arena_), s, ballot,
                                         tuning_.sortScanless);
        if (res == kSortNoSpace) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
        sortedKeys_ = kb[res];
        sortedVals_ = vb[res];
        blendRun = vb[res];
    }
    unsortedKeys_ = keep ? arena_.keysKeep : nullptr;
    unsortedVals_ = keep ? arena_.valsKeep : nullptr;
    timer_.record(4, s);
    if (fullRadix) launch_headers(sortedKeys_, g, arena_, s);  // else done inside the sort
    // the blend walks per-half lists without the entries its half provably skips (k_scatter flags);
    // the tile sort writes them, the 4-pass sort needs the separate pass
    if (fullRadix)
        launch_half_lists(sortedVals_, 0u, frame_tiles(g), arena_, tileCount_, s);
    arena_.blendTrace = (profiling & 4) ? traceBuf_ : nullptr;
    // the schedule from the walks the previous frame's blend recorded (same stream: no join)
    timer_.record(5, s, true);
    BlendOptions bo;
    bo.costOrder = costOrder;
    bo.colorFormat = (int)config_.color_format;
    bo.waves = tuning_.blendWaves;
    bo.claim = tuning_.blendClaim;
    bo.pairs = tuning_.blendPairs;
    bo.arrive = rq.blendArrive;
    bo.pick = rq.pick;
    bo.occluder = rq.occluder;
    bo.sortedVals = blendRun;
    bo.batchExtras = unionWalk ? batch->extras : nullptr;
    bo.numCUs = dev_.numCUs;
    lastBlendKernel_ = launch_blend(g, arena_, tg, bo, s);
    timer_.record(6, s, true);
    timer_.frameDone();
    if (hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
    return GSM_OK;
}

gsm_status GlobalRenderer::counters(gsm_debug_counters* out) {
    hipSetDevice(dev_.id);
    TileAssignmentHeader h;
    if (hipMemcpy(&h, arena_.header, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess)
        return GSM_ERR_RENDER_FAILED;
    out->total_assignments = h.totalAssignments;
    out->max_capacity = h.maxCapacity;
    out->padded_count = h.paddedCount;
    out->overflow = h.overflow;
    out->tiles_x = tilesX_;
    out->tiles_y = tilesY_;
    out->tile_count = tileCount_;
    out->gaussian_count = lastCount_;
    return GSM_OK;
}

gsm_status GlobalRenderer::debugCopy(int which, void* dst, size_t bytes, size_t* needed) {
    hipSetDevice(dev_.id);
    gsm_debug_counters c;
    gsm_status st = counters(&c);
    if (st != GSM_OK) return st;
    // (the per-gaussian arrays are indexed by item: after a composite, 256 per block of every object)
    const size_t n = lastItems_, tot = c.total_assignments;
    const void* src = nullptr;
    size_t full = 0;
    switch (which) {
        case GSM_BUF_RENDER_DATA:
            if (!keptRenderData_) return GSM_ERR_MISSING_REQUIRED_BUFFER;  // frame not profiled (gsm_debug.h)
            src = arena_.renderData;
            full = n * 16;
            break;
        case GSM_BUF_BOUNDS: full = n * 16; break;
        case GSM_BUF_TILE_COUNTS: src = arena_.tileCounts; full = n * 4; break;
        case GSM_BUF_KEYS: src = unsortedKeys_; full = tot * 4; break;
        case GSM_BUF_VALUES: src = unsortedVals_; full = tot * 4; break;
        case GSM_BUF_SORTED_KEYS:  // kept by captured frames only (gsm_debug.h)
            if (!sortedKeys_) return GSM_ERR_MISSING_REQUIRED_BUFFER;
            src = sortedKeys_;
            full = tot * 4;
            break;
        case GSM_BUF_SORTED_VALUES:
            if (!sortedVals_) return GSM_ERR_MISSING_REQUIRED_BUFFER;
            src = sortedVals_;
            full = tot * 4;
            break;
        case GSM_BUF_HEADERS: full = (size_t)tileCount_ * 8; break;
        case GSM_BUF_EXP_TABLE: src = arena_.expTable; full = 65536 * 2; break;
        case GSM_BUF_BLEND_TRACE: src = (timer_.flags() & 4) ? traceBuf_ : nullptr; full = (size_t)tileCount_ * 4 * 4 * 8; break;
        default: return GSM_ERR_INVALID_ARGUMENT;
    }
    if (needed) *needed = full;
    if (!dst || bytes == 0) return GSM_OK;
    size_t cpy = bytes < full ? bytes : full;
    // {offset = lower_bound, count} per tile, as the reference
    if (which == GSM_BUF_BOUNDS) return copy_bounds_int4(arena_.bounds, n, dst, bytes);
    if (which == GSM_BUF_HEADERS) return copy_headers(arena_.tileStart, tileCount_, dst, bytes);
    if (!src) return full == 0 ? GSM_OK : GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (cpy && hipMemcpy(dst, src, cpy, hipMemcpyDeviceToHost) != hipSuccess) return GSM_ERR_RENDER_FAILED;
    if (which == GSM_BUF_VALUES || which == GSM_BUF_SORTED_VALUES) {  // the reference's ids: no skip flags
        uint32_t* v = (uint32_t*)dst;
        for (size_t i = 0; i < cpy / 4; ++i) v[i] &= kGidMask;
    }
    return GSM_OK;
}

gsm_status GlobalRenderer::setTileRows(uint32_t b, uint32_t e, uint32_t stride) {
    if (b == 0 && e == 0) {
        rowBegin_ = 0;
        rowEnd_ = tilesY_;
        rowStride_ = 1;
        return GSM_OK;
    }
    if (b >= e || e > tilesY_ || stride == 0) return GSM_ERR_INVALID_ARGUMENT;
    rowBegin_ = b;
    rowEnd_ = e;
    rowStride_ = stride;
    return GSM_OK;
}

gsm_status GlobalRenderer::setProfiling(int flags) {
    hipSetDevice(dev_.id);
    if ((flags & 2) && !arena_.keysKeep) {
        gsm_status st = allocs_.alloc((void**)&arena_.keysKeep, (size_t)maxAssignments_ * 4);
        if (st == GSM_OK) st = allocs_.alloc((void**)&arena_.valsKeep, (size_t)maxAssignments_ * 4);
        if (st != GSM_OK) return st;
    }
    if ((flags & 4) && !traceBuf_) {
        gsm_status st = allocs_.alloc((void**)&traceBuf_, (size_t)tileCount_ * 4 * 4 * 8);
        if (st != GSM_OK) return st;
    }
    return timer_.setProfiling(flags);  // bit 0 (every stage) or bit 3 (blend only); restarts the averaging window
}
}  // namespace gsm

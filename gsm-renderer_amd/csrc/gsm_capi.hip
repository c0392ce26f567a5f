// gsm_capi.hip -- extern "C" entry points declared in include/gsm_renderer.h and
// include/gsm_debug.h.  Thin, exception-free shims over gsm::GlobalRenderer.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/gsm_debug.h"
#include "../../include/gsm_multigpu.h"
#include "../../include/gsm_renderer.h"
#include "gsm_internal.h"
#include "gsm_frame_sort_check.h"
#include "gsm_renderer_impl.h"

namespace gsm {

// gsm_debug_frame_sort (include/gsm_debug.h): what a renderer owns for its frame sort, and the calls
// runFrame and the DepthFirst frame make on it.  No kernel of its own.
class FrameSorter {
   public:
    static gsm_status create(uint32_t capacity, uint32_t maxTiles, int device, FrameSorter** out) {
        FrameSorter* f = new (std::nothrow) FrameSorter;
        if (!f) return GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
        gsm_status st = pick_device(device, &f->dev_);
        if (st == GSM_OK) {
            f->allocs_.setDevice(f->dev_.id);
            f->tuning_ = tuning_from_env(f->dev_.id);  // GSM_SORT_RANK / _WIDE / _SCAN, as a renderer's create
            f->capacity_ = capacity;
            f->maxTiles_ = maxTiles;
            DeviceAllocations& M = f->allocs_;
            for (int i = 0; i < 2; ++i) {
                M.alloc(st, f->keys_[i], (size_t)capacity * 4);
                M.alloc(st, f->vals_[i], (size_t)capacity * 4);
                M.alloc(st, f->half_[i], (size_t)capacity * 4);
            }
            M.alloc(st, f->count_, 4);
            f->histBytes_ = sort_workspace_bytes(capacity);
            M.alloc(st, f->hist_, f->histBytes_);
            M.alloc(st, f->binTotals_, kSortTotalsWords * sizeof(uint32_t));
            M.alloc(st, f->buckets_, ((size_t)kWideBins + 1) * sizeof(uint32_t));
            M.alloc(st, f->tileStart_, ((size_t)maxTiles + 1) * sizeof(uint32_t));
            M.alloc(st, f->halfCount_, (size_t)maxTiles * 2 * sizeof(uint32_t));
            // the workspace is zeroed here and never again (the scanless row sets: every sort leaves them zero)
            if (st == GSM_OK && (hipMemset(f->hist_, 0, f->histBytes_) != hipSuccess ||
                                 hipMemset(f->tileStart_, 0, ((size_t)maxTiles + 1) * sizeof(uint32_t)) != hipSuccess))
                st = GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
        }
        if (st != GSM_OK) {
            delete f;
            return st;
        }
        *out = f;
        return GSM_OK;
    }

    gsm_status run(hipStream_t s, const gsm_debug_frame_sort_desc* desc, const void* keys, const void* values,
                   uint32_t n, gsm_debug_frame_sort_out* out) {
        gsm_status st = frame_sort_run_check(capacity_, maxTiles_, desc, keys, values, n, out);
        if (st != GSM_OK) return st;
        if (hipSetDevice(dev_.id) != hipSuccess) return GSM_ERR_DEVICE_NOT_AVAILABLE;
        (void)hipGetLastError();  // (an error left by an earlier call of the process is not this call's)
        const gsm_debug_frame_sort_desc d = *desc;
        out->plan = 0u;
        hostCount_ = n;
        if (n > 0u) {
            hipMemcpyAsync(keys_[0], keys, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
            hipMemcpyAsync(vals_[0], values, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
        }
        hipMemcpyAsync(count_, &hostCount_, 4, hipMemcpyHostToDevice, s);
        const SortSpace ws{hist_, histBytes_, binTotals_, kSortTotalsWords};
        const bool ballot = tuning_.ballotRank;
        // GlobalRenderer::runFrame (shift 16) and DepthFirstRenderer::sortTiles (shift 0): radix_sort_tiles_wide's
        // plan and radix_sort_tiles', whose kind is the plan reported
        const SortPlan plan = d.all_tiles > kFrameSortMaxTiles16
                                  ? plan_sort_tiles_wide(capacity_, d.all_tiles)
                                  : plan_sort_tiles(capacity_, d.shift, 0u, d.num_tiles, d.all_tiles, tuning_.wideSort,
                                                    tuning_.sortScanless);
        const int res = run_sort_plan(plan, keys_, vals_, count_, ws, tileStart_, buckets_, s, ballot);
        if (res == kSortNoSpace) return GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;  // (nothing of the sort launched)
        out->plan = plan.kind;
        int sorted = res;
        if (d.depth_sort) {
            // k_tile_sort indexes the runs by the starts: they are checked here first (a renderer does not look)
            starts_.resize((size_t)d.num_tiles + 1);
            if (hipMemcpyAsync(starts_.data(), tileStart_, starts_.size() * 4, hipMemcpyDeviceToHost, s) != hipSuccess ||
                hipStreamSynchronize(s) != hipSuccess || !frame_sort_starts_in_range(starts_.data(), d.num_tiles, n)) {
                st = GSM_ERR_RENDER_FAILED;
            } else {
                tile_depth_sort(keys_[res], vals_[res], keys_[res ^ 1], vals_[res ^ 1], tileStart_, 0u, d.num_tiles, s,
                                ballot, half_[0], half_[1], halfCount_, d.all_tiles, d.full != 0u, dev_.numCUs);
                sorted = res ^ 1;
            }
        }
        auto copy_out = [&](uint32_t* dst, const uint32_t* src, size_t words) {
            if (dst && words) hipMemcpyAsync(dst, src, words * 4, hipMemcpyDeviceToHost, s);
        };
        copy_out(out->sorted_keys, keys_[sorted], n);
        copy_out(out->sorted_values, vals_[sorted], n);
        copy_out(out->tile_start, tileStart_, (size_t)d.all_tiles + 1);
        if (d.depth_sort && st == GSM_OK) {
            copy_out(out->half0, half_[0], n);
            copy_out(out->half1, half_[1], n);
            copy_out(out->half_count, halfCount_, (size_t)d.all_tiles * 2);
        }
        if (hipStreamSynchronize(s) != hipSuccess || hipGetLastError() != hipSuccess) return GSM_ERR_RENDER_FAILED;
        return st;
    }

   private:
    FrameSorter() = default;
    Device dev_;
    DeviceAllocations allocs_;
    Tuning tuning_;
    uint32_t capacity_ = 0, maxTiles_ = 0, hostCount_ = 0;
    uint32_t *keys_[2] = {nullptr, nullptr}, *vals_[2] = {nullptr, nullptr}, *half_[2] = {nullptr, nullptr};
    uint32_t *count_ = nullptr, *hist_ = nullptr, *binTotals_ = nullptr, *buckets_ = nullptr, *tileStart_ = nullptr,
             *halfCount_ = nullptr;
    size_t histBytes_ = 0;
    std::vector<uint32_t> starts_;
};

}  // namespace gsm

struct gsm_debug_frame_sort : gsm::Handle<gsm::FrameSorter> {};

extern "C" {

int gsm_abi_version(void) { return GSM_ABI_VERSION; }

const char* gsm_status_string(gsm_status s) {
    // RendererError.description (GaussianRendererProtocol.swift:294-323)
    switch (s) {
        case GSM_OK: return "ok";
        case GSM_ERR_DEVICE_NOT_AVAILABLE: return "HIP device not available";
        case GSM_ERR_FAILED_TO_CREATE_LIBRARY: return "Failed to create kernel library";
        case GSM_ERR_FAILED_TO_CREATE_PIPELINE: return "Failed to create pipeline";
        case GSM_ERR_FAILED_TO_ALLOCATE_BUFFER: return "Failed to allocate buffer";
        case GSM_ERR_FAILED_TO_ALLOCATE_TEXTURE: return "Failed to allocate texture";
        case GSM_ERR_INVALID_GAUSSIAN_COUNT: return "Gaussian count exceeds maximum";
        case GSM_ERR_INVALID_DIMENSIONS: return "Dimensions exceed maximum";
        case GSM_ERR_INVALID_BUFFER_SIZE: return "Buffer has invalid size";
        case GSM_ERR_INVALID_TILE_COUNT: return "Tile count exceeds maximum";
        case GSM_ERR_INVALID_ASSIGNMENT_CAPACITY: return "Required tile assignment capacity exceeds available";
        case GSM_ERR_RENDER_FAILED: return "Render failed";
        case GSM_ERR_ENCODER_CREATION_FAILED: return "Failed to create stage";
        case GSM_ERR_MISSING_REQUIRED_BUFFER: return "Missing required buffer";
        case GSM_ERR_INVALID_ARGUMENT: return "Invalid argument";
        case GSM_ERR_UNSUPPORTED: return "GlobalRenderer does not support stereo rendering";
        case GSM_ERR_PHASE_ORDER: return "Multi-GPU frame phase called out of order (gsm_multigpu_finish_frame)";
    }
    return "unknown status";
}

void gsm_renderer_config_default(gsm_renderer_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->max_gaussians = 6000000u;
    c->max_width = 1920u;
    c->max_height = 1080u;
    c->precision = GSM_PRECISION_FLOAT16;
    c->color_format = 0u;
    c->gaussian_color_space = GSM_COLOR_SPACE_SRGB;
    c->back_to_front = 0u;
}

void gsm_camera_params_init(gsm_camera_params* cam, const float view[16], const float proj[16],
                            const float position[3], float focal_x, float focal_y) {
    if (!cam) return;
    std::memset(cam, 0, sizeof(*cam));
    if (view) std::memcpy(cam->view, view, sizeof(cam->view));
    if (proj) std::memcpy(cam->proj, proj, sizeof(cam->proj));
    if (position) std::memcpy(cam->position, position, sizeof(cam->position));
    cam->focal_x = focal_x;
    cam->focal_y = focal_y;
    cam->near_plane = 0.1f;
    cam->far_plane = 10.0f;
}

gsm_status gsm_global_create(const gsm_renderer_config* config, int hip_device, gsm_renderer** out) {
    if (!out) return GSM_ERR_INVALID_ARGUMENT;
    gsm_renderer_config cfg;
    if (config) cfg = *config;
    else gsm_renderer_config_default(&cfg);
    return gsm_renderer::create(out, cfg, hip_device);
}

void gsm_global_destroy(gsm_renderer* r) { gsm_renderer::destroy(r); }

gsm_status gsm_global_render(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                             const gsm_camera_params* camera, uint32_t width, uint32_t height,
                             void* color, size_t color_pitch, void* depth, size_t depth_pitch) {
    if (!r || !r->impl || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderFrame((hipStream_t)stream, *input, *camera, width, height,
                                gsm::FrameTargets{color, color_pitch, depth, depth_pitch});
}

gsm_status gsm_global_render_views(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                   const gsm_camera_params* cameras, uint32_t view_count, uint32_t width,
                                   uint32_t height, void* color, size_t color_pitch, size_t color_view_stride,
                                   void* depth, size_t depth_pitch, size_t depth_view_stride) {
    if (!r || !r->impl || !input) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderViews((hipStream_t)stream, *input, cameras, view_count, width, height, color, color_pitch,
                                color_view_stride, depth, depth_pitch, depth_view_stride);
}

gsm_status gsm_global_render_batch(gsm_renderer* r, void* stream, const gsm_global_view* views, uint32_t view_count) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderBatch((hipStream_t)stream, views, view_count);
}

gsm_status gsm_global_render_composite(gsm_renderer* r, void* stream, const gsm_global_object* objects,
                                       uint32_t object_count, uint32_t width, uint32_t height, void* color,
                                       size_t color_pitch, void* depth, size_t depth_pitch) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->composeFrame((hipStream_t)stream, objects, object_count, width, height,
                                 gsm::FrameTargets{color, color_pitch, depth, depth_pitch});
}

gsm_status gsm_global_render_pick(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                  const gsm_camera_params* camera, uint32_t width, uint32_t height, void* color,
                                  size_t color_pitch, void* depth, size_t depth_pitch, void* pick,
                                  size_t pick_pitch) {
    if (!r || !r->impl || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::PickTarget pt{pick, pick_pitch};
    gsm::FrameExtras extras;
    extras.pick = &pt;
    return r->impl->renderFrame((hipStream_t)stream, *input, *camera, width, height,
                                gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_render_composite_pick(gsm_renderer* r, void* stream, const gsm_global_object* objects,
                                            uint32_t object_count, uint32_t width, uint32_t height, void* color,
                                            size_t color_pitch, void* depth, size_t depth_pitch, void* pick,
                                            size_t pick_pitch) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::PickTarget pt{pick, pick_pitch};
    gsm::FrameExtras extras;
    extras.pick = &pt;
    return r->impl->composeFrame((hipStream_t)stream, objects, object_count, width, height,
                                 gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_render_occluded(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                      const gsm_camera_params* camera, uint32_t width, uint32_t height, void* color,
                                      size_t color_pitch, void* depth, size_t depth_pitch, const void* occluder,
                                      size_t occluder_pitch) {
    if (!r || !r->impl || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::OccluderSource os{occluder, occluder_pitch};
    gsm::FrameExtras extras;
    extras.occluder = &os;
    return r->impl->renderFrame((hipStream_t)stream, *input, *camera, width, height,
                                gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_render_composite_occluded(gsm_renderer* r, void* stream, const gsm_global_object* objects,
                                                uint32_t object_count, uint32_t width, uint32_t height, void* color,
                                                size_t color_pitch, void* depth, size_t depth_pitch,
                                                const void* occluder, size_t occluder_pitch) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::OccluderSource os{occluder, occluder_pitch};
    gsm::FrameExtras extras;
    extras.occluder = &os;
    return r->impl->composeFrame((hipStream_t)stream, objects, object_count, width, height,
                                 gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_render_styled(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                    const gsm_camera_params* camera, uint32_t width, uint32_t height, void* color,
                                    size_t color_pitch, void* depth, size_t depth_pitch, void* pick, size_t pick_pitch,
                                    const gsm_global_state* state, const gsm_global_style* styles,
                                    uint32_t style_count) {
    if (!r || !r->impl || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::PickTarget pt{pick, pick_pitch};
    const gsm::StyleSource ss{state, styles, style_count};
    gsm::FrameExtras extras;
    extras.pick = pick ? &pt : nullptr;  // (a null pick pointer: the plain blend)
    extras.style = &ss;
    return r->impl->renderFrame((hipStream_t)stream, *input, *camera, width, height,
                                gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_render_composite_styled(gsm_renderer* r, void* stream, const gsm_global_object* objects,
                                              uint32_t object_count, uint32_t width, uint32_t height, void* color,
                                              size_t color_pitch, void* depth, size_t depth_pitch, void* pick,
                                              size_t pick_pitch, const gsm_global_state* states,
                                              const gsm_global_style* styles, uint32_t style_count) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::PickTarget pt{pick, pick_pitch};
    const gsm::StyleSource ss{states, styles, style_count};
    gsm::FrameExtras extras;
    extras.pick = pick ? &pt : nullptr;  // (a null pick pointer: the plain blend)
    extras.style = &ss;
    return r->impl->composeFrame((hipStream_t)stream, objects, object_count, width, height,
                                 gsm::FrameTargets{color, color_pitch, depth, depth_pitch}, extras);
}

gsm_status gsm_global_select_mask(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                  const gsm_camera_params* camera, uint32_t width, uint32_t height, const void* mask,
                                  size_t mask_pitch, uint8_t* state, const gsm_global_style* styles,
                                  uint32_t style_count, uint32_t and_mask, uint32_t xor_mask, uint32_t* matched) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->selectMask((hipStream_t)stream, input, camera, width, height, mask, mask_pitch, state, styles,
                               style_count, and_mask, xor_mask, matched);
}

gsm_status gsm_global_select_mask_ortho(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                        const gsm_camera_params* camera, uint32_t width, uint32_t height,
                                        const void* mask, size_t mask_pitch, uint8_t* state,
                                        const gsm_global_style* styles, uint32_t style_count, uint32_t and_mask,
                                        uint32_t xor_mask, uint32_t* matched) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->selectMask((hipStream_t)stream, input, camera, width, height, mask, mask_pitch, state, styles,
                               style_count, and_mask, xor_mask, matched, true);
}

gsm_status gsm_global_render_frame(gsm_renderer* r, void* stream, const gsm_global_frame* f) {
    if (!r || !r->impl || !f || (f->flags & ~GSM_FRAME_ORTHOGRAPHIC)) return GSM_ERR_INVALID_ARGUMENT;
    const gsm::PickTarget pt{f->pick_r32u, f->pick_pitch_bytes};
    const gsm::OccluderSource os{f->occluder_r32f, f->occluder_pitch_bytes};
    const gsm::StyleSource ss{f->states, f->styles, f->style_count};
    gsm::FrameExtras extras;  // (a null pointer: the option is not given)
    extras.pick = f->pick_r32u ? &pt : nullptr;
    extras.occluder = f->occluder_r32f ? &os : nullptr;
    extras.style = (f->states || f->styles) ? &ss : nullptr;  // (one without the other: the styled row refuses)
    extras.orthographic = (f->flags & GSM_FRAME_ORTHOGRAPHIC) != 0;
    const gsm::FrameTargets targets{f->color, f->color_pitch_bytes, f->depth_r16f, f->depth_pitch_bytes};
    if (f->object_count == 1 && f->objects)  // one object: the single frame
        return r->impl->renderFrame((hipStream_t)stream, f->objects[0].input, f->objects[0].camera, f->width,
                                    f->height, targets, extras);
    return r->impl->composeFrame((hipStream_t)stream, f->objects, f->object_count, f->width, f->height, targets,
                                 extras);
}

gsm_status gsm_global_select_pick(gsm_renderer* r, void* stream, const void* pick, size_t pick_pitch, uint32_t width,
                                  uint32_t height, const void* mask, size_t mask_pitch, uint32_t object,
                                  uint8_t* state, uint32_t gaussian_count, uint32_t and_mask, uint32_t xor_mask,
                                  uint32_t* matched) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->selectPick((hipStream_t)stream, pick, pick_pitch, width, height, mask, mask_pitch, object, state,
                               gaussian_count, and_mask, xor_mask, matched);
}

gsm_status gsm_global_render_frames(gsm_renderer* r, void* stream, const gsm_global_frame* frames,
                                    uint32_t frame_count) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderFrames((hipStream_t)stream, frames, frame_count);
}

gsm_status gsm_global_select_pick_ids(gsm_renderer* r, void* stream, const void* pick, size_t pick_pitch,
                                      uint32_t width, uint32_t height, const void* mask, size_t mask_pitch,
                                      uint8_t* state, uint32_t gaussian_count, uint32_t and_mask, uint32_t xor_mask,
                                      uint32_t* matched) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->selectPickIds((hipStream_t)stream, pick, pick_pitch, width, height, mask, mask_pitch, state,
                                  gaussian_count, and_mask, xor_mask, matched);
}

void gsm_global_keep_visible(const gsm_global_style* styles, uint32_t style_count, uint32_t keep[8]) {
    gsm::keep_visible(styles, style_count, keep);
}

void gsm_global_keep_masked(uint32_t test_mask, uint32_t test_value, uint32_t keep[8]) {
    gsm::keep_masked(test_mask, test_value, keep);
}

gsm_status gsm_global_extract(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                              const gsm_global_state* state, const uint32_t keep[8], const gsm_global_extract_out* out,
                              uint32_t* kept) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->extract((hipStream_t)stream, input, state, keep, out, kept);
}

gsm_status gsm_global_state_histogram(gsm_renderer* r, void* stream, const uint8_t* state, uint32_t gaussian_count,
                                      uint32_t* histogram) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->stateHistogram((hipStream_t)stream, state, gaussian_count, histogram);
}

void gsm_global_select_query_default(gsm_global_select_query* q) { gsm::select_query_default(q); }

gsm_status gsm_global_select_where(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                   const gsm_global_select_query* query, uint8_t* state,
                                   const gsm_global_style* styles, uint32_t style_count, uint32_t and_mask,
                                   uint32_t xor_mask, uint32_t* matched) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->selectWhere((hipStream_t)stream, input, query, state, styles, style_count, and_mask, xor_mask,
                                matched);
}

gsm_status gsm_global_state_bounds(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                   const gsm_global_state* state, const uint32_t keep[8], gsm_global_bounds* bounds) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->stateBounds((hipStream_t)stream, input, state, keep, bounds);
}

gsm_status gsm_global_transform_from_pose(const float rotation[9], float scale, const float translation[3],
                                          gsm_global_transform_desc* out) {
    return gsm::transform_from_pose(rotation, scale, translation, out);
}

gsm_status gsm_global_transform(gsm_renderer* r, void* stream, const gsm_global_scene* scene,
                                const gsm_global_state* state, const uint32_t keep[8],
                                const gsm_global_transform_desc* desc) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->transform((hipStream_t)stream, scene, state, keep, desc);
}

gsm_status gsm_global_pick_owner(gsm_renderer* r, const uint32_t* items, uint32_t n, uint32_t* object,
                                 uint32_t* gaussian) {
    if (!r || !r->impl || (n > 0 && (!items || !object || !gaussian))) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->pickOwner(items, n, object, gaussian);
}

gsm_status gsm_global_project_partition(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                        const gsm_camera_params* camera, uint32_t width, uint32_t height,
                                        uint32_t first, uint32_t count, const uint32_t* slab_rows,
                                        uint32_t num_slabs, void* send, uint64_t send_capacity,
                                        uint32_t* send_counts) {
    if (!r || !r->impl || !input || !camera) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->projectPartition((hipStream_t)stream, *input, *camera, width, height, first, count,
                                     slab_rows, num_slabs, send, send_capacity, send_counts);
}

gsm_status gsm_global_render_records(gsm_renderer* r, void* stream, const void* records, uint32_t count,
                                     uint32_t width, uint32_t height, void* color, size_t color_pitch,
                                     void* depth, size_t depth_pitch) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderRecords((hipStream_t)stream, records, count, width, height, color, color_pitch,
                                  depth, depth_pitch);
}

gsm_status gsm_global_render_stereo_sbs(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                        const gsm_camera_params* left, const gsm_camera_params* right,
                                        uint32_t width_per_eye, uint32_t height, void* color, size_t color_pitch,
                                        void* depth, size_t depth_pitch) {
    if (!r || !r->impl || !input || !left || !right) return GSM_ERR_INVALID_ARGUMENT;
    if (!color) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    gsm_status st = r->impl->renderFrame((hipStream_t)stream, *input, *left, width_per_eye, height,
                                         gsm::FrameTargets{color, color_pitch, depth, depth_pitch});
    if (st != GSM_OK) return st;
    char* rc = (char*)color + (size_t)width_per_eye * 8;
    char* rd = depth ? (char*)depth + (size_t)width_per_eye * 2 : nullptr;
    return r->impl->renderFrame((hipStream_t)stream, *input, *right, width_per_eye, height,
                                gsm::FrameTargets{rc, color_pitch, rd, depth_pitch});
}

gsm_status gsm_global_render_stereo(gsm_renderer* r, void*, const gsm_gaussian_input*,
                                    const gsm_camera_params*, const gsm_camera_params*, uint32_t,
                                    uint32_t, void*, size_t, void*, size_t) {
    if (!r) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_ERR_UNSUPPORTED;  // GlobalRenderer.swift:248-254 fatalError
}

uint32_t gsm_global_debug_read_total_assignments(gsm_renderer* r) {
    if (!r || !r->impl) return 0;
    gsm_debug_counters c;
    if (r->impl->counters(&c) != GSM_OK) return 0;
    return c.total_assignments;
}

gsm_status gsm_global_last_gpu_time(gsm_renderer* r, double* seconds) {
    if (!r || !r->impl || !seconds) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->lastGpuTime(seconds);
}

gsm_status gsm_global_debug_counters(gsm_renderer* r, gsm_debug_counters* out) {
    if (!r || !r->impl || !out) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->counters(out);
}

gsm_status gsm_global_debug_blend_kernel(gsm_renderer* r, int* kind) {
    if (!r || !r->impl || !kind) return GSM_ERR_INVALID_ARGUMENT;
    *kind = r->impl->lastBlendKernel();
    return GSM_OK;
}

gsm_status gsm_global_debug_copy(gsm_renderer* r, int which, void* dst, size_t bytes, size_t* needed) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->debugCopy(which, dst, bytes, needed);
}

gsm_status gsm_global_set_profiling(gsm_renderer* r, int enable) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->setProfiling(enable);
}

gsm_status gsm_global_stage_times(gsm_renderer* r, float* ms, int n) {
    if (!r || !r->impl || !ms) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->stageTimes(ms, n);
}

gsm_status gsm_global_set_tile_rows(gsm_renderer* r, uint32_t b, uint32_t e) {
    if (!r || !r->impl) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->setTileRows(b, e);
}

size_t gsm_debug_sort_workspace_bytes(uint32_t capacity) { return gsm::sort_workspace_bytes(capacity); }

gsm_status gsm_debug_sort_plan_fits(uint32_t capacity, uint32_t key_bits, int wide, size_t hist_bytes) {
    if (key_bits == 0 || key_bits > 32) return GSM_ERR_INVALID_ARGUMENT;
    // (placeholder pointers: the plan only compares footprints, nothing is dereferenced or launched)
    const gsm::SortSpace ws{(uint32_t*)(uintptr_t)16, hist_bytes, (uint32_t*)(uintptr_t)16, gsm::kSortTotalsWords};
    return gsm::sort_bits_plan_fits(capacity, key_bits, wide != 0, ws) ? GSM_OK : GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
}

gsm_status gsm_sort_pairs_u32(void* keys, void* values, uint32_t n, uint32_t key_bits, void* stream) {
    if ((!keys || !values) && n > 0) return GSM_ERR_INVALID_ARGUMENT;
    if (n == 0) return GSM_OK;
    if (key_bits == 0 || key_bits > 32) key_bits = 32;
    hipStream_t s = (hipStream_t)stream;
    uint32_t *k2 = nullptr, *v2 = nullptr, *hist = nullptr, *bins = nullptr, *np = nullptr;
    gsm_status st = GSM_OK;
    if (hipMalloc(&k2, (size_t)n * 4) != hipSuccess || hipMalloc(&v2, (size_t)n * 4) != hipSuccess ||
        hipMalloc(&hist, gsm::sort_workspace_bytes(n)) != hipSuccess || hipMalloc(&bins, 256 * 4) != hipSuccess ||
        hipMalloc(&np, 4) != hipSuccess) {
        st = GSM_ERR_FAILED_TO_ALLOCATE_BUFFER;
    }
    if (st == GSM_OK) {
        hipMemcpyAsync(np, &n, 4, hipMemcpyHostToDevice, s);
        hipMemsetAsync(hist, 0, gsm::sort_workspace_bytes(n), s);
        uint32_t* kb[2] = {(uint32_t*)keys, k2};
        uint32_t* vb[2] = {(uint32_t*)values, v2};
        const int digits = (int)((key_bits + 7) / 8);
        int dev = 0;
        hipGetDevice(&dev);
        const gsm::Tuning tn = gsm::tuning_from_env(dev);  // read per call: no renderer here
        const gsm::SortSpace ws{hist, gsm::sort_workspace_bytes(n), bins, 256};
        int res = gsm::radix_sort_pairs(kb, vb, np, n, 0, digits, ws, s, tn.ballotRank, tn.sortScanless);
        if (res == gsm::kSortNoSpace) st = GSM_ERR_INVALID_ASSIGNMENT_CAPACITY;
        if (res == 1) {
            hipMemcpyAsync(keys, k2, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
            hipMemcpyAsync(values, v2, (size_t)n * 4, hipMemcpyDeviceToDevice, s);
        }
        if (hipStreamSynchronize(s) != hipSuccess) st = GSM_ERR_RENDER_FAILED;
    }
    hipFree(k2);
    hipFree(v2);
    hipFree(hist);
    hipFree(bins);
    hipFree(np);
    return st;
}

gsm_status gsm_debug_frame_sort_create(uint32_t capacity, uint32_t max_tiles, int hip_device,
                                       gsm_debug_frame_sort** out) {
    const gsm_status st = gsm::frame_sort_create_check(capacity, max_tiles, out);
    if (st != GSM_OK) return st;
    return gsm_debug_frame_sort::create(out, capacity, max_tiles, hip_device);
}

void gsm_debug_frame_sort_destroy(gsm_debug_frame_sort* f) { gsm_debug_frame_sort::destroy(f); }

gsm_status gsm_debug_frame_sort_run(gsm_debug_frame_sort* f, void* stream, const gsm_debug_frame_sort_desc* desc,
                                    const void* keys, const void* values, uint32_t n, gsm_debug_frame_sort_out* out) {
    if (!f || !f->impl) return GSM_ERR_INVALID_ARGUMENT;
    return f->impl->run((hipStream_t)stream, desc, keys, values, n, out);
}

gsm_status gsm_debug_sort_rank_probe(int hip_device, int* lane_ordered) {
    if (!lane_ordered) return GSM_ERR_INVALID_ARGUMENT;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || hip_device < 0 || hip_device >= ndev) {
        (void)hipGetLastError();
        return GSM_ERR_DEVICE_NOT_AVAILABLE;
    }
    *lane_ordered = gsm::sort_lane_ordered_atomics(hip_device) ? 1 : 0;
    return GSM_OK;
}

gsm_status gsm_debug_partition_counts(gsm_renderer* r, void* stream, const gsm_gaussian_input* input,
                                      const gsm_camera_params* camera, uint32_t width, uint32_t height,
                                      uint32_t first, uint32_t count, const uint32_t* slab_rows,
                                      uint32_t num_slabs, uint32_t* d_send_counts) {
    if (!r || !r->impl || !input || !camera || !slab_rows || !d_send_counts) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->partitionCounts((hipStream_t)stream, *input, *camera, width, height, first, count, slab_rows,
                                    num_slabs, d_send_counts);
}

gsm_status gsm_debug_partition_push(gsm_renderer* r, void* stream, uint32_t world, uint32_t rank,
                                    const uint32_t* d_counts, void* const* recv_buffers, uint32_t* d_recv_count) {
    if (!r || !r->impl || !d_counts || !recv_buffers || !d_recv_count || world < 1 || world > gsm::kMaxSlabs ||
        rank >= world)
        return GSM_ERR_INVALID_ARGUMENT;
    gsm::SlabPeers peers{};
    for (uint32_t p = 0; p < world; ++p) {
        if (!recv_buffers[p]) return GSM_ERR_INVALID_ARGUMENT;
        peers.recv[p] = (gsm::SplatRecord*)recv_buffers[p];
        peers.cap[p] = r->impl->maxGaussians();  // (gsm_debug.h: each holds max_gaussians records)
    }
    return r->impl->partitionPush((hipStream_t)stream, world, rank, d_counts, peers, d_recv_count, gsm::MgArrive{});
}

gsm_status gsm_debug_render_records_device_count(gsm_renderer* r, void* stream, const void* records,
                                                 uint32_t capacity, const uint32_t* d_count, uint32_t width,
                                                 uint32_t height, void* color, size_t color_pitch, void* depth,
                                                 size_t depth_pitch) {
    if (!r || !r->impl || !d_count) return GSM_ERR_INVALID_ARGUMENT;
    return r->impl->renderRecords((hipStream_t)stream, records, capacity, width, height, color, color_pitch, depth,
                                  depth_pitch, d_count);
}

}  // extern "C"

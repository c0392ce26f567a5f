// gsm_frame_plan.h -- what the Global frame entries refuse, in which order, and where each view or object lies in the
// handle's item and tile space (host only, plain C++17: no HIP).  Every entry of gsm_renderer.hip is check (here), then
// device and lazy allocation, then fill from the layout (here), then runFrame; validate_frame is the part the DepthFirst
// and Local renderers share.  tests/host/frame_plan_test.cpp holds every row and layout to values written by hand.
// DESIGN.md 35.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "../../include/gsm_renderer.h"
#include "gsm_blend_plan.h"
#include "gsm_types.h"

namespace gsm {

// ---- constants the checks share with the kernels ----
constexpr int kProjectBlock = 256;        // gaussians of a projection workgroup: a view's or object's items start on one
constexpr uint32_t kStyleEntries = 256;   // styles of the handle's table: one per state byte
constexpr uint32_t kMaxSlabs = 16;        // tile-row slabs of a partitioned frame
constexpr uint32_t kBatchIndexMax = 65535u;  // a batch's tiles and a composite's objects: 16-bit table entries

// ---- the rules, each once ----
constexpr uint32_t blocks_of(uint32_t count) { return (uint32_t)(((uint64_t)count + kProjectBlock - 1) / kProjectBlock); }
// a view's or object's items, padded to whole blocks
constexpr uint64_t padded_items(uint32_t count) { return (uint64_t)blocks_of(count) * kProjectBlock; }
constexpr uint32_t tiles_x(uint32_t width) { return (width + kTileWidth - 1) / kTileWidth; }
constexpr uint32_t tiles_y(uint32_t height) { return (height + kTileHeight - 1) / kTileHeight; }
constexpr uint32_t tiles_of(uint32_t width, uint32_t height) { return tiles_x(width) * tiles_y(height); }
// the most views a batch of that tile space holds (every view takes at least one tile)
constexpr uint32_t max_batch_views(uint32_t tileCount) { return tileCount < kBatchIndexMax ? tileCount : kBatchIndexMax; }
// the most entries of a composite (every entry takes at least one block)
constexpr uint32_t max_compose_entries(uint32_t maxBlocks) { return maxBlocks < kBatchIndexMax ? maxBlocks : kBatchIndexMax; }
// a batch's tiles within the handle's tile space and the 16-bit tile field
constexpr bool batch_tiles_ok(uint64_t allTiles, uint32_t tileCount) {
    return allTiles <= tileCount && allTiles <= kBatchIndexMax;
}

// What a handle contributes to the checks.
struct FrameLimits {
    uint32_t colorFormat = 0;  // gsm_color_format of the colour target
    uint32_t maxGaussians = 1, maxWidth = 1, maxHeight = 1;
    uint32_t tileCount = 1, tilesY = 1;
    bool rowsRestricted = false;  // set_tile_rows holds the handle to some of its rows
    uint32_t rowStride = 1;
    uint32_t maxBlocks() const { return blocks_of(maxGaussians); }
    bool sizeOk(uint32_t width, uint32_t height) const {
        return width != 0 && height != 0 && width <= maxWidth && height <= maxHeight;
    }
};

// ---- what an entry is given ----
inline uint32_t color_bytes_per_pixel(uint32_t format) {
    return format == GSM_COLOR_FORMAT_RGBA16F ? 8u : (format == GSM_COLOR_FORMAT_RGBA32F ? 16u : 4u);
}
// the colour and depth targets of a frame (depth nullable; a Views frame's are view 0's, a Batch's are per view)
struct FrameTargets {
    void* color = nullptr;
    size_t colorPitch = 0;
    void* depth = nullptr;
    size_t depthPitch = 0;
};
// pick (nullable): a pick frame's third target (one uint32_t per pixel, required like colour); it joins the
// missing-buffer row and the buffer-size row.
struct PickTarget {
    void* pixels;
    size_t pitch;
};
// occluder (nullable): an occluded frame's depth image (one float per pixel, read only, required like colour); it
// joins the same two rows.
struct OccluderSource {
    const void* pixels;
    size_t pitch;
};
// style: the style of every gaussian's state byte applied in the projection -- the caller's states,
// one per object, and its table: host memory, consumed by the call.
struct StyleSource {
    const gsm_global_state* states;
    const gsm_global_style* styles;
    uint32_t styleCount;
};
// What the entries of a family add to the plain frame, all nullable and independent (gsm_global_render_frame
// passes any combination).  orthographic: the frame's flag GSM_FRAME_ORTHOGRAPHIC.
struct FrameExtras {
    const PickTarget* pick = nullptr;
    const OccluderSource* occluder = nullptr;
    const StyleSource* style = nullptr;
    bool orthographic = false;
};

// ---- validate_frame: the Global, DepthFirst and Local single frames ----
// What a frame call refuses, in this precedence: count, dimensions, missing buffer, buffer size.
// widthFactor: frames a row of the colour target holds (2: side by side).  depth may be null.
inline gsm_status validate_frame(uint32_t colorFormat, uint32_t maxGaussians, uint32_t maxWidth, uint32_t maxHeight,
                                 uint32_t count, bool allowEmpty, bool inputMissing, uint32_t width, uint32_t height,
                                 const void* color, size_t colorPitch, uint32_t widthFactor, const void* depth,
                                 size_t depthPitch, const PickTarget* pick = nullptr,
                                 const OccluderSource* occluder = nullptr) {
    // validateLimits (GlobalRenderer.swift:372-376) -- errors instead of a silent skip
    if (count > maxGaussians || (count == 0 && !allowEmpty)) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (width == 0 || height == 0 || width > maxWidth || height > maxHeight) return GSM_ERR_INVALID_DIMENSIONS;
    if (!color || (pick && !pick->pixels) || (occluder && !occluder->pixels) || (count > 0 && inputMissing))
        return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (colorPitch < (size_t)widthFactor * width * color_bytes_per_pixel(colorFormat)) return GSM_ERR_INVALID_BUFFER_SIZE;
    // the blend stores at least 4-byte words of colour and 2-byte depth values
    if ((((uintptr_t)color) & 3u) || (colorPitch & 3u)) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (depth && (depthPitch < (size_t)width * 2 || (depthPitch & 1u) || (((uintptr_t)depth) & 1u)))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    // the blend stores 4-byte words of pick
    if (pick && (pick->pitch < (size_t)width * 4 || (pick->pitch & 3u) || (((uintptr_t)pick->pixels) & 3u)))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    // the blend loads 4-byte words of the occluder
    if (occluder &&
        (occluder->pitch < (size_t)width * 4 || (occluder->pitch & 3u) || (((uintptr_t)occluder->pixels) & 3u)))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    return GSM_OK;
}
inline gsm_status validate_frame(const gsm_renderer_config& cfg, uint32_t maxGaussians, uint32_t maxWidth,
                                 uint32_t maxHeight, uint32_t count, bool allowEmpty, bool inputMissing, uint32_t width,
                                 uint32_t height, const void* color, size_t colorPitch, uint32_t widthFactor,
                                 const void* depth, size_t depthPitch, const PickTarget* pick = nullptr,
                                 const OccluderSource* occluder = nullptr) {
    return validate_frame(cfg.color_format, maxGaussians, maxWidth, maxHeight, count, allowEmpty, inputMissing, width,
                          height, color, colorPitch, widthFactor, depth, depthPitch, pick, occluder);
}
// the Global form: an empty scene is a frame, one frame per row
inline gsm_status validate_frame(const FrameLimits& L, uint32_t count, bool inputMissing, uint32_t width, uint32_t height,
                                 const FrameTargets& t, const PickTarget* pick = nullptr,
                                 const OccluderSource* occluder = nullptr) {
    return validate_frame(L.colorFormat, L.maxGaussians, L.maxWidth, L.maxHeight, count, true, inputMissing, width,
                          height, t.color, t.colorPitch, 1, t.depth, t.depthPitch, pick, occluder);
}

// a styled entry's own refusals (GSM_ERR_INVALID_ARGUMENT), checked after the plain entry's
inline bool style_source_ok(const StyleSource& style, uint32_t stateCount) {
    if (!style.styles || style.styleCount == 0 || style.styleCount > kStyleEntries || !style.states) return false;
    for (uint32_t o = 0; o < stateCount; ++o)
        if (style.states[o].default_state > 255u) return false;
    return true;
}

// ---- the single frame (gsm_global_render and its pick / occluded / styled / orthographic forms) ----
inline gsm_status check_frame(const FrameLimits& L, const gsm_gaussian_input& in, uint32_t width, uint32_t height,
                              const FrameTargets& t, const FrameExtras& extras) {
    const gsm_status st = validate_frame(L, in.gaussian_count, !in.gaussians || !in.harmonics, width, height, t,
                                         extras.pick, extras.occluder);
    if (st != GSM_OK) return st;
    if (extras.style && !style_source_ok(*extras.style, 1)) return GSM_ERR_INVALID_ARGUMENT;
    // (set_tile_rows: a pick frame, an occluded frame, a styled frame and an orthographic frame are whole frames)
    if ((extras.pick || extras.occluder || extras.style || extras.orthographic) && L.rowsRestricted)
        return GSM_ERR_UNSUPPORTED;
    // the projection's tile tests walk contiguous rows; interleaved row sets come from the records path only
    if (L.rowStride != 1) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

// ---- several views of one scene (gsm_global_render_views) ----
struct ViewsLayout {
    uint32_t blocksPerView, tilesPerView;
};
inline ViewsLayout views_layout(uint32_t count, uint32_t width, uint32_t height) {
    return ViewsLayout{blocks_of(count), tiles_of(width, height)};
}
// validate_frame's precedence: count, dimensions, (tiles,) a missing buffer, sizes.  A view's items start on a
// projection-block boundary, and the values keep 30 bits of item.
inline gsm_status check_views(const FrameLimits& L, const gsm_gaussian_input& in, const gsm_camera_params* cameras,
                              uint32_t viewCount, uint32_t width, uint32_t height, const FrameTargets& t,
                              size_t colorStride, size_t depthStride) {
    // (a count above max_gaussians is refused here too: a view's padded items are at least its count)
    if (viewCount == 0 || (uint64_t)viewCount * padded_items(in.gaussian_count) > L.maxGaussians)
        return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!L.sizeOk(width, height)) return GSM_ERR_INVALID_DIMENSIONS;
    if (!batch_tiles_ok((uint64_t)viewCount * tiles_of(width, height), L.tileCount)) return GSM_ERR_INVALID_TILE_COUNT;
    if (!cameras) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    const gsm_status st = validate_frame(L, in.gaussian_count, !in.gaussians || !in.harmonics, width, height, t);
    if (st != GSM_OK) return st;
    // a view's rows fit in its stride, and every view's first row is as aligned as validate_frame asks of the first
    if (colorStride < (size_t)height * t.colorPitch || (colorStride & 3u)) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (t.depth && (depthStride < (size_t)height * t.depthPitch || (depthStride & 1u))) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (L.rowsRestricted) return GSM_ERR_UNSUPPORTED;  // (set_tile_rows)
    return GSM_OK;
}

// ---- views of different scenes and sizes (gsm_global_render_batch, gsm_global_render_frames) ----
// What a frame of renderFrames adds to its view (host memory of the caller, consumed by the call); pixels null:
// the option is not given; styled: states and styles as gsm_global_render_frame takes them for one object.
struct BatchViewOptions {
    PickTarget pick{nullptr, 0};
    OccluderSource occluder{nullptr, 0};
    bool styled = false;
    StyleSource style{nullptr, nullptr, 0};
    bool orthographic = false;  // the frame's flag: this view's projection rule
};
// One view as the batch's rows and its layout read it, whichever array it comes from.
struct BatchViewDesc {
    gsm_gaussian_input input;
    uint32_t width, height;
    FrameTargets targets;
    BatchViewOptions options;
};
// the views of renderBatch (options null: none has any), and of enqueueBatch after renderFrames' copy
struct BatchViewArray {
    const gsm_global_view* views;
    const BatchViewOptions* options;
    bool null() const { return !views; }
    const gsm_gaussian_input& input(uint32_t v) const { return views[v].input; }
    BatchViewOptions optionsAt(uint32_t v) const { return options ? options[v] : BatchViewOptions{}; }
    BatchViewDesc at(uint32_t v) const {
        const gsm_global_view& V = views[v];
        return BatchViewDesc{V.input, V.width, V.height, FrameTargets{V.color, V.color_pitch_bytes, V.depth, V.depth_pitch_bytes},
                             optionsAt(v)};
    }
};
// the frames of renderFrames, read in place once check_frames_front has passed (one object each, none null)
struct BatchFrameArray {
    const gsm_global_frame* frames;
    bool null() const { return !frames; }
    const gsm_gaussian_input& input(uint32_t v) const { return frames[v].objects[0].input; }
    BatchViewOptions optionsAt(uint32_t v) const {
        const gsm_global_frame& F = frames[v];
        BatchViewOptions O;
        O.pick = PickTarget{F.pick_r32u, F.pick_pitch_bytes};  // (a null pointer: the option is not given)
        O.occluder = OccluderSource{F.occluder_r32f, F.occluder_pitch_bytes};
        O.styled = F.states || F.styles;  // (one without the other: the styled row refuses)
        O.style = StyleSource{F.states, F.styles, F.style_count};
        O.orthographic = (F.flags & GSM_FRAME_ORTHOGRAPHIC) != 0;
        return O;
    }
    BatchViewDesc at(uint32_t v) const {
        const gsm_global_frame& F = frames[v];
        return BatchViewDesc{F.objects[0].input, F.width, F.height,
                             FrameTargets{F.color, F.color_pitch_bytes, F.depth_r16f, F.depth_pitch_bytes}, optionsAt(v)};
    }
};

// The rows renderFrames puts in front of the batch's, each over all frames: the first failing row
// decides, within it the lowest frame.  (frame_count == 0 falls through to the batch's first row.)
inline gsm_status check_frames_front(const gsm_global_frame* frames, uint32_t frameCount) {
    if (frameCount >= 1 && !frames) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    for (uint32_t v = 0; v < frameCount; ++v)
        if (frames[v].flags & ~GSM_FRAME_ORTHOGRAPHIC) return GSM_ERR_INVALID_ARGUMENT;
    for (uint32_t v = 0; v < frameCount; ++v)  // (composites inside a batch: out of scope)
        if (frames[v].object_count != 1) return GSM_ERR_UNSUPPORTED;
    for (uint32_t v = 0; v < frameCount; ++v)
        if (!frames[v].objects) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    return GSM_OK;
}

// Every check of a batch, one kind of check after another over all views (the first failing kind decides, within it
// the lowest view): counts, dimensions, tiles, missing buffers, sizes, sh_components, styles, tile rows.  (The counts
// of a NULL array cannot be read: that is the missing buffer.)  Views: BatchViewArray or BatchFrameArray.
template <class Views>
gsm_status check_batch(const FrameLimits& L, const Views& views, uint32_t viewCount) {
    if (viewCount == 0) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (views.null()) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    uint64_t items = 0, allTiles = 0;
    // (gsm_global_render's rule per view: an empty scene is a frame; a single count above max_gaussians is refused
    // by the sum, which cannot wrap: fewer than 2^32 views of at most 2^32 items)
    for (uint32_t v = 0; v < viewCount; ++v) items += padded_items(views.input(v).gaussian_count);
    if (items > L.maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;  // (the values keep 30 bits of item)
    for (uint32_t v = 0; v < viewCount; ++v) {
        const BatchViewDesc V = views.at(v);
        if (!L.sizeOk(V.width, V.height)) return GSM_ERR_INVALID_DIMENSIONS;
        allTiles += tiles_of(V.width, V.height);
    }
    if (!batch_tiles_ok(allTiles, L.tileCount)) return GSM_ERR_INVALID_TILE_COUNT;
    for (uint32_t v = 0; v < viewCount; ++v) {
        const BatchViewDesc V = views.at(v);
        if (!V.targets.color || (V.input.gaussian_count > 0 && (!V.input.gaussians || !V.input.harmonics)))
            return GSM_ERR_MISSING_REQUIRED_BUFFER;
    }
    for (uint32_t v = 0; v < viewCount; ++v) {  // (everything above passed: what is left of validate_frame is sizes)
        const BatchViewDesc V = views.at(v);
        // (a view's pick target and occluder, where given, join the size row as for gsm_global_render_frame)
        const gsm_status st = validate_frame(L, V.input.gaussian_count, false, V.width, V.height, V.targets,
                                             V.options.pick.pixels ? &V.options.pick : nullptr,
                                             V.options.occluder.pixels ? &V.options.occluder : nullptr);
        if (st != GSM_OK) return st;
    }
    const uint32_t sh = views.input(0).sh_components;
    for (uint32_t v = 1; v < viewCount; ++v)
        if (views.input(v).sh_components != sh) return GSM_ERR_INVALID_ARGUMENT;
    // the styled row, per view; the batch has one style table, so every styled view must give the same one (the
    // six meaningful bytes of every style; pad is ignored)
    bool haveTable = false;
    StyleSource table{nullptr, nullptr, 0};
    for (uint32_t v = 0; v < viewCount; ++v) {
        const BatchViewOptions O = views.optionsAt(v);
        if (!O.styled) continue;
        if (!style_source_ok(O.style, 1)) return GSM_ERR_INVALID_ARGUMENT;
        if (!haveTable) {
            haveTable = true;
            table = O.style;
            continue;
        }
        if (O.style.styleCount != table.styleCount) return GSM_ERR_INVALID_ARGUMENT;
        for (uint32_t i = 0; i < table.styleCount; ++i)
            if (std::memcmp(&O.style.styles[i], &table.styles[i], offsetof(gsm_global_style, pad)) != 0)
                return GSM_ERR_INVALID_ARGUMENT;
    }
    if (L.rowsRestricted) return GSM_ERR_UNSUPPORTED;  // (set_tile_rows)
    return GSM_OK;
}

// Where a view of a batch lies: its blocks and tiles follow the earlier views' (a running cursor: nothing is stored).
struct BatchViewLayout {
    uint32_t blockBase, tileBase;  // its first projection block and tile in the handle's spaces
    uint32_t tilesX, tilesY;       // its own grid
    uint32_t vec;                  // kBlendWide where its targets are aligned for the wide stores (BatchTarget::vec)
    uint32_t align;                // kBlendPick8 | kBlendOcc8 of its options (BatchExtras::align)
    uint32_t itemBase;             // its first item: 256 * blockBase
};
struct BatchLayout {
    static constexpr uint32_t kNoTable = 0xFFFFFFFFu;
    uint32_t views = 0, blocks = 0, tiles = 0, countSum = 0;  // the totals so far
    bool anyPick = false, anyOccluder = false, anyOrtho = false;
    uint32_t tableView = kNoTable;  // the first styled view: its table is the batch's
    BatchViewLayout place(const BatchViewDesc& V) {
        const BatchViewOptions& O = V.options;
        const FrameTargets& t = V.targets;
        BatchViewLayout l;
        l.blockBase = blocks;
        l.tileBase = tiles;
        l.tilesX = tiles_x(V.width);
        l.tilesY = tiles_y(V.height);
        // plan_blend's rules for a single frame, on this view's own pointers and pitches; the bytes are the same
        // either way
        l.vec = blend_wide((uintptr_t)t.color, t.colorPitch, (uintptr_t)t.depth, t.depthPitch) ? (uint32_t)kBlendWide : 0u;
        l.align = (uint32_t)(blend_pick8((uintptr_t)O.pick.pixels, O.pick.pitch) |
                             blend_occ8((uintptr_t)O.occluder.pixels, O.occluder.pitch));
        l.itemBase = blocks * (uint32_t)kProjectBlock;
        anyPick = anyPick || O.pick.pixels;
        anyOccluder = anyOccluder || O.occluder.pixels;
        anyOrtho = anyOrtho || O.orthographic;
        if (O.styled && tableView == kNoTable) tableView = views;
        views += 1;
        blocks += blocks_of(V.input.gaussian_count);
        tiles += l.tilesX * l.tilesY;
        countSum += V.input.gaussian_count;
        return l;
    }
};

// ---- several posed scenes in one frame (gsm_global_render_composite and its forms) ----
// Every check, one kind after another over all objects (the first failing kind decides, within it the lowest
// object): counts, dimensions, missing buffers, sizes, sh_components, styles, tile rows.
inline gsm_status check_compose(const FrameLimits& L, const gsm_global_object* objects, uint32_t objectCount,
                                uint32_t width, uint32_t height, const FrameTargets& t, const FrameExtras& extras) {
    const PickTarget* pick = extras.pick;
    const OccluderSource* occluder = extras.occluder;
    if (objectCount == 0) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!objects) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (objectCount > kBatchIndexMax) return GSM_ERR_INVALID_GAUSSIAN_COUNT;  // (a block's entry is a 16-bit index)
    uint64_t items = 0;
    uint32_t countSum = 0;
    // (a single count above max_gaussians is refused by the sum: an object's padded items are at least its count)
    for (uint32_t o = 0; o < objectCount; ++o) items += padded_items(objects[o].input.gaussian_count);
    if (items > L.maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;  // (the values keep 30 bits of item)
    if (!L.sizeOk(width, height)) return GSM_ERR_INVALID_DIMENSIONS;
    // the missing-buffer row: every object's input here; the colour target and a pick target or occluder without
    // pixels in validate_frame below, whose earlier rows have passed
    for (uint32_t o = 0; o < objectCount; ++o) {
        const gsm_gaussian_input& in = objects[o].input;
        if (in.gaussian_count > 0 && (!in.gaussians || !in.harmonics)) return GSM_ERR_MISSING_REQUIRED_BUFFER;
        countSum += in.gaussian_count;  // (<= items <= max_gaussians)
    }
    const gsm_status st = validate_frame(L, countSum, false, width, height, t, pick, occluder);
    if (st != GSM_OK) return st;
    for (uint32_t o = 1; o < objectCount; ++o)
        if (objects[o].input.sh_components != objects[0].input.sh_components) return GSM_ERR_INVALID_ARGUMENT;
    if (extras.style && !style_source_ok(*extras.style, objectCount)) return GSM_ERR_INVALID_ARGUMENT;
    if (L.rowsRestricted) return GSM_ERR_UNSUPPORTED;  // (set_tile_rows)
    return GSM_OK;
}

// The entries of a composite: an object without gaussians takes no block and no entry (a running cursor).
struct ComposeEntry {
    uint32_t object;     // the object's index in the call
    uint32_t blockBase;  // its first projection block; its items start at 256 * blockBase
};
struct ComposeLayout {
    uint32_t objects = 0, entries = 0, blocks = 0, countSum = 0;  // the totals so far
    // the next object of the call: whether it takes an entry, and which
    bool place(uint32_t count, ComposeEntry* e) {
        const uint32_t o = objects++;
        if (count == 0) return false;
        *e = ComposeEntry{o, blocks};
        entries += 1;
        blocks += blocks_of(count);
        countSum += count;
        return true;
    }
};

// ---- the selects ----
// gsm_global_select_mask.  (The count of a NULL input cannot be read: that is the missing buffer, before every other
// check.)
inline gsm_status check_select_mask(const FrameLimits& L, const gsm_gaussian_input* in, const gsm_camera_params* camera,
                                    uint32_t width, uint32_t height, const void* mask, size_t maskPitch,
                                    const uint8_t* state, const gsm_global_style* styles, uint32_t styleCount,
                                    const uint32_t* matched) {
    if (!in) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (in->gaussian_count > L.maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!L.sizeOk(width, height)) return GSM_ERR_INVALID_DIMENSIONS;
    if (!camera || !mask || (in->gaussian_count > 0 && (!in->gaussians || !state))) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (maskPitch < width || (((uintptr_t)matched) & 3u)) return GSM_ERR_INVALID_BUFFER_SIZE;
    if (styles ? (styleCount == 0 || styleCount > kStyleEntries) : styleCount != 0) return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}
// What gsm_global_select_pick and gsm_global_select_pick_ids share: the count, the size (frameWidth x frameHeight:
// the pick frame the image must be of; select_pick_ids has none and passes the image's own), the buffers, and the
// pitches and alignment of the image, the mask and `matched`.
inline gsm_status check_select_pick(const FrameLimits& L, uint32_t gaussianCount, uint32_t width, uint32_t height,
                                    uint32_t frameWidth, uint32_t frameHeight, const void* pick, size_t pickPitch,
                                    const void* mask, size_t maskPitch, const uint8_t* state, const uint32_t* matched) {
    if (gaussianCount > L.maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!L.sizeOk(width, height) || width != frameWidth || height != frameHeight) return GSM_ERR_INVALID_DIMENSIONS;
    if (!pick || (gaussianCount > 0 && !state)) return GSM_ERR_MISSING_REQUIRED_BUFFER;
    if (pickPitch < (size_t)width * 4 || (pickPitch & 3u) || (((uintptr_t)pick) & 3u) || (mask && maskPitch < width) ||
        (((uintptr_t)matched) & 3u))
        return GSM_ERR_INVALID_BUFFER_SIZE;
    return GSM_OK;
}

// ---- the partition of a multi-GPU frame: the argument rows of preparePartition ----
inline gsm_status check_partition(const FrameLimits& L, const gsm_gaussian_input& in, uint32_t width, uint32_t height,
                                  uint32_t first, uint32_t count, const uint32_t* slabRows, uint32_t numSlabs,
                                  bool needSend, const void* send, const uint32_t* sendCounts, bool interleave) {
    if ((uint64_t)first + count > in.gaussian_count || count > L.maxGaussians) return GSM_ERR_INVALID_GAUSSIAN_COUNT;
    if (!L.sizeOk(width, height)) return GSM_ERR_INVALID_DIMENSIONS;
    if (!slabRows || numSlabs == 0 || numSlabs > kMaxSlabs) return GSM_ERR_INVALID_ARGUMENT;
    if (!sendCounts || (count > 0 && ((needSend && !send) || !in.gaussians || !in.harmonics)))
        return GSM_ERR_MISSING_REQUIRED_BUFFER;
    for (uint32_t i = 0; i <= numSlabs; ++i)  // slab boundaries within the handle's rows, ascending unless interleaved
        if (slabRows[i] > L.tilesY || (!interleave && i > 0 && slabRows[i] < slabRows[i - 1]))
            return GSM_ERR_INVALID_ARGUMENT;
    return GSM_OK;
}

}  // namespace gsm

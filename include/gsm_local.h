/*
 * gsm_local.h -- C ABI of the LocalRenderer frame (libgsm_amd.so).
 *
 * Drop-in for the reference's LocalRenderer.render (Sources/Renderer/LocalRenderer/LocalRenderer.swift:83-257,
 * kernels in LocalShaders.metal), the compute renderer without a global sort:
 *   - the projection writes the 32-byte ProjectedGaussian (BridgingTypes.h:106-114) with every field
 *     rounded to fp16; screen positions use ndcToScreenCentered; culls in the order scale, near plane
 *     (clip w), far plane, opacity < 0.005, radius, total ink (2.0), invalid tile rect
 *     (localProjectStore, LocalShaders.metal:53-184);
 *   - the visible records are compacted in gaussian order (localCompact, :201-214);
 *   - every 16x16 tile owns 2048 slots; a gaussian is entered into each tile of its rect that passes
 *     intersectsTile on the fp16 record (localScatterSimd16, :573-667);
 *   - each tile is sorted on its own by the 16-bit depth key bits(half(clip w)) ^ 0x8000
 *     (localPerTileSort16, :362-437);
 *   - one group per tile blends 4x2 pixels per thread in fp16, depth = the fp32 depth of the first
 *     entry with alpha > 0.1 (localRender16, :440-571); tiles without entries hold the clear value,
 *     colour (0, 0, 0, 0) and depth 0 (localClearTextures, :27-39).
 * Declared choices where the reference leaves the result to chance:
 *   - ties in the depth key are ordered by the compacted index (the reference: by the slot an atomic
 *     race handed out);
 *   - a tile with more than 2048 passing gaussians keeps some 2048 of them (which is unspecified), sorts
 *     and walks exactly 2048, and the counters report overflow = 1 and the largest count (the reference
 *     walks `count` entries past the tile's slots and never sets its overflow flag);
 *   - invalid calls return an error where the reference returns silently (:139-141).
 * renderStereo is a fatalError in the reference (:108-123); there is no stereo entry.
 * Same conventions as gsm_renderer.h: device pointers, the stream as void*, enqueue-only.
 */
#ifndef GSM_LOCAL_H
#define GSM_LOCAL_H

#include "gsm_renderer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsm_local gsm_local;

#define GSM_LOCAL_TILE 16u           /* LocalRenderer.tileWidth / tileHeight */
#define GSM_LOCAL_MAX_PER_TILE 2048u /* LocalRenderer.maxPerTile */

/* ProjectedGaussian (BridgingTypes.h:106-114): fp16 fields as raw bits. */
typedef struct {
    uint16_t posX, posY;
    uint16_t conicA, conicB, conicC, depth;
    uint16_t colorR, colorG;
    uint16_t colorB, opacity;
    uint16_t minTile[2]; /* inclusive */
    uint16_t maxTile[2]; /* exclusive */
    uint16_t obbExtentX, obbExtentY;
} gsm_local_projected;

/* LocalRenderer.init(device:config:) (LocalRenderer.swift:40-81).  Everything is allocated here: two
 * max_gaussians record buffers and tiles x 2048 slots of keys and indices for the 16x16 tile grid of
 * max_width x max_height.  max_gaussians > 30M -> GSM_ERR_INVALID_GAUSSIAN_COUNT; a grid of more than
 * 65535 tiles (ProjectedGaussian holds tile coordinates in 16 bits; 512 MiB of slots) ->
 * GSM_ERR_INVALID_TILE_COUNT; GSM_ERR_FAILED_TO_ALLOCATE_BUFFER when the device has no room. */
gsm_status gsm_local_create(const gsm_renderer_config *config, int hip_device, gsm_local **out);
void gsm_local_destroy(gsm_local *renderer);

/* render(commandBuffer:colorTexture:depthTexture:input:camera:width:height:) (LocalRenderer.swift:83-106,
 * 125-257).  Enqueue-only on `stream`.
 * color: width x height pixels of config.color_format, rows color_pitch_bytes apart (4-byte aligned).
 * depth_r16f: width x height fp16, rows depth_pitch_bytes apart (2-byte aligned), or NULL: then no depth
 * is written.
 * gaussian_count 0 or above max_gaussians -> GSM_ERR_INVALID_GAUSSIAN_COUNT; width or height 0 or above
 * the configured maximum -> GSM_ERR_INVALID_DIMENSIONS; null colour or input buffers ->
 * GSM_ERR_MISSING_REQUIRED_BUFFER; a pitch below a row or misaligned -> GSM_ERR_INVALID_BUFFER_SIZE. */
gsm_status gsm_local_render(gsm_local *renderer, void *stream, const gsm_gaussian_input *input,
                            const gsm_camera_params *camera, uint32_t width, uint32_t height,
                            void *color, size_t color_pitch_bytes,
                            void *depth_r16f, size_t depth_pitch_bytes);

/* Counters of the last frame (after a stream sync). */
typedef struct {
    uint32_t gaussian_count;
    uint32_t visible;        /* records after compaction */
    uint32_t tiles_x, tiles_y, tile_count;
    uint32_t active_tiles;   /* tiles with a nonzero count */
    uint32_t total_entries;  /* sum of min(count, max_per_tile) */
    uint32_t max_tile_count; /* the largest unclamped count */
    uint32_t max_per_tile;   /* 2048 */
    uint32_t overflow;       /* 1 when max_tile_count > max_per_tile */
} gsm_local_counters;

typedef enum {
    GSM_LOCAL_BUF_PROJECTED = 0,   /* gsm_local_projected[visible], compacted [compactedGaussians] */
    GSM_LOCAL_BUF_TILE_COUNTS = 1, /* uint32[tile_count], unclamped [tileCounts] */
    GSM_LOCAL_BUF_TILE_LISTS = 2   /* uint32[tile_count][2048] compacted indices in blend order,
                                      defined up to min(count, 2048) */
} gsm_local_buffer;

gsm_status gsm_local_debug_counters(gsm_local *renderer, gsm_local_counters *out);
/* Copies min(bytes, size) bytes; *needed (nullable) receives the full size. */
gsm_status gsm_local_debug_copy(gsm_local *renderer, int which, void *host_dst, size_t bytes, size_t *needed);

/* The per-tile sort stage alone (LocalSortEncoder.encode16), on caller device buffers: tile t owns the
 * slots [t * max_per_tile, (t + 1) * max_per_tile) of keys16 (uint16), indices (uint32) and
 * out_local_idx (uint16); counts is uint32[tile_count].  out_local_idx receives, for each tile, the slots
 * of its first min(count, max_per_tile) entries ascending by (key, index, slot).  max_per_tile in
 * [1, 2048], else GSM_ERR_INVALID_ARGUMENT.  Enqueue-only; needs no renderer. */
gsm_status gsm_local_debug_sort_tiles(void *stream, const void *keys16, const void *indices, const void *counts,
                                      uint32_t tile_count, uint32_t max_per_tile, void *out_local_idx);

/* nonzero: bracket every stage with HIP events. */
gsm_status gsm_local_set_profiling(gsm_local *renderer, int enable);
typedef enum {
    GSM_LOCAL_STAGE_PROJECT = 0, /* clear, projection, compaction */
    GSM_LOCAL_STAGE_SCATTER = 1,
    GSM_LOCAL_STAGE_SORT = 2,
    GSM_LOCAL_STAGE_BLEND = 3,   /* clear of the targets + blend */
    GSM_LOCAL_STAGE_COUNT = 4
} gsm_local_stage;
/* Average milliseconds per stage over the profiled frames (after stream sync). */
gsm_status gsm_local_stage_times(gsm_local *renderer, float *ms, int n);
/* LocalRenderer.lastGPUTime: seconds of the last profiled frame. */
gsm_status gsm_local_last_gpu_time(gsm_local *renderer, double *seconds);

#ifdef __cplusplus
}
#endif
#endif

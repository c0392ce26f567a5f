/*
 * gsm_depthfirst.h -- C ABI of the DepthFirst stereo side-by-side path (libgsm_amd.so).
 *
 * Drop-in for the reference's DepthFirstRenderer.renderStereo(target: .sideBySide)
 * (Sources/Renderer/DepthFirstRenderer/DepthFirstRenderer.swift:205-223, 469-512, 595-831;
 * SURVEY.md 8(f) rank 1).  Its semantics differ from running the Global path once per eye:
 *   - one projection pass projects every gaussian into both eyes; SH colour is evaluated once,
 *     from the midpoint of the two camera centres (DepthFirstShaders.metal:419-424);
 *   - screen positions use ndcToScreen without the half-pixel shift (:291);
 *   - a gaussian is binned into the union of its two eyes' 16x16-tile rects (:426-442),
 *     depth-sorted first by the centre depth as a 32-bit float key (:33-37, :496), then the
 *     per-tile instances are stably sorted by tile (DepthFirstRenderer.swift:683-768);
 *   - one 64-lane wave per 16x16 tile blends both eyes, 2x2 pixels per lane with a joint
 *     left/right saturation break and the r^2 <= 9 cutoff (DepthFirstShaders.metal:1825-1982);
 *   - the two eyes land side by side in the target through the copy pass
 *     (DepthFirstStereoCopyEncoder.swift:29-99), which flips rows (target row y of an eye is
 *     row height-1-y of its slice; DESIGN.md "DepthFirst stereo").
 * Same conventions as gsm_renderer.h: device pointers, the stream as void*, enqueue-only.
 */
#ifndef GSM_DEPTHFIRST_H
#define GSM_DEPTHFIRST_H

#include "gsm_renderer.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct gsm_depthfirst gsm_depthfirst;

/* DepthFirstRenderer.init(device:config:depthSortKeyPrecision:tileIdPrecision:)
 * (DepthFirstRenderer.swift:45-101) with its defaults: 32-bit depth keys, 16-bit tile ids
 * (gsm_depthfirst_create_with_options below sets the other two).
 * Errors as GlobalRenderer.init: max_gaussians > 30M -> GSM_ERR_INVALID_GAUSSIAN_COUNT
 * (:51-56); a 16x16 tile grid of max_width x max_height over 65535 tiles (16-bit tile ids,
 * 0xFFFF is the tile sort's sentinel) -> GSM_ERR_INVALID_TILE_COUNT.  Scratch is allocated
 * here: max_gaussians records and 4 * max_gaussians instances (DepthFirstResources.swift:399). */
gsm_status gsm_depthfirst_create(const gsm_renderer_config *config, int hip_device, gsm_depthfirst **out);
void gsm_depthfirst_destroy(gsm_depthfirst *renderer);

/* The two other constructor arguments of DepthFirstRenderer.init (DepthFirstRenderer.swift:45-50),
 * fixed for the life of the handle and applied to both of its frames (mono and stereo).
 *   depth_key_bits 16 (depthSortKeyPrecision: .bits16): the compaction replaces the 32-bit key by
 *     uint(bits(half(sortable_uint_to_float(key))) ^ 0x8000) (visibilityScatterCompactKernel,
 *     DepthFirstShaders.metal:589-621; fp32 -> fp16 rounds to nearest even, depths above 65504
 *     become +inf) and the depth sort is a stable sort of those 16 bits (2 passes,
 *     DepthRadixSortEncoder.swift:13-24).  Gaussians whose depths share an fp16 value keep their
 *     ascending ids, so the blend order differs from the 32-bit order there.
 *   tile_id_bits 32 (tileIdPrecision: .bits32): the instance expansion writes the whole tile id and
 *     the tile sort covers ceil(log2(tile count)) bits, so the 16x16 grid of max_width x max_height
 *     may hold up to GSM_DF_MAX_TILES_32 tiles (one 9..11-bit pass and one 8-bit pass: 19 bits);
 *     above it, or with more than GSM_DF_MAX_TILES_AXIS tiles along one axis (tile rects are 16-bit
 *     signed), -> GSM_ERR_INVALID_TILE_COUNT.  Up to 65,535 tiles the frame is byte for byte the
 *     16-bit handle's.  With tile_id_bits 16 the limit stays 65,535 tiles.
 * struct_bytes must be sizeof(gsm_depthfirst_options), the bit counts 16 or 32 and reserved 0,
 * else GSM_ERR_INVALID_ARGUMENT.  A NULL options pointer means the defaults. */
#define GSM_DF_MAX_TILES_32 524288u
#define GSM_DF_MAX_TILES_AXIS 32767u
typedef struct {
    uint32_t struct_bytes;    /* sizeof(gsm_depthfirst_options) == 16 */
    uint32_t depth_key_bits;  /* 16 or 32; default 32 */
    uint32_t tile_id_bits;    /* 16 or 32; default 16 */
    uint32_t reserved;        /* must be 0 */
} gsm_depthfirst_options;
void gsm_depthfirst_default_options(gsm_depthfirst_options *out);
gsm_status gsm_depthfirst_create_with_options(const gsm_renderer_config *config, int hip_device,
                                              const gsm_depthfirst_options *options, gsm_depthfirst **out);
gsm_status gsm_depthfirst_get_options(gsm_depthfirst *renderer, gsm_depthfirst_options *out);

/* renderStereo(commandBuffer:target:.sideBySide(colorTexture:depthTexture:)input:camera:width:height:)
 * (DepthFirstRenderer.swift:205-223, 469-512).  width/height are per eye (<= config max_width /
 * max_height); the colour target is 2 * width columns of config.color_format by height rows of
 * color_pitch_bytes: left eye in columns [0, width), right eye in [width, 2 * width).  The
 * reference ignores the depth texture of this target (:472), so there is none here.
 * near/far planes come from the left camera (makeStereoCameraUniforms, :583-584).
 * scene_transform: NULL for the identity of the side-by-side path, or 16 floats column-major
 * (StereoConfiguration.sceneTransform, GaussianRendererProtocol.swift:100-116).
 * Returns an error where the reference silently skips the frame (:478, :607). */
gsm_status gsm_depthfirst_render_stereo_sbs(gsm_depthfirst *renderer, void *stream,
                                            const gsm_gaussian_input *input,
                                            const gsm_camera_params *left, const gsm_camera_params *right,
                                            const float *scene_transform, uint32_t width, uint32_t height,
                                            void *color, size_t color_pitch_bytes);

/* render(commandBuffer:colorTexture:depthTexture:input:camera:width:height:)
 * (DepthFirstRenderer.swift:166-203, 237-465): the mono frame, the only DepthFirst path that writes a
 * depth target.  Enqueue-only on `stream`, on the same handle as the stereo entry; either may be
 * called on any frame.  It is not "stereo with two equal eyes":
 *   - the projection writes the 16-byte GaussianRenderData (depthFirstProjectCullKernel,
 *     DepthFirstShaders.metal:46-219): ndcToScreen without the half-pixel shift, far-plane cull,
 *     SH colour from camera->position;
 *   - a tile of the gaussian's 16x16-tile rect counts only when minQuadRect(tile) <=
 *     computeD2Cutoff(opacity, 0.005) on the quantised record (:166-216, GaussianShared.h:525-593),
 *     and the instance expansion writes only those tiles (:642-716);
 *   - one wave per 16x16 tile blends 2x2 pixels per lane with the Global blend's per-entry
 *     arithmetic, no r^2 cutoff, and accumulates depth (:1703-1811); no row flip;
 *   - tiles without instances get the clear value: colour (0, 0, 0, 1), depth 0 (:2020-2034).
 * Binning parameters are the reference's (GlobalRenderer.swift:54-69): alpha threshold 0.005,
 * total-ink threshold 2.0, 16x16 tiles; capacity 4 * max_gaussians instances, instances past it are
 * dropped from the tail of the depth order and `overflow` is set, as in the stereo frame.
 * color: width x height pixels of config.color_format, rows color_pitch_bytes apart (4-byte
 * aligned).  depth_r16f: width x height fp16, rows depth_pitch_bytes apart (2-byte aligned), or
 * NULL: then no depth is written.
 * Returns an error where the reference silently returns (:249): gaussian_count 0 or above
 * max_gaussians -> GSM_ERR_INVALID_GAUSSIAN_COUNT; width or height 0 or above the configured maximum
 * -> GSM_ERR_INVALID_DIMENSIONS; null colour (or input buffers) -> GSM_ERR_MISSING_REQUIRED_BUFFER;
 * a pitch below a row or misaligned -> GSM_ERR_INVALID_BUFFER_SIZE. */
gsm_status gsm_depthfirst_render(gsm_depthfirst *renderer, void *stream,
                                 const gsm_gaussian_input *input, const gsm_camera_params *camera,
                                 uint32_t width, uint32_t height,
                                 void *color, size_t color_pitch_bytes,
                                 void *depth_r16f, size_t depth_pitch_bytes);

/* DepthFirstHeader (BridgingTypes.h:209-219) + frame counters of the last frame, whichever kind. */
typedef struct {
    uint32_t gaussian_count;
    uint32_t visible;         /* visibleCount after compaction */
    uint32_t total_instances; /* after the clamp to max_instances */
    uint32_t max_instances;   /* 4 * max_gaussians */
    uint32_t overflow;        /* 1 when the clamp fired (DepthFirstShaders.metal:2191-2194) */
    uint32_t tiles_x, tiles_y, tile_count;
} gsm_depthfirst_counters;

/* Buffers of the last frame that can be copied back (reference resource in brackets).  The
 * comments describe a stereo frame.  After a mono frame (gsm_depthfirst_render):
 *   RENDER_DATA is GaussianRenderData[count], 16 B (BridgingTypes.h:75-84); culled entries undefined;
 *   BOUNDS is the mono tile rect, (0, -1, 0, -1) for a gaussian with no passing tile;
 *   TOUCHED is the number of tiles of that rect that passed the per-tile test;
 *   DEPTH_KEYS is float_to_sortable_uint(clip w); the reference leaves preDepthKeys unwritten on three
 *     of its early returns (DepthFirstShaders.metal:111-122, :133-137) -- every gaussian without a
 *     passing tile has 0xFFFFFFFF here;
 *   the others are as for a stereo frame. */
typedef enum {
    GSM_DF_BUF_RENDER_DATA = 0,      /* StereoTiledRenderData[count], 32 B [renderData]; culled entries undefined */
    GSM_DF_BUF_BOUNDS = 1,           /* int32[count][4] union tile rect [bounds] */
    GSM_DF_BUF_TOUCHED = 2,          /* uint32[count] tiles of the union rect [nTouchedTiles] */
    GSM_DF_BUF_DEPTH_KEYS = 3,       /* uint32[count] float_to_sortable_uint(centre depth) [preDepthKeys] */
    GSM_DF_BUF_DEPTH_ORDER = 4,      /* int32[visible] ids after the depth sort [primitiveIndices] */
    GSM_DF_BUF_INSTANCE_TILES = 5,   /* uint32[total_instances] sorted tile ids [instanceTileIds] */
    GSM_DF_BUF_INSTANCE_GAUSSIANS = 6, /* int32[total_instances] [instanceGaussianIndices] */
    GSM_DF_BUF_HEADERS = 7,          /* GaussianHeader[tile_count] {offset, count} [tileHeaders] */
    GSM_DF_BUF_BLEND_STATS = 8,      /* uint64[4] (profiling bit 1): list entries the blend walked, of
                                        which had the eye's mean, of which blended; list entries */
    GSM_DF_BUF_SORTED_DEPTH_KEYS = 9 /* uint32[visible] the compacted keys as the depth sort left them
                                        [depthKeys]: the 32-bit keys, or with depth_key_bits 16 the
                                        quantised keys in the low 16 bits; DEPTH_KEYS stays the 32-bit
                                        preDepthKeys in every mode (the compaction quantises) */
} gsm_depthfirst_buffer;

gsm_status gsm_depthfirst_debug_counters(gsm_depthfirst *renderer, gsm_depthfirst_counters *out);
/* Copies min(bytes, size) bytes; *needed (nullable) receives the full size. */
gsm_status gsm_depthfirst_debug_copy(gsm_depthfirst *renderer, int which, void *host_dst, size_t bytes,
                                     size_t *needed);
/* bit 0: bracket every stage with HIP events (GSM_DF_STAGE_*); bit 1: count the blend's walk
 * (GSM_DF_BUF_BLEND_STATS); bit 3: only the blend (two events per frame, for timing the blend
 * inside a timed loop); bits 8-15 with bit 3: a period P > 1 brackets every P-th frame only. */
gsm_status gsm_depthfirst_set_profiling(gsm_depthfirst *renderer, int enable);
typedef enum {
    GSM_DF_STAGE_PROJECT = 0, /* project both eyes + visibility compaction */
    GSM_DF_STAGE_DEPTH_SORT = 1,
    GSM_DF_STAGE_INSTANCES = 2, /* ordered counts, scan, instance expansion */
    GSM_DF_STAGE_TILE_SORT = 3, /* stable tile sort + tile ranges */
    GSM_DF_STAGE_BLEND = 4,     /* both eyes, written side by side into the target */
    GSM_DF_STAGE_COUNT = 5
} gsm_depthfirst_stage;
/* Average milliseconds per stage over the profiled frames (after stream sync). */
gsm_status gsm_depthfirst_stage_times(gsm_depthfirst *renderer, float *ms, int n);
/* DepthFirstRenderer.lastGPUTime (DepthFirstRenderer.swift:43): seconds of the last profiled frame. */
gsm_status gsm_depthfirst_last_gpu_time(gsm_depthfirst *renderer, double *seconds);

#ifdef __cplusplus
}
#endif
#endif

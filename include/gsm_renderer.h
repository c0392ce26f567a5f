/*
 * gsm_renderer.h -- C ABI of the MI355X-native GlobalRenderer (libgsm_amd.so).
 *
 * Drop-in boundary for the reference's GlobalRenderer operator surface
 * (LuckyIYI/gsm-renderer, Swift + Metal).  Each declaration cites the reference
 * interface it replaces (paths relative to the reference repository root).
 * Plain pointers and sizes only: device buffers are HIP device pointers, the
 * stream is a hipStream_t passed as void*.  No torch / HIP types appear here.
 *
 * Threading: one in-flight frame per handle (the reference's GlobalRenderer owns
 * a single scratch set, GlobalRenderer.swift:72,94); handles are independent and
 * each is bound to one HIP device.
 */
#ifndef GSM_RENDERER_H
#define GSM_RENDERER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GSM_ABI_VERSION 1

/* RendererError (Sources/Renderer/Shared/GaussianRendererProtocol.swift:274-292). */
typedef enum {
    GSM_OK = 0,
    GSM_ERR_DEVICE_NOT_AVAILABLE = 1,        /* .deviceNotAvailable */
    GSM_ERR_FAILED_TO_CREATE_LIBRARY = 2,    /* .failedToCreateLibrary */
    GSM_ERR_FAILED_TO_CREATE_PIPELINE = 3,   /* .failedToCreatePipeline */
    GSM_ERR_FAILED_TO_ALLOCATE_BUFFER = 4,   /* .failedToAllocateBuffer */
    GSM_ERR_FAILED_TO_ALLOCATE_TEXTURE = 5,  /* .failedToAllocateTexture */
    GSM_ERR_INVALID_GAUSSIAN_COUNT = 6,      /* .invalidGaussianCount */
    GSM_ERR_INVALID_DIMENSIONS = 7,          /* .invalidDimensions */
    GSM_ERR_INVALID_BUFFER_SIZE = 8,         /* .invalidBufferSize */
    GSM_ERR_INVALID_TILE_COUNT = 9,          /* .invalidTileCount */
    GSM_ERR_INVALID_ASSIGNMENT_CAPACITY = 10,/* .invalidAssignmentCapacity */
    GSM_ERR_RENDER_FAILED = 11,              /* .renderFailed */
    GSM_ERR_ENCODER_CREATION_FAILED = 12,    /* .encoderCreationFailed */
    GSM_ERR_MISSING_REQUIRED_BUFFER = 13,    /* .missingRequiredBuffer */
    GSM_ERR_INVALID_ARGUMENT = 14,           /* null handle / pointer (no Swift analogue) */
    GSM_ERR_UNSUPPORTED = 15,                /* renderStereo on Global: fatalError in the reference */
    GSM_ERR_PHASE_ORDER = 16                 /* gsm_multigpu_render_phase out of order (gsm_multigpu.h) */
} gsm_status;

/* RenderPrecision (GaussianRendererProtocol.swift:4-7). */
typedef enum { GSM_PRECISION_FLOAT32 = 0, GSM_PRECISION_FLOAT16 = 1 } gsm_precision;
/* RendererConfig.GaussianColorSpace (GaussianRendererProtocol.swift:196-201). */
typedef enum { GSM_COLOR_SPACE_LINEAR = 0, GSM_COLOR_SPACE_SRGB = 1 } gsm_color_space;

/* Pixel format of the colour target (RendererConfig.colorFormat, GaussianRendererProtocol.swift:207;
 * the reference's Global path writes half4 into whatever texture it is given and Metal converts
 * on the write, GlobalShaders.metal:1155-1186).  With raw device pointers the format of the
 * target is declared here.  Conversion of the blended fp16 value c (alpha = 1 - T):
 *   RGBA16F: as is (8 B/px);  RGBA32F: exact widening (16 B/px);
 *   *8_UNORM: u8 = RTNE(clamp(c, 0, 1) * 255), clamp by IEEE maxNum/minNum (NaN -> 0) (4 B/px);
 *   *8_UNORM_SRGB: the same after the linear->sRGB encode of R, G, B:
 *     c <= 0.0031308 ? 12.92 c : 1.055 powr(c, 1 / 2.4) - 0.055 (fp32, powr of the numeric contract).
 * BGRA formats store B, G, R, A.  The Metal rounding of unorm / sRGB writes is not specified
 * to the bit: parity for the 8-bit formats is against this definition. */
typedef enum {
    GSM_COLOR_FORMAT_RGBA16F = 0,
    GSM_COLOR_FORMAT_RGBA32F = 1,
    GSM_COLOR_FORMAT_RGBA8_UNORM = 2,
    GSM_COLOR_FORMAT_RGBA8_UNORM_SRGB = 3,
    GSM_COLOR_FORMAT_BGRA8_UNORM = 4,
    GSM_COLOR_FORMAT_BGRA8_UNORM_SRGB = 5 /* the reference's RendererConfig default (.bgra8Unorm_srgb) */
} gsm_color_format;

/* RendererConfig (GaussianRendererProtocol.swift:195-228).  back_to_front is accepted and
 * ignored, as in the reference Global path. */
typedef struct {
    uint32_t max_gaussians;        /* default 6_000_000, <= 30_000_000 (GlobalRenderer.swift:73) */
    uint32_t max_width;            /* default 1920 */
    uint32_t max_height;           /* default 1080 */
    uint32_t precision;            /* gsm_precision, default FLOAT16 */
    uint32_t color_format;         /* gsm_color_format of the colour target, default RGBA16F */
    uint32_t gaussian_color_space; /* gsm_color_space, default SRGB */
    uint32_t back_to_front;        /* ignored */
} gsm_renderer_config;

/* GaussianInput (GaussianRendererProtocol.swift:9-26).  Device pointers owned by
 * the caller; they must stay valid until the stream work of the frame is done.
 * gaussians: PackedWorldGaussian (48 B) when precision == FLOAT32, else
 * PackedWorldGaussianHalf (32 B) (BridgingTypes.h:57-73).  harmonics: planar
 * per-gaussian SH [R0..Rk-1, G0.., B0..], float (FLOAT32) or half (FLOAT16). */
typedef struct {
    const void *gaussians;
    const void *harmonics;
    uint32_t gaussian_count;
    uint32_t sh_components;
} gsm_gaussian_input;

/* CameraParams (GaussianRendererProtocol.swift:28-54).  Matrices are column-major
 * (simd_float4x4 memory layout).  focal_x/focal_y are ignored by the Global path
 * (focal comes from the projection matrix, GaussianShared.h:353-355). */
typedef struct {
    float view[16];
    float proj[16];
    float position[3];
    float focal_x;
    float focal_y;
    float near_plane; /* default 0.1 */
    float far_plane;  /* default 10.0 */
} gsm_camera_params;

typedef struct gsm_renderer gsm_renderer;

/* RendererConfig() defaults (GaussianRendererProtocol.swift:211-219). */
void gsm_renderer_config_default(gsm_renderer_config *config);
/* CameraParams.init defaults near = 0.1, far = 10 (GaussianRendererProtocol.swift:37-45). */
void gsm_camera_params_init(gsm_camera_params *camera, const float view[16], const float proj[16],
                            const float position[3], float focal_x, float focal_y);

/* GlobalRenderer.init(device:config:) (GlobalRenderer.swift:110-193).  Allocates
 * every scratch buffer up front (4 * max_gaussians assignment capacity,
 * GlobalResources.swift:79).  hip_device < 0 selects the current device. */
gsm_status gsm_global_create(const gsm_renderer_config *config, int hip_device, gsm_renderer **out);
void gsm_global_destroy(gsm_renderer *renderer);

/* GlobalRenderer.render(commandBuffer:colorTexture:depthTexture:input:camera:width:height:)
 * (GlobalRenderer.swift:201-238; protocol GaussianRendererProtocol.swift:248-256).
 * Enqueue-only on `stream` (the analogue of encoding into the caller's command
 * buffer; the caller synchronises).  color: config.color_format (rgba16Float by default),
 * height rows of color_pitch bytes; depth: r16Float or NULL (the reference then renders into
 * its own internal depth texture, GlobalRenderer.swift:350).  Returns an error
 * where the reference silently skips the frame (GlobalRenderer.swift:295-299). */
gsm_status gsm_global_render(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                             const gsm_camera_params *camera, uint32_t width, uint32_t height,
                             void *color_rgba16f, size_t color_pitch_bytes, void *depth_r16f,
                             size_t depth_pitch_bytes);

/* Several views of one scene in one frame (no reference analogue): view_count cameras
 * over the same input, every view width x height, rendered by one launch chain over a combined tile
 * space.  View v's colour target starts at color + v * color_view_stride_bytes (height rows of
 * color_pitch bytes), its depth target at depth + v * depth_view_stride_bytes (depth may be NULL).
 * Every view's bytes equal those of gsm_global_render for its camera; view_count == 1 is allowed.
 * Enqueue-only on `stream`; `cameras` is host memory and is consumed before the call returns.
 *
 * The batch runs inside the handle's allocations (gsm_global_create sizes them; only a small
 * per-view constant array is allocated, by the handle's first batch).  Checked before anything is
 * enqueued, in this order:
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   view_count == 0, or view_count * roundup(gaussian_count, 256)
 *                                    > max_gaussians (a view's items start on a 256-item boundary);
 *   GSM_ERR_INVALID_DIMENSIONS       width > max_width or height > max_height (or zero);
 *   GSM_ERR_INVALID_TILE_COUNT       view_count * tiles(width, height) exceeds the handle's tile count
 *                                    (tiles(max_width, max_height), 32 x 16 pixel tiles) or 65535;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  cameras or color NULL (or the input's buffers, with a count > 0);
 *   GSM_ERR_INVALID_BUFFER_SIZE      a pitch smaller than a row, a view stride smaller than height
 *                                    rows, or one that misaligns a view (colour 4 bytes, depth 2);
 *   GSM_ERR_UNSUPPORTED              the handle is restricted to tile rows (gsm_global_set_tile_rows).
 * The assignment capacity (4 * max_gaussians) is shared by the batch: a batch whose views together
 * exceed it sets the overflow counter (gsm_debug.h), and no parity is promised for that frame. */
gsm_status gsm_global_render_views(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                   const gsm_camera_params *cameras, uint32_t view_count,
                                   uint32_t width, uint32_t height,
                                   void *color, size_t color_pitch_bytes, size_t color_view_stride_bytes,
                                   void *depth, size_t depth_pitch_bytes, size_t depth_view_stride_bytes);

/* One view of a batch (gsm_global_render_batch): its own scene, camera, frame size and targets. */
typedef struct {
    gsm_gaussian_input input;      /* this view's scene: device pointers, count, sh_components */
    gsm_camera_params  camera;
    uint32_t width, height;        /* this view's frame */
    void    *color;  size_t color_pitch_bytes;   /* config.color_format, height rows */
    void    *depth;  size_t depth_pitch_bytes;   /* r16f or NULL (per view) */
} gsm_global_view;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_view) == 224, "gsm_global_view is 224 bytes");
#else
_Static_assert(sizeof(gsm_global_view) == 224, "gsm_global_view is 224 bytes");
#endif

/* Views of different scenes and sizes in one frame (no reference analogue): view_count views,
 * each with its own input, camera, width x height and targets, rendered by one launch chain over a combined
 * item and tile space.  Every view's bytes equal those of gsm_global_render for that view alone.  Views may
 * share or differ in scene, count, size and targets (a side-by-side pair: two views into one target, the
 * second starting width * bytes-per-pixel into the row, both with the shared pitch), but two views must not
 * overlap in target memory -- this is not checked.  All views use the handle's precision and colour format
 * and the same sh_components; depth may be NULL for some views and not for others.
 * Enqueue-only on `stream`; `views` is host memory and is consumed before the call returns.  Only small
 * per-view arrays are allocated, by the handle's first batch; nothing per frame after it.
 *
 * Checked before anything is enqueued; the first failing check in this order decides, within a check the
 * lowest view index:
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   view_count == 0, a gaussian_count > max_gaussians, or
 *                                    sum of roundup(gaussian_count, 256) > max_gaussians (a view's items
 *                                    start on a 256-item boundary; a count of 0 is an empty frame, as for
 *                                    gsm_global_render);
 *   GSM_ERR_INVALID_DIMENSIONS       a width or height of zero, or above max_width / max_height;
 *   GSM_ERR_INVALID_TILE_COUNT       sum of tiles(width, height) exceeds the handle's tile count
 *                                    (tiles(max_width, max_height), 32 x 16 pixel tiles) or 65535;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  views NULL (with view_count >= 1: before every other check, since
 *                                    nothing of it can be read), a view's color NULL, or its gaussians /
 *                                    harmonics NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      a pitch smaller than a row, or a target or pitch misaligned (colour
 *                                    4 bytes, depth 2);
 *   GSM_ERR_INVALID_ARGUMENT         views that differ in sh_components;
 *   GSM_ERR_UNSUPPORTED              the handle is restricted to tile rows (gsm_global_set_tile_rows).
 * The assignment capacity (4 * max_gaussians) is shared by the batch: a batch whose views together
 * exceed it sets the overflow counter (gsm_debug.h), and no parity is promised for that frame. */
gsm_status gsm_global_render_batch(gsm_renderer *renderer, void *stream,
                                   const gsm_global_view *views, uint32_t view_count);

/* One object of a composite (gsm_global_render_composite): a resident scene and the frame's camera as seen
 * from that scene's own space. */
typedef struct {
    gsm_gaussian_input input;      /* this object's scene: device pointers, count, sh_components */
    gsm_camera_params  camera;     /* the frame's camera in this object's space (below) */
} gsm_global_object;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_object) == 184, "gsm_global_object is 184 bytes");
#else
_Static_assert(sizeof(gsm_global_object) == 184, "gsm_global_object is 184 bytes");
#endif

/* Several posed scenes composed into one frame (no reference analogue): object_count objects,
 * each a resident scene with its own pose, rendered by one launch chain into one width x height target.  The
 * splats of all objects are sorted and blended together, so objects interleave in depth per tile as the
 * gaussians of one scene do.
 *
 * The pose is a camera.  Object o is projected exactly as gsm_global_render would project it with
 * objects[o].camera; the device sees cameras only, and no arithmetic is added to the numeric contract.  For an
 * object with model matrix M (object space -> world space) under the frame's camera (view, proj, position) the
 * caller passes
 *     view_o = view * M,   position_o = M^-1 * position,   proj, near_plane and far_plane unchanged,
 * so the spherical-harmonics view directions are taken in the object's own frame.  That is exact for a rotation,
 * a translation and a uniform scale.  The gaussians' scales, and the cull of scales below 0.0005, are in object
 * space: M does not rescale them.  For an M that is no similarity the object is whatever the projection gives
 * for view * M.
 *
 * Order.  The frame is the Global frame of the concatenated objects: one assignment list sorted by
 * (tile, 16-bit depth); equal keys keep ascending object index, then ascending gaussian id.  With one camera
 * for all objects the bytes equal those of gsm_global_render of the concatenated buffers.
 *
 * Layout.  Object o's items start at 256 * B_o, B_o = sum over u < o of ceil(count_u / 256); an object with
 * count 0 owns no block.  All objects use the handle's tile grid and the one target, as gsm_global_render does
 * for width x height.  After a captured composite gsm_global_debug_copy returns the per-gaussian buffers
 * (render data, bounds, tile counts) indexed by item -- 256 entries per block of the composite, 256 * sum over
 * o of ceil(count_o / 256) in all -- and the sort values hold items.  Unspecified in those buffers: every entry
 * at or past its object's count, and, as after gsm_global_render, the render data of a culled gaussian (one
 * whose bounds are empty: only visible gaussians write render data).
 *
 * Enqueue-only on `stream`; `objects` is host memory and is consumed before the call returns.  Only small
 * per-object arrays are allocated, by the handle's first composite; nothing per frame after it.  All objects
 * use the handle's precision and colour format.
 *
 * Checked before anything is enqueued; the first failing check in this order decides, within a check the
 * lowest object index:
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   object_count == 0 or > 65535, a gaussian_count > max_gaussians, or
 *                                    sum of roundup(gaussian_count, 256) > max_gaussians (all counts 0 is an
 *                                    empty frame: the clear value everywhere);
 *   GSM_ERR_INVALID_DIMENSIONS       width or height zero, or above max_width / max_height;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  objects NULL (with object_count >= 1: before every other check, since
 *                                    nothing of it can be read), color NULL, or an object's gaussians /
 *                                    harmonics NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      a pitch smaller than a row, or a target or pitch misaligned (colour
 *                                    4 bytes, depth 2);
 *   GSM_ERR_INVALID_ARGUMENT         objects that differ in sh_components;
 *   GSM_ERR_UNSUPPORTED              the handle is restricted to tile rows (gsm_global_set_tile_rows).
 * The assignment capacity (4 * max_gaussians) is shared by the objects: a composite that exceeds it sets the
 * overflow counter (gsm_debug.h), and no parity is promised for that frame.  The counters report the
 * composite; gaussian_count is the sum of the objects' counts. */
gsm_status gsm_global_render_composite(gsm_renderer *renderer, void *stream,
                                       const gsm_global_object *objects, uint32_t object_count,
                                       uint32_t width, uint32_t height,
                                       void *color, size_t color_pitch_bytes,
                                       void *depth_r16f, size_t depth_pitch_bytes);

/* A per-pixel pick target (no reference analogue): gsm_global_render and
 * gsm_global_render_composite with a third target that answers "which splat is under this pixel?".
 *
 * Colour and depth: their bytes equal those of the plain entry for the same arguments.
 *
 * Pick target: height rows of pick_pitch_bytes, one uint32_t per pixel.  Every pixel of width x height is
 * written every frame (the caller does not clear it); bytes of a row past 4 * width are not touched.
 *
 * Pick value.  Walk the pixel's tile list front to back as the blend does.  For every entry the pixel's 4x2
 * group blends -- reached before the group's saturation break, and not skipped because the group's eight
 * alphas are all zero -- take the fp16 weight w = alpha * T, with T the pixel's transmittance before that
 * entry.  The pick is the item of the heaviest w: the earliest entry wins ties, and a weight of zero or NaN
 * never wins.  A pixel of an empty tile, or one that no entry reaches with w > 0, holds GSM_PICK_NONE.
 *
 * Items.  For gsm_global_render_pick the item is the gaussian id.  For gsm_global_render_composite_pick it is
 * the item of the composite's layout, 256 * B_o + id (above); gsm_global_pick_owner maps it back.
 *
 * Checks: the plain entry's, in its order, with the pick target joining the rows it belongs to --
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  also: pick NULL;
 *   GSM_ERR_INVALID_BUFFER_SIZE      also: pick_pitch_bytes < 4 * width, or the pointer or the pitch not
 *                                    4-byte aligned;
 *   GSM_ERR_UNSUPPORTED              (both entries, after every other check) the handle is restricted to tile
 *                                    rows (gsm_global_set_tile_rows).
 * Enqueue-only and capturable like the plain entries; nothing is allocated per frame.  A batch of views with pick
 * targets is gsm_global_render_frames (below); gsm_global_render_views, the DepthFirst and Local renderers and the
 * multi-GPU frame have no pick entry. */
#define GSM_PICK_NONE 0xFFFFFFFFu
gsm_status gsm_global_render_pick(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                  const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                  void *color, size_t color_pitch_bytes, void *depth_r16f,
                                  size_t depth_pitch_bytes, void *pick_r32u, size_t pick_pitch_bytes);
gsm_status gsm_global_render_composite_pick(gsm_renderer *renderer, void *stream,
                                            const gsm_global_object *objects, uint32_t object_count,
                                            uint32_t width, uint32_t height,
                                            void *color, size_t color_pitch_bytes,
                                            void *depth_r16f, size_t depth_pitch_bytes,
                                            void *pick_r32u, size_t pick_pitch_bytes);

/* Items of the handle's last enqueued pick frame -> (object index of that call, gaussian id within the
 * object); after gsm_global_render_pick the object is 0.  Host work only: no device work, no sync (the items
 * are the caller's copy of pick pixels).  GSM_PICK_NONE, an item at or past the frame's items and an item at
 * or past its object's count give GSM_PICK_NONE in both outputs.  GSM_ERR_RENDER_FAILED when the handle's last
 * enqueued frame was not a pick frame; GSM_ERR_INVALID_ARGUMENT for a NULL array with n > 0. */
gsm_status gsm_global_pick_owner(gsm_renderer *renderer, const uint32_t *items, uint32_t n,
                                 uint32_t *object, uint32_t *gaussian);

/* Occlusion by a depth image (no reference analogue): gsm_global_render and
 * gsm_global_render_composite with one more input, the view-space depth of the opaque geometry the application
 * draws itself.  Splats behind that surface disappear, pixel by pixel, inside the blend.
 *
 * Occluder: height rows of occluder_pitch_bytes, one float per pixel, in device memory; the frame only reads it.
 * The value is the depth of the opaque surface at that pixel in the unit of the frame's own depth target: clip.w
 * of the frame camera (of the shared projection for a composite).  INTEGRATION.md says how to get it from a
 * hardware depth buffer.
 *
 * Rule, on the blend's walk of a pixel's tile list (front to back, per 4x2 pixel group).  Z = fp16(occluder
 * value), one round-to-nearest-even conversion, denormals kept.  A pixel is closed from the first evaluated entry
 * on whose fp16 depth dep lies behind the surface, Z < dep (false when either is NaN).  A closed pixel's alpha is
 * +0 for that entry and every later one, and the group's saturation break takes a closed pixel's transmittance
 * as +0; everything else of the walk is the plain entry's.  (Every entry of the tile's list counts, also one
 * whose alpha is 0 on all of the group's pixels: it blends nothing, but it closes pixels.)  So:
 *   - a splat at exactly the surface's fp16 depth is drawn (the cut moves in fp16 steps: 0.0625 near depth 100);
 *   - an occluder value of +inf, NaN, or anything that rounds to fp16 +inf (above 65519) occludes nothing;
 *   - a value at or below the near plane closes the pixel before its first entry;
 *   - with an occluder of all +inf (or all NaN) the colour and depth bytes equal the plain entry's.
 * Active tiles are those with list entries, whatever the occluder says: pixels of inactive tiles hold the clear
 * value (alpha 1); a fully occluded pixel of an active tile holds colour 0, alpha 1 - 1 = +0 and depth 0.  Every
 * gsm_color_format and both precisions; depth may be NULL.
 *
 * Checks: the plain entry's, in its order, with the occluder joining the rows it belongs to --
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  also: occluder NULL;
 *   GSM_ERR_INVALID_BUFFER_SIZE      also: occluder_pitch_bytes < 4 * width, or the pointer or the pitch not
 *                                    4-byte aligned;
 *   GSM_ERR_UNSUPPORTED              (both entries, after every other check) the handle is restricted to tile
 *                                    rows (gsm_global_set_tile_rows).
 * Enqueue-only and capturable like the plain entries; nothing is allocated per frame.  gsm_global_render_frame
 * (below) combines an occluder with a pick target and with styles, gsm_global_render_frames does so for a batch of
 * views; gsm_global_render_views, the DepthFirst and Local renderers and the multi-GPU frame have no occluded
 * entry. */
gsm_status gsm_global_render_occluded(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                      const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                      void *color, size_t color_pitch_bytes, void *depth_r16f,
                                      size_t depth_pitch_bytes, const void *occluder_r32f,
                                      size_t occluder_pitch_bytes);
gsm_status gsm_global_render_composite_occluded(gsm_renderer *renderer, void *stream,
                                                const gsm_global_object *objects, uint32_t object_count,
                                                uint32_t width, uint32_t height,
                                                void *color, size_t color_pitch_bytes,
                                                void *depth_r16f, size_t depth_pitch_bytes,
                                                const void *occluder_r32f, size_t occluder_pitch_bytes);

/* Per-gaussian styles (no reference analogue): gsm_global_render and gsm_global_render_composite
 * with one state byte per gaussian and a table of at most 256 styles, so an application shows a selection --
 * hides, highlights or fades splats -- without rewriting its scene while the user is selecting.  The step that
 * does rewrite it (delete, crop, separate, export) is gsm_global_extract, below.
 *
 * Rule.  A gaussian's state s is its byte of the state array, or default_state when the array is NULL.  Its style
 * is S = styles[s] when s < style_count, otherwise the identity {tint_amount 0, opacity_scale 255, hidden 0}.  For
 * a gaussian that passed every cull of the projection and formed its four u8 bytes (colour r, g, b and opacity of
 * GaussianRenderData):
 *   - S.hidden != 0: the gaussian is culled -- empty bounds (0, -1, 0, -1), no tiles, never listed, never picked;
 *   - otherwise each colour byte c becomes (c * (255 - k) + t * k + 127) / 255, k = tint_amount, t the tint byte
 *     of that channel, and the opacity byte o becomes (o * opacity_scale + 127) / 255, in unsigned integers.
 * Everything after that point is the plain frame applied to the styled bytes: the tile test's level, the blend
 * record's fp16 colour and opacity, the skip band, the sort and the blend.  An opacity byte of 0 gives the
 * gaussian no tiles but leaves it visible (its bounds stay).  So: with every reachable style the identity (or every
 * state at or above style_count) the bytes equal the plain entry's; with only hidden styles in use the colour and
 * depth equal gsm_global_render of the scene with the hidden gaussians removed.
 *
 * pick_r32u may be NULL: the frame then uses the plain blend and pick_pitch_bytes is ignored.  Non-NULL: the pick
 * frame above, and gsm_global_pick_owner works after it.  `styles`, `state` / `states` (the structs) are host
 * memory, consumed before the call returns; the state arrays are device memory the frame only reads.  A composite
 * takes one gsm_global_state per object: {NULL, 1} highlights or hides an object as a whole.
 *
 * Checks: the plain entry's (the pick entry's when pick_r32u is non-NULL), in its order; then
 *   GSM_ERR_INVALID_ARGUMENT  styles NULL, style_count 0 or above 256, state / states NULL, or a default_state
 *                             above 255 (the lowest object index decides);
 *   GSM_ERR_UNSUPPORTED       the handle is restricted to tile rows (gsm_global_set_tile_rows).
 * Enqueue-only and capturable; a captured frame replays the table and the state pointers it was captured with.
 * Nothing is allocated per frame (the handle's first styled frame allocates the 2 KiB table).
 * gsm_global_render_frame (below) combines styles with an occluder, gsm_global_render_frames does so for a batch
 * of views; gsm_global_render_views, the DepthFirst and Local renderers and the multi-GPU frame have no styled
 * entry.  A style changes neither position nor scale. */
typedef struct {
    uint8_t tint_r, tint_g, tint_b; /* in the u8 colour space of GaussianRenderData: after the SH evaluation and,
                                       for gaussian_color_space SRGB, after the decode to linear */
    uint8_t tint_amount;            /* 0: colour unchanged ... 255: colour replaced by the tint */
    uint8_t opacity_scale;          /* 255: opacity unchanged ... 0: opacity byte 0 */
    uint8_t hidden;                 /* nonzero: the gaussian is culled */
    uint8_t pad[2];                 /* ignored */
} gsm_global_style;
typedef struct {
    const uint8_t *state;   /* device memory, one byte per gaussian of the scene, or NULL */
    uint32_t default_state; /* 0..255: every gaussian's state when `state` is NULL; ignored otherwise */
    uint32_t pad;
} gsm_global_state;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_style) == 8, "gsm_global_style is 8 bytes");
static_assert(sizeof(gsm_global_state) == 16, "gsm_global_state is 16 bytes");
#else
_Static_assert(sizeof(gsm_global_style) == 8, "gsm_global_style is 8 bytes");
_Static_assert(sizeof(gsm_global_state) == 16, "gsm_global_state is 16 bytes");
#endif
gsm_status gsm_global_render_styled(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                    const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                    void *color, size_t color_pitch_bytes, void *depth_r16f,
                                    size_t depth_pitch_bytes, void *pick_r32u, size_t pick_pitch_bytes,
                                    const gsm_global_state *state, const gsm_global_style *styles,
                                    uint32_t style_count);
gsm_status gsm_global_render_composite_styled(gsm_renderer *renderer, void *stream,
                                              const gsm_global_object *objects, uint32_t object_count,
                                              uint32_t width, uint32_t height,
                                              void *color, size_t color_pitch_bytes,
                                              void *depth_r16f, size_t depth_pitch_bytes,
                                              void *pick_r32u, size_t pick_pitch_bytes,
                                              const gsm_global_state *states /* [object_count] */,
                                              const gsm_global_style *styles, uint32_t style_count);

/* Selection by a screen mask: "every splat whose centre lies under these pixels" -- rectangle, brush
 * and lasso selection -- on the device, into the state array the styled frames read.
 *
 * Gaussian g < gaussian_count matches when (1) it passes every cull of the projection for camera, width, height
 * (input.harmonics is not read and may be NULL, sh_components is ignored); (2) `styles` is NULL or the style of its
 * current state byte is not hidden; (3) mx and my, the fp16 mean of its GaussianRenderData, are finite; (4) px =
 * floor(mx + 0.5) lies in [0, width), py = floor(my + 0.5) in [0, height), and the mask byte at (px, py) is
 * nonzero.  A matching gaussian's state becomes ((old & and_mask) ^ xor_mask) & 0xFF -- set a bit (and ~b, xor b),
 * clear it (and ~b, xor 0), toggle it (and 0xFF, xor b), assign (and 0, xor v); every other byte of `state`, and
 * every byte at or past gaussian_count, keeps its value.  `matched` (device, nullable) receives the number of
 * matching gaussians: it is overwritten, not added to.  mask_u8: device memory, height rows of mask_pitch_bytes.
 * For a composite, call it once per object with that object's camera.  Enqueue-only and capturable.
 *
 * Checks, in this order:
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians;
 *   GSM_ERR_INVALID_DIMENSIONS       width or height zero, or above max_width / max_height;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  input, camera or mask_u8 NULL; gaussians or state NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      mask_pitch_bytes < width, or matched not 4-byte aligned;
 *   GSM_ERR_INVALID_ARGUMENT         styles NULL with style_count != 0, or styles non-NULL with style_count 0 or
 *                                    above 256.
 * A count of 0 is a no-op that writes *matched = 0. */
gsm_status gsm_global_select_mask(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                  const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                  const void *mask_u8, size_t mask_pitch_bytes, uint8_t *state,
                                  const gsm_global_style *styles, uint32_t style_count,
                                  uint32_t and_mask, uint32_t xor_mask, uint32_t *matched);

/* One descriptor for every Single and Compose frame (no reference analogue): the plain, pick,
 * occluded and styled entries above and every combination of their options, which those entries do not offer --
 * an occluder with a pick target, an occluder with styles, all three.  `frame` is host memory, consumed before the
 * call returns, as are the arrays it points to (objects, states, styles); the targets, the occluder and the state
 * bytes are device memory.
 *
 * Semantics, composed from the rules above: styles apply in the projection (the styled entries' rule); the list is
 * the composite's (one object: gsm_global_render's); with an occluder the walk is the occluded one; the pick is the
 * pick entries' rule applied to the walk that runs.  Under an occluder a closed pixel's alpha is +0, so its weight
 * alpha * T is 0 and never wins: the pick of a pixel is the heaviest contribution in front of the surface, and a
 * pixel closed before its first entry holds GSM_PICK_NONE.  No arithmetic is added to the numeric contract.
 *
 * Identities: with object_count == 1 the bytes are those of the single-scene entries; with an option NULL the bytes
 * are those of the entry without it (colour, depth and pick equal gsm_global_render, _pick, _occluded, _styled and
 * their composite forms for the same arguments); an occluder of all +inf gives the pick frame's three targets; an
 * identity style table gives the unstyled frame.  gsm_global_pick_owner and gsm_global_select_pick work after any
 * frame of this entry that had a pick target.
 *
 * Checked before anything is enqueued; the first failing check in this order decides:
 *   GSM_ERR_INVALID_ARGUMENT         frame NULL or a flags bit other than GSM_FRAME_ORTHOGRAPHIC set (before
 *                                    everything else; bit 0 stays reserved: flags == 1 and flags == 3 are refused);
 *   then the checks of gsm_global_render (object_count == 1 with objects non-NULL) or gsm_global_render_composite
 *   (every other object_count, 0 included), in that entry's order, each optional buffer joining its rows --
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   as that entry;
 *   GSM_ERR_INVALID_DIMENSIONS       as that entry;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  as that entry (a NULL pick, occluder or depth pointer is "not given", never
 *                                    missing);
 *   GSM_ERR_INVALID_BUFFER_SIZE      also: pick_pitch_bytes < 4 * width or occluder_pitch_bytes < 4 * width, or
 *                                    either pointer or pitch not 4-byte aligned;
 *   GSM_ERR_INVALID_ARGUMENT         objects that differ in sh_components; then the styled row: styles without
 *                                    states, states without styles, style_count 0 or above 256, or a default_state
 *                                    above 255 (both NULL: no styles, style_count ignored);
 *   GSM_ERR_UNSUPPORTED              last: the handle is restricted to tile rows (gsm_global_set_tile_rows) and
 *                                    the frame has a pick target, an occluder, styles or the orthographic flag, or
 *                                    more than one object.
 * Enqueue-only and capturable; nothing is allocated per frame beyond what the entries above allocate once.
 * Several descriptors in one batch -- a quad view, a stereo pair -- are gsm_global_render_frames (below).  Out of
 * scope: gsm_global_render_views, gsm_global_render_records, the DepthFirst and Local renderers and the multi-GPU
 * frame take no pick target, occluder or styles. */
typedef struct {
    const gsm_global_object *objects;  uint32_t object_count;   /* 1 object = a single frame */
    uint32_t width, height;
    void *color;  size_t color_pitch_bytes;
    void *depth_r16f;  size_t depth_pitch_bytes;                /* nullable */
    void *pick_r32u;  size_t pick_pitch_bytes;                  /* nullable */
    const void *occluder_r32f;  size_t occluder_pitch_bytes;    /* nullable */
    const gsm_global_state *states;                             /* [object_count], nullable with styles */
    const gsm_global_style *styles;  uint32_t style_count;      /* nullable */
    uint32_t flags;                                             /* 0 or GSM_FRAME_ORTHOGRAPHIC */
} gsm_global_frame;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_frame) == 112, "gsm_global_frame is 112 bytes");
#else
_Static_assert(sizeof(gsm_global_frame) == 112, "gsm_global_frame is 112 bytes");
#endif
gsm_status gsm_global_render_frame(gsm_renderer *renderer, void *stream, const gsm_global_frame *frame);

/* Orthographic cameras (no reference analogue): the top, front and side viewports of an editor.  A
 * frame is orthographic when gsm_global_frame.flags has GSM_FRAME_ORTHOGRAPHIC; the kind is requested, never detected
 * from the matrix.  Bit 0 of flags stays reserved and refused.  The flag holds for every object of the frame; in
 * gsm_global_render_frames it is per frame, so one batch may mix perspective and orthographic views.
 *
 * The rule, for a gaussian under an object's camera (everything not named is the perspective rule unchanged: the
 * scale cull, the alpha threshold, the 3-D covariance, the stabilisation, theta and the sigmas, the radius cull, the
 * extents, the screen-bounds cull, the tile bounds, the record, the tile count, the scatter, the sort, the blend):
 *   vp = view * (pos, 1), clip = proj * vp; row 3 of proj is not used;
 *   depth   d = sigma * vp.z with sigma = +1 when proj[10] >= 0 and -1 otherwise (the project's convention is
 *           proj[10] > 0, looking down +z).  The near cull is !(d > near_plane); d replaces clip.w wherever the
 *           perspective rule uses it: the fp16 depth of GaussianRenderData, the sort key, the depth target and the
 *           total-ink cull's depth;
 *   screen  ndc = (clip.x, clip.y) without a division, then the same pixel-centred mapping;
 *   cov     J = diag(width * proj[0] * 0.5f, height * proj[5] * 0.5f), the signed entries, every other entry 0:
 *           no 1/z, no tan clamp, no third column; then T = J W, T C T^T and + 0.3f on the diagonal as before;
 *   colour  all rays are parallel: the SH direction is the uniform normalize(-sigma * (view[2], view[6], view[10])),
 *           from the scene toward the camera; camera.position is ignored.  Degree 0 is unchanged.
 * A perspective frame's bytes, kernels and schedule are what they were; an orthographic frame keeps blend-unit costs
 * of its own.  Out of scope: reversed-Z or otherwise unconventional proj[10]; skewed or oblique projections
 * (proj[1], proj[4], proj[8], proj[9] act on the mean through clip, but not on J); gsm_global_render, _views, _batch
 * and the older single-purpose entries, which get no flag; the DepthFirst, Local and multi-GPU renderers. */
#define GSM_FRAME_ORTHOGRAPHIC 2u

/* gsm_global_select_mask in an orthographic viewport: the same signature, checks (in the same order), match rule
 * and state update, with the gaussians projected by the orthographic rule above -- the means are those of an
 * orthographic frame of the same camera, width and height. */
gsm_status gsm_global_select_mask_ortho(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                        const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                        const void *mask_u8, size_t mask_pitch_bytes, uint8_t *state,
                                        const gsm_global_style *styles, uint32_t style_count,
                                        uint32_t and_mask, uint32_t xor_mask, uint32_t *matched);

/* Select what is visible: the state bytes of the gaussians of one object that a pick image shows
 * under a mask.  The handle's last enqueued frame must be a pick frame (any entry with a pick target) of
 * width x height; pick_r32u is that frame's pick target or a copy of it.  With the composite layout above -- object
 * o's items start at 256 * B_o and number count_o; a single frame is object 0 with B_0 = 0 -- let
 *   S = { item - 256 * B_object : pixel (x, y) of width x height has a nonzero mask byte (or mask_u8 is NULL), and
 *         item = pick[y][x] lies in [256 * B_object, 256 * B_object + min(count_object, gaussian_count)) }.
 * Every id in S gets state[id] = ((old & and_mask) ^ xor_mask) & 0xFF exactly once, however many pixels it covers
 * (a toggle does not cancel itself); every other byte of `state`, and every byte at or past gaussian_count, keeps
 * its value.  `matched` (device, nullable) receives |S|: overwritten, not added to.  After an occluded pick frame S
 * holds only splats in front of the surface: "select the visible surface".  The layout is host state of the last
 * pick frame, as for gsm_global_pick_owner.  Enqueue-only and capturable; the handle's first call allocates a
 * bitmap of max_gaussians / 8 bytes, nothing after it.
 *
 * Checks, in this order:
 *   GSM_ERR_RENDER_FAILED            the handle's last enqueued frame was not a pick frame;
 *   GSM_ERR_INVALID_ARGUMENT         object at or past that frame's object count;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians;
 *   GSM_ERR_INVALID_DIMENSIONS       width or height zero, above max_width / max_height, or not the pick frame's;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  pick_r32u NULL, or state NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      pick_pitch_bytes < 4 * width, the pick pointer or pitch not 4-byte aligned,
 *                                    mask_pitch_bytes < width (mask_u8 non-NULL), or matched not 4-byte aligned.
 * A count of 0 is a no-op that writes *matched = 0. */
gsm_status gsm_global_select_pick(gsm_renderer *renderer, void *stream,
                                  const void *pick_r32u, size_t pick_pitch_bytes, uint32_t width, uint32_t height,
                                  const void *mask_u8, size_t mask_pitch_bytes,
                                  uint32_t object, uint8_t *state, uint32_t gaussian_count,
                                  uint32_t and_mask, uint32_t xor_mask, uint32_t *matched);

/* Several frame descriptors in one batch (no reference analogue): a quad view, a main view with
 * thumbnails, a stereo pair -- every viewport with its own selection shown, its own mesh cutting the splats and
 * its own pick image.  frame_count frames are rendered by one launch chain over the combined item and tile space of
 * gsm_global_render_batch; each frame has its own scene, camera, size and targets and its own nullable pick target,
 * occluder and states.  gsm_global_frame is used unchanged; every frame has object_count == 1.
 *
 * Bytes.  For every frame v the colour, depth and pick bytes equal those of gsm_global_render_frame(&frames[v])
 * called alone.  A pick pixel therefore holds the gaussian id of frame v's scene, or GSM_PICK_NONE -- never the
 * batch item: the walk subtracts the view's first item before the store.  The options are independent per frame:
 * one frame may have a pick target and no occluder while its neighbour has the reverse, or neither; the depth, pick
 * and occluder pointers of different frames may be NULL in any mixture.  With every option NULL in every frame the
 * bytes equal gsm_global_render_batch of the same views (and that entry's path runs); with frame_count == 1 they
 * equal gsm_global_render_frame.
 *
 * Layout: gsm_global_render_batch's.  Frame v's items start at 256 * B_v, B_v = sum over u < v of
 * ceil(count_u / 256), its tiles at the sum of the tiles of the frames before it, on its own grid.
 *
 * Memory.  Targets of different frames must not overlap, pick targets included; this is not checked, as for the
 * batch.  Occluders and state arrays are only read and may be shared between frames.  A side-by-side stereo pair is
 * two frames into one colour, one depth and one pick image and out of one occluder image: the second frame's
 * pointers start `width` pixels into the row and both use the shared pitch.
 *
 * Styles.  The batch has one style table: every frame whose `styles` is non-NULL must give the same style_count and
 * the same six meaningful bytes per style (pad is ignored).  A frame with styles == NULL and states == NULL is
 * unstyled; a frame with styles uses states[0], as gsm_global_render_frame does for one object.
 *
 * Enqueue-only and capturable; `frames` and what it points to in host memory are consumed before the call returns.
 * Nothing is allocated per frame beyond small per-view arrays on the handle's first such call.  After the call the
 * handle's "last pick frame" state is cleared: gsm_global_pick_owner and gsm_global_select_pick return
 * GSM_ERR_RENDER_FAILED, as after any frame without a pick target -- the pick pixels already are gaussian ids of the
 * view's scene, so no owner lookup is needed, and gsm_global_select_pick_ids (below) selects from them.
 *
 * Checked before anything is enqueued; the first failing row decides, within a row the lowest frame index:
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  frames NULL with frame_count >= 1;
 *   GSM_ERR_INVALID_ARGUMENT         a frame with a flags bit other than GSM_FRAME_ORTHOGRAPHIC set;
 *   GSM_ERR_UNSUPPORTED              a frame with object_count != 1 (composites inside a batch are out of scope);
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  a frame's objects NULL;
 *   then the rows of gsm_global_render_batch, in its order, applied to (objects[0].input, objects[0].camera, width,
 *   height, color, depth_r16f) of every frame -- frame_count == 0 gives GSM_ERR_INVALID_GAUSSIAN_COUNT -- with the
 *   pick target and the occluder joining the rows as they do for gsm_global_render_frame:
 *   GSM_ERR_INVALID_BUFFER_SIZE      also: pick_pitch_bytes < 4 * width or occluder_pitch_bytes < 4 * width, or
 *                                    either pointer or pitch not 4-byte aligned (NULL: not given, never missing);
 *   GSM_ERR_INVALID_ARGUMENT         frames that differ in sh_components;
 *   GSM_ERR_INVALID_ARGUMENT         the styled row of gsm_global_render_frame, per frame; or two frames whose
 *                                    style tables differ;
 *   GSM_ERR_UNSUPPORTED              the handle is restricted to tile rows (gsm_global_set_tile_rows).
 * Out of scope: composites inside a batch (object_count > 1); gsm_global_render_views keeps its signature and
 * stays without options. */
gsm_status gsm_global_render_frames(gsm_renderer *renderer, void *stream,
                                    const gsm_global_frame *frames, uint32_t frame_count);

/* The stateless form of gsm_global_select_pick, for pick images that hold gaussian ids (a frame of
 * gsm_global_render_frames, or a single-scene pick frame).  With
 *   S = { id : pixel (x, y) of width x height has a nonzero mask byte (or mask_u8 is NULL) and
 *         id = pick[y][x] < gaussian_count },
 * every id of S gets state[id] = ((old & and_mask) ^ xor_mask) & 0xFF exactly once, however many pixels it covers;
 * every other byte of `state`, and every byte at or past gaussian_count, keeps its value.  `matched` (device,
 * nullable) receives |S|: overwritten, not added to.  GSM_PICK_NONE never matches.  It neither reads nor changes
 * the handle's last-pick state; it shares the handle's bitmap with gsm_global_select_pick.  Enqueue-only and
 * capturable.
 *
 * Checks, in this order:
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians;
 *   GSM_ERR_INVALID_DIMENSIONS       width or height zero, or above max_width / max_height;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  pick_r32u NULL, or state NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      pick_pitch_bytes < 4 * width, the pick pointer or pitch not 4-byte aligned,
 *                                    mask_pitch_bytes < width (mask_u8 non-NULL), or matched not 4-byte aligned.
 * A count of 0 is a no-op that writes *matched = 0. */
gsm_status gsm_global_select_pick_ids(gsm_renderer *renderer, void *stream,
                                      const void *pick_r32u, size_t pick_pitch_bytes, uint32_t width, uint32_t height,
                                      const void *mask_u8, size_t mask_pitch_bytes,
                                      uint8_t *state, uint32_t gaussian_count,
                                      uint32_t and_mask, uint32_t xor_mask, uint32_t *matched);

/* Rewriting the scene by its state bytes (no reference analogue): the step after the selection --
 * delete it, crop to it, separate it into an object of its own (which gsm_global_render_composite then poses),
 * export what is visible -- on the device, from the state bytes the selects write and the styled frames read.
 *
 * A keep set is 256 bits, one per state value: bit (s & 31) of keep[s >> 5] says that a gaussian whose state byte
 * is s is kept.  Two host-only helpers fill one:
 *   gsm_global_keep_visible  bit s is set unless s < style_count and styles[s].hidden != 0 -- exactly the states the
 *                            styled frames do not cull; styles NULL or style_count 0 sets all 256 bits, a
 *                            style_count above 256 is read as 256;
 *   gsm_global_keep_masked   bit s is set when (s & test_mask & 0xFF) == (test_value & 0xFF): "selection bit set"
 *                            (b, b), "selection bit clear" (b, 0), "state equals v" (0xFF, v).
 *
 * gsm_global_extract.  Gaussian g < gaussian_count has the state s_g = state->state[g], or state->default_state
 * when that pointer is NULL, and is kept when bit s_g of `keep` is set.  With g_0 < g_1 < ... < g_{K-1} the kept ids
 * in ascending order, for every j < min(K, capacity): row j of out->gaussians is the byte copy of input record g_j
 * (48 B, or 32 B for a half-precision handle), row j of out->harmonics the byte copy of input row g_j (3 *
 * sh_components floats or halfs), out->state[j] = s_g_j and out->ids[j] = g_j.  *kept = K, the full count, not the
 * clamped one: K > capacity says that the output is a prefix and how much room a second call needs.  No byte of any
 * output at or past row min(K, capacity) is written; every byte before it is.  The ascending order is part of the
 * contract: the Global sort breaks equal (tile, depth) keys by ascending id, so only an order-preserving removal
 * keeps the styled entries' identity above byte for byte -- gsm_global_render of the scene extracted with
 * gsm_global_keep_visible equals gsm_global_render_styled of the full scene when the hidden styles' other fields
 * are the identity.  Rows are copied, never re-encoded: no arithmetic is added to the numeric contract.
 *
 * The structs and `keep` are host memory, consumed before the call returns; everything they point to, and `kept`,
 * is device memory.  Enqueue-only on `stream` and capturable: a captured call replays the pointers, the keep set and
 * default_state it was captured with, and reads the state bytes of the replay.  Nothing is allocated per call (the
 * handle's first extract allocates ceil(max_gaussians / 256) words).  It neither reads nor changes the handle's
 * last-frame state, and gsm_global_set_tile_rows does not concern it.  Extraction in place is not offered.
 *
 * Checks, all before anything is enqueued; the first failing row in this order decides:
 *   GSM_ERR_INVALID_ARGUMENT         renderer NULL;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians (the count of a NULL input cannot be read: that
 *                                    call falls to the next row);
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  input, state, keep, out or kept NULL;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  with a count > 0: input->gaussians NULL, or input->harmonics NULL while
 *                                    sh_components > 0;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  with a count > 0 and a capacity > 0: out->gaussians NULL, or out->harmonics
 *                                    NULL while sh_components > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      kept or out->ids not 4-byte aligned;
 *   GSM_ERR_INVALID_BUFFER_SIZE      out->gaussians not 16-byte aligned;
 *   GSM_ERR_INVALID_BUFFER_SIZE      out->harmonics not aligned to its element (2 or 4 bytes);
 *   GSM_ERR_INVALID_ARGUMENT         default_state > 255;
 *   GSM_ERR_INVALID_ARGUMENT         an output's byte range meets one of the byte ranges the call reads or another
 *                                    output's range: the outputs are `capacity` rows each and `kept` is 4 bytes; the
 *                                    ranges read are gaussian_count rows each of the records, the harmonics and the
 *                                    state array.
 * A count of 0 writes *kept = 0 and nothing else.
 *
 * gsm_global_state_histogram.  histogram[s] (device, 256 words) becomes the number of g < gaussian_count with
 * state[g] == s: overwritten, not added to; a count of 0 writes 256 zeros.  An editor's "n selected" readout, and,
 * summed over a keep set, the exact capacity for an extract.  Enqueue-only and capturable.  Checks, in this order:
 *   GSM_ERR_INVALID_ARGUMENT         renderer NULL;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  histogram NULL, or state NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      histogram not 4-byte aligned.
 *
 * Transforming the kept gaussians is gsm_global_transform's (below; baking a pose rotates the SH rows: arithmetic,
 * stated there).  Out of scope: merging scenes (a plain copy concatenates their rows), extraction in place, and the
 * DepthFirst, Local and multi-GPU renderers, which have no state bytes. */
typedef struct {
    void *gaussians;   /* capacity records of the handle's precision (48 B or 32 B) */
    void *harmonics;   /* capacity rows of 3 * sh_components floats or halfs; ignored when sh_components == 0 */
    uint8_t *state;    /* nullable: capacity bytes, the kept gaussians' state bytes */
    uint32_t *ids;     /* nullable: capacity words, the kept gaussians' ids in the input */
    uint32_t capacity; /* rows the outputs can hold */
    uint32_t pad;      /* ignored */
} gsm_global_extract_out;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_extract_out) == 40, "gsm_global_extract_out is 40 bytes");
#else
_Static_assert(sizeof(gsm_global_extract_out) == 40, "gsm_global_extract_out is 40 bytes");
#endif
void gsm_global_keep_visible(const gsm_global_style *styles, uint32_t style_count, uint32_t keep[8]);
void gsm_global_keep_masked(uint32_t test_mask, uint32_t test_value, uint32_t keep[8]);
gsm_status gsm_global_extract(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                              const gsm_global_state *state, const uint32_t keep[8],
                              const gsm_global_extract_out *out, uint32_t *kept /* device */);
gsm_status gsm_global_state_histogram(gsm_renderer *renderer, void *stream, const uint8_t *state,
                                      uint32_t gaussian_count, uint32_t *histogram /* device, 256 words */);

/* Selecting in the scene's own space, and the extent of a selection (no reference analogue).  Every
 * select above is a screen-space select: it needs a camera and cannot reach what is hidden or off screen.
 * gsm_global_select_where updates state bytes by a predicate on the records themselves -- inside or outside a box
 * or an ellipsoid, opacity in a range, largest scale in a range, the current state -- and gsm_global_state_bounds
 * gives the axis-aligned box and the count of the gaussians in a keep set: "frame the selection", a gizmo's pivot,
 * the pose of an object separated by gsm_global_extract.
 *
 * gsm_global_select_where, the match rule.  Gaussian g < gaussian_count has the old state byte `old` and its record
 * in the handle's precision: the position is three fp32 values, the opacity and the three scales are fp32, or fp16
 * widened exactly.  It matches when all of these hold:
 *   1. (old & test_mask & 0xFF) == (test_value & 0xFF);
 *   2. styles is NULL, or the style of `old` is not hidden (gsm_global_select_mask's rule, the identity for
 *      old >= style_count);
 *   3. the shape test.  With A = to_shape (row-major 3x4) and p the position, for every row r
 *        q_r = ((A[r][0]*px + A[r][1]*py) + A[r][2]*pz) + A[r][3],
 *      each multiplication and addition one IEEE fp32 operation in exactly this order, none fused;
 *        GSM_SELECT_BOX        inside = |q_0| <= 1 && |q_1| <= 1 && |q_2| <= 1,
 *        GSM_SELECT_ELLIPSOID  inside = ((q_0*q_0 + q_1*q_1) + q_2*q_2) <= 1.
 *      A gaussian with a NaN in q never matches, with or without GSM_SELECT_OUTSIDE; otherwise the test is
 *      inside != (flags & GSM_SELECT_OUTSIDE).  GSM_SELECT_ALL skips this step and never reads to_shape;
 *   4. unless the opacity range is exactly (-inf, +inf): opacity_min <= o && o <= opacity_max (false for a NaN o);
 *   5. unless the scale range is exactly (-inf, +inf): the same test on m = maxNum(maxNum(sx, sy), sz), which is
 *      NaN, and fails, only when all three scales are NaN.
 * No camera is involved and none of the projection's culls applies: a record the frame never draws (behind the
 * near plane, a scale below 0.0005) is selectable, so that it can be deleted.
 * A matching gaussian's state becomes ((old & and_mask) ^ xor_mask) & 0xFF.  Every other byte of `state`, and every
 * byte at or past gaussian_count, keeps its value.  `matched` (device, nullable) receives the number of matching
 * gaussians: overwritten, not added to.  input->harmonics is not read and may be NULL; sh_components is ignored.
 * `query` and `styles` are host memory, consumed before the call returns.  Enqueue-only and capturable: a captured
 * call replays the query, the style table and the pointers it was captured with and reads the state bytes of the
 * replay.  It neither reads nor changes the handle's last-frame or last-pick state, and gsm_global_set_tile_rows
 * does not concern it.
 *
 * Checks, all before anything is enqueued; the first failing row in this order decides:
 *   GSM_ERR_INVALID_ARGUMENT         renderer NULL;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians (the count of a NULL input cannot be read: that
 *                                    call falls to the next row);
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  input or query NULL; input->gaussians or state NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      matched not 4-byte aligned;
 *   GSM_ERR_INVALID_ARGUMENT         shape > 2; a flags bit other than bit 0; GSM_SELECT_ALL with GSM_SELECT_OUTSIDE;
 *                                    a NaN among the four range bounds; with a shape, a non-finite entry of to_shape;
 *   GSM_ERR_INVALID_ARGUMENT         styles NULL with style_count != 0, or styles non-NULL with style_count 0 or
 *                                    above 256.
 * A count of 0 is a no-op that writes *matched = 0.
 *
 * gsm_global_state_bounds.  The state and the keep set are gsm_global_extract's: s_g is state->state[g], or
 * state->default_state when that pointer is NULL, and gaussian g takes part when bit s_g of `keep` is set; {NULL, s}
 * with a full keep set gives the bounds of the whole scene.  min and max are the exact componentwise minimum and
 * maximum of the positions taking part whose three coordinates are finite; a coordinate of -0 counts as +0, so the
 * result has one bit pattern whatever the reduction order.  count is the number of those gaussians, skipped the
 * number taking part with a NaN or infinite coordinate (they are not in the box): count + skipped is the number
 * taking part.  The result is overwritten, not accumulated.  The centre and the radius are the caller's arithmetic
 * on the six numbers; no centroid is formed (a sum's rounding depends on its order).  `state` and `keep` are host
 * memory, `bounds` is device memory.  Enqueue-only and capturable; the handle's first call allocates 32 bytes per
 * 256 gaussians of max_gaussians, nothing is allocated after it.
 *
 * Checks, in this order:
 *   GSM_ERR_INVALID_ARGUMENT         renderer NULL;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  input, state, keep or bounds NULL;
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  input->gaussians NULL with a count > 0;
 *   GSM_ERR_INVALID_BUFFER_SIZE      bounds not 4-byte aligned;
 *   GSM_ERR_INVALID_ARGUMENT         default_state > 255.
 *
 * Transforming the records is gsm_global_transform's (below).  Out of scope: re-encoding records, colour or SH
 * predicates, a centroid or covariance, shapes beyond an affine image of the unit cube and the unit ball, selection
 * growth, and the DepthFirst, Local and multi-GPU renderers, which have no state bytes. */
#define GSM_SELECT_ALL        0u   /* no shape: to_shape is not read */
#define GSM_SELECT_BOX        1u
#define GSM_SELECT_ELLIPSOID  2u
#define GSM_SELECT_OUTSIDE    1u   /* flags bit 0: the complement of the shape */
typedef struct {
    uint32_t shape;            /* GSM_SELECT_ALL, _BOX or _ELLIPSOID */
    uint32_t flags;            /* 0 or GSM_SELECT_OUTSIDE */
    float    to_shape[12];     /* row-major 3x4: scene space -> the shape's unit space */
    float    opacity_min, opacity_max;  /* inclusive; (-inf, +inf): not applied */
    float    scale_min, scale_max;      /* on the largest of the three scales; inclusive; (-inf, +inf): not applied */
    uint32_t test_mask, test_value;     /* on the current state byte; (0, 0): every state */
} gsm_global_select_query;
typedef struct {
    float    min[3];   /* +inf when count == 0 */
    float    max[3];   /* -inf when count == 0 */
    uint32_t count;    /* gaussians in the keep set with three finite coordinates */
    uint32_t skipped;  /* gaussians in the keep set with a NaN or infinite coordinate: not in the box */
} gsm_global_bounds;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_select_query) == 80, "gsm_global_select_query is 80 bytes");
static_assert(sizeof(gsm_global_bounds) == 32, "gsm_global_bounds is 32 bytes");
#else
_Static_assert(sizeof(gsm_global_select_query) == 80, "gsm_global_select_query is 80 bytes");
_Static_assert(sizeof(gsm_global_bounds) == 32, "gsm_global_bounds is 32 bytes");
#endif
/* ALL, flags 0, identity rows, both ranges (-inf, +inf), test (0, 0) */
void gsm_global_select_query_default(gsm_global_select_query *q);
gsm_status gsm_global_select_where(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                   const gsm_global_select_query *query, uint8_t *state,
                                   const gsm_global_style *styles, uint32_t style_count,
                                   uint32_t and_mask, uint32_t xor_mask, uint32_t *matched /* device, nullable */);
gsm_status gsm_global_state_bounds(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                   const gsm_global_state *state, const uint32_t keep[8],
                                   gsm_global_bounds *bounds /* device */);

/* Moving a selection for good (no reference analogue): gsm_global_transform bakes a similarity -- a
 * rotation R, a uniform scale s > 0 and a translation t -- into the records and the harmonics of the gaussians of a
 * keep set, in place.  It is what a move-rotate-scale gizmo ends in; until then the same pose can be previewed as an
 * object of gsm_global_render_composite, whose pose does not rescale the gaussians while this entry does.
 *
 * gsm_global_transform_from_pose (host only, no handle) derives the descriptor.  It refuses, with
 * GSM_ERR_INVALID_ARGUMENT, a NULL pointer, a non-finite input, scale <= 0, and a rotation whose R R^T differs from
 * the identity by more than 1e-4 in any entry or whose determinant is negative.  Otherwise it works in double,
 * takes for R the rotation nearest to the nine floats (the orthogonal factor of their polar decomposition; an
 * orthonormal input is kept bit for bit) and rounds every output once to fp32: matrix = s R | t; quaternion = the unit quaternion of R with w >= 0; scale = s;
 * sh1, sh2, sh3 = the band matrices D_1, D_2, D_3 of R, D_l being the (2l+1) x (2l+1) matrix with
 *     sum_k (D_l c)_k b_k(d) = sum_k c_k b_k(R^T d)   for every coefficient vector c of band l and unit direction d,
 * b the renderer's own basis (the signs and constants of its SH evaluation).  D_l is solved once, without iteration,
 * over 2l+1 fixed directions; the identity rotation gives identity matrices exactly.
 *
 * gsm_global_transform.  The state and the keep set are gsm_global_extract's: gaussian g < gaussian_count takes part
 * when bit s_g of `keep` is set; {NULL, default_state} with a full set transforms the whole scene.  A gaussian that
 * does not take part keeps every byte, and so does every byte at or past gaussian_count.  For one that takes part,
 * every multiplication and addition below is one IEEE fp32 operation in exactly the written order, none fused; fp16
 * fields are widened exactly and rounded back once, to nearest even.  With m = desc->matrix, a = desc->quaternion:
 *   position   p'_r = ((m[r][0]*px + m[r][1]*py) + m[r][2]*pz) + m[r][3]   for each row r;
 *   scales     s'_k = s_k * desc->scale;
 *   rotation   (x, y, z, w), the Hamilton product a (x) q, not renormalised (the projection normalises):
 *                x' = ((aw*x + ax*w) + ay*z) - az*y
 *                y' = ((aw*y - ax*z) + ay*w) + az*x
 *                z' = ((aw*z + ax*y) - ay*x) + az*w
 *                w' = ((aw*w - ax*x) - ay*y) - az*z;
 *   opacity, the pad words and the band-0 coefficients: unchanged, byte for byte;
 *   harmonics  for each channel and each band l present (sh_components 4: band 1; 9: bands 1-2; 16: bands 1-3), with
 *              c the band's 2l+1 coefficients in the planar row and D = desc->sh<l> (row-major):
 *                c'_i = (...((D[i][0]*c_0 + D[i][1]*c_1) + D[i][2]*c_2)...) + D[i][2l]*c_2l.
 * With sh_components 0 or 1, harmonics is neither read nor written and may be NULL.  The descriptor is applied as
 * given: a caller who fills one by hand gets that arithmetic.  The fp16 row of 16 components is read and written as
 * six 16-byte accesses, as the projection reads it, so that harmonics pointer must be 16-byte aligned; every other
 * row needs its element's alignment and goes as 16-byte accesses where its address allows.
 *
 * The structs and `keep` are host memory, consumed before the call returns; what the scene points to is device
 * memory.  Enqueue-only on `stream`, capturable, nothing is allocated.  A captured call replays the descriptor, the
 * keep set and the pointers it was captured with and reads the state bytes of the replay; every replay applies the
 * transform again, on top of the last.  It neither reads nor changes the handle's last-frame or last-pick state.
 *
 * Checks, all before anything is enqueued; the first failing row in this order decides:
 *   GSM_ERR_INVALID_ARGUMENT         renderer NULL;
 *   GSM_ERR_INVALID_GAUSSIAN_COUNT   gaussian_count > max_gaussians (the count of a NULL scene cannot be read: that
 *                                    call falls to the next row);
 *   GSM_ERR_MISSING_REQUIRED_BUFFER  scene, state, keep or desc NULL; with a count > 0: scene->gaussians NULL, or
 *                                    scene->harmonics NULL while sh_components > 1;
 *   GSM_ERR_INVALID_BUFFER_SIZE      scene->gaussians not 16-byte aligned; with sh_components > 1, scene->harmonics
 *                                    not aligned to its element (2 or 4 bytes; 16 bytes for fp16 rows of 16);
 *   GSM_ERR_INVALID_ARGUMENT         default_state > 255; sh_components not in {0, 1, 4, 9, 16}; a non-finite entry
 *                                    of the descriptor; desc->scale <= 0; the records' and the harmonics' byte ranges
 *                                    meeting.
 * A count of 0 is a no-op.
 *
 * Out of scope: a non-uniform scale or a shear (the record cannot hold the result), transforms out of place, merging
 * scenes, a centroid, and the DepthFirst, Local and multi-GPU renderers. */
typedef struct {            /* the mutable twin of gsm_gaussian_input */
    void *gaussians;
    void *harmonics;
    uint32_t gaussian_count;
    uint32_t sh_components;
} gsm_global_scene;
typedef struct {
    float matrix[12];       /* row-major 3x4: s*R | t, scene space -> scene space */
    float quaternion[4];    /* x, y, z, w of R, unit */
    float scale;            /* s > 0 */
    float sh1[9], sh2[25], sh3[49];  /* row-major band matrices D_1, D_2, D_3 of R */
} gsm_global_transform_desc;
#ifdef __cplusplus
static_assert(sizeof(gsm_global_scene) == 24, "gsm_global_scene is 24 bytes");
static_assert(sizeof(gsm_global_transform_desc) == 400, "gsm_global_transform_desc is 400 bytes");
#else
_Static_assert(sizeof(gsm_global_scene) == 24, "gsm_global_scene is 24 bytes");
_Static_assert(sizeof(gsm_global_transform_desc) == 400, "gsm_global_transform_desc is 400 bytes");
#endif
gsm_status gsm_global_transform_from_pose(const float rotation[9] /* row-major */, float scale,
                                          const float translation[3], gsm_global_transform_desc *out);
gsm_status gsm_global_transform(gsm_renderer *renderer, void *stream, const gsm_global_scene *scene,
                                const gsm_global_state *state, const uint32_t keep[8],
                                const gsm_global_transform_desc *desc);

/* GlobalRenderer.renderStereo (GlobalRenderer.swift:240-255) calls fatalError for
 * every target; this entry returns GSM_ERR_UNSUPPORTED instead. */
gsm_status gsm_global_render_stereo(gsm_renderer *renderer, void *stream,
                                    const gsm_gaussian_input *input,
                                    const gsm_camera_params *left, const gsm_camera_params *right,
                                    uint32_t width_per_eye, uint32_t height, void *color_rgba16f,
                                    size_t color_pitch_bytes, void *depth_r16f,
                                    size_t depth_pitch_bytes);

/* Config 5: both eyes of a stereo pair through the Global
 * path into one side-by-side target -- left eye in columns [0, width_per_eye), right eye in
 * [width_per_eye, 2 * width_per_eye) of rows of color_pitch bytes.  Each half equals
 * gsm_global_render of that eye (the two views are independent Global frames; the
 * DepthFirst renderer's shared-colour stereo semantics are not reproduced).  width_per_eye
 * is bounded by config.max_width. */
gsm_status gsm_global_render_stereo_sbs(gsm_renderer *renderer, void *stream,
                                        const gsm_gaussian_input *input,
                                        const gsm_camera_params *left, const gsm_camera_params *right,
                                        uint32_t width_per_eye, uint32_t height, void *color_rgba16f,
                                        size_t color_pitch_bytes, void *depth_r16f,
                                        size_t depth_pitch_bytes);

/* GlobalRenderer.debugReadTotalAssignments() (GlobalRenderer.swift:196-199): reads
 * the GPU counter; call after the frame's stream work has completed. */
uint32_t gsm_global_debug_read_total_assignments(gsm_renderer *renderer);

/* GaussianRenderer.lastGPUTime (GaussianRendererProtocol.swift:245, declared but
 * never assigned in the reference).  Seconds of the last frame measured with HIP
 * events when profiling is enabled (gsm_debug.h); returns GSM_ERR_RENDER_FAILED
 * when no measurement is available. */
gsm_status gsm_global_last_gpu_time(gsm_renderer *renderer, double *seconds);

const char *gsm_status_string(gsm_status status);
int gsm_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif

/*
 * gsm_debug.h -- introspection, stage profiling, multi-GPU slab control and
 * stand-alone sort for libgsm_amd.so.
 *
 * The reference exposes its intermediate buffers to its own tests through
 * `@testable import Renderer` (Tests/RendererTests/GlobalUnitTests.swift:2) and
 * per-view resources (GlobalResources.swift:6-362); these entry points are the
 * C-ABI equivalent used by the parity tests and the benchmark.  All readbacks
 * are synchronous host copies: call them after the frame's stream work is done.
 */
#ifndef GSM_DEBUG_H
#define GSM_DEBUG_H

#include "gsm_renderer.h"

#ifdef __cplusplus
extern "C" {
#endif

/* TileAssignmentHeader (BridgingTypes.h:99-104) + derived frame counters. */
typedef struct {
    uint32_t total_assignments; /* after the clamp to max_capacity */
    uint32_t max_capacity;      /* 4 * max_gaussians */
    uint32_t padded_count;      /* roundup(total, 1024) (GlobalShaders.metal:711-712) */
    uint32_t overflow;          /* 1 when the clamp fired (GlobalShaders.metal:697-701) */
    uint32_t tiles_x, tiles_y, tile_count;
    uint32_t gaussian_count;    /* of the last frame */
} gsm_debug_counters;

/* Buffers that can be copied back (reference resource named in brackets). */
typedef enum {
    GSM_BUF_RENDER_DATA = 0,   /* GaussianRenderData[count], 16 B each [interleavedGaussians]; kept only
                                  by captured frames (profiling bit 1 or 4; else
                                  GSM_ERR_MISSING_REQUIRED_BUFFER): the blend reads its own records */
    GSM_BUF_BOUNDS = 1,        /* int32[count][4] minTX,maxTX,minTY,maxTY [boundsCache] */
    GSM_BUF_TILE_COUNTS = 2,   /* uint32[count] tiles per gaussian [coverageBuffer] */
    GSM_BUF_KEYS = 3,          /* uint32[total] unsorted sort keys [sortKeys before sort] */
    GSM_BUF_VALUES = 4,        /* int32[total] unsorted gaussian ids [tileIndices] */
    GSM_BUF_SORTED_KEYS = 5,   /* uint32[total] [sortKeys after sort]; captured frames only (as
                                  RENDER_DATA): the blend walks per-half-tile lists instead */
    GSM_BUF_SORTED_VALUES = 6, /* int32[total] [sortedIndices]; captured frames only */
    GSM_BUF_HEADERS = 7,       /* GaussianHeader[tile_count] {offset,count} [orderedHeaders] */
    GSM_BUF_EXP_TABLE = 8,     /* uint16[65536] blend exp table indexed by fp16 quad-form bits */
    GSM_BUF_BLEND_TRACE = 9    /* uint64[blend units][4] {start, end (100 MHz ticks), count<<32 | entries
                                  walked, XCC_ID<<32 | HW_ID} of the last profiled frame (bit 2) */
} gsm_buffer_id;

gsm_status gsm_global_debug_counters(gsm_renderer *renderer, gsm_debug_counters *out);

/* The blend kernel the last enqueued frame launched (host-side choice, no sync): k_blend_px with
 * 16x8 quadrant units (small frames and multi-GPU slabs), k_blend_px with 16x16 half-tile units, or
 * the pair walk k_blend_pw (>= 6 half-tile units per wave slot on one GPU).  The benchmark attributes
 * its blend roofline and PMC counters to this kernel. */
typedef enum {
    GSM_BLEND_KERNEL_NONE = 0,
    GSM_BLEND_KERNEL_QUADRANT = 1,
    GSM_BLEND_KERNEL_HALF_TILE = 2,
    GSM_BLEND_KERNEL_PAIR_WALK = 3
} gsm_blend_kernel;
gsm_status gsm_global_debug_blend_kernel(gsm_renderer *renderer, int *kind);
/* Copies up to `bytes` of buffer `which` into host memory; *needed receives the full size. */
gsm_status gsm_global_debug_copy(gsm_renderer *renderer, int which, void *host_dst, size_t bytes,
                                 size_t *needed);
/* `enable` is a bit set: bit 0 brackets every stage by HIP events on the frame's stream,
 * bit 1 keeps the unsorted keys (GSM_BUF_KEYS/VALUES) for readback and captures (bit 4),
 * bit 4 captures the reference's intermediates the product path does not write
 * (GSM_BUF_RENDER_DATA, GSM_BUF_SORTED_KEYS/VALUES; the frame costs their writes), bit 2 records a
 * per-unit blend trace (GSM_BUF_BLEND_TRACE), bit 3 (without bit 0) brackets only the blend
 * (two events per frame; the other stages then report 0); bits 8-15, with bit 3: a period P > 1
 * brackets the blend on every P-th frame only (the average is over the bracketed frames).
 * Every event costs frame time (~10 us per bracketed frame at config 2). */
gsm_status gsm_global_set_profiling(gsm_renderer *renderer, int enable);

enum {
    GSM_STAGE_PROJECT = 0, /* project + cull + SH + tile count */
    GSM_STAGE_SCAN = 1,    /* prefix scan of tile counts */
    GSM_STAGE_SCATTER = 2, /* duplicate-with-keys */
    GSM_STAGE_SORT = 3,    /* radix sort */
    GSM_STAGE_HEADERS = 4, /* tile headers */
    GSM_STAGE_BLEND = 5,   /* clear + front-to-back blend */
    GSM_STAGE_COUNT = 6
};
/* Milliseconds of each stage of the last profiled frame (after stream sync). */
gsm_status gsm_global_stage_times(gsm_renderer *renderer, float *ms, int n);

/* Multi-GPU screen-slab partition: restrict tile assignment,
 * sort, headers and blend to tile rows [row_begin, row_end).  Pixels outside the
 * slab are not written.  (0, 0) restores the full frame. */
gsm_status gsm_global_set_tile_rows(gsm_renderer *renderer, uint32_t row_begin, uint32_t row_end);

/* Stable LSD radix sort of n (uint32 key, uint32 value) pairs in device memory,
 * in place, `key_bits` low key bits significant (the RadixSortEncoder unit-test
 * surface, GlobalUnitTests.swift:23-178).  Allocates its scratch; synchronises
 * `stream` before returning. */
gsm_status gsm_sort_pairs_u32(void *keys, void *values, uint32_t n, uint32_t key_bits, void *stream);

/* The create-time device probe behind the sorts' stable ranks: *lane_ordered = 1 when the lanes
 * of one ds_add_rtn_u32 that hit the same LDS address on `hip_device` receive their old values in
 * lane order (the sorts then rank with one LDS atomic per key), 0 when they do not (ranks from
 * ballot matches).  GSM_SORT_RANK=ballot in the environment at create forces the ballot ranks.
 * Cached per device and process; no reference counterpart (a gfx950 design choice). */
gsm_status gsm_debug_sort_rank_probe(int hip_device, int *lane_ordered);

/* The sorts' workspace guard (host only, no device call): the digit-count workspace bytes every
 * renderer allocates for a sort of `capacity` keys, and whether the passes the LSD sort plans for
 * `key_bits` bits (wide 9..11-bit digits allowed or not) fit `hist_bytes` of it -- GSM_OK, or
 * GSM_ERR_INVALID_ASSIGNMENT_CAPACITY, the status a frame whose sort would overrun its workspace
 * returns before launching any of its passes (an undersized histogram workspace faulted an r05
 * A/B build). */
size_t gsm_debug_sort_workspace_bytes(uint32_t capacity);
gsm_status gsm_debug_sort_plan_fits(uint32_t capacity, uint32_t key_bits, int wide, size_t hist_bytes);

/* The production frame sort on caller keys (debug only): the tile passes whose last pass writes
 * the tile starts -- what a Global or DepthFirst frame runs after its scatter -- and, when asked, the per-tile
 * depth sort with its half-tile lists.  A handle owns what a renderer owns for the sort: two key and two value
 * buffers of `capacity` words, the device count word, the digit-count workspace (zeroed once, at create; it
 * persists between runs like a renderer's), the digit totals, the low-digit buckets, tileStart[max_tiles + 1],
 * the two half lists and halfCount[2 * max_tiles].  GSM_SORT_RANK, GSM_SORT_WIDE and GSM_SORT_SCAN are read
 * from the environment at create, as by a renderer.  hip_device < 0: the current device.
 * create: GSM_ERR_INVALID_ASSIGNMENT_CAPACITY for capacity 0, GSM_ERR_INVALID_TILE_COUNT for max_tiles 0 or above
 * 524,288 (19 bits: one wide pass + one 8-bit pass). */
typedef struct gsm_debug_frame_sort gsm_debug_frame_sort;

typedef struct {
    uint32_t shift;      /* the tile field's first bit: 16 (Global keys, tile << 16 | depth16) or 0 (DepthFirst
                            instance keys: the tile alone) */
    uint32_t num_tiles;  /* the frame's tiles: every key's tile field is below it (1 .. all_tiles) */
    uint32_t all_tiles;  /* the configuration's tiles (<= max_tiles; <= 65,536 with shift 16) */
    uint32_t depth_sort; /* 1: the depth sort of tiles [0, num_tiles) after the tile passes (shift 16 only) */
    uint32_t full;       /* 1: the depth sort also writes the sorted keys and values (captured frames) */
    uint32_t reserved;   /* 0 */
} gsm_debug_frame_sort_desc;

/* The passes a run took (chosen by all_tiles, num_tiles and GSM_SORT_WIDE). */
typedef enum {
    GSM_FRAME_SORT_ONE_NARROW = 1,      /* <= 256 tiles: one pass of 4..8 bits */
    GSM_FRAME_SORT_TWO_NARROW = 2,      /* <= 65,536 tiles: two passes of 4..8 bits each */
    GSM_FRAME_SORT_ONE_WIDE = 3,        /* > 256 tiles, num_tiles <= 2048: one pass of 9..11 bits */
    GSM_FRAME_SORT_WIDE_THEN_NARROW = 4 /* > 65,536 tiles: 9..11 bits, then 8 bits over up to 2048 buckets */
} gsm_frame_sort_plan;

/* Host destinations, each optional (NULL: not copied). */
typedef struct {
    uint32_t *sorted_keys;   /* [n]; after a depth sort with full = 0 their content is not specified */
    uint32_t *sorted_values; /* [n]; as sorted_keys */
    uint32_t *tile_start;    /* [all_tiles + 1] */
    uint32_t *half0, *half1; /* [n]: tile t's kept ids from tile_start[t]; written by a depth sort only */
    uint32_t *half_count;    /* [2 * all_tiles]: half h of tile t at h * all_tiles + t, for t < num_tiles;
                                written by a depth sort only */
    uint32_t plan;           /* out: gsm_frame_sort_plan */
    uint32_t reserved;       /* 0 */
} gsm_debug_frame_sort_out;

gsm_status gsm_debug_frame_sort_create(uint32_t capacity, uint32_t max_tiles, int hip_device,
                                       gsm_debug_frame_sort **out);
void gsm_debug_frame_sort_destroy(gsm_debug_frame_sort *sorter);
/* Copies the n <= capacity device pairs (keys, values: device memory, read only) into the handle, writes n to
 * the device count word, runs the tile passes (and the depth sort), copies the results out and synchronises
 * `stream`.  The value word's bits 30 and 31 are the half-tile skip flags, the bits below the id the half lists
 * hold.  Before the depth sort the tile starts are read back and checked (non-decreasing, at most n): starts that
 * are not end the run with GSM_ERR_RENDER_FAILED, the depth sort not launched -- its workgroups index the runs by
 * them.  GSM_ERR_INVALID_ARGUMENT: n > capacity, a shift other than 0 or 16, depth_sort without shift 16,
 * num_tiles = 0 or > all_tiles, all_tiles > max_tiles (> 65,536 with shift 16);
 * GSM_ERR_INVALID_ASSIGNMENT_CAPACITY: the plan does not fit the workspace (nothing launched). */
gsm_status gsm_debug_frame_sort_run(gsm_debug_frame_sort *sorter, void *stream,
                                    const gsm_debug_frame_sort_desc *desc, const void *keys, const void *values,
                                    uint32_t n, gsm_debug_frame_sort_out *out);

/* The device steps of gsm_multigpu_render (gsm_multigpu.h) without RCCL, so W virtual ranks can run
 * the native exchange in one process on one GPU (tests): the caller plays the collectives --
 * gathers every rank's per-slab counts into the W x W matrix (row r = rank r) on the device and
 * orders the pushes before the renders by stream order.
 *   partition_counts: project ids [first, first + count) and count the records per slab
 *     (slab_rows: num_slabs + 1 tile-row boundaries) into d_send_counts (device, num_slabs words);
 *   partition_push: write every record of the last partition_counts straight into its slab
 *     owner's receive buffer (recv_buffers: host array of `world` device pointers, each holding
 *     GSM_SPLAT_RECORD_BYTES x max_gaussians) at the offset the count matrix d_counts gives;
 *     d_recv_count (device) receives this rank's incoming record count;
 *   render_records_device_count: gsm_global_render_records with the record count read on the
 *     device (d_count) and `capacity` records the grids cover. */
gsm_status gsm_debug_partition_counts(gsm_renderer *renderer, void *stream, const gsm_gaussian_input *input,
                                      const gsm_camera_params *camera, uint32_t width, uint32_t height,
                                      uint32_t first, uint32_t count, const uint32_t *slab_rows,
                                      uint32_t num_slabs, uint32_t *d_send_counts);
gsm_status gsm_debug_partition_push(gsm_renderer *renderer, void *stream, uint32_t world, uint32_t rank,
                                    const uint32_t *d_counts, void *const *recv_buffers, uint32_t *d_recv_count);
gsm_status gsm_debug_render_records_device_count(gsm_renderer *renderer, void *stream, const void *records,
                                                 uint32_t capacity, const uint32_t *d_count, uint32_t width,
                                                 uint32_t height, void *color, size_t color_pitch, void *depth,
                                                 size_t depth_pitch);

#ifdef __cplusplus
}
#endif
#endif

// gsm_local_internal.h -- device buffers, kernel arguments and launchers of the LocalRenderer frame
// (gsm_local_kernels.hip; host orchestration and C ABI in gsm_local.hip, include/gsm_local.h).
// Reference: Sources/Renderer/LocalRenderer/ (LocalRenderer.swift:83-257, LocalShaders.metal).
// DESIGN.md 13.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsm_internal.h"
#include "gsm_types.h"

namespace gsm {

constexpr uint32_t kLocalTile = 16;         // LocalRenderer.swift tileWidth / tileHeight
constexpr uint32_t kLocalMaxPerTile = 2048;  // LocalRenderer.maxPerTile (SORT_MAX_SIZE_16, LocalShaders.metal:353)
constexpr int kLocalBlock = 256;

// ProjectedGaussian (BridgingTypes.h:106-114), 32 B: two 16-byte words.
//   a.x = posX | posY << 16     a.y = conicA | conicB << 16  a.z = conicC | depth << 16
//   a.w = colorR | colorG << 16 b.x = colorB | opacity << 16 b.y = minTile.x | minTile.y << 16
//   b.z = maxTile.x | maxTile.y << 16 (exclusive; 0 marks a culled record of the uncompacted buffer)
//   b.w = obbExtentX | obbExtentY << 16
struct LocalProjected {
    uint4 a, b;
};
static_assert(sizeof(LocalProjected) == 32, "ProjectedGaussian must be 32 B");

// CameraUniforms + TileBinningParams of one frame (LocalRenderer.swift:147-167) with the uniform terms
// of projectCovariance2D / stabilizeCovariance2D / computeDepthFactor evaluated once on the host.
struct LocalArgs {
    float view[16], proj[16];
    float limX, limY, focalX, focalY;
    float width, height, nearPlane, farPlane;
    float maxEig, adjFar, adjDen;
    float camPos[3];
    float inputIsSRGB;
    uint32_t shComponents, count, tilesX, tilesY, tileCount;
};

// per-frame device counters (gsm_local_debug_counters)
struct LocalStats {
    uint32_t activeTiles;   // tiles with a nonzero count
    uint32_t totalEntries;  // sum of min(count, 2048)
    uint32_t maxTileCount;  // largest unclamped count
    uint32_t pad;
};

// The LocalViewResources analogue, sized at create time.
struct LocalArena {
    LocalProjected* temp = nullptr;       // [maxG] tempProjection
    LocalProjected* compacted = nullptr;  // [maxG] compactedGaussians
    uint32_t* blockSums = nullptr;        // [ceil(maxG / 256) + 1] visible counts per block, then offsets
    TileAssignmentHeader* visHdr = nullptr;  // totalAssignments = visibleCount
    uint32_t* queue = nullptr;            // the scan's side output (not read by this frame)
    uint32_t* tileCounts = nullptr;       // [maxTiles] unclamped
    uint16_t* depthKeys = nullptr;        // [maxTiles * 2048] depthKeys16
    uint32_t* slotIndices = nullptr;      // [maxTiles * 2048] compacted index of each slot (sortIndices)
    uint16_t* sortedLocal = nullptr;      // [maxTiles * 2048] sortedLocalIdx
    uint32_t* lists = nullptr;            // [maxTiles * 2048] compacted indices in blend order
    LocalStats* stats = nullptr;
    uint16_t* expTable = nullptr;         // [65536] the Global blend's alpha table (blend_exp_table_entry)
};

// localClear (LocalShaders.metal:10-25): tile counters and frame counters
void local_launch_clear(const LocalArgs& a, const LocalArena& A, hipStream_t stream);
// localProjectStore (:53-184) + per-block visible counts
void local_launch_project(bool halfInput, uint32_t shDegree, const void* world, const void* harmonics,
                          const LocalArgs& a, const LocalArena& A, hipStream_t stream);
// localCompact (:201-214): ascending gaussian order (A.blockSums scanned by launch_scan_sums before)
void local_launch_compact(const LocalArgs& a, const LocalArena& A, hipStream_t stream);
// localScatterSimd16 (:573-667)
void local_launch_scatter(const LocalArgs& a, const LocalArena& A, hipStream_t stream);
// localPerTileSort16 (:362-437) by (depth16, compacted index, slot); stats / lists may be null
void local_launch_sort(const uint16_t* keys16, const uint32_t* indices, const uint32_t* counts, uint32_t tileCount,
                       uint32_t maxPerTile, uint16_t* sortedLocal, uint32_t* lists, LocalStats* stats,
                       hipStream_t stream);
// localClearTextures + localRender16 (:27-39, :440-571) over every tile; depth may be null
void local_launch_blend(const LocalArgs& a, const LocalArena& A, void* color, size_t pitch, int colorFormat,
                        void* depth, size_t depthPitch, int numCUs, hipStream_t stream);

}  // namespace gsm

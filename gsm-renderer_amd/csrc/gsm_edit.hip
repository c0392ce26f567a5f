// gsm_edit.hip -- gfx950 kernels of the Global renderer's scene-editing entries:
// gsm_global_extract, a stable compaction of a scene's rows by its state bytes, and gsm_global_state_histogram.
// No reference analogue.  Nothing here computes: rows are copied byte for byte.
//
// The extract is three launches in stream order and the launch boundary is the only barrier between workgroups:
// no kernel here waits for another workgroup (no look-back, no flag, no ticket).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gsm_device.h"
#include "gsm_internal.h"

namespace gsm {

constexpr uint32_t kEditBlock = 256;

// bit s of the keep set, without indexing the kernel argument by a lane's value
__device__ __forceinline__ bool keep_has(const KeepSet& keep, uint32_t s) {
    uint32_t w = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) w = (s >> 5) == k ? keep.w[k] : w;
    return ((w >> (s & 31u)) & 1u) != 0;
}

// this thread's gaussian of the block: its state and whether it is kept (false at or past count)
__device__ __forceinline__ bool thread_kept(const uint8_t* __restrict__ state, uint32_t defaultState, uint32_t count,
                                            const KeepSet& keep, uint32_t* s) {
    const uint32_t g = blockIdx.x * kEditBlock + threadIdx.x;
    *s = defaultState;
    if (g >= count) return false;
    if (state) *s = state[g];
    return keep_has(keep, *s);
}

// launch 1: per block of 256 gaussians, the number kept, from the four waves' ballots
__global__ __launch_bounds__(kEditBlock) void k_extract_count(const uint8_t* __restrict__ state, uint32_t defaultState,
                                                              uint32_t count, KeepSet keep,
                                                              uint32_t* __restrict__ blockCounts) {
    __shared__ uint32_t waveCount[kEditBlock / 64];
    uint32_t s;
    const bool kept = thread_kept(state, defaultState, count, keep, &s);
    const unsigned long long b = __ballot(kept);
    if ((threadIdx.x & 63u) == 0) waveCount[threadIdx.x >> 6] = (uint32_t)__popcll(b);
    __syncthreads();
    if (threadIdx.x == 0) blockCounts[blockIdx.x] = waveCount[0] + waveCount[1] + waveCount[2] + waveCount[3];
}

// launch 2: one workgroup turns the block counts into their exclusive scan, in place, 1024 counts a round with a
// running carry, and writes the total to *kept (blocks == 0: just that)
__global__ __launch_bounds__(kEditBlock) void k_extract_scan(uint32_t* __restrict__ blockCounts, uint32_t blocks,
                                                             uint32_t* __restrict__ kept) {
    __shared__ uint32_t lds[kEditBlock / 64];
    uint32_t carry = 0;
    for (uint32_t c = 0; c < blocks; c += 4u * kEditBlock) {  // (uniform)
        const uint32_t i = c + 4u * threadIdx.x;
        uint32_t v[4], sum = 0;
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            v[k] = i + k < blocks ? blockCounts[i + k] : 0u;
            sum += v[k];
        }
        uint32_t total;
        uint32_t off = carry + block_exclusive_scan<(int)kEditBlock>(sum, lds, &total);
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (i + k < blocks) blockCounts[i + k] = off;
            off += v[k];
        }
        carry += total;
    }
    if (threadIdx.x == 0) *kept = carry;
}

template <int W> struct Chunk;
template <> struct Chunk<16> { using type = uint4; };
template <> struct Chunk<8> { using type = uint2; };
template <> struct Chunk<4> { using type = uint32_t; };
template <> struct Chunk<2> { using type = uint16_t; };
template <> struct Chunk<1> { using type = uint8_t; };

// `rows` kept rows of the block, W bytes a chunk: all 256 lanes walk (row, chunk) pairs, so consecutive lanes store
// consecutive chunks of output rows dstRow0 .. dstRow0 + rows, which are contiguous.  Row j comes from input row
// srcRow0 + ids[j] (ids: the block's kept local ids, in LDS).  Every byte offset is 64-bit.
template <int W>
__device__ __forceinline__ void copy_rows(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t rowBytes,
                                          uint32_t srcRow0, uint32_t dstRow0, uint32_t rows, const uint8_t* ids) {
    using T = typename Chunk<W>::type;
    const uint64_t chunks = rowBytes / (uint64_t)W;
    if (chunks <= 0xFFFFu) {
        const uint32_t cpr = (uint32_t)chunks, pairs = rows * cpr;  // (rows <= 256: below 2^24)
        for (uint32_t p = threadIdx.x; p < pairs; p += kEditBlock) {
            const uint32_t j = p / cpr, c = p - j * cpr;
            const uint64_t from = (uint64_t)(srcRow0 + ids[j]) * rowBytes + (uint64_t)c * W;
            const uint64_t to = ((uint64_t)dstRow0 + j) * rowBytes + (uint64_t)c * W;
            *(T*)(dst + to) = *(const T*)(src + from);
        }
    } else {  // (rows wider than any scene's: row by row)
        for (uint32_t j = 0; j < rows; ++j) {
            const uint64_t from = (uint64_t)(srcRow0 + ids[j]) * rowBytes, to = ((uint64_t)dstRow0 + j) * rowBytes;
            for (uint64_t c = threadIdx.x; c < chunks; c += kEditBlock)
                *(T*)(dst + to + c * W) = *(const T*)(src + from + c * W);
        }
    }
}

__device__ __forceinline__ void copy_rows_w(uint32_t w, const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                            uint64_t rowBytes, uint32_t srcRow0, uint32_t dstRow0, uint32_t rows,
                                            const uint8_t* ids) {
    switch (w) {  // (uniform)
        case 16: copy_rows<16>(src, dst, rowBytes, srcRow0, dstRow0, rows, ids); break;
        case 8: copy_rows<8>(src, dst, rowBytes, srcRow0, dstRow0, rows, ids); break;
        case 4: copy_rows<4>(src, dst, rowBytes, srcRow0, dstRow0, rows, ids); break;
        case 2: copy_rows<2>(src, dst, rowBytes, srcRow0, dstRow0, rows, ids); break;
        default: copy_rows<1>(src, dst, rowBytes, srcRow0, dstRow0, rows, ids); break;
    }
}

// launch 3: the move.  The block finds its kept gaussians again (one state byte each), ranks them by ballot prefix
// and lists their local ids in LDS; its rows land at output rows base .. base + n, base from the scan.  Ranks at or
// past the capacity are not stored; a block without a kept gaussian does nothing.
// recordChunk / harmonicsChunk: the widest power of two <= 16 that divides both sides' addresses and the row.
__global__ __launch_bounds__(kEditBlock) void k_extract_move(ExtractArgs a, uint32_t recordChunk,
                                                             uint32_t harmonicsChunk) {
    __shared__ uint32_t waveCount[kEditBlock / 64];
    __shared__ uint8_t ids[kEditBlock];
    __shared__ uint8_t states[kEditBlock];
    uint32_t s;
    const bool kept = thread_kept(a.state, a.defaultState, a.count, a.keep, &s);
    const unsigned long long b = __ballot(kept);
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (lane == 0) waveCount[wave] = (uint32_t)__popcll(b);
    __syncthreads();
    uint32_t before = 0, n = 0;
#pragma unroll
    for (uint32_t w = 0; w < kEditBlock / 64; ++w) {
        const uint32_t c = waveCount[w];
        if (w < wave) before += c;
        n += c;
    }
    if (n == 0) return;  // (uniform)
    if (kept) {
        const uint32_t rank = before + (uint32_t)__popcll(b & ((1ull << lane) - 1ull));
        ids[rank] = (uint8_t)threadIdx.x;
        states[rank] = (uint8_t)s;
    }
    __syncthreads();
    const uint32_t base = a.blockBase[blockIdx.x];
    if (base >= a.capacity) return;  // (uniform)
    const uint32_t rows = min(n, a.capacity - base), row0 = blockIdx.x * kEditBlock;
    copy_rows_w(recordChunk, a.records, a.outRecords, a.recordBytes, row0, base, rows, ids);
    if (a.harmonicsBytes)
        copy_rows_w(harmonicsChunk, a.harmonics, a.outHarmonics, a.harmonicsBytes, row0, base, rows, ids);
    if (threadIdx.x < rows) {
        const uint64_t j = (uint64_t)base + threadIdx.x;
        if (a.outState) a.outState[j] = states[threadIdx.x];
        if (a.outIds) a.outIds[j] = row0 + ids[threadIdx.x];
    }
}

// gsm_global_state_histogram, launch 1: the 256 words start from 0
__global__ __launch_bounds__(256) void k_state_histogram_clear(uint32_t* __restrict__ histogram) {
    histogram[threadIdx.x] = 0u;
}

// launch 2: per-workgroup LDS bins over a grid-stride walk of the bytes, four a load where the
// address allows (the unaligned head and the tail are block 0's), then one atomic add per non-empty bin.
__global__ __launch_bounds__(kEditBlock) void k_state_histogram(const uint8_t* __restrict__ state, uint32_t count,
                                                                uint32_t* __restrict__ histogram) {
    __shared__ uint32_t bins[256];
    bins[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t head = min(count, (uint32_t)((0u - (uint32_t)(uintptr_t)state) & 3u));
    const uint32_t words = (count - head) / 4u, tail0 = head + 4u * words;
    const uint32_t* __restrict__ w32 = (const uint32_t*)(state + head);
    for (uint32_t i = blockIdx.x * kEditBlock + threadIdx.x; i < words; i += gridDim.x * kEditBlock) {
        const uint32_t w = w32[i];
        atomicAdd(&bins[w & 0xFFu], 1u);
        atomicAdd(&bins[(w >> 8) & 0xFFu], 1u);
        atomicAdd(&bins[(w >> 16) & 0xFFu], 1u);
        atomicAdd(&bins[w >> 24], 1u);
    }
    if (blockIdx.x == 0) {
        if (threadIdx.x < head) atomicAdd(&bins[state[threadIdx.x]], 1u);
        if (threadIdx.x < count - tail0) atomicAdd(&bins[state[tail0 + threadIdx.x]], 1u);
    }
    __syncthreads();
    const uint32_t v = bins[threadIdx.x];
    if (v) atomicAdd(&histogram[threadIdx.x], v);
}

// the widest chunk (a power of two, at most 16 bytes) that both addresses and the row width are multiples of
static uint32_t chunk_width(const void* src, const void* dst, uint64_t rowBytes) {
    const uint64_t x = (uint64_t)(uintptr_t)src | (uint64_t)(uintptr_t)dst | rowBytes | 16u;
    return (uint32_t)(x & (0 - x));
}

void launch_extract(const ExtractArgs& a, uint32_t* kept, hipStream_t s) {
    const uint32_t blocks = (a.count + kEditBlock - 1u) / kEditBlock;
    if (blocks)
        hipLaunchKernelGGL(k_extract_count, dim3(blocks), dim3(kEditBlock), 0, s, a.state, a.defaultState, a.count,
                           a.keep, a.blockBase);
    hipLaunchKernelGGL(k_extract_scan, dim3(1), dim3(kEditBlock), 0, s, a.blockBase, blocks, kept);
    if (blocks == 0 || a.capacity == 0) return;
    hipLaunchKernelGGL(k_extract_move, dim3(blocks), dim3(kEditBlock), 0, s, a,
                       chunk_width(a.records, a.outRecords, a.recordBytes),
                       chunk_width(a.harmonics, a.outHarmonics, a.harmonicsBytes));
}

void launch_state_histogram(const uint8_t* state, uint32_t count, uint32_t* histogram, hipStream_t s) {
    // overwritten, not added to (a kernel, not a memset node: a replayed graph zeroes the words the same way)
    hipLaunchKernelGGL(k_state_histogram_clear, dim3(1), dim3(256), 0, s, histogram);
    if (count == 0) return;
    const uint32_t grid = std::min(std::max((count / 4u + 2047u) / 2048u, 1u), 1024u);
    hipLaunchKernelGGL(k_state_histogram, dim3(grid), dim3(kEditBlock), 0, s, state, count, histogram);
}

}  // namespace gsm

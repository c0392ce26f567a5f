// gsm_edit.hip -- gfx950 kernels of the Global renderer's scene-editing entries:
// gsm_global_extract, a stable compaction of a scene's rows by its state bytes, gsm_global_state_histogram,
// gsm_global_select_where, a select by a world-space and attribute predicate, gsm_global_state_bounds, the box
// of a keep set, and gsm_global_transform, which bakes a pose into the rows of a keep set.  No reference analogue.
// The extract copies rows byte for byte; the select's only arithmetic is the nine products and nine sums of its shape
// test, unfused (-ffp-contract=off), the bounds only compare, and the transform applies given fp32 matrices in the
// order the header writes down, unfused.
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

// gsm_global_select_where: *matched starts from 0 (a kernel, not a memset node, as k_state_histogram_clear)
__global__ __launch_bounds__(64) void k_select_where_clear(uint32_t* __restrict__ matched) {
    if (threadIdx.x == 0) *matched = 0u;
}

// gsm_global_select_where: one thread per gaussian.  The record's first 32 bytes (fp32: two 16-byte
// loads; the quaternion is not read) or first 20 (fp16: one 16-byte and one 4-byte load) give the position, the
// opacity and the scales; the state byte is loaded and stored by its own thread alone.  The query is a kernel
// argument, so the shape and the two range switches are scalar branches.  One ballot count per wave, one integer
// add per workgroup with a match.
template <bool HALF>
__global__ __launch_bounds__(kEditBlock) void k_select_where(const void* __restrict__ world, SelectWhereArgs q,
                                                             uint8_t* __restrict__ state,
                                                             const uint2* __restrict__ styleTable,
                                                             uint32_t* __restrict__ matched) {
    __shared__ uint32_t waveCount[kEditBlock / 64];
    const uint32_t g = blockIdx.x * kEditBlock + threadIdx.x;
    bool match = false;
    if (g < q.count) {
        float px, py, pz, o, sx, sy, sz;
        if constexpr (HALF) {
            const uint8_t* rec = (const uint8_t*)world + (size_t)g * sizeof(PackedWorldGaussianHalf);
            const uint4 w0 = *(const uint4*)rec;
            const uint32_t w1 = *(const uint32_t*)(rec + 16);
            px = __builtin_bit_cast(float, w0.x);
            py = __builtin_bit_cast(float, w0.y);
            pz = __builtin_bit_cast(float, w0.z);
            o = hbits_to_f((uint16_t)(w0.w & 0xFFFFu));
            sx = hbits_to_f((uint16_t)(w0.w >> 16));
            sy = hbits_to_f((uint16_t)(w1 & 0xFFFFu));
            sz = hbits_to_f((uint16_t)(w1 >> 16));
        } else {
            const float4* wp = (const float4*)((const PackedWorldGaussian*)world + g);
            const float4 w0 = wp[0], w1 = wp[1];
            px = w0.x; py = w0.y; pz = w0.z; o = w0.w;
            sx = w1.x; sy = w1.y; sz = w1.z;
        }
        const uint32_t old = state[g];
        match = (old & q.testMask) == q.testValue;
        if (styleTable && ((styleTable[old].y >> 8) & 0xFFu)) match = false;  // hidden: not selectable
        if (q.shape != GSM_SELECT_ALL) {  // (uniform)
            float v[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) v[r] = ((q.A[4 * r] * px + q.A[4 * r + 1] * py) + q.A[4 * r + 2] * pz) + q.A[4 * r + 3];
            bool inside;
            if (q.shape == GSM_SELECT_BOX)  // (uniform)
                inside = __builtin_fabsf(v[0]) <= 1.0f && __builtin_fabsf(v[1]) <= 1.0f && __builtin_fabsf(v[2]) <= 1.0f;
            else
                inside = ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) <= 1.0f;
            const bool nan = v[0] != v[0] || v[1] != v[1] || v[2] != v[2];
            if (nan || inside == (q.outside != 0)) match = false;
        }
        if (q.opacityOn && !(q.opacityMin <= o && o <= q.opacityMax)) match = false;  // (uniform switch)
        if (q.scaleOn) {                                                               // (uniform)
            const float m = __builtin_fmaxf(__builtin_fmaxf(sx, sy), sz);  // maxNum: NaN only when all three are
            if (!(q.scaleMin <= m && m <= q.scaleMax)) match = false;
        }
        if (match) state[g] = (uint8_t)(((old & q.andMask) ^ q.xorMask) & 0xFFu);
    }
    if (matched) {  // (uniform)
        const unsigned long long b = __ballot(match);
        if ((threadIdx.x & 63u) == 0) waveCount[threadIdx.x >> 6] = (uint32_t)__popcll(b);
        __syncthreads();
        if (threadIdx.x == 0) {
            const uint32_t n = waveCount[0] + waveCount[1] + waveCount[2] + waveCount[3];
            if (n) atomicAdd(matched, n);
        }
    }
}

// gsm_global_state_bounds: the extrema and counts a thread, a wave, a block or the grid has seen.  min / max of
// finite values with -0 stored as +0: exact and the same bits in any order.
struct BoundsAcc {
    float mn[3], mx[3];
    uint32_t n, skipped;
};

__device__ __forceinline__ void bounds_empty(BoundsAcc& a) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = __builtin_inff();
        a.mx[k] = -__builtin_inff();
    }
    a.n = a.skipped = 0u;
}

__device__ __forceinline__ void bounds_merge(BoundsAcc& a, const BoundsAcc& b) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.mn[k] = __builtin_fminf(a.mn[k], b.mn[k]);
        a.mx[k] = __builtin_fmaxf(a.mx[k], b.mx[k]);
    }
    a.n += b.n;
    a.skipped += b.skipped;
}

// the block's accumulators into one, valid in thread 0: a butterfly inside each wave, then the four waves through LDS
__device__ __forceinline__ void bounds_block_reduce(BoundsAcc& a, BoundsAcc* lds) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        BoundsAcc b;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            b.mn[k] = __shfl_xor(a.mn[k], off);
            b.mx[k] = __shfl_xor(a.mx[k], off);
        }
        b.n = __shfl_xor(a.n, off);
        b.skipped = __shfl_xor(a.skipped, off);
        bounds_merge(a, b);
    }
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = a;
    __syncthreads();
    if (threadIdx.x == 0)
        for (uint32_t w = 1; w < kEditBlock / 64; ++w) bounds_merge(a, lds[w]);
}

// launch 1: per block of 256 gaussians.  A gaussian in the keep set loads its record's first 16 bytes (the position
// is three fp32 values in both formats); one with a NaN or infinite coordinate is counted apart and not in the box.
template <bool HALF>
__global__ __launch_bounds__(kEditBlock) void k_bounds_partial(const void* __restrict__ world,
                                                               const uint8_t* __restrict__ state,
                                                               uint32_t defaultState, uint32_t count, KeepSet keep,
                                                               uint4* __restrict__ partials) {
    __shared__ BoundsAcc lds[kEditBlock / 64];
    uint32_t s;
    BoundsAcc a;
    bounds_empty(a);
    if (thread_kept(state, defaultState, count, keep, &s)) {
        const size_t g = (size_t)blockIdx.x * kEditBlock + threadIdx.x;
        const uint4 w = *(const uint4*)((const uint8_t*)world + g * (HALF ? sizeof(PackedWorldGaussianHalf)
                                                                          : sizeof(PackedWorldGaussian)));
        uint32_t bits[3] = {w.x, w.y, w.z};
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if ((bits[k] & 0x7F800000u) == 0x7F800000u) finite = false;
            if (bits[k] == 0x80000000u) bits[k] = 0u;  // -0 counts as +0
        }
        if (finite) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.mn[k] = a.mx[k] = __builtin_bit_cast(float, bits[k]);
            a.n = 1u;
        } else {
            a.skipped = 1u;
        }
    }
    bounds_block_reduce(a, lds);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)blockIdx.x] = make_uint4(__builtin_bit_cast(uint32_t, a.mn[0]), __builtin_bit_cast(uint32_t, a.mn[1]),
                                                      __builtin_bit_cast(uint32_t, a.mn[2]), __builtin_bit_cast(uint32_t, a.mx[0]));
        partials[2 * (size_t)blockIdx.x + 1] = make_uint4(__builtin_bit_cast(uint32_t, a.mx[1]), __builtin_bit_cast(uint32_t, a.mx[2]),
                                                          a.n, a.skipped);
    }
}

// launch 2: one workgroup walks the partials 256 a round and writes the eight words of *bounds (blocks == 0: the
// empty result)
__global__ __launch_bounds__(kEditBlock) void k_bounds_final(const uint4* __restrict__ partials, uint32_t blocks,
                                                             uint32_t* __restrict__ bounds) {
    __shared__ BoundsAcc lds[kEditBlock / 64];
    BoundsAcc a;
    bounds_empty(a);
    for (uint32_t i = threadIdx.x; i < blocks; i += kEditBlock) {
        const uint4 lo = partials[2 * (size_t)i], hi = partials[2 * (size_t)i + 1];
        BoundsAcc b;
        b.mn[0] = __builtin_bit_cast(float, lo.x);
        b.mn[1] = __builtin_bit_cast(float, lo.y);
        b.mn[2] = __builtin_bit_cast(float, lo.z);
        b.mx[0] = __builtin_bit_cast(float, lo.w);
        b.mx[1] = __builtin_bit_cast(float, hi.x);
        b.mx[2] = __builtin_bit_cast(float, hi.y);
        b.n = hi.z;
        b.skipped = hi.w;
        bounds_merge(a, b);
    }
    bounds_block_reduce(a, lds);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            bounds[k] = __builtin_bit_cast(uint32_t, a.mn[k]);
            bounds[3 + k] = __builtin_bit_cast(uint32_t, a.mx[k]);
        }
        bounds[6] = a.n;
        bounds[7] = a.skipped;
    }
}

// The fp32 value rounded once to fp16, to nearest even.  The empty asm keeps the compiler from folding the operation
// that made f into the conversion: for a product it emits v_fma_mixlo_f16 with an addend of +0, which turns a product
// of -0 into +0 (seen in the assembly; the numpy restatement keeps the -0).
__device__ __forceinline__ uint16_t transform_round_h(float f) {
    asm("" : "+v"(f));
    return f_to_hbits(f);
}

// gsm_global_transform.  c'_i = (..(D[i][0]*c_0 + D[i][1]*c_1) + ..) + D[i][N-1]*c_{N-1} for one band
// of one channel, in place.  D is a member of the kernel argument and, after unrolling, every index is a constant: the
// entries are scalar operands.
template <int N>
__device__ __forceinline__ void transform_band(float* c, const float (&D)[N * N]) {
    float o[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
        float acc = D[i * N] * c[0];
#pragma unroll
        for (int j = 1; j < N; ++j) acc = acc + D[i * N + j] * c[j];
        o[i] = acc;
    }
#pragma unroll
    for (int i = 0; i < N; ++i) c[i] = o[i];
}

// bands 1..DEG of the K = (DEG + 1)^2 coefficients of one channel
template <int DEG>
__device__ __forceinline__ void transform_channel(float* c, const gsm_global_transform_desc& t) {
    if constexpr (DEG >= 1) transform_band<3>(c + 1, t.sh1);
    if constexpr (DEG >= 2) transform_band<5>(c + 4, t.sh2);
    if constexpr (DEG >= 3) transform_band<7>(c + 9, t.sh3);
}

// The harmonics row of gaussian g: 3 channels of K coefficients, planar.  wide (uniform): the row is a multiple of
// 16 bytes at a 16-byte aligned address and goes as 16-byte loads and stores, band 0 with its own bits; otherwise
// element by element, and band 0 is neither loaded nor stored.
template <bool HALF, int DEG>
__device__ __forceinline__ void transform_harmonics(void* __restrict__ harm, size_t g,
                                                    const gsm_global_transform_desc& t, bool wide) {
    constexpr int K = (DEG + 1) * (DEG + 1), E = 3 * K;
    float c[E];
    if constexpr (HALF) {
        uint16_t* row = (uint16_t*)harm + g * (size_t)E;
        if constexpr (DEG == 3) {  // 96 bytes, 16-byte aligned (checked on the host): six accesses, as sh_color reads it
            uint4* p = (uint4*)row;
            uint32_t hw[E / 2];  // coefficient 2k in the low half of hw[k], 2k + 1 in the high half
#pragma unroll
            for (int q = 0; q < E / 8; ++q) {
                const uint4 v = p[q];
                hw[4 * q] = v.x;
                hw[4 * q + 1] = v.y;
                hw[4 * q + 2] = v.z;
                hw[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int i = 0; i < E; ++i) c[i] = hbits_to_f((uint16_t)((i & 1) ? hw[i >> 1] >> 16 : hw[i >> 1] & 0xFFFFu));
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) transform_channel<DEG>(c + ch * K, t);
#pragma unroll
            for (int i = 0; i < E; ++i) {
                if (i % K == 0) continue;  // band 0 keeps its bits
                const uint32_t h = transform_round_h(c[i]);
                hw[i >> 1] = (i & 1) ? (hw[i >> 1] & 0x0000FFFFu) | (h << 16) : (hw[i >> 1] & 0xFFFF0000u) | h;
            }
#pragma unroll
            for (int q = 0; q < E / 8; ++q) p[q] = make_uint4(hw[4 * q], hw[4 * q + 1], hw[4 * q + 2], hw[4 * q + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i % K != 0) c[i] = hbits_to_f(row[i]);
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) transform_channel<DEG>(c + ch * K, t);
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i % K != 0) row[i] = transform_round_h(c[i]);
        }
    } else {
        float* row = (float*)harm + g * (size_t)E;
        if (E % 4 == 0 && wide) {  // (uniform)
            float4* p = (float4*)row;
#pragma unroll
            for (int q = 0; q < E / 4; ++q) {
                const float4 v = p[q];
                c[4 * q] = v.x;
                c[4 * q + 1] = v.y;
                c[4 * q + 2] = v.z;
                c[4 * q + 3] = v.w;
            }
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) transform_channel<DEG>(c + ch * K, t);
#pragma unroll
            for (int q = 0; q < E / 4; ++q) p[q] = make_float4(c[4 * q], c[4 * q + 1], c[4 * q + 2], c[4 * q + 3]);
        } else {
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i % K != 0) c[i] = row[i];
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) transform_channel<DEG>(c + ch * K, t);
#pragma unroll
            for (int i = 0; i < E; ++i)
                if (i % K != 0) row[i] = c[i];
        }
    }
}

// a (x) q, the Hamilton product of the descriptor's quaternion and the record's, (x, y, z, w), in the header's order
__device__ __forceinline__ void transform_quaternion(const float (&a)[4], float& x, float& y, float& z, float& w) {
    const float ax = a[0], ay = a[1], az = a[2], aw = a[3];
    const float nx = ((aw * x + ax * w) + ay * z) - az * y;
    const float ny = ((aw * y - ax * z) + ay * w) + az * x;
    const float nz = ((aw * z + ax * y) - ay * x) + az * w;
    const float nw = ((aw * w - ax * x) - ay * y) - az * z;
    x = nx; y = ny; z = nz; w = nw;
}

// One thread per gaussian.  A thread not in the keep set loads its state byte and nothing else.  The fp32 record is
// three 16-byte loads and three stores, the fp16 one two and two; the opacity and the pad words go back with the bits
// they came with.  Every store is to the thread's own record and row.
template <bool HALF, int DEG>
__global__ __launch_bounds__(kEditBlock) void k_transform(void* __restrict__ world, void* __restrict__ harm,
                                                          const uint8_t* __restrict__ state, uint32_t defaultState,
                                                          uint32_t count, KeepSet keep, gsm_global_transform_desc t,
                                                          uint32_t wideRows) {
    uint32_t s;
    if (!thread_kept(state, defaultState, count, keep, &s)) return;
    const size_t g = (size_t)blockIdx.x * kEditBlock + threadIdx.x;
    if constexpr (HALF) {
        uint4* rec = (uint4*)((uint8_t*)world + g * sizeof(PackedWorldGaussianHalf));
        uint4 w0 = rec[0], w1 = rec[1];
        const float px = __builtin_bit_cast(float, w0.x), py = __builtin_bit_cast(float, w0.y),
                    pz = __builtin_bit_cast(float, w0.z);
        float p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            p[r] = ((t.matrix[4 * r] * px + t.matrix[4 * r + 1] * py) + t.matrix[4 * r + 2] * pz) + t.matrix[4 * r + 3];
        const float sx = hbits_to_f((uint16_t)(w0.w >> 16)) * t.scale;
        const float sy = hbits_to_f((uint16_t)(w1.x & 0xFFFFu)) * t.scale;
        const float sz = hbits_to_f((uint16_t)(w1.x >> 16)) * t.scale;
        float qx = hbits_to_f((uint16_t)(w1.y & 0xFFFFu)), qy = hbits_to_f((uint16_t)(w1.y >> 16));
        float qz = hbits_to_f((uint16_t)(w1.z & 0xFFFFu)), qw = hbits_to_f((uint16_t)(w1.z >> 16));
        transform_quaternion(t.quaternion, qx, qy, qz, qw);
        w0.x = __builtin_bit_cast(uint32_t, p[0]);
        w0.y = __builtin_bit_cast(uint32_t, p[1]);
        w0.z = __builtin_bit_cast(uint32_t, p[2]);
        w0.w = (w0.w & 0xFFFFu) | ((uint32_t)transform_round_h(sx) << 16);
        w1.x = (uint32_t)transform_round_h(sy) | ((uint32_t)transform_round_h(sz) << 16);
        w1.y = (uint32_t)transform_round_h(qx) | ((uint32_t)transform_round_h(qy) << 16);
        w1.z = (uint32_t)transform_round_h(qz) | ((uint32_t)transform_round_h(qw) << 16);
        rec[0] = w0;
        rec[1] = w1;
    } else {
        uint4* rec = (uint4*)((uint8_t*)world + g * sizeof(PackedWorldGaussian));
        uint4 w0 = rec[0], w1 = rec[1], w2 = rec[2];
        const float px = __builtin_bit_cast(float, w0.x), py = __builtin_bit_cast(float, w0.y),
                    pz = __builtin_bit_cast(float, w0.z);
        float p[3];
#pragma unroll
        for (int r = 0; r < 3; ++r)
            p[r] = ((t.matrix[4 * r] * px + t.matrix[4 * r + 1] * py) + t.matrix[4 * r + 2] * pz) + t.matrix[4 * r + 3];
        float qx = __builtin_bit_cast(float, w2.x), qy = __builtin_bit_cast(float, w2.y);
        float qz = __builtin_bit_cast(float, w2.z), qw = __builtin_bit_cast(float, w2.w);
        transform_quaternion(t.quaternion, qx, qy, qz, qw);
        w0.x = __builtin_bit_cast(uint32_t, p[0]);
        w0.y = __builtin_bit_cast(uint32_t, p[1]);
        w0.z = __builtin_bit_cast(uint32_t, p[2]);
        w1.x = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, w1.x) * t.scale);
        w1.y = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, w1.y) * t.scale);
        w1.z = __builtin_bit_cast(uint32_t, __builtin_bit_cast(float, w1.z) * t.scale);
        w2 = make_uint4(__builtin_bit_cast(uint32_t, qx), __builtin_bit_cast(uint32_t, qy),
                        __builtin_bit_cast(uint32_t, qz), __builtin_bit_cast(uint32_t, qw));
        rec[0] = w0;
        rec[1] = w1;
        rec[2] = w2;
    }
    if constexpr (DEG > 0) transform_harmonics<HALF, DEG>(harm, g, t, wideRows != 0);
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

void launch_select_where(bool halfInput, const void* world, const SelectWhereArgs& a, uint8_t* state,
                         const uint2* styleTable, uint32_t* matched, hipStream_t s) {
    // overwritten, not added to (a kernel, not a memset node: launch_state_histogram's note)
    if (matched) hipLaunchKernelGGL(k_select_where_clear, dim3(1), dim3(64), 0, s, matched);
    const uint32_t blocks = (a.count + kEditBlock - 1u) / kEditBlock;
    if (blocks == 0) return;
    const auto k = halfInput ? k_select_where<true> : k_select_where<false>;
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kEditBlock), 0, s, world, a, state, styleTable, matched);
}

void launch_state_bounds(bool halfInput, const void* world, const uint8_t* state, uint32_t defaultState,
                         uint32_t count, const KeepSet& keep, uint4* partials, uint32_t* bounds, hipStream_t s) {
    const uint32_t blocks = (count + kEditBlock - 1u) / kEditBlock;
    if (blocks) {
        const auto k = halfInput ? k_bounds_partial<true> : k_bounds_partial<false>;
        hipLaunchKernelGGL(k, dim3(blocks), dim3(kEditBlock), 0, s, world, state, defaultState, count, keep, partials);
    }
    hipLaunchKernelGGL(k_bounds_final, dim3(1), dim3(kEditBlock), 0, s, (const uint4*)partials, blocks, bounds);
}

template <bool HALF>
static auto transform_kernel(uint32_t shDegree) {
    switch (shDegree) {
        case 0: return k_transform<HALF, 0>;
        case 1: return k_transform<HALF, 1>;
        case 2: return k_transform<HALF, 2>;
        default: return k_transform<HALF, 3>;
    }
}

void launch_transform(bool halfInput, uint32_t shDegree, void* world, void* harmonics, const uint8_t* state,
                      uint32_t defaultState, uint32_t count, const KeepSet& keep, const gsm_global_transform_desc& desc,
                      bool wideRows, hipStream_t s) {
    const uint32_t blocks = (count + kEditBlock - 1u) / kEditBlock;
    if (blocks == 0) return;
    const auto k = halfInput ? transform_kernel<true>(shDegree) : transform_kernel<false>(shDegree);
    hipLaunchKernelGGL(k, dim3(blocks), dim3(kEditBlock), 0, s, world, harmonics, state, defaultState, count, keep, desc,
                       wideRows ? 1u : 0u);
}

}  // namespace gsm

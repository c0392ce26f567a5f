// gsm_blend_common.h -- the device helpers the two Global blend translation units share (gsm_blend.hip and
// gsm_blend_pw.hip, and the kernel texts they include): packed-fp16 types and casts, the colour accumulate, the sRGB
// encode, the wave-level LDS hand-off and the exp table's index.  Nothing here is used by one of them only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "gsm_detmath.h"

namespace gsm {

typedef _Float16 h1;
typedef _Float16 h2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ h2 as_h2(uint32_t u) { return __builtin_bit_cast(h2, u); }
__device__ __forceinline__ uint32_t as_u32(h2 v) { return __builtin_bit_cast(uint32_t, v); }
__device__ __forceinline__ h2 splat_lo(h2 v) { return h2{v.x, v.x}; }
__device__ __forceinline__ h2 splat_hi(h2 v) { return h2{v.y, v.y}; }
__device__ __forceinline__ float h_bits_to_f(uint16_t b) { return (float)__builtin_bit_cast(h1, b); }
// `color += gColor * w` (GlobalShaders.metal:1137-1145, DepthFirstShaders.metal:1783-1786): one
// fused multiply-add, a single rounding per channel (the numeric contract; the oracle's hfma)
__device__ __forceinline__ h2 blend_acc(h2 acc, h2 c, h2 w) { return __builtin_elementwise_fma(c, w, acc); }
// linear -> sRGB encode of a [0, 1] value (include/gsm_renderer.h), powr of the numeric contract
__device__ __forceinline__ float srgb_encode(float c) {
    return c <= 0.0031308f ? c * 12.92f : 1.055f * det_powrf(c, 1.0f / 2.4f) - 0.055f;
}

// Lanes of one wave hand LDS words to each other: the compiler must not forward a lane's own
// store past them (no instruction; the hardware keeps a wave's LDS operations in order).
__device__ __forceinline__ void blend_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// The table index of a packed pair of quadratic forms: its fp16 bits.  (The far-field clamp and the
// dead-lane columns that cut the gathers' bank conflicts, and the duplicate-read attribution build, are
// kept as tools/exp/rejected_variants.patch: bit-exact, no faster)
__device__ __forceinline__ uint32_t tbl_bits(h2 p) {
    return as_u32(p);
}

}  // namespace gsm

// gsm_select_mask_body.h -- the text of k_select_mask, compiled twice by gsm_kernels.hip: as gsm_global_select_mask's
// kernel, the kernel it was, and under GSM_ORTHO as k_select_mask_ortho (gsm_global_select_mask_ortho),
// the same select with project_gaussian's orthographic rule.  No include guard.
// gsm_global_select_mask: one thread per gaussian.  project_gaussian's kProjMean mode runs the
// frame's culls and forms the fp16 mean with the frame's own functions; the mean's pixel is looked up in the mask
// and a matching gaussian's state byte becomes (old & andMask) ^ xorMask.  No SH, no record, no tile test; byte
// loads and stores, one integer add per workgroup for the count (*matched: zeroed by the launcher).
template <bool HALF>
#ifdef GSM_ORTHO
__global__ __launch_bounds__(kProjectBlock) void k_select_mask_ortho(
#else
__global__ __launch_bounds__(kProjectBlock) void k_select_mask(
#endif
    const void* __restrict__ world, ProjectArgs P, const float2* __restrict__ sincos,
    const uint8_t* __restrict__ mask, size_t maskPitch, uint32_t width, uint32_t height, uint8_t* __restrict__ state,
    const uint2* __restrict__ styleTable, uint32_t andMask, uint32_t xorMask, uint32_t* __restrict__ matched) {
    __shared__ uint32_t lds[kProjectBlock / 64];
    __shared__ ByteLut lut;  // (kProjMean reads no entry of it)
    const uint32_t gid = blockIdx.x * kProjectBlock + threadIdx.x;
    uint32_t hit = 0;
    if (gid < P.count) {
#ifdef GSM_ORTHO
        const ProjOut o = project_gaussian<HALF, 0, kProjMean, kOrthoOn>(world, nullptr, gid, P, sincos, lut);
#else
        const ProjOut o = project_gaussian<HALF, 0, kProjMean>(world, nullptr, gid, P, sincos, lut);
#endif
        const uint32_t old = state[gid];
        bool match = o.vis;
        if (styleTable && ((styleTable[old].y >> 8) & 0xFFu)) match = false;  // hidden: not selectable
        const uint16_t hmx = (uint16_t)(o.rd.x & 0xFFFFu), hmy = (uint16_t)(o.rd.x >> 16);
        if ((hmx & 0x7C00u) == 0x7C00u || (hmy & 0x7C00u) == 0x7C00u) match = false;  // inf or NaN
        // floor(m + 0.5): exact in fp32 for every finite fp16 m
        const float fx = __builtin_floorf(hbits_to_f(hmx) + 0.5f), fy = __builtin_floorf(hbits_to_f(hmy) + 0.5f);
        if (!(fx >= 0.0f && fx < (float)width && fy >= 0.0f && fy < (float)height)) match = false;
        if (match) {
            match = mask[(size_t)(uint32_t)fy * maskPitch + (uint32_t)fx] != 0;
            if (match) state[gid] = (uint8_t)(((old & andMask) ^ xorMask) & 0xFFu);
        }
        hit = match ? 1u : 0u;
    }
    if (matched) {  // (uniform)
        const uint32_t s = block_reduce_add<kProjectBlock>(hit, lds);
        if (threadIdx.x == 0 && s) atomicAdd(matched, s);
    }
}

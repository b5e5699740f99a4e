// torch's CPU bilinear resize (align_corners=False) as device functions: the mask-target crops (mask.hip) and the evaluation's resize of
// the pasted masks (mask_eval.hip) must reproduce its fp32 results bit for bit, so both take the arithmetic from here.
#pragma once
#include <hip/hip_runtime.h>

namespace {

// torch's bilinear source index, align_corners=False: (index of the first tap, of the second tap, weight of the second tap).  The operation
// order is the one the reference's CPU run shows (tests/golden/mask_head.npz is reproduced bit for bit by it and by no other): the source
// coordinate is ONE fused multiply-add, the four tap weights are multiplied first and the taps accumulated in a chain of fused multiply-adds
// -- so a uint8 target pixel whose four taps are all 1 can still truncate to 0 where the rounded weights sum to 1 - 2^-24, as it does there.
#pragma clang fp contract(off)
__device__ __forceinline__ void bilinear_tap(const float scale, const int dst, const int in_size, int& i0, int& i1, float& l1) {
    float s = __fmaf_rn(scale, (float)dst + 0.5f, -0.5f);
    if (s < 0.f) s = 0.f;
    i0 = min((int)floorf(s), in_size - 1);
    l1 = fminf(fmaxf(s - (float)i0, 0.f), 1.f);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
}

#pragma clang fp contract(off)
__device__ __forceinline__ float bilinear_mix(const float v00, const float v01, const float v10, const float v11, const float lx, const float ly) {
    const float wx0 = 1.f - lx, wy0 = 1.f - ly;
    const float w00 = wy0 * wx0, w01 = wy0 * lx, w10 = ly * wx0, w11 = ly * lx;
    return __fmaf_rn(w11, v11, __fmaf_rn(w10, v10, __fmaf_rn(w01, v01, w00 * v00)));
}

// The same interpolation in the operation order of torch's OTHER CPU kernel.  upsample_bilinear2d on a contiguous NCHW float tensor runs
// the four-weight sum above only while out_h + out_w <= 128 (the mask-target crops at M = 8, 14 or 28 among them); beyond that it runs a separable kernel whose
// compiled form is row = fma(v0, 1 - lx, v1 * lx) and out = fma(row0, 1 - ly, row1 * ly).  On 0/1 masks the two differ exactly where the
// rounded weights of four set taps sum to 1 - 2^-24 in one order and to 1 in the other, which the uint8 truncation turns into a 0 or a 1.
// Established on the CPU against torch 2.10 over 1200 random (source, destination) size pairs, with no differing pixel.
#pragma clang fp contract(off)
__device__ __forceinline__ float bilinear_mix_separable(const float v00, const float v01, const float v10, const float v11, const float lx,
                                                        const float ly) {
    const float wx0 = 1.f - lx, wy0 = 1.f - ly;
    const float r0 = __fmaf_rn(v00, wx0, v01 * lx), r1 = __fmaf_rn(v10, wx0, v11 * lx);
    return __fmaf_rn(r0, wy0, r1 * ly);
}

// which of the two torch runs for an output of out_h x out_w
__host__ __device__ __forceinline__ bool bilinear_four_weight_path(const int out_h, const int out_w) { return out_h + out_w <= 128; }

}  // namespace

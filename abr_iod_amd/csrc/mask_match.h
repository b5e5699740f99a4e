// The instance a RoI's mask target is taken from: the FIRST maximum of the IoU between the RoI and the image's ground-truth boxes
// (mask_head/loss.py:55-66 with torch.max's tie rule).  Shared by the bitmask route (mask.hip, abr_mask_targets) and the polygon route
// (poly.hip, abr_poly_mask_targets) so that both pick the same instance bit for bit.
#pragma once
#include <hip/hip_runtime.h>

namespace abr {

__device__ __forceinline__ float mask_box_iou(const float4 g, const float4 b) {
#pragma clang fp contract(off)
    // structures/boxlist_ops.py:53-88, TO_REMOVE = 1 (the arithmetic of rpn.hip's box_iou)
    const float area1 = (g.z - g.x + 1) * (g.w - g.y + 1);
    const float area2 = (b.z - b.x + 1) * (b.w - b.y + 1);
    const float lx = fmaxf(g.x, b.x), ly = fmaxf(g.y, b.y), rx = fminf(g.z, b.z), ry = fminf(g.w, b.w);
    const float w = fmaxf(rx - lx + 1, 0.f), h = fmaxf(ry - ly + 1, 0.f);
    const float inter = w * h;
    return inter / (area1 + area2 - inter);
}

// index of the first maximum over gt[0 .. G) (0 when G <= 0 or every IoU is NaN)
__device__ __forceinline__ int mask_match_gt(const float4* __restrict__ gt, const int G, const float4 b) {
    float best = -1.f;
    int bi = 0;
    for (int g = 0; g < G; g++) {
        const float v = mask_box_iou(gt[g], b);
        if (v > best) { best = v; bi = g; }      // first max wins (torch.max)
    }
    return bi;
}

}  // namespace abr

// The instance a RoI's mask target is taken from: the FIRST maximum of the IoU (abr::box_iou, common.h) between the RoI and the image's
// ground-truth boxes (mask_head/loss.py:55-66 with torch.max's tie rule).  Shared by the bitmask route (mask.hip, abr_mask_targets) and the polygon route
// (poly.hip, abr_poly_mask_targets) so that both pick the same instance bit for bit.
#pragma once
#include "common.h"

namespace abr {

// index of the first maximum over gt[0 .. G) (0 when G <= 0 or every IoU is NaN)
__device__ __forceinline__ int mask_match_gt(const float4* __restrict__ gt, const int G, const float4 b) {
    float best = -1.f;
    int bi = 0;
    for (int g = 0; g < G; g++) {
        const float v = box_iou(gt[g], b);
        if (v > best) { best = v; bi = g; }      // first max wins (torch.max)
    }
    return bi;
}

}  // namespace abr

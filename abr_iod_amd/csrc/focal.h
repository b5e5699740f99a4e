// Sigmoid focal loss, the element: value and derivative of one (logit, class) pair -- csrc/cuda/SigmoidFocalLoss_cuda.cu:20-101.  The one
// definition behind abr_sigmoid_focal_* (losses.hip: one value per logit, for T = float and T = double) and the RetinaNet loss over a pyramid
// (retinanet_loss.hip: summed where the logits lie), which must agree bit for bit.
// The reference's template keeps its expf / powf / logf calls and its `1.` literals with every T: float transcendentals inside double
// sub-expressions (kept so, it is elementwise and fp64 is cheap on CDNA4); gamma / alpha are `const float` there too.
// x: the logit of class d + 1; t: the anchor's label (the class, 0 background, < 0 ignored: the value and the derivative are then 0).
#pragma once
#include <float.h>

#include "common.h"

namespace abr {

template <typename T>
__device__ __forceinline__ T focal_value(const T x, const int t, const int d, const float gamma, const float alpha) {
    const T c1 = (t == d + 1), c2 = (t >= 0) & (t != d + 1);
    const T zn = (1.0 - alpha), zp = alpha;
    const T p = 1. / (1. + expf((float)-x));
    const T term1 = powf((float)(1. - p), gamma) * logf((float)fmax(p, (T)FLT_MIN));
    const T term2 = powf((float)p, gamma) * (-1. * x * (x >= 0) - logf((float)(1. + expf((float)(x - 2. * x * (x >= 0))))));
    T l = 0;
    l += -c1 * term1 * zp;
    l += -c2 * term2 * zn;
    return l;
}

// d focal_value / dx (the caller multiplies by the upstream gradient)
template <typename T>
__device__ __forceinline__ T focal_deriv(const T x, const int t, const int d, const float gamma, const float alpha) {
    const T c1 = (t == d + 1), c2 = (t >= 0) & (t != d + 1);
    const T zn = (1.0 - alpha), zp = alpha;
    const T p = 1. / (1. + expf((float)-x));
    const T term1 = powf((float)(1. - p), gamma) * (1. - p - (p * gamma * logf((float)fmax(p, (T)FLT_MIN))));
    const T term2 = powf((float)p, gamma) *
                    ((-1. * x * (x >= 0) - logf((float)(1. + expf((float)(x - 2. * x * (x >= 0)))))) * (1. - p) * gamma - p);
    T g = 0;
    g += -c1 * term1 * zp;
    g += -c2 * term2 * zn;
    return g;
}

}  // namespace abr

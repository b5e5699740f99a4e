// Box coder, matcher and label arithmetic: the one definition behind every kernel that encodes, decodes, clips, matches or labels boxes
// (rpn.hip, roi_targets.h, rpn_pyramid.hip, detect.hip, nms.hip, retinanet.hip), beside abr::box_iou (common.h).  Those kernels' results must agree with the reference's
// and with each other bit for bit, so each function here rounds once per operation: the library is built with the compiler's default
// contraction, and every body switches it off for itself (a fused dx * w + cx would change results).  Operation order is the reference's,
// divisions included.
#pragma once
#include "common.h"

namespace abr {

constexpr float kBoxDeltaClip = 4.135166556742356f;   // log(1000/16), box_coder.py:20 bbox_xform_clip

// BoxCoder.encode (box_coder.py:22-50): the regression target of ground truth `gt` against the example box `ex`
__device__ __forceinline__ float4 box_encode(const float4 gt, const float4 ex, float wx, float wy, float ww, float wh) {
#pragma clang fp contract(off)
    const float ew = ex.z - ex.x + 1, eh = ex.w - ex.y + 1;
    const float ecx = ex.x + 0.5f * ew, ecy = ex.y + 0.5f * eh;
    const float gw = gt.z - gt.x + 1, gh = gt.w - gt.y + 1;
    const float gcx = gt.x + 0.5f * gw, gcy = gt.y + 0.5f * gh;
    return make_float4(wx * (gcx - ecx) / ew, wy * (gcy - ecy) / eh, ww * logf(gw / ew), wh * logf(gh / eh));
}

// BoxCoder.decode (box_coder.py:52-95): the four deltas d applied to the anchor / RoI b
__device__ __forceinline__ float4 box_decode(const float4 b, const float* d, float wx, float wy, float ww, float wh) {
#pragma clang fp contract(off)
    const float w = b.z - b.x + 1, h = b.w - b.y + 1;               // :66-69
    const float cx = b.x + 0.5f * w, cy = b.y + 0.5f * h;
    const float dx = d[0] / wx, dy = d[1] / wy;
    const float dw = fminf(d[2] / ww, kBoxDeltaClip), dh = fminf(d[3] / wh, kBoxDeltaClip);
    const float pcx = dx * w + cx, pcy = dy * h + cy;
    const float pw = expf(dw) * w, ph = expf(dh) * h;
    return make_float4(pcx - 0.5f * pw, pcy - 0.5f * ph, pcx + 0.5f * pw - 1, pcy + 0.5f * ph - 1);
}

// BoxList.clip_to_image (bounding_box.py:214-225), TO_REMOVE = 1: W1 = width - 1, H1 = height - 1
__device__ __forceinline__ float4 box_clip(const float4 o, float W1, float H1) {
#pragma clang fp contract(off)
    return make_float4(fminf(fmaxf(o.x, 0.f), W1), fminf(fmaxf(o.y, 0.f), H1), fminf(fmaxf(o.z, 0.f), W1), fminf(fmaxf(o.w, 0.f), H1));
}

// Greedy NMS's test of a kept box a (area_a = (a.z - a.x + 1) * (a.w - a.y + 1)) against a later box b (nms_cpu.cpp:5-75): IoU in the reference's
// form inter / (a + b - inter); `ovr >= thr` suppresses (strict_gt = 0, the CPU rule, canonical here) or `ovr > thr` (nms.cu).  Shared by nms.hip
// and retinanet.hip, so their keep lists agree pair for pair.
__device__ __forceinline__ bool nms_suppresses(const float4 a, float area_a, const float4 b, float thr, int strict_gt) {
#pragma clang fp contract(off)
    const float xx1 = fmaxf(a.x, b.x), yy1 = fmaxf(a.y, b.y);
    const float xx2 = fminf(a.z, b.z), yy2 = fminf(a.w, b.w);
    const float w = fmaxf(0.f, xx2 - xx1 + 1), h = fmaxf(0.f, yy2 - yy1 + 1);
    const float inter = w * h;
    const float area_b = (b.z - b.x + 1) * (b.w - b.y + 1);
    const float ovr = inter / (area_a + area_b - inter);
    return strict_gt ? (ovr > thr) : (ovr >= thr);
}

// Matcher's scan of one box against G ground truths (matcher.py:64-66 max over dim 0: the FIRST maximum wins, as torch.max does).  `rowmax`
// (per ground truth the bit pattern of its largest IoU with any box, or nullptr) switches on set_low_quality_matches_'s test (:83-112): lq =
// the box reaches some ground truth's maximum.  The test is decided outside the loop (LQ), so the loop of a kernel that always or never
// wants it holds no branch on the pointer.
struct MatchScan { float best; int bi; bool lq; };
template <bool LQ>
__device__ __forceinline__ MatchScan match_scan_lq(const float* gt, int G, const float4 b, const unsigned* rowmax) {
#pragma clang fp contract(off)
    MatchScan s{-1.f, 0, false};
    for (int g = 0; g < G; g++) {
        const float v = box_iou(reinterpret_cast<const float4*>(gt)[g], b);
        if (v > s.best) { s.best = v; s.bi = g; }
        if (LQ && v == __uint_as_float(rowmax[g])) s.lq = true;
    }
    return s;
}
__device__ __forceinline__ MatchScan match_scan(const float* gt, int G, const float4 b, const unsigned* rowmax) {
    return rowmax ? match_scan_lq<true>(gt, G, b, rowmax) : match_scan_lq<false>(gt, G, b, nullptr);
}

// Matcher.set_low_quality_matches_'s first pass (matcher.py:83-112): per ground truth its maximum IoU over all boxes, as the bit pattern
// match_scan_lq compares against.  The maximum over a 256-thread workgroup (all threads call; s_m: 4 floats): ONE atomic per workgroup and
// ground-truth box then goes to the shared word: with one per WAVE, the ~560 waves of the RPN call queued on a handful of addresses (80 us
// for 35 910 anchors x 5 boxes)
__device__ __forceinline__ float block_max_256(float m, float* s_m) {
    m = wave_max(m);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_m[threadIdx.x >> 6] = m;
    __syncthreads();
    return fmaxf(fmaxf(s_m[0], s_m[1]), fmaxf(s_m[2], s_m[3]));
}
// the pass itself, for one image's G ground truths (G == 0: nothing is read): all 256 threads of every workgroup along x call, each with its
// first box j0 and the grid's stride along x (read off blockDim in the kernel, where the compiler knows the launch is uniform); rowmax zeroed
// by the caller.  Shared by the RPN's targets (rpn.hip) and RetinaNet's (retinanet_loss.hip).
__device__ __forceinline__ void gt_row_max(const float* boxes, int n, unsigned j0, unsigned stride, const float* gt, int G, unsigned* rowmax) {
    __shared__ float s_m[4];
    for (int g = 0; g < G; g++) {
        const float4 gb = reinterpret_cast<const float4*>(gt)[g];
        float m = 0.f;
        for (int j = j0; j < n; j += stride)
            m = fmaxf(m, box_iou(gb, reinterpret_cast<const float4*>(boxes)[j]));
        m = block_max_256(m, s_m);
        if (threadIdx.x == 0) atomicMax(rowmax + g, __float_as_uint(m));  // IoU >= 0: bit pattern is monotone
    }
}

// Matcher's result for a scanned box (matcher.py:68-75, low-quality matches restored :108-112): the ground truth's index, -1 BELOW_LOW_THRESHOLD,
// -2 BETWEEN_THRESHOLDS.  The ground truth a caller then reads is row max(m, 0) (clamp(min=0) of rpn/loss.py:59, box_head/loss.py:52).
__device__ __forceinline__ int match_index(float best, int bi, bool lq, float hi, float lo) {
#pragma clang fp contract(off)
    int m = best < lo ? -1 : (best < hi ? -2 : bi);
    if (lq) m = bi;
    return m;
}

// RPN objectness label of a matched anchor (rpn/loss.py:78-92): 1 matched, 0 background, -1 ignored (between thresholds, or not visible)
__device__ __forceinline__ float rpn_label(int m, bool visible) {
#pragma clang fp contract(off)
    float l = m >= 0 ? 1.f : 0.f;
    if (!visible) l = -1.f;
    if (m == -2) l = -1.f;
    return l;
}

// Box-head class label of a matched proposal (box_head/loss.py:66-75): the class of ground truth gi = max(m, 0) (1 without a label table),
// 0 background, -1 ignored
__device__ __forceinline__ int64_t head_label(int m, const int64_t* gt_labels, int gi) {
#pragma clang fp contract(off)
    int64_t l = gt_labels ? gt_labels[gi] : 1;
    if (m == -1) l = 0;
    if (m == -2) l = -1;
    return l;
}

}  // namespace abr

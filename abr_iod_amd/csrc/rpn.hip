// RPN / RoI-head glue kernels: anchors, proposal decode+clip, IoU+Matcher+labels+BoxCoder.encode.
// In the reference these are dozens of small ATen index kernels per image (and several nonzero() host syncs);
// here each is one launch and nothing leaves the device.
#include "box_math.h"
#include "roi_targets.h"

namespace {

// anchor_generator.py:84-110 : (shifts[:,None] + cell[None]).reshape(-1,4), location-major / anchor-minor
__global__ void grid_anchors_kernel(const float* __restrict__ cell, int A, int H, int W, int stride, int img_h, int img_w,
                                    int straddle, float* __restrict__ out, uint8_t* __restrict__ vis) {
    const int total = H * W * A;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const int a = i % A, x = (i / A) % W, y = i / (A * W);
        const float sx = (float)(x * stride), sy = (float)(y * stride);
        const float x1 = sx + cell[4 * a], y1 = sy + cell[4 * a + 1], x2 = sx + cell[4 * a + 2], y2 = sy + cell[4 * a + 3];
        reinterpret_cast<float4*>(out)[i] = make_float4(x1, y1, x2, y2);
        if (vis)
            vis[i] = straddle >= 0 ? (x1 >= -straddle && y1 >= -straddle && x2 < img_w + straddle && y2 < img_h + straddle) : 1;
    }
}

#pragma clang fp contract(off)
__global__ void decode_clip_kernel(const float* __restrict__ reg, int reg_stride, int reg_col0, int A,
                                   const float* __restrict__ anchors, const int64_t* __restrict__ idx, int N, int n_anchor,
                                   int k, const int32_t* __restrict__ img_hw, float wx, float wy, float ww, float wh,
                                   float* __restrict__ out) {
    const int total = N * k;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        const int i = t / k;
        const int64_t a = idx[t];
        // anchor a = location*A + a': its 4 deltas sit in row `location` of reg at columns reg_col0 + 4a' (NHWC head output)
        const float* d = reg + ((size_t)i * (n_anchor / A) + a / A) * reg_stride + reg_col0 + 4 * (a % A);
        float4 o = abr::box_decode(reinterpret_cast<const float4*>(anchors)[a], d, wx, wy, ww, wh);
        if (img_hw) o = abr::box_clip(o, (float)(img_hw[2 * i + 1] - 1), (float)(img_hw[2 * i] - 1));
        reinterpret_cast<float4*>(out)[t] = o;
    }
}

// pass 1: per-gt maximum IoU over all boxes (needed only for Matcher.set_low_quality_matches_, matcher.py:83-112)
// (the pass itself is abr::gt_row_max, box_math.h)
using abr::gt_row_max;

__global__ __launch_bounds__(256) void gt_max_iou_kernel(const float* __restrict__ boxes, int n, const float* __restrict__ gt, int G,
                                  unsigned* __restrict__ rowmax) {
    gt_row_max(boxes, n, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, gt, G, rowmax);
}

#pragma clang fp contract(off)
__global__ void match_encode_kernel(const float* __restrict__ boxes, int n, const float* __restrict__ gt,
                                    const int64_t* __restrict__ gt_labels, int G, const uint8_t* __restrict__ vis, float hi,
                                    float lo, const unsigned* __restrict__ rowmax, float wx, float wy, float ww,
                                    float wh, int64_t* __restrict__ matched, float* __restrict__ labels_f32,
                                    int64_t* __restrict__ labels_i64, float* __restrict__ reg_targets) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const float4 b = reinterpret_cast<const float4*>(boxes)[j];
        const abr::MatchScan s = abr::match_scan(gt, G, b, rowmax);                 // rowmax: only with allow_low_quality_matches
        const int m = abr::match_index(s.best, s.bi, s.lq, hi, lo);
        if (matched) matched[j] = m;
        const int gi = m < 0 ? 0 : m;                                               // clamp(min=0)
        if (labels_f32) labels_f32[j] = abr::rpn_label(m, !vis || vis[j]);
        if (labels_i64) labels_i64[j] = abr::head_label(m, gt_labels, gi);
        if (reg_targets)
            reinterpret_cast<float4*>(reg_targets)[j] = abr::box_encode(reinterpret_cast<const float4*>(gt)[gi], b, wx, wy, ww, wh);
    }
}

// (the box-head training targets' kernels -- candidate matching, merge + gather -- live in roi_targets.h: abr_roi_head_targets_table of
//  box_head_fpn.hip shares them)

// rows picks[i*P + j] of image i's post-NMS list -> rois [N*P, 5] = (i, box), obj [N*P] (the 64 distillation proposals of the source
// model: generalized_rcnn.py:140-158; the post-NMS list is already in descending objectness order)
__global__ void gather_proposals_kernel(const float* __restrict__ props, const float* __restrict__ scores, const int32_t* __restrict__ keep,
                                        int k_pre, int post, const int64_t* __restrict__ picks, int N, int P, float* __restrict__ rois,
                                        float* __restrict__ obj) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N * P) return;
    const int i = t / P;
    const int src = keep[(int64_t)i * post + picks[t]];
    const float4 b = reinterpret_cast<const float4*>(props)[(int64_t)i * k_pre + src];
    float* r = rois + (int64_t)t * 5;
    r[0] = (float)i; r[1] = b.x; r[2] = b.y; r[3] = b.z; r[4] = b.w;
    if (obj) obj[t] = scores[(int64_t)i * k_pre + src];
}

// ---------------------------------------------------------------------------------------------------------------------------------
// RPN training targets for the whole batch (abr_rpn_targets_batched): the anchors are shared by the images (same feature-map size), the
// GT boxes and the visibility masks are per image.  gt_max_iou_kernel's pass (gt_row_max) and match_encode_kernel's functions (abr::match_scan,
// match_index, rpn_label, box_encode: box_math.h), blockIdx.y = image.
__global__ __launch_bounds__(256) void gt_max_iou_batched_kernel(const float* __restrict__ boxes, int n, const float* const* __restrict__ gt_ptrs,
                                          const int32_t* __restrict__ n_gt, int g_max, unsigned* __restrict__ rowmax) {
    const int i = blockIdx.y;
    gt_row_max(boxes, n, blockIdx.x * blockDim.x + threadIdx.x, gridDim.x * blockDim.x, gt_ptrs[i], n_gt[i], rowmax + (size_t)i * g_max);
}

#pragma clang fp contract(off)
__global__ void rpn_match_batched_kernel(const float* __restrict__ boxes, int n, const float* const* __restrict__ gt_ptrs,
                                         const int32_t* __restrict__ n_gt, int g_max, const uint8_t* const* __restrict__ vis_ptrs, float hi,
                                         float lo, const unsigned* __restrict__ rowmax, float wx, float wy, float ww, float wh,
                                         float* __restrict__ labels, float* __restrict__ reg_targets) {
    const int i = blockIdx.y;
    const float* gt = gt_ptrs[i];
    const uint8_t* vis = vis_ptrs[i];
    const int G = n_gt[i];
    const unsigned* rm = rowmax + (size_t)i * g_max;
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        const float4 b = reinterpret_cast<const float4*>(boxes)[j];
        const abr::MatchScan s = abr::match_scan_lq<true>(gt, G, b, rm);           // always with allow_low_quality_matches
        const int m = abr::match_index(s.best, s.bi, s.lq, hi, lo);
        const int gi = m < 0 ? 0 : m;                                               // clamp(min=0)
        labels[(size_t)i * n + j] = abr::rpn_label(m, !vis || vis[j]);
        reinterpret_cast<float4*>(reg_targets)[(size_t)i * n + j] = abr::box_encode(reinterpret_cast<const float4*>(gt)[gi], b, wx, wy, ww, wh);
    }
}

// RPN loss bookkeeping in one launch: the sampler's two padded lists -> the concatenated "all sampled" list, the flat positions of their
// objectness logits and box deltas inside the fused NHWC head output (anchor j of the flattened batch: row j / A, columns j % A and
// A + 4 (j % A) of a row of Cf columns), and the number of sampled anchors as a float (the losses' normaliser, rpn/loss.py:136,146).
__global__ void rpn_loss_indices_kernel(const int64_t* __restrict__ pos, int n_pos, const int64_t* __restrict__ neg, int n_neg,
                                        const int32_t* __restrict__ counts, int n_img, int A, int Cf, int64_t* __restrict__ samp,
                                        int64_t* __restrict__ obj_flat, int64_t* __restrict__ pos_row, int64_t* __restrict__ pos_col,
                                        float* __restrict__ denom) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < n_pos + n_neg) {
        const int64_t v = t < n_pos ? pos[t] : neg[t - n_pos];
        samp[t] = v;
        const int64_t row = v >= 0 ? v / A : -1;
        obj_flat[t] = v >= 0 ? row * Cf + (v - row * A) : -1;
        if (t < n_pos) {
            pos_row[t] = row;
            pos_col[t] = v >= 0 ? A + 4 * (v - row * A) : 0;
        }
    }
    if (t == 0) {
        int c = 0;
        for (int i = 0; i < 2 * n_img; i++) c += counts[i];
        *denom = (float)c;
    }
}

// BoxCoder.encode row-wise (box_coder.py:22-50): out[i] = encode(gt[i], ex[i])
#pragma clang fp contract(off)
__global__ void box_encode_kernel(const float* __restrict__ gt, const float* __restrict__ ex, int n, float wx, float wy,
                                  float ww, float wh, float* __restrict__ out) {
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < n; j += gridDim.x * blockDim.x) {
        reinterpret_cast<float4*>(out)[j] = abr::box_encode(reinterpret_cast<const float4*>(gt)[j], reinterpret_cast<const float4*>(ex)[j], wx, wy, ww, wh);
    }
}

}  // namespace

extern "C" int abr_box_encode(const float* gt, const float* ex, int n, float wx, float wy, float ww, float wh, float* out,
                              void* stream) {
    ABR_REQUIRE(n >= 0, "box_encode: bad n");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(gt && ex && out, "box_encode: null pointer");
    box_encode_kernel<<<abr::cdiv(n, 256), 256, 0, abr::as_stream(stream)>>>(gt, ex, n, wx, wy, ww, wh, out);
    ABR_CHECK_LAUNCH("box_encode");
    return ABR_OK;
}

extern "C" int abr_grid_anchors(const float* cell, int A, int H, int W, int stride, int img_h, int img_w, int straddle,
                                float* out, uint8_t* vis, void* stream) {
    ABR_REQUIRE(cell && out && A > 0 && H > 0 && W > 0, "grid_anchors: bad args");
    grid_anchors_kernel<<<abr::cdiv((int64_t)H * W * A, 256), 256, 0, abr::as_stream(stream)>>>(cell, A, H, W, stride, img_h,
                                                                                                  img_w, straddle, out, vis);
    ABR_CHECK_LAUNCH("grid_anchors");
    return ABR_OK;
}

extern "C" int abr_rpn_decode_clip(const float* reg, int reg_stride, int reg_col0, int A, const float* anchors, const int64_t* idx,
                                   int N, int n_anchor, int k, const int32_t* img_hw, float wx, float wy, float ww, float wh,
                                   float* out, void* stream) {
    ABR_REQUIRE(N >= 0 && k >= 0 && reg_stride >= 4 && A >= 1 && n_anchor % A == 0, "rpn_decode_clip: bad args");
    if (N == 0 || k == 0) return ABR_OK;
    ABR_REQUIRE(reg && anchors && idx && out, "rpn_decode_clip: null pointer");
    decode_clip_kernel<<<abr::cdiv((int64_t)N * k, 256), 256, 0, abr::as_stream(stream)>>>(
        reg, reg_stride, reg_col0, A, anchors, idx, N, n_anchor, k, img_hw, wx, wy, ww, wh, out);
    ABR_CHECK_LAUNCH("rpn_decode_clip");
    return ABR_OK;
}

extern "C" int64_t abr_match_workspace_bytes(int n, int G) { return (int64_t)(G > 0 ? G : 1) * 4; }

extern "C" int abr_match_encode(const float* boxes, int n, const float* gt, const int64_t* gt_labels, int G,
                                const uint8_t* vis, float hi, float lo, int allow_low_quality, float wx, float wy, float ww,
                                float wh, int64_t* matched, float* labels_f32, int64_t* labels_i64, float* reg_targets,
                                void* workspace, int64_t workspace_bytes, void* stream) {
    ABR_REQUIRE(n >= 0, "match_encode: bad n");
    // Matcher raises on empty GT (matcher.py:53-62 "No ground-truth boxes available for one of the images")
    ABR_REQUIRE(G > 0, "match_encode: no ground-truth boxes available for one of the images during training");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(boxes && gt, "match_encode: null pointer");
    hipStream_t st = abr::as_stream(stream);
    unsigned* rowmax = nullptr;
    if (allow_low_quality) {
        ABR_REQUIRE(workspace && workspace_bytes >= abr_match_workspace_bytes(n, G), "match_encode: workspace too small");
        rowmax = (unsigned*)workspace;
        if (hipMemsetAsync(rowmax, 0, 4 * (size_t)G, st) != hipSuccess) return ABR_E_LAUNCH;
        gt_max_iou_kernel<<<std::min(abr::cdiv(n, 1024), 64u), 256, 0, st>>>(boxes, n, gt, G, rowmax);
    }
    match_encode_kernel<<<abr::cdiv(n, 256), 256, 0, st>>>(boxes, n, gt, gt_labels, G, vis, hi, lo, rowmax,
                                                           wx, wy, ww, wh, matched, labels_f32, labels_i64, reg_targets);
    ABR_CHECK_LAUNCH("match_encode");
    return ABR_OK;
}

extern "C" int abr_roi_head_targets(const float* props, const int32_t* keep, const int32_t* n_keep, int N, int k_pre, int post,
                                    const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt, int g_max,
                                    float hi, float lo, float wx, float wy, float ww, float wh, int batch_size, int max_pos,
                                    uint64_t seed, float* cand, int64_t* labels_all, float* regt_all, int32_t* n_cand, int64_t* pos_idx,
                                    int64_t* neg_idx, int32_t* counts, float* rois, int64_t* labels, float* reg_targets,
                                    int64_t* sampled_idx, float* n_valid, const float* scores, float* obj_all, float* obj,
                                    int64_t* pos_rows, int64_t* col0, int num_classes, int cls_agnostic, void* stream) {
    ABR_REQUIRE(N > 0 && k_pre > 0 && post > 0 && g_max > 0 && batch_size > 0 && max_pos >= 0 && max_pos <= batch_size,
                "roi_head_targets: bad sizes");
    ABR_REQUIRE(props && keep && n_keep && gt_ptrs && gt_label_ptrs && n_gt && cand && labels_all && regt_all && n_cand && pos_idx && neg_idx &&
                counts && rois && labels && reg_targets && sampled_idx && n_valid && scores && obj_all && obj && pos_rows && col0,
                "roi_head_targets: null pointer");
    const abr::roi_targets::KeepFetch f{props, scores, keep, n_keep, k_pre, post};
    const abr::roi_targets::Outputs o{cand, labels_all, regt_all, n_cand, pos_idx, neg_idx, counts, rois, labels, reg_targets, sampled_idx, n_valid,
                                      obj_all, obj, pos_rows, col0};
    return abr::roi_targets::run("roi_head_targets", f, N, post + g_max, gt_ptrs, gt_label_ptrs, n_gt, hi, lo, wx, wy, ww, wh, batch_size, max_pos,
                                 seed, o, num_classes, cls_agnostic, stream);
}

extern "C" int abr_gather_proposals(const float* props, const float* scores, const int32_t* keep, int N, int k_pre, int post,
                                    const int64_t* picks, int P, float* rois, float* obj, void* stream) {
    ABR_REQUIRE(N >= 0 && P >= 0 && k_pre > 0 && post > 0, "gather_proposals: bad sizes");
    if (N * P == 0) return ABR_OK;
    ABR_REQUIRE(props && keep && picks && rois && (!obj || scores), "gather_proposals: null pointer");
    gather_proposals_kernel<<<abr::cdiv((int64_t)N * P, 256), 256, 0, abr::as_stream(stream)>>>(props, scores, keep, k_pre, post, picks, N, P, rois, obj);
    ABR_CHECK_LAUNCH("gather_proposals");
    return ABR_OK;
}

extern "C" int abr_rpn_targets_batched(const float* anchors, int n, int N, const float* const* gt_ptrs, const int32_t* n_gt, int g_max,
                                       const uint8_t* const* vis_ptrs, float hi, float lo, float wx, float wy, float ww, float wh,
                                       float* labels, float* reg_targets, void* workspace, int64_t workspace_bytes, void* stream) {
    ABR_REQUIRE(n >= 0 && N > 0 && g_max > 0, "rpn_targets_batched: bad sizes");
    if (n == 0) return ABR_OK;
    ABR_REQUIRE(anchors && gt_ptrs && n_gt && vis_ptrs && labels && reg_targets && workspace, "rpn_targets_batched: null pointer");
    ABR_REQUIRE(workspace_bytes >= (int64_t)N * g_max * 4, "rpn_targets_batched: workspace too small");
    hipStream_t st = abr::as_stream(stream);
    unsigned* rowmax = (unsigned*)workspace;
    if (hipMemsetAsync(rowmax, 0, 4 * (size_t)N * g_max, st) != hipSuccess) return ABR_E_LAUNCH;
    gt_max_iou_batched_kernel<<<dim3(std::min(abr::cdiv(n, 1024), 64u), N), 256, 0, st>>>(anchors, n, gt_ptrs, n_gt, g_max, rowmax);
    rpn_match_batched_kernel<<<dim3(abr::cdiv(n, 256), N), 256, 0, st>>>(anchors, n, gt_ptrs, n_gt, g_max, vis_ptrs, hi, lo, rowmax, wx, wy, ww, wh,
                                                                          labels, reg_targets);
    ABR_CHECK_LAUNCH("rpn_targets_batched");
    return ABR_OK;
}

extern "C" int abr_rpn_loss_indices(const int64_t* pos, int n_pos, const int64_t* neg, int n_neg, const int32_t* counts, int n_img, int A,
                                    int Cf, int64_t* samp, int64_t* obj_flat, int64_t* pos_row, int64_t* pos_col, float* denom, void* stream) {
    ABR_REQUIRE(n_pos >= 0 && n_neg >= 0 && n_img > 0 && A > 0 && Cf >= 5 * A, "rpn_loss_indices: bad sizes");
    ABR_REQUIRE(pos && neg && counts && samp && obj_flat && pos_row && pos_col && denom, "rpn_loss_indices: null pointer");
    rpn_loss_indices_kernel<<<abr::cdiv(std::max(n_pos + n_neg, 1), 256), 256, 0, abr::as_stream(stream)>>>(pos, n_pos, neg, n_neg, counts, n_img, A, Cf,
                                                                                                             samp, obj_flat, pos_row, pos_col, denom);
    ABR_CHECK_LAUNCH("rpn_loss_indices");
    return ABR_OK;
}

// Box-head training targets for the whole batch without leaving the device: the device code shared by abr_roi_head_targets (rpn.hip: the
// candidates are rows keep[i, :n_keep[i]] of the decoded score-sorted boxes) and abr_roi_head_targets_table (box_head_fpn.hip: the candidates
// are rows [0, n_out[i]) of the pyramid selector's table).  One copy of the matching, encoding and gathering; the two entry points differ only
// in how a candidate row is fetched (the `Fetch` functor below).
//   candidate list of image i = its proposals followed by its ground-truth boxes (rpn/inference.py:53-74 add_gt_proposals); every candidate
//   is matched against the image's GT (Matcher 0.5 / 0.5, no low-quality rule), labelled and encoded (box_head/loss.py:56-84) -- through the
//   functions match_encode_kernel (rpn.hip) calls: abr::match_scan, match_index, head_label, box_encode (box_math.h).
#pragma once
#include "box_math.h"

extern "C" int abr_sample_pos_neg(const void* labels, int labels_are_int64, int N, int n, int64_t stride, int batch_size, int max_pos,
                                  uint64_t seed, int first_image, int64_t index_offset_per_image, int64_t* pos_idx,
                                  int64_t* neg_idx, int32_t* counts, void* stream);

namespace abr {
namespace roi_targets {

// proposals through the NMS keep lists: row j of image i is props[i, keep[i, j]], j < min(n_keep[i], post)
struct KeepFetch {
    const float* props;
    const float* scores;
    const int32_t* keep;
    const int32_t* n_keep;
    int k_pre, post;
    __device__ __forceinline__ int count(int i) const { return min(n_keep[i], post); }
    __device__ __forceinline__ int64_t row(int i, int j) const { return (int64_t)i * k_pre + keep[(int64_t)i * post + j]; }
};

// proposals as a dense table: row j of image i is rois[i, j], j < min(n_out[i], cap) (the pyramid selector's output: no indirection)
struct TableFetch {
    const float* props;
    const float* scores;
    const int32_t* n_out;
    int cap;
    __device__ __forceinline__ int count(int i) const { return min(n_out[i], cap); }
    __device__ __forceinline__ int64_t row(int i, int j) const { return (int64_t)i * cap + j; }
};

template <class Fetch>
__global__ void cand_match_kernel(const Fetch f, const float* const* __restrict__ gt_ptrs, const int64_t* const* __restrict__ gt_label_ptrs,
                                  const int32_t* __restrict__ n_gt, int Pmax, float hi, float lo, float wx, float wy, float ww, float wh,
                                  float* __restrict__ cand, int64_t* __restrict__ labels_all, float* __restrict__ regt_all,
                                  float* __restrict__ obj_all, int32_t* __restrict__ n_cand, float* __restrict__ n_valid) {
#pragma clang fp contract(off)
    const int i = blockIdx.y;
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int nk = f.count(i), G = n_gt[i];
    const int nc = nk + G;
    if (j == 0) {
        n_cand[i] = nc;
        if (i == 0) *n_valid = 0.f;   // (accumulated by roi_merge_gather_kernel, a later launch on the same stream)
    }
    if (j >= Pmax) return;
    const float* gt = gt_ptrs[i];
    const int64_t* gt_labels = gt_label_ptrs[i];
    const int64_t o = (int64_t)i * Pmax + j;
    if (j >= nc) {
        labels_all[o] = -1;   // never sampled
        obj_all[o] = 0.f;
        reinterpret_cast<float4*>(cand)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        reinterpret_cast<float4*>(regt_all)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
    const int64_t src = j < nk ? f.row(i, j) : 0;
    const float4 b = j < nk ? reinterpret_cast<const float4*>(f.props)[src] : reinterpret_cast<const float4*>(gt)[j - nk];
    obj_all[o] = j < nk ? f.scores[src] : 1.f;                                  // GT boxes join with objectness 1 (inference.py:66-68)
    const abr::MatchScan s = abr::match_scan(gt, G, b, nullptr);                // no low-quality rule in the box head
    const int m = abr::match_index(s.best, s.bi, false, hi, lo);
    const int gi = m < 0 ? 0 : m;                                               // clamp(min=0)
    labels_all[o] = abr::head_label(m, gt_labels, gi);
    reinterpret_cast<float4*>(cand)[o] = b;
    reinterpret_cast<float4*>(regt_all)[o] = abr::box_encode(reinterpret_cast<const float4*>(gt)[gi], b, wx, wy, ww, wh);
}

__device__ __forceinline__ int lower_bound_i64(const int64_t* a, int n, int64_t v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The sampler's two ascending index lists of image i merged into ONE ascending list (box_head/loss.py:108-114 takes
// nonzero(pos_mask | neg_mask), i.e. ascending candidate order) and the sampled rows gathered: rois (batch index, box), labels,
// regression targets.  Rows past the number drawn are padding: label -1 (ignored by the loss kernels), a zero box of image i.
static __global__ __launch_bounds__(256) void roi_merge_gather_kernel(const float* __restrict__ cand, const int64_t* __restrict__ labels_all,
                                                                      const float* __restrict__ regt_all, const float* __restrict__ obj_all,
                                                                      int Pmax, const int64_t* __restrict__ pos_idx, int max_pos,
                                                                      const int64_t* __restrict__ neg_idx, int batch,
                                                                      const int32_t* __restrict__ counts, float* __restrict__ rois,
                                                                      int64_t* __restrict__ labels, float* __restrict__ reg_targets,
                                                                      int64_t* __restrict__ sampled_idx, float* __restrict__ obj,
                                                                      int64_t* __restrict__ pos_rows, int64_t* __restrict__ col0,
                                                                      int num_classes, int cls_agnostic, float* __restrict__ n_valid) {
    const int i = blockIdx.x;
    const int cp = counts[2 * i], cn = counts[2 * i + 1];
    const int64_t* pos = pos_idx + (int64_t)i * max_pos;
    const int64_t* neg = neg_idx + (int64_t)i * batch;
    for (int e = threadIdx.x; e < batch; e += blockDim.x) {
        int64_t v = -1;
        int rank;
        if (e < cp) {
            v = pos[e];
            rank = e + lower_bound_i64(neg, cn, v);
        } else if (e < cp + cn) {
            v = neg[e - cp];
            rank = (e - cp) + lower_bound_i64(pos, cp, v);
        } else {
            rank = e;   // padding rows keep their place behind the drawn ones
        }
        const int64_t row = (int64_t)i * batch + rank;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f), t = b;
        int64_t l = -1;
        float ob = 0.f;
        if (v >= 0) {
            const int64_t o = (int64_t)i * Pmax + v;
            b = reinterpret_cast<const float4*>(cand)[o];
            t = reinterpret_cast<const float4*>(regt_all)[o];
            l = labels_all[o];
            ob = obj_all[o];
        }
        obj[row] = ob;
        pos_rows[row] = l > 0 ? row : -1;                                      // rows entering the box-regression loss (loss.py:166)
        col0[row] = num_classes + (cls_agnostic ? 4 : 4 * (l > 0 ? l : 0));    // their 4 columns of the fused predictor output (:168-171)
        float* r = rois + row * 5;
        r[0] = (float)i; r[1] = b.x; r[2] = b.y; r[3] = b.z; r[4] = b.w;
        labels[row] = l;
        reinterpret_cast<float4*>(reg_targets)[row] = t;
        sampled_idx[row] = v;
    }
    if (threadIdx.x == 0) atomicAdd(n_valid, (float)(cp + cn));
}

// everything the two entry points write besides the fetch: see abr_roi_head_targets (include/abr_iod_hip.h)
struct Outputs {
    float* cand; int64_t* labels_all; float* regt_all; int32_t* n_cand; int64_t* pos_idx; int64_t* neg_idx; int32_t* counts;
    float* rois; int64_t* labels; float* reg_targets; int64_t* sampled_idx; float* n_valid; float* obj_all; float* obj;
    int64_t* pos_rows; int64_t* col0;
    bool complete() const {
        return cand && labels_all && regt_all && n_cand && pos_idx && neg_idx && counts && rois && labels && reg_targets && sampled_idx &&
               n_valid && obj_all && obj && pos_rows && col0;
    }
};

// match -> sample -> merge + gather: three launches on `stream`, Pmax = (rows a Fetch can hand out) + g_max candidates per image
template <class Fetch>
int run(const char* what, const Fetch& f, int N, int Pmax, const float* const* gt_ptrs, const int64_t* const* gt_label_ptrs, const int32_t* n_gt,
        float hi, float lo, float wx, float wy, float ww, float wh, int batch_size, int max_pos, uint64_t seed, const Outputs& o,
        int num_classes, int cls_agnostic, void* stream) {
    hipStream_t st = abr::as_stream(stream);
    cand_match_kernel<Fetch><<<dim3(abr::cdiv(Pmax, 256), N), 256, 0, st>>>(f, gt_ptrs, gt_label_ptrs, n_gt, Pmax, hi, lo, wx, wy, ww, wh, o.cand,
                                                                             o.labels_all, o.regt_all, o.obj_all, o.n_cand, o.n_valid);
    ABR_CHECK_LAUNCH(what);
    const int rc = abr_sample_pos_neg(o.labels_all, 1, N, Pmax, Pmax, batch_size, max_pos, seed, 0, 0, o.pos_idx, o.neg_idx, o.counts, stream);
    if (rc != ABR_OK) return rc;
    roi_merge_gather_kernel<<<N, 256, 0, st>>>(o.cand, o.labels_all, o.regt_all, o.obj_all, Pmax, o.pos_idx, max_pos, o.neg_idx, batch_size, o.counts,
                                               o.rois, o.labels, o.reg_targets, o.sampled_idx, o.obj, o.pos_rows, o.col0, num_classes, cls_agnostic,
                                               o.n_valid);
    ABR_CHECK_LAUNCH(what);
    return ABR_OK;
}

}  // namespace roi_targets
}  // namespace abr

// COCO detection scoring (evaluation/coco/coco_eval.py): the per-image work of pycocotools' COCOeval, restated.
// A GROUP is one (image, category) pair: its detections in rank order (score descending, stable, at most maxDets) and its ground truths
// in file order.  All groups of a batch lie flat behind offset tables and every kernel runs once for the batch:
//   box IoU    bbIou on xywh boxes in float64: one thread per (detection, ground truth) pair, its group found by bisection
//   mask IoU   the integer counts of abr_mask_pair_counts -> float64 under the same crowd rule
//   match      evaluateImg for all area ranges and IoU thresholds at once: one wave per group, one lane per (area range, threshold);
//              the loop over detections is serial by definition, a lane's state is one bit per ground truth
// Every float64 expression is written one rounding per operation (contraction off): the results are the host restatement's bit for bit.
#include "common.h"

namespace {

constexpr int kMaxGt = ABR_COCO_MATCH_MAX_GT;   // ground truths per group the match kernel holds (two 64-bit words of per-lane state)
constexpr int kMaxAreas = 8;

// the group that owns flat element e: the last g with off[g] <= e (empty groups have off[g] == off[g+1] and are stepped over)
__device__ __forceinline__ int owner_group(const int64_t* __restrict__ off, int n_groups, int64_t e) {
    int lo = 0, hi = n_groups - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (off[mid] <= e) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__global__ __launch_bounds__(256) void coco_box_iou_kernel(const double* __restrict__ det, const double* __restrict__ gt,
                                                           const uint8_t* __restrict__ gt_crowd, const int64_t* __restrict__ det_off,
                                                           const int64_t* __restrict__ gt_off, const int64_t* __restrict__ iou_off, int n_groups,
                                                           int64_t total, double* __restrict__ iou) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int grp = owner_group(iou_off, n_groups, e);
    const int64_t G = gt_off[grp + 1] - gt_off[grp];
    if (G <= 0) return;                                    // (tables that disagree: nothing is read through them)
    const int64_t r = e - iou_off[grp];
    const int64_t di = det_off[grp] + r / G, gi = gt_off[grp] + r % G;
    const double dx = det[4 * di], dy = det[4 * di + 1], dw = det[4 * di + 2], dh = det[4 * di + 3];
    const double gx = gt[4 * gi], gy = gt[4 * gi + 1], gw = gt[4 * gi + 2], gh = gt[4 * gi + 3];
    double out = 0.0;
    const double w = fmin(dw + dx, gw + gx) - fmax(dx, gx);
    const double h = fmin(dh + dy, gh + gy) - fmax(dy, gy);
    if (w > 0.0 && h > 0.0) {
        const double da = dw * dh, ga = gw * gh, i = w * h;
        const double u = gt_crowd[gi] ? da : da + ga - i;
        out = i / u;
    }
    iou[e] = out;
}

__global__ __launch_bounds__(256) void coco_mask_iou_kernel(const int32_t* __restrict__ inter, const int32_t* __restrict__ area_p,
                                                            const int32_t* __restrict__ area_t, const uint8_t* __restrict__ gt_crowd, int64_t total,
                                                            int T, double* __restrict__ iou) {
#pragma clang fp contract(off)
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int64_t p = e / T, t = e % T;
    const int64_t i = inter[e];
    const int64_t u = gt_crowd[t] ? (int64_t)area_p[p] : (int64_t)area_p[p] + (int64_t)area_t[t] - i;
    iou[e] = i > 0 ? (double)i / (double)u : 0.0;     // (i > 0 implies u >= i > 0)
}

// One wave per group.  Lane p < A * T owns (area range p / T, threshold p % T).  gt_ignore is the protocol's `ignore` flag of a ground truth
// (boxes and masks: its crowd flag; keypoints: crowd or no labelled keypoint); gt_crowd alone lets a matched ground truth match again.  Groups with more than kMaxGt ground truths are counted in
// *n_over and left untouched: the caller scores them on the host.
__global__ __launch_bounds__(64) void coco_match_kernel(const double* __restrict__ iou, const int64_t* __restrict__ iou_off,
                                                        const int64_t* __restrict__ det_off, const int64_t* __restrict__ gt_off,
                                                        const double* __restrict__ det_area, const double* __restrict__ gt_area,
                                                        const uint8_t* __restrict__ gt_crowd, const uint8_t* __restrict__ gt_ignore,
                                                        const double* __restrict__ area_rng, int A, const double* __restrict__ thrs, int T, int64_t d_total, int64_t g_total,
                                                        int32_t* __restrict__ dt_gt, uint8_t* __restrict__ dt_ig, uint8_t* __restrict__ gt_ig,
                                                        int32_t* __restrict__ n_over) {
    __shared__ double s_row[kMaxGt];                       // the current detection's IoUs, shared by all lanes
    __shared__ uint8_t s_order[kMaxAreas][kMaxGt];         // per area range: ground-truth rows, the non-ignored first, stable
    __shared__ unsigned long long s_ig[kMaxAreas][2];      // per area range: bit g set iff ground truth g is ignored
    __shared__ unsigned long long s_crowd[2];
    const int grp = blockIdx.x, lane = threadIdx.x;
    const int64_t d0 = det_off[grp], g0 = gt_off[grp];
    const int D = (int)(det_off[grp + 1] - d0), G = (int)(gt_off[grp + 1] - g0);
    if (G > kMaxGt) {                                      // (block-uniform)
        if (lane == 0) atomicAdd(n_over, 1);
        return;
    }
    if (lane < A) {
        const double lo = area_rng[2 * lane], hi = area_rng[2 * lane + 1];
        unsigned long long ig[2] = {0ull, 0ull}, cr[2] = {0ull, 0ull};
        int k = 0;
        for (int g = 0; g < G; g++) {
            const double a = gt_area[g0 + g];
            const bool crowd = gt_crowd[g0 + g] != 0;
            const bool ignored = gt_ignore[g0 + g] != 0 || a < lo || a > hi;
            if (ignored) ig[g >> 6] |= 1ull << (g & 63); else s_order[lane][k++] = (uint8_t)g;
            if (crowd) cr[g >> 6] |= 1ull << (g & 63);
            gt_ig[(int64_t)lane * g_total + g0 + g] = ignored ? 1 : 0;
        }
        for (int g = 0; g < G; g++)
            if ((ig[g >> 6] >> (g & 63)) & 1ull) s_order[lane][k++] = (uint8_t)g;
        s_ig[lane][0] = ig[0];
        s_ig[lane][1] = ig[1];
        if (lane == 0) {
            s_crowd[0] = cr[0];
            s_crowd[1] = cr[1];
        }
    }
    __syncthreads();
    const bool active = lane < A * T;
    const int a = active ? lane / T : 0, t = active ? lane % T : 0;
    const double lo = area_rng[2 * a], hi = area_rng[2 * a + 1];
    const double thr = fmin(thrs[t], 1.0 - 1e-10);
    const unsigned long long ig0 = s_ig[a][0], ig1 = s_ig[a][1], cr0 = s_crowd[0], cr1 = s_crowd[1];
    unsigned long long m0 = 0ull, m1 = 0ull;               // bit g set iff ground truth g is matched at this (area range, threshold)
    const double* mat = iou + iou_off[grp];
    for (int d = 0; d < D; d++) {
        __syncthreads();                                   // (the previous row has been read by every lane)
        for (int g = lane; g < G; g += 64) s_row[g] = mat[(int64_t)d * G + g];
        __syncthreads();
        if (!active) continue;
        double best = thr;
        int m = -1;
        bool m_ig = false;
        for (int k = 0; k < G; k++) {
            const int g = s_order[a][k];
            const unsigned long long bit = 1ull << (g & 63);
            const bool hi_word = g >= 64;
            const bool matched = ((hi_word ? m1 : m0) & bit) != 0, crowd = ((hi_word ? cr1 : cr0) & bit) != 0;
            const bool g_ig = ((hi_word ? ig1 : ig0) & bit) != 0;
            if (matched && !crowd) continue;
            if (m >= 0 && !m_ig && g_ig) break;
            const double v = s_row[g];
            if (v < best) continue;
            best = v;
            m = g;
            m_ig = g_ig;
        }
        const int64_t o = ((int64_t)a * T + t) * d_total + d0 + d;
        if (m >= 0) {
            if (m >= 64) m1 |= 1ull << (m & 63); else m0 |= 1ull << (m & 63);
            dt_gt[o] = m;
            dt_ig[o] = m_ig ? 1 : 0;
        } else {
            const double da = det_area[d0 + d];
            dt_gt[o] = -1;
            dt_ig[o] = (da < lo || da > hi) ? 1 : 0;
        }
    }
}

}  // namespace

extern "C" int abr_coco_match_max_gt(void) { return kMaxGt; }

extern "C" int abr_coco_box_iou(const double* det, const double* gt, const uint8_t* gt_crowd, const int64_t* det_off, const int64_t* gt_off,
                                const int64_t* iou_off, int n_groups, int64_t total, double* iou, void* stream) {
    ABR_REQUIRE(n_groups >= 0 && total >= 0, "coco_box_iou: bad args (n_groups, total >= 0)");
    if (n_groups == 0 || total == 0) return ABR_OK;
    ABR_REQUIRE(det && gt && gt_crowd && det_off && gt_off && iou_off && iou, "coco_box_iou: null pointer");
    ABR_REQUIRE((total + 255) / 256 < ((int64_t)1 << 31), "coco_box_iou: too many pairs for one launch");
    coco_box_iou_kernel<<<abr::cdiv(total, 256), 256, 0, abr::as_stream(stream)>>>(det, gt, gt_crowd, det_off, gt_off, iou_off, n_groups, total, iou);
    ABR_CHECK_LAUNCH("coco_box_iou");
    return ABR_OK;
}

extern "C" int abr_coco_mask_iou(const int32_t* inter, const int32_t* area_p, const int32_t* area_t, const uint8_t* gt_crowd, int P, int T,
                                 double* iou, void* stream) {
    ABR_REQUIRE(P >= 0 && T >= 0, "coco_mask_iou: bad args (P, T >= 0)");
    if (P == 0 || T == 0) return ABR_OK;
    ABR_REQUIRE(inter && area_p && area_t && gt_crowd && iou, "coco_mask_iou: null pointer");
    const int64_t total = (int64_t)P * T;
    coco_mask_iou_kernel<<<abr::cdiv(total, 256), 256, 0, abr::as_stream(stream)>>>(inter, area_p, area_t, gt_crowd, total, T, iou);
    ABR_CHECK_LAUNCH("coco_mask_iou");
    return ABR_OK;
}

extern "C" int abr_coco_match_ig(const double* iou, const int64_t* iou_off, const int64_t* det_off, const int64_t* gt_off, const double* det_area,
                                 const double* gt_area, const uint8_t* gt_crowd, const uint8_t* gt_ignore, int n_groups, int64_t d_total,
                                 int64_t g_total, const double* area_rng, int A, const double* thrs, int T, int32_t* dt_gt, uint8_t* dt_ig,
                                 uint8_t* gt_ig, int32_t* n_over, void* stream) {
    ABR_REQUIRE(n_groups >= 0 && d_total >= 0 && g_total >= 0, "coco_match: bad args (n_groups, d_total, g_total >= 0)");
    ABR_REQUIRE(A >= 1 && A <= kMaxAreas && T >= 1 && A * T <= 64, "coco_match: bad args (1 <= A <= 8, T >= 1, A * T <= 64: one lane per pair)");
    if (n_groups == 0) return ABR_OK;
    ABR_REQUIRE(iou_off && det_off && gt_off && area_rng && thrs && n_over, "coco_match: null pointer");
    ABR_REQUIRE((d_total == 0 || (det_area && dt_gt && dt_ig)) && (g_total == 0 || (gt_area && gt_crowd && gt_ignore && gt_ig)) &&
                    (d_total == 0 || g_total == 0 || iou), "coco_match: null pointer");
    coco_match_kernel<<<n_groups, 64, 0, abr::as_stream(stream)>>>(iou, iou_off, det_off, gt_off, det_area, gt_area, gt_crowd, gt_ignore, area_rng, A,
                                                                   thrs, T, d_total, g_total, dt_gt, dt_ig, gt_ig, n_over);
    ABR_CHECK_LAUNCH("coco_match");
    return ABR_OK;
}

// boxes and masks: a ground truth is ignored exactly when it is a crowd
extern "C" int abr_coco_match(const double* iou, const int64_t* iou_off, const int64_t* det_off, const int64_t* gt_off, const double* det_area,
                              const double* gt_area, const uint8_t* gt_crowd, int n_groups, int64_t d_total, int64_t g_total,
                              const double* area_rng, int A, const double* thrs, int T, int32_t* dt_gt, uint8_t* dt_ig, uint8_t* gt_ig,
                              int32_t* n_over, void* stream) {
    return abr_coco_match_ig(iou, iou_off, det_off, gt_off, det_area, gt_area, gt_crowd, gt_crowd, n_groups, d_total, g_total, area_rng, A, thrs, T,
                             dt_gt, dt_ig, gt_ig, n_over, stream);
}

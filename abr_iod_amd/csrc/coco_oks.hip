// COCO keypoint scoring (evaluation/coco/coco_eval.py, iou type "keypoints"): pycocotools' computeOks restated.
// Object keypoint similarity of every (detection, ground truth) pair of every group of a batch in one launch, in float64, written in
// abr_coco_box_iou's layout: the groups' row-major D_k x G_k matrices behind iou_off.
//   oks(d, g) = sum_k exp(-e_k) / n,   e_k = (dx_k^2 + dy_k^2) / var_k / (area_g + 2^-52) / 2
// over the ground truth's visible keypoints (n = their count k1), or, when it has none, over all K with dx, dy the distances to the
// ground truth's doubled box.  Every e_k is written one rounding per operation (contraction off) and the sum runs serially in keypoint
// order: against the host restatement only exp can differ.
//
// Shape.  A pair costs K float64 exps (some tens of float64 VALU instructions each) for 8 bytes written and 32 * K bytes of operands,
// so the kernel sits under the float64 VALU bound as long as the operands come from LDS: one thread per pair reading them from global
// memory would put 32 * K bytes per pair through the CU's 64 B/clk L1.  A workgroup owns a group; it walks the group's tiles of at most
// 32 ground truths x 64 detections (at most 256 pairs, one per thread, ground truth fastest so that the stores coalesce and few waves
// are busy in a small group) and, inside a tile, chunks of 24 keypoints, staged keypoint-major in LDS: lanes with consecutive ground
// truths read consecutive 16-byte words, lanes of one detection read one word (a broadcast).  gridDim.y workgroups share a group's
// detection tiles.  K, D and G are unbounded: LDS holds a chunk, never a whole row.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kTg = 32;      // ground truths per tile
constexpr int kTd = 64;      // detections per tile (and kTd * tg <= kThreads)
constexpr int kKc = 24;      // keypoints per staged chunk: (65 + 33) * 16 B * 24 = 37 KB of LDS, four workgroups per CU

__global__ __launch_bounds__(kThreads) void coco_oks_kernel(const double* __restrict__ det_kp, const double* __restrict__ gt_kp,
                                                            const double* __restrict__ gt_box, const double* __restrict__ gt_area,
                                                            const double* __restrict__ var, const int64_t* __restrict__ det_off,
                                                            const int64_t* __restrict__ gt_off, const int64_t* __restrict__ iou_off, int K,
                                                            double* __restrict__ oks) {
#pragma clang fp contract(off)
    __shared__ double2 s_d[kKc][kTd + 1];                  // (x, y) of the tile's detections; rows padded by one word: conflict-free staging
    __shared__ double2 s_g[kKc][kTg + 1];                  // (x, y) of the tile's ground truths
    __shared__ uint8_t s_v[kKc][kTg];                      // the ground truth's keypoint is visible (v > 0)
    __shared__ int s_k1[kTg];                              // visible keypoints of each ground truth of the tile
    const int grp = blockIdx.x, tid = threadIdx.x;
    const int64_t d_base = det_off[grp], g_base = gt_off[grp];
    const int64_t D = det_off[grp + 1] - d_base, G = gt_off[grp + 1] - g_base;
    if (D <= 0 || G <= 0 || iou_off[grp + 1] - iou_off[grp] != D * G) return;      // (block-uniform; tables that disagree: nothing is written)
    double* __restrict__ mat = oks + iou_off[grp];
    for (int64_t g0 = 0; g0 < G; g0 += kTg) {
        const int tg = (int)(G - g0 < kTg ? G - g0 : kTg);
        const int td_cap = kThreads / tg < kTd ? kThreads / tg : kTd;
        for (int64_t d0 = (int64_t)blockIdx.y * td_cap; d0 < D; d0 += (int64_t)gridDim.y * td_cap) {
            const int td = (int)(D - d0 < td_cap ? D - d0 : td_cap);
            const int dl = tid / tg, gl = tid % tg;
            const bool active = dl < td;
            __syncthreads();                               // (the previous tile's s_k1 has been read)
            if (tid < tg) {
                const double* v = gt_kp + (g_base + g0 + tid) * K * 3 + 2;
                int c = 0;
                for (int k = 0; k < K; k++) c += v[3 * (int64_t)k] > 0.0 ? 1 : 0;
                s_k1[tid] = c;
            }
            __syncthreads();
            int k1 = 0;
            double x0 = 0.0, x1 = 0.0, y0 = 0.0, y1 = 0.0, den = 1.0;
            if (active) {
                const int64_t gi = g_base + g0 + gl;
                k1 = s_k1[gl];
                const double bx = gt_box[4 * gi], by = gt_box[4 * gi + 1], bw = gt_box[4 * gi + 2], bh = gt_box[4 * gi + 3];
                x0 = bx - bw;
                x1 = bx + bw * 2.0;
                y0 = by - bh;
                y1 = by + bh * 2.0;
                den = gt_area[gi] + 0x1p-52;
            }
            double sum = 0.0;
            for (int kc = 0; kc < K; kc += kKc) {
                const int kn = K - kc < kKc ? K - kc : kKc;
                __syncthreads();                           // (the previous chunk has been read by every thread)
                for (int i = tid; i < td * kn; i += kThreads) {
                    const int r = i / kn, k = i % kn;
                    const double* p = det_kp + ((d_base + d0 + r) * K + kc + k) * 3;
                    s_d[k][r] = make_double2(p[0], p[1]);
                }
                for (int i = tid; i < tg * kn; i += kThreads) {
                    const int r = i / kn, k = i % kn;
                    const double* p = gt_kp + ((g_base + g0 + r) * K + kc + k) * 3;
                    s_g[k][r] = make_double2(p[0], p[1]);
                    s_v[k][r] = p[2] > 0.0 ? 1 : 0;
                }
                __syncthreads();
                if (!active) continue;
                for (int k = 0; k < kn; k++) {
                    const double2 d = s_d[k][dl], g = s_g[k][gl];
                    double dx, dy;
                    if (k1 > 0) {
                        if (!s_v[k][gl]) continue;
                        dx = d.x - g.x;
                        dy = d.y - g.y;
                    } else {
                        dx = fmax(0.0, x0 - d.x) + fmax(0.0, d.x - x1);
                        dy = fmax(0.0, y0 - d.y) + fmax(0.0, d.y - y1);
                    }
                    const double e = (dx * dx + dy * dy) / var[kc + k] / den / 2.0;
                    sum = sum + exp(-e);
                }
            }
            if (active) mat[(d0 + dl) * G + g0 + gl] = sum / (double)(k1 > 0 ? k1 : K);
        }
    }
}

}  // namespace

extern "C" int abr_coco_oks(const double* det_kp, const double* gt_kp, const double* gt_box, const double* gt_area, const double* var, int K,
                            const int64_t* det_off, const int64_t* gt_off, const int64_t* iou_off, int n_groups, int64_t total, double* oks,
                            void* stream) {
    ABR_REQUIRE(n_groups >= 0 && total >= 0 && K >= 1, "coco_oks: bad args (n_groups, total >= 0, K >= 1)");
    if (n_groups == 0 || total == 0) return ABR_OK;
    ABR_REQUIRE(det_kp && gt_kp && gt_box && gt_area && var && det_off && gt_off && iou_off && oks, "coco_oks: null pointer");
    // a group's detection tiles are shared by gridDim.y workgroups: as many as an average group has tiles of 256 pairs, at most 64
    const int64_t per_group = (total + n_groups - 1) / n_groups;
    const int64_t gy = (per_group + kThreads - 1) / kThreads;
    coco_oks_kernel<<<dim3((unsigned)n_groups, (unsigned)(gy < 1 ? 1 : gy > 64 ? 64 : gy)), kThreads, 0, abr::as_stream(stream)>>>(
        det_kp, gt_kp, gt_box, gt_area, var, det_off, gt_off, iou_off, K, oks);
    ABR_CHECK_LAUNCH("coco_oks");
    return ABR_OK;
}

#!/usr/bin/env python
"""Time the COCO keypoint scoring kernels beside the host restatement on the same synthetic groups.

    python tools/coco_kp_eval_bench.py --images 5000

Synthetic detections of a person-keypoint dataset: one category, 17 keypoints, at most 20 detections and a few ground truths per image
(some crowds, some without a labelled keypoint, visibilities in {0, 1, 2}), most ground truths with a detection near them.  Measured:
  * ops.coco_oks + ops.coco_match(gt_ignore=...) for the whole batch, uploads and the read-back of the results included (what the
    evaluator pays), best of --repeats after a warm-up; coco_eval_host.oks + evaluate_img over the same groups, once;
  * the OKS kernel alone (abr_coco_oks on resident inputs, device events over --kernel-iters launches) as exp terms per second, against
    the bound DESIGN.md section 4 names for it: float64 VALU issue.  A term is one exp(-e_k): about 57 float64 vector instructions in the
    compiled kernel (two IEEE divisions 22, exp 27, the differences, squares and sum 8); the chip issues 256 CUs x 4 SIMDs x 16 float64
    lanes x 2.4 GHz = 39.3e12 of them per second, so no more than 0.69e12 terms per second.  Reported for the batch above, whose groups
    are small (a fraction of one wave per workgroup), and for --dense-groups groups of 128 x 128 pairs, where every tile is full.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

K = 17
F64_VALU_PER_TERM = 57
F64_LANE_INSTR_PER_S = 256 * 4 * 16 * 2.4e9


def make_groups(n_images, rng):
    groups = []
    for _ in range(n_images):
        G = int(min(12, rng.geometric(0.4))) - int(rng.random() < 0.2)
        D = int(rng.integers(0, 21))
        if D == 0 and G == 0:
            continue
        box = np.concatenate([rng.uniform(0, 400, (G, 2)), rng.uniform(20, 200, (G, 2))], axis=1)
        gt = np.zeros((G, K, 3))
        gt[:, :, 0] = box[:, None, 0] + box[:, None, 2] * rng.random((G, K))
        gt[:, :, 1] = box[:, None, 1] + box[:, None, 3] * rng.random((G, K))
        gt[:, :, 2] = rng.integers(0, 3, (G, K))
        crowd = rng.random(G) < 0.05
        gt[crowd | (rng.random(G) < 0.1), :, 2] = 0
        area = box[:, 2] * box[:, 3] * rng.uniform(0.3, 0.8, G)
        det = np.zeros((D, K, 3))
        det[:, :, :2] = rng.uniform(0, 600, (D, K, 2))
        det[:, :, 2] = 1
        k = min(D, G)
        det[:k, :, :2] = gt[:k, :, :2] + rng.normal(0, 0.05, (k, 1, 1)) * np.sqrt(area[:k, None, None]) * rng.normal(0, 1, (k, K, 2))
        x, y = det[:, :, 0], det[:, :, 1]
        groups.append({"det_kp": det, "gt_kp": gt, "gt_box": box, "gt_area": area, "gt_crowd": crowd,
                       "gt_ignore": crowd | ~(gt[:, :, 2] > 0).any(1),
                       "det_area": (x.max(1) - x.min(1)) * (y.max(1) - y.min(1)) if D else np.zeros(0)})
    return groups


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--dense-groups", type=int, default=512, help="groups of 128 x 128 for the full-tile measurement of the OKS kernel")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from abr_iod_amd import _lib as L
    from abr_iod_amd import ops
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H

    groups = make_groups(args.images, np.random.default_rng(args.seed))
    dc = np.array([len(g["det_area"]) for g in groups])
    gc = np.array([len(g["gt_area"]) for g in groups])
    cat = lambda key, shape: np.concatenate([g[key].reshape(shape) for g in groups])      # noqa: E731
    det, gt, box, area = cat("det_kp", (-1, K, 3)), cat("gt_kp", (-1, K, 3)), cat("gt_box", (-1, 4)), cat("gt_area", (-1,))
    crowd, ignore, d_area = cat("gt_crowd", (-1,)), cat("gt_ignore", (-1,)), cat("det_area", (-1,))
    total = int((dc * gc).sum())
    labelled = (gt[:, :, 2] > 0).sum(1)
    terms = int(sum(int(d) * int(np.where(labelled[o: o + g] > 0, labelled[o: o + g], K).sum())
                    for d, g, o in zip(dc, gc, np.concatenate(([0], np.cumsum(gc)[:-1])))))

    def device_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        oks, _ = ops.coco_oks(det, gt, box, area, H.KPT_OKS_SIGMAS, dc, gc)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = ops.coco_match(oks, dc, gc, d_area, area, crowd, H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=ignore)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, out, oks

    device_pass()
    runs = [device_pass() for _ in range(max(1, args.repeats))]
    oks_s, match_s = min(r[0] for r in runs), min(r[1] for r in runs)
    out, oks_dev = runs[-1][2], runs[-1][3].cpu().numpy()

    # the kernel alone, inputs resident: the batch above, and full tiles (--dense-groups groups of 128 x 128, every point labelled)
    def kernel_seconds(det, gt, box, area, dc, gc):
        dev = torch.device("cuda")
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float64)).to(dev)      # noqa: E731
        off = lambda c: torch.from_numpy(np.concatenate(([0], np.cumsum(c))).astype(np.int64)).to(dev)      # noqa: E731
        bufs = [t(det), t(gt), t(box), t(area), t((H.KPT_OKS_SIGMAS * 2) ** 2)]
        offs = [off(dc), off(gc), off(dc * gc)]
        total = int((dc * gc).sum())
        res = torch.empty((total,), dtype=torch.float64, device=dev)

        def launch():
            L.check(L.lib().abr_coco_oks(*[L.ptr(b) for b in bufs], K, *[L.ptr(o) for o in offs], len(dc), total, L.ptr(res), L.stream()), "coco_oks")

        for _ in range(3):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            launch()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e-3 / args.kernel_iters

    kernel_s = kernel_seconds(det, gt, box, area, dc, gc)
    bound_terms_per_s = F64_LANE_INSTR_PER_S / F64_VALU_PER_TERM
    rng = np.random.default_rng(args.seed + 1)
    n, side = args.dense_groups, 128
    dense_gt = np.concatenate([rng.uniform(0, 400, (n * side, K, 2)), np.full((n * side, K, 1), 2.0)], axis=2)
    dense_det = dense_gt.reshape(n, side, K, 3)[:, ::-1].reshape(-1, K, 3) + rng.normal(0, 8, (n * side, K, 3))
    dense_s = kernel_seconds(dense_det, dense_gt, np.tile([0.0, 0.0, 400.0, 400.0], (n * side, 1)), np.full(n * side, 2e4),
                             np.full(n, side), np.full(n, side))
    dense_terms = n * side * side * K

    t0 = time.perf_counter()
    want_oks = [H.oks(g["det_kp"], g["gt_kp"], g["gt_box"], g["gt_area"]) for g in groups]
    t1 = time.perf_counter()
    want = [H.evaluate_img(m, g["det_area"], g["gt_area"], g["gt_crowd"], H.KP_AREA_RNG, H.IOU_THRS, g["gt_ignore"]) for m, g in zip(want_oks, groups)]
    t2 = time.perf_counter()
    host_flat = np.concatenate([m.reshape(-1) for m in want_oks]) if want_oks else np.zeros(0)
    worst = float(np.abs(host_flat - oks_dev).max()) if host_flat.size else 0.0
    same = bool((np.concatenate([w["dt_gt"] for w in want], axis=2) == out["dt_gt"]).all())

    ms = lambda s: round(1e3 * s / args.images, 5)      # noqa: E731
    print(json.dumps({"tool": "coco_kp_eval_bench", "images": args.images, "groups": len(groups), "detections": int(dc.sum()),
                      "ground_truths": int(gc.sum()), "pairs": total, "exp_terms": terms,
                      "device_oks_ms": round(1e3 * oks_s, 3), "device_match_ms": round(1e3 * match_s, 3),
                      "device_oks_ms_per_image": ms(oks_s), "device_match_ms_per_image": ms(match_s),
                      "host_oks_ms_per_image": ms(t1 - t0), "host_match_ms_per_image": ms(t2 - t1),
                      "oks_kernel_us": round(kernel_s * 1e6, 2), "oks_kernel_terms_per_s": round(terms / kernel_s, 1),
                      "f64_valu_bound_terms_per_s": round(bound_terms_per_s, 1),
                      "oks_kernel_share_of_f64_valu_bound": round(terms / kernel_s / bound_terms_per_s, 4),
                      "dense_pairs": n * side * side, "dense_oks_kernel_us": round(dense_s * 1e6, 2),
                      "dense_oks_kernel_terms_per_s": round(dense_terms / dense_s, 1),
                      "dense_oks_kernel_share_of_f64_valu_bound": round(dense_terms / dense_s / bound_terms_per_s, 4),
                      "oks_max_abs_error_vs_host": worst, "fallback_groups": int(out["n_fallback"]), "device_matching_equals_host": same}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

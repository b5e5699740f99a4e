#!/usr/bin/env python
"""Time the COCO scoring kernels beside the host restatement on the same synthetic groups.

    python tools/coco_eval_bench.py --images 500

Synthetic detections of a COCO-like dataset: 80 categories, at most 100 detections per image spread over the categories present, a few
ground truths per (image, category) group, some of them crowds, and a small share of crowded groups with more ground truths than the
match kernel holds (they take the host fallback inside ops.coco_match; the share is reported).  Measured: ops.coco_box_iou + ops.coco_match
for the whole batch (uploads and the read-back of the results included: what the evaluator pays), best of --repeats after a warm-up, and
coco_eval_host.box_iou + evaluate_img over the same groups, once.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_groups(n_images, rng, crowded_share):
    groups = []
    for _ in range(n_images):
        cats = rng.choice(80, size=int(rng.integers(1, 12)), replace=False)
        left = 100
        for _c in cats:
            crowded = rng.random() < crowded_share
            G = int(rng.integers(129, 161)) if crowded else int(min(20, rng.geometric(0.35))) - int(rng.random() < 0.15)
            D = int(min(left, rng.integers(0, 30)))
            left -= D
            if D == 0 and G == 0:
                continue
            gt = np.concatenate([rng.uniform(0, 500, (G, 2)), rng.uniform(4, 200, (G, 2))], axis=1)
            det = np.concatenate([rng.uniform(0, 500, (D, 2)), rng.uniform(4, 200, (D, 2))], axis=1)
            k = min(D, G)
            det[:k] = gt[:k] + rng.normal(0, 4, (k, 4))           # most ground truths have a detection near them
            det[:, 2:] = np.maximum(det[:, 2:], 1.0)
            groups.append({"det": det, "gt": gt, "gt_crowd": rng.random(G) < 0.05, "det_area": det[:, 2] * det[:, 3],
                           "gt_area": gt[:, 2] * gt[:, 3]})
    return groups


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--crowded-share", type=float, default=0.002, help="share of groups with 129..160 ground truths (over the kernel's cap)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from abr_iod_amd import ops
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H

    groups = make_groups(args.images, np.random.default_rng(args.seed), args.crowded_share)
    dc = np.array([len(g["det_area"]) for g in groups])
    gc = np.array([len(g["gt_area"]) for g in groups])
    cat = lambda key, shape: np.concatenate([g[key].reshape(shape) for g in groups])      # noqa: E731
    det, gt, crowd, d_area, g_area = cat("det", (-1, 4)), cat("gt", (-1, 4)), cat("gt_crowd", (-1,)), cat("det_area", (-1,)), cat("gt_area", (-1,))

    def device_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        iou, _ = ops.coco_box_iou(det, gt, crowd, dc, gc)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        out = ops.coco_match(iou, dc, gc, d_area, g_area, crowd, H.AREA_RNG, H.IOU_THRS)
        t2 = time.perf_counter()
        return t1 - t0, t2 - t1, out

    device_pass()
    runs = [device_pass() for _ in range(max(1, args.repeats))]
    iou_s, match_s = min(r[0] for r in runs), min(r[1] for r in runs)
    out = runs[-1][2]

    t0 = time.perf_counter()
    ious = [H.box_iou(g["det"], g["gt"], g["gt_crowd"]) for g in groups]
    t1 = time.perf_counter()
    want = [H.evaluate_img(m, g["det_area"], g["gt_area"], g["gt_crowd"]) for m, g in zip(ious, groups)]
    t2 = time.perf_counter()
    same = bool((np.concatenate([w["dt_gt"] for w in want], axis=2) == out["dt_gt"]).all())

    ms = lambda s: round(1e3 * s / args.images, 4)      # noqa: E731
    print(json.dumps({"tool": "coco_eval_bench", "images": args.images, "groups": len(groups), "detections": int(dc.sum()),
                      "ground_truths": int(gc.sum()), "pairs": int((dc * gc).sum()),
                      "device_iou_ms_per_image": ms(iou_s), "device_match_ms_per_image": ms(match_s),
                      "host_iou_ms_per_image": ms(t1 - t0), "host_match_ms_per_image": ms(t2 - t1),
                      "fallback_groups": int(out["n_fallback"]), "fallback_share": round(out["n_fallback"] / max(1, len(groups)), 5),
                      "device_equals_host": same}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

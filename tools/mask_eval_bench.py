"""Instance-mask evaluation per image: the three kernels of csrc/mask_eval.hip, the host matching, and the bytes that cross to the host.

Workload: synthetic VOC-sized images -- the network's 600x1000 canvas, original sizes such as 375x500, 100 detections (pasted uint8
ellipses) of 20 classes and a handful of ground truths.  Per image it reports the device time of resize+pack, pack and pair counts from
device events (median over --iters launches after --warmup), their algorithmic bytes over the HBM peak (8 TB/s), the host time of the
numpy matching over the 9 thresholds, the bytes copied to the host packed against unpacked with the time of each copy, and the time of a
numpy restatement of the reference's masklist_iou on the same masks (its pair loop, run once, times the 9 thresholds the reference runs
it for).  Informational: nothing is asserted.  Prints one JSON line.

    python tools/mask_eval_bench.py --images 4 --iters 20 --warmup 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

NET_H, NET_W = 600, 1000
ORIG = [(375, 500), (333, 500), (500, 375), (480, 640)]     # (height, width)
HBM_PEAK = 8.0e12


def ellipses(rng, n, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        cx, cy, rx, ry = rng.uniform(0.1, 0.9) * W, rng.uniform(0.1, 0.9) * H, rng.uniform(0.05, 0.3) * W, rng.uniform(0.05, 0.3) * H
        out[i] = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1
    return out


def device_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def masklist_iou_numpy(target, predicted, labels_t, labels_p):
    """the reference's pair loop over full-image float masks, for the pairs the metric looks at (same class)"""
    target, predicted = target.astype(np.float32), predicted.astype(np.float32)
    ious = np.zeros((len(predicted), len(target)))
    for p in range(len(predicted)):
        for t in range(len(target)):
            if labels_p[p] != labels_t[t]:
                continue
            d = target[t] - predicted[p]
            tp, fp, fn = int((d[target[t] == 1] == 0).sum()), int((d[target[t] == 0] == -1).sum()), int((d[target[t] == 1] == 1).sum())
            ious[p, t] = tp / (tp + fp + fn) if tp + fp + fn else 0.0
    return ious


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=4)
    ap.add_argument("--dets", type=int, default=100)
    ap.add_argument("--gts", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from abr_iod_amd import ops
    from abr_iod_amd.data.datasets.evaluation.voc import voc_eval_inst as V
    rng = np.random.default_rng(0)
    rows = []
    for i in range(args.images):
        H, W = ORIG[i % len(ORIG)]
        P, T = args.dets, args.gts
        pred = torch.from_numpy(ellipses(rng, P, NET_H, NET_W)).cuda()
        gt = torch.from_numpy(ellipses(rng, T, H, W)).cuda()
        pl, gl = torch.from_numpy(rng.integers(1, 4, P)).cuda(), torch.from_numpy(rng.integers(1, 4, T)).cuda()
        Wq = ops.mask_words_per_row(W)
        t_resize = device_ms(lambda: ops.mask_resize_pack_bits(pred, H, W), args.iters, args.warmup)
        t_pack = device_ms(lambda: ops.mask_pack_bits(gt), args.iters, args.warmup)
        pb, gb = ops.mask_resize_pack_bits(pred, H, W), ops.mask_pack_bits(gt)
        t_pairs = device_ms(lambda: ops.mask_pair_counts(pb, gb, W, pl, gl), args.iters, args.warmup)
        same = float((pl[:, None] == gl[None, :]).sum())
        # algorithmic bytes: each destination pixel reads up to 4 source bytes (neighbours share them in cache: 1 byte/pixel of the source
        # footprint is the floor); a pair reads both masks' words once
        b_resize = P * (min(NET_H * NET_W, 4 * H * W) + H * Wq * 8)
        b_pack = T * (H * W + H * Wq * 8)
        b_pairs = (P + same + T) * H * Wq * 8
        inter, a_p, a_t = ops.mask_pair_counts(pb, gb, W, pl, gl)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed_host = pb.cpu()
        t_copy_packed = time.perf_counter() - t0
        t0 = time.perf_counter()
        unpacked_host = pred.cpu()
        t_copy_unpacked = time.perf_counter() - t0
        boxes = torch.rand(P, 4) * 100
        boxes[:, 2:] += boxes[:, :2] + 10
        from abr_iod_amd.structures.bounding_box import BoxList
        pbl, gbl = BoxList(boxes, (W, H)), BoxList(boxes[:T].clone(), (W, H))
        pbl.add_field("labels", pl.cpu())
        pbl.add_field("scores", torch.rand(P))
        gbl.add_field("labels", gl.cpu())
        iou = V.mask_iou_from_counts(inter.cpu().numpy(), a_p.cpu().numpy(), a_t.cpu().numpy())
        rec = [V.image_record(pbl, gbl, iou)]
        t0 = time.perf_counter()
        for th in V.IOU_THRESHOLDS:
            V.calc_detection_voc_prec_rec(rec, th)
        t_match = time.perf_counter() - t0
        resized = torch.nn.functional.interpolate(unpacked_host[None].float(), size=(H, W), mode="bilinear", align_corners=False)[0].to(torch.uint8).numpy()
        t0 = time.perf_counter()
        ref_iou = masklist_iou_numpy(gt.cpu().numpy(), resized, gl.cpu().numpy(), pl.cpu().numpy())
        t_ref = time.perf_counter() - t0
        rows.append({"orig_hw": [H, W], "P": P, "T": T, "same_class_pairs": int(same),
                     "resize_pack_ms": t_resize, "resize_pack_hbm_frac": b_resize / (t_resize * 1e-3) / HBM_PEAK,
                     "pack_ms": t_pack, "pack_hbm_frac": b_pack / (t_pack * 1e-3) / HBM_PEAK,
                     "pair_counts_ms": t_pairs, "pair_counts_hbm_frac": b_pairs / (t_pairs * 1e-3) / HBM_PEAK,
                     "bytes": {"resize_pack": int(b_resize), "pack": int(b_pack), "pair_counts": int(b_pairs)},
                     "host_matching_9_thresholds_ms": t_match * 1e3,
                     "to_host_packed_bytes": packed_host.numel() * 8, "to_host_unpacked_bytes": unpacked_host.numel(),
                     "to_host_packed_ms": t_copy_packed * 1e3, "to_host_unpacked_ms": t_copy_unpacked * 1e3,
                     "masklist_iou_numpy_once_ms": t_ref * 1e3, "masklist_iou_numpy_9_thresholds_ms": 9 * t_ref * 1e3,
                     "iou_equal_to_numpy_restatement": bool((iou == ref_iou).all())})
    print(json.dumps({"tool": "mask_eval_bench", "net_hw": [NET_H, NET_W], "images": rows}))


if __name__ == "__main__":
    main()

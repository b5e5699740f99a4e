#!/usr/bin/env python
"""Time the proposal-recall kernel beside the host restatement on the same synthetic images.

    python tools/proposal_recall_bench.py --images 500

Synthetic images: 1000 ranked proposals each, ground-truth counts drawn like COCO's (geometric, most images below 10, a tail that passes
the kernel's cap of 128), most ground truths with a proposal near them, areas spread over the small / medium / large ranges.  The
protocol's eight cells per image: limits (100, 1000) x areas (all, small, medium, large).  Measured:
  * ops.proposal_cover for the whole batch, uploads, the read-back of the results and the host fallback of the images over a cap
    included (what the evaluator pays), best of --repeats after a warm-up;
  * the host restatement (coco_eval_host.proposal_cover per cell) over --host-images of the same images, once, scaled per image;
  * the kernel alone on resident inputs: warm-up launches, then device events around --kernel-iters launches;
  * the share of images that took the fallback, and whether the device's overlaps equal the host's bit for bit on the host's images.
Prints one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LIMITS = (100, 1000)


def make_images(n_images, n_prop, rng):
    """-> (prop [n * n_prop, 4], gt [G_total, 4], gt_area [G_total] float32, proposal counts, ground-truth counts)"""
    props, gts, areas, gc = [], [], [], []
    for _ in range(n_images):
        G = int(rng.geometric(0.14)) - 1
        if rng.random() < 0.01:
            G += int(rng.integers(100, 200))              # the tail: crowded scenes
        wh = np.exp(rng.uniform(np.log(8), np.log(300), (G, 2)))
        xy = rng.uniform(0, 600, (G, 2))
        gt = np.concatenate([xy, xy + wh], 1)
        p_wh = np.exp(rng.uniform(np.log(8), np.log(400), (n_prop, 2)))
        p_xy = rng.uniform(0, 640, (n_prop, 2))
        prop = np.concatenate([p_xy, p_xy + p_wh], 1)
        k = min(G, n_prop // 2)
        if k:                                             # a proposal near most ground truths, somewhere in the ranking
            at = rng.choice(n_prop, k, replace=False)
            prop[at] = gt[:k] + rng.normal(0, 0.08, (k, 4)) * np.tile(wh[:k], 2)
            prop[at, 2:] = np.maximum(prop[at, 2:], prop[at, :2])
        props.append(prop)
        gts.append(gt)
        areas.append(wh[:, 0] * wh[:, 1] * rng.uniform(0.4, 1.0, G))
        gc.append(G)
    f32 = lambda parts, shape: np.concatenate(parts).reshape(shape).astype(np.float32)      # noqa: E731
    return f32(props, (-1, 4)), f32(gts, (-1, 4)), f32(areas, (-1,)), np.full(n_images, n_prop, np.int64), np.asarray(gc, np.int64)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=500)
    ap.add_argument("--proposals", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--host-images", type=int, default=100, help="how many of the images the host restatement scores (its time is scaled per image)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    import torch
    from abr_iod_amd import _lib as L
    from abr_iod_amd import ops
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H

    prop, gt, area, pc, gc = make_images(args.images, args.proposals, np.random.default_rng(args.seed))
    ranges = np.asarray(H.PROPOSAL_AREA_RNG[:4], np.float32)
    thrs = H.proposal_thresholds()

    def device_pass():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = ops.proposal_cover(prop, gt, area, pc, gc, ranges, LIMITS, thrs)
        return time.perf_counter() - t0, out

    device_pass()
    runs = [device_pass() for _ in range(max(1, args.repeats))]
    device_s, out = min(r[0] for r in runs), runs[-1][1]

    # the kernel alone, inputs resident (the images over a cap return at once, as in the evaluator's launch)
    dev = torch.device("cuda")
    off = lambda c: torch.from_numpy(np.concatenate(([0], np.cumsum(c))).astype(np.int64)).to(dev)      # noqa: E731
    bufs = [torch.from_numpy(a).to(dev) for a in (prop, gt, area)]
    offs = [off(pc), off(gc)]
    rng_d, lim_d, thr_d = torch.from_numpy(ranges).to(dev), torch.tensor(LIMITS, dtype=torch.int32, device=dev), thrs.to(dev)
    A, Ln, T, Gt = len(ranges), len(LIMITS), len(thrs), int(gc.sum())
    res = torch.empty((Ln, A, Gt), dtype=torch.float32, device=dev)
    counts = torch.zeros((Ln * A * T + A + 1,), dtype=torch.int32, device=dev)
    hits, num_pos, n_over = counts[: Ln * A * T], counts[Ln * A * T: Ln * A * T + A], counts[Ln * A * T + A:]

    def launch():
        L.check(L.lib().abr_proposal_cover(*[L.ptr(b) for b in bufs], *[L.ptr(o) for o in offs], len(pc), int(pc.sum()), Gt, L.ptr(rng_d), A,
                                           L.ptr(lim_d), Ln, L.ptr(thr_d), T, L.ptr(res), L.ptr(hits), L.ptr(num_pos), L.ptr(n_over), L.stream()),
                "proposal_cover")

    kernel_s = None
    if Gt:
        for _ in range(5):
            launch()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.kernel_iters):
            launch()
        e1.record()
        torch.cuda.synchronize()
        kernel_s = e0.elapsed_time(e1) * 1e-3 / args.kernel_iters

    # the host restatement on the first --host-images images
    n_host = min(args.host_images, args.images)
    po, go = np.concatenate(([0], np.cumsum(pc))), np.concatenate(([0], np.cumsum(gc)))
    prop_t, gt_t, area_t = torch.from_numpy(prop), torch.from_numpy(gt), torch.from_numpy(area)
    same = True
    t0 = time.perf_counter()
    for k in range(n_host):
        p, g, ar = prop_t[po[k]: po[k + 1]], gt_t[go[k]: go[k + 1]], area_t[go[k]: go[k + 1]]
        for a in range(A):
            valid = (ar >= float(ranges[a, 0])) & (ar <= float(ranges[a, 1]))
            if not bool(valid.any()):
                continue
            for li, lim in enumerate(LIMITS):
                vec = H.proposal_cover(p[:lim], g[valid]).numpy()
                got = out["overlaps"][li, a, go[k]: go[k] + len(vec)]
                same = same and bool(np.array_equal(vec.view(np.int32), np.ascontiguousarray(got).view(np.int32)))
    host_s = time.perf_counter() - t0

    ar = {}
    for li, lim in enumerate(LIMITS):
        for a, name in enumerate(("", "s", "m", "l")):
            v = torch.from_numpy(out["overlaps"][li, a])
            ar["AR{}@{}".format(name, lim)] = round(H.proposal_summary(v[v >= 0], out["hits"][li, a], int(out["num_pos"][a]), thrs)["ar"].item(), 4)
    ms = lambda s, n: round(1e3 * s / max(n, 1), 5)      # noqa: E731
    print(json.dumps({"tool": "proposal_recall_bench", "images": args.images, "proposals_per_image": args.proposals, "ground_truths": Gt,
                      "median_ground_truths": float(np.median(gc)), "max_ground_truths": int(gc.max()) if len(gc) else 0,
                      "cells_per_image": Ln * A, "device_ms": round(1e3 * device_s, 3), "device_ms_per_image": ms(device_s, args.images),
                      "host_images": n_host, "host_ms_per_image": ms(host_s, n_host),
                      "kernel_us": None if kernel_s is None else round(kernel_s * 1e6, 2),
                      "kernel_us_per_image": None if kernel_s is None else round(kernel_s * 1e6 / max(args.images, 1), 4),
                      "fallback_images": int(out["n_fallback"]), "fallback_share": round(out["n_fallback"] / max(args.images, 1), 5),
                      "device_overlaps_equal_host_bit_for_bit": same, **ar}))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""RetinaNet's post-processor (ops.retina_detect: csrc/retinanet.hip, 1 memset + 4 launches) at full size: N images of 800 x 1344, five levels,
A = 9, 80 classes, default thresholds (INFERENCE_TH 0.05, PRE_NMS_TOP_N 1000, NMS_TH 0.4, DETECTIONS_PER_IMG 100), on random head outputs with the
prior-probability bias: logit = -log(99) + sigma * N(0, 1), delta = 0.5 * N(0, 1).  Event-timed, median of --reps calls after --warmup
(MEASUREMENTS.md, "RetinaNet post-processor").  Prints one JSON line per sigma."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from abr_iod_amd import ops  # noqa: E402
from abr_iod_amd.config import cfg  # noqa: E402
from abr_iod_amd.modeling.rpn.retinanet import make_anchor_generator_retinanet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--sigma", type=float, nargs="+", default=[0.7, 1.0])
    a = ap.parse_args()
    N, H, W, A, C = a.batch, 800, 1344, 9, cfg.MODEL.RETINANET.NUM_CLASSES - 1
    r = cfg.MODEL.RETINANET
    maps = [((H + s - 1) // s, (W + s - 1) // s) for s in r.ANCHOR_STRIDES]
    ag = make_anchor_generator_retinanet(cfg).cuda()
    anchors = [ag.grid(h, w, (H, W), l)[0] for l, (h, w) in enumerate(maps)]
    img_hw = torch.tensor([[H, W]] * N, dtype=torch.int32).cuda()
    torch.manual_seed(0)
    for sigma in a.sigma:
        cls = [torch.randn(N, h * w, A * C, device="cuda") * sigma - float(np.log(99.0)) for h, w in maps]
        reg = [torch.randn(N, h * w, 4 * A, device="cuda") * 0.5 for h, w in maps]

        def call():
            return ops.retina_detect(cls, reg, anchors, A, C, img_hw, r.INFERENCE_TH, r.PRE_NMS_TOP_N, r.NMS_TH, cfg.TEST.DETECTIONS_PER_IMG)
        for _ in range(a.warmup):
            out = call()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = call()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        n_logits = sum(c.numel() for c in cls)
        frac = float(sum((c.sigmoid() > r.INFERENCE_TH).sum() for c in cls)) / n_logits
        print(json.dumps(dict(sigma=sigma, batch=N, logits=n_logits, candidate_fraction=round(frac, 5), median_ms=round(float(np.median(ts)), 4),
                              min_ms=round(min(ts), 4), max_ms=round(max(ts), 4), launches=4, memsets=1, detections=out[3].tolist())))
        del cls, reg


if __name__ == "__main__":
    main()

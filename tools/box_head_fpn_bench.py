"""First measurements of the FPN box head (modeling/roi_heads/box_head/fpn_box_head.py, csrc/box_head_fpn.hip) at R-50-FPN shapes: an
800 x 1344 image, B = 2, 512 RoIs per image (K = 1024), C = 256, 7 x 7 bins, MLP_HEAD_DIM 1024, 81 classes.

  (a) box-head targets from the pyramid selector's table: ops.roi_head_targets_table (three launches, nothing read back) against the path it
      replaces on the same table -- RPNPostProcessor.collect (+ add_gt_proposals) and FastRCNNLossComputation.subsample -- in us per call
      and host read-backs per call (torch's sync debug mode at "warn", warnings counted);
  (b) fc6 (M = 1024, N = 1024, K = 12544), fc7 (K = 1024) and the fused predictor (N = 408): forward, input gradient and weight gradient
      under the fp32 MFMA arithmetic and under f16x3, device events around --reps back-to-back calls, operands tagged with their amax
      words as the head hands them over;
  (c) one training step of the whole R-50-FPN detector (forward, backward, FusedSGD.step) in the default arithmetic.

Nothing here is a threshold.  Prints the tables, then one JSON line.

    python tools/box_head_fpn_bench.py --reps 20
"""
import argparse
import json
import os
import sys
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IMG_H, IMG_W, C, RES, DIM, CLASSES, ROIS = 2, 800, 1344, 256, 7, 1024, 81, 512
SCALES = (0.25, 0.125, 0.0625, 0.03125)
FPN_CFG = ["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", C, "MODEL.RPN.USE_FPN", True,
           "MODEL.RPN.ANCHOR_STRIDE", (4, 8, 16, 32, 64), "MODEL.RPN.ANCHOR_SIZES", (32, 64, 128, 256, 512),
           "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 2000, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 2000, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 2000,
           "MODEL.ROI_HEADS.USE_FPN", True, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", ROIS,
           "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor", "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor",
           "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", RES, "MODEL.ROI_BOX_HEAD.POOLER_SCALES", SCALES, "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2,
           "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", DIM, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", CLASSES]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3   # us


def host_timed(fn, reps):
    """wall time per call including whatever the host waits for (the read-backs are the point), us"""
    import time
    fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / reps * 1e6


def read_backs(fn):
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            fn()
            torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode(before)
    return sum("synchroniz" in str(w.message) for w in seen)


def targets_rows(cfg, reps):
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import make_roi_box_loss_evaluator
    from abr_iod_amd.modeling.rpn.rpn import LazyPyramidProposals, make_rpn_postprocessor
    from abr_iod_amd.structures.bounding_box import BoxList
    g = torch.Generator(device="cuda").manual_seed(1)
    cap = 2000
    xy = torch.rand(B, cap, 2, device="cuda", generator=g) * torch.tensor([IMG_W - 40.0, IMG_H - 40.0], device="cuda")
    wh = torch.exp(torch.rand(B, cap, 2, device="cuda", generator=g) * 4.0 + 2.0)
    rois = torch.cat((xy, torch.minimum(xy + wh, torch.tensor([IMG_W - 1.0, IMG_H - 1.0], device="cuda"))), 2).contiguous()
    scores = torch.rand(B, cap, device="cuda", generator=g).sort(1, descending=True).values.contiguous()
    n_out = torch.tensor([1100, 900], dtype=torch.int32, device="cuda")      # FPN_POST_NMS_PER_BATCH: 2000 over the batch, split unevenly
    targets = []
    for i in range(B):
        gt = rois[i, 5:400:80].clone()
        t = BoxList(gt, (IMG_W, IMG_H), mode="xyxy")
        t.add_field("labels", torch.arange(1, 1 + gt.shape[0], device="cuda"))
        targets.append(t)
    sel = make_rpn_postprocessor(cfg, BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)), is_train=True).train()
    ev = make_roi_box_loss_evaluator(cfg)

    def pending():
        return dict(rois=rois, objectness=scores, src=None, n_out=n_out, sizes=[(IMG_W, IMG_H)] * B)

    def fused():
        ev.subsample_fused(LazyPyramidProposals(sel, pending(), targets), targets, CLASSES)

    def generic():
        ev.subsample(sel.collect(pending(), targets), targets)

    out = []
    for name, fn in (("roi_head_targets_table (fused)", fused), ("collect + subsample", generic)):
        out.append({"path": name, "us": round(host_timed(fn, reps), 1), "read_backs": read_backs(fn)})
    return out


def gemm_rows(reps):
    from abr_iod_amd import ops
    K = B * ROIS
    n_pred = (CLASSES * 5 + 3) // 4 * 4
    g = torch.Generator(device="cuda").manual_seed(2)
    rows, alive = [], []      # (the library keeps what it derives from a weight per (address, version): the weights outlive the timing)
    for idx, (lname, kin, nout) in enumerate((("fc6", C * RES * RES, DIM), ("fc7", DIM, DIM), ("predictor", DIM, n_pred))):
        x = torch.randn(K, 1, 1, kin, device="cuda", generator=g).clamp_(min=0)
        w = torch.randn(nout, 1, 1, kin, device="cuda", generator=g) * (3.0 / kin) ** 0.5
        gy = torch.randn(K, 1, 1, nout, device="cuda", generator=g)
        wt = ops.conv_dgrad_weights(w)
        dw = torch.zeros_like(w)
        alive.append((w, wt))
        ver = 101 + 2 * idx
        ops.amax_compute(x)
        ops.amax_compute(gy)
        flops = 2.0 * K * kin * nout
        for mname, m in (("f32", ops.MATH_F32), ("f16x3", ops.MATH_F16X3)):
            for op, fn in (("forward", lambda: ops.conv_forward(x, w, 1, 0, relu=True, math=m, w_version=ver)),
                           ("dgrad", lambda: ops.conv_forward(gy, wt, 1, 0, math=m, w_version=ver)),
                           ("wgrad", lambda: ops.conv_wgrad(x, gy, dw, 1, 0, math=m))):
                us = timed(fn, reps)
                rows.append({"layer": lname, "M": K, "N": nout, "K": kin, "math": mname, "op": op, "us": round(us, 1),
                             "TFLOPs": round(flops / us / 1e6, 1)})
    torch.cuda.synchronize()
    ops.conv_cache_clear()
    del alive
    return rows


def step_row(cfg, reps):
    from abr_iod_amd import ops
    from abr_iod_amd.engine.synthetic import build_models, synthetic_batch
    from abr_iod_amd.solver.build import FusedSGD
    from abr_iod_amd.structures.image_list import ImageList
    _, model = build_models(None, cfg, seed=0, need_source=False)
    opt = FusedSGD(model, 0.002, 0.9, 1e-4, 2.0, 0.0)
    images, targets = synthetic_batch(B, IMG_H, IMG_W, seed=5, label_range=(1, CLASSES))
    images = ImageList(images, [(IMG_H, IMG_W)] * B)

    def step():
        opt.zero_grad()
        losses = model(images, targets)[0]
        sum(losses.values()).backward()
        opt.step()

    for _ in range(3):
        step()
    before = tuple(ops.amax_reductions)
    us = timed(step, reps)
    calls = (ops.amax_reductions[0] - before[0]) / (reps + 1)
    mb = (ops.amax_reductions[1] - before[1]) / (reps + 1) / 1e6
    return {"ms_per_step": round(us / 1e3, 3), "conv_math": model.conv_math, "amax_reductions_per_step": round(calls, 1),
            "amax_reduced_MB_per_step": round(mb, 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="leave out (c), the whole detector's training step")
    a = ap.parse_args()
    from abr_iod_amd.engine.synthetic import make_cfgs
    torch.cuda.set_device(0)
    cfg = make_cfgs("15-5", overrides=FPN_CFG)[1]
    cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES = CLASSES
    out = {"shape": {"B": B, "image": [IMG_H, IMG_W], "rois_per_image": ROIS, "C": C, "res": RES, "dim": DIM, "classes": CLASSES}}
    out["targets"] = targets_rows(cfg, a.reps)
    print("(a) box-head targets, B = %d, %d RoIs per image, table of 2000 rows per image" % (B, ROIS))
    for r in out["targets"]:
        print("    %-34s %9.1f us   %d host read-backs" % (r["path"], r["us"], r["read_backs"]))
    out["gemms"] = gemm_rows(a.reps)
    print("(b) contractions, M = %d" % (B * ROIS))
    for r in out["gemms"]:
        print("    %-10s N %5d K %6d  %-6s %-8s %9.1f us  %7.1f TFLOP/s" % (r["layer"], r["N"], r["K"], r["math"], r["op"], r["us"], r["TFLOPs"]))
    if not a.skip_step:
        out["step"] = step_row(cfg, max(a.reps // 2, 3))
        print("(c) R-50-FPN detector training step: %(ms_per_step).3f ms (%(conv_math)s; %(amax_reductions_per_step).1f amax reductions, "
              "%(amax_reduced_MB_per_step).2f MB reduced per step)" % out["step"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

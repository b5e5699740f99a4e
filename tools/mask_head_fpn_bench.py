"""First measurements of the FPN mask head (modeling/roi_heads/mask_head/fpn_mask_head.py, the indexed pyramid pooler of csrc/roi_align.hip) at
R-50-FPN shapes: 2 images of 800 x 1344, C = 256, 512 sampled RoIs per image (a table of 1024 rows), p_max = 256 positives, pooler 14 x 14
with sampling ratio 2 over P2..P5, CONV_LAYERS (256, 256, 256, 256), 81 classes, 28 x 28 targets.

  (a) select + targets: MaskRCNNLossComputation.select on the fused table (compaction and the bitmask targets of the batch, nothing read back);
  (b) the indexed pooler, forward and backward, against the route it replaces: an 8-wide ops.mask_gather_rows copy of the table's rows and
      the unindexed pooler on the copy (padding rows pooled as degenerate boxes);
  (c) one mask_fcn (the four have one shape): forward, input gradient and weight gradient; the predictor's forward; the loss -- in the three
      arithmetics, device events around --reps back-to-back calls, operands tagged with their amax words;
  (d) the conv stack at n_pos = 32 of 256: the padded [256,14,14,256] stack against the same 32 rows alone -- how much of the conv time goes
      to padding rows (a finding for later work, nothing here skips them).

Nothing here is a threshold.  Prints the tables, then one JSON line.

    python tools/mask_head_fpn_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IMG_H, IMG_W, C, RES, M, CLASSES, ROIS, P_MAX = 2, 800, 1344, 256, 14, 28, 81, 512, 256
SCALES = (0.25, 0.125, 0.0625, 0.03125)
RULE = (2.0, 5.0)
LAYERS = (256, 256, 256, 256)
MASK_CFG = ["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.MASK_ON", True, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", CLASSES,
            "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", ROIS, "MODEL.ROI_HEADS.POSITIVE_FRACTION", 0.25,
            "MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor", "MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNC4Predictor",
            "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", RES,
            "MODEL.ROI_MASK_HEAD.POOLER_SCALES", SCALES, "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_MASK_HEAD.RESOLUTION", M,
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", LAYERS]


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


def scene(n_pos_per_image):
    """the sampled set as the fused sampler leaves it: a [1024,5] table (sides log-uniform 16 .. 900 px: every level), labels with
    n_pos_per_image positives per image, and per image 8 ground-truth boxes with ellipse masks"""
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    g = torch.Generator(device="cuda").manual_seed(1)
    K = B * ROIS
    side = torch.exp(torch.rand(K, 2, device="cuda", generator=g) * 4.0 + 2.8)
    xy = torch.rand(K, 2, device="cuda", generator=g) * torch.tensor([IMG_W - 20.0, IMG_H - 20.0], device="cuda")
    x2y2 = torch.minimum(xy + side, torch.tensor([IMG_W - 1.0, IMG_H - 1.0], device="cuda"))
    img = torch.arange(B, device="cuda").repeat_interleave(ROIS).float()[:, None]
    rois = torch.cat((img, xy, x2y2), 1).contiguous()
    labels = torch.zeros(K, dtype=torch.int64, device="cuda")
    props, targets = [], []
    ys, xs = torch.meshgrid(torch.arange(IMG_H, device="cuda"), torch.arange(IMG_W, device="cuda"), indexing="ij")
    for b in range(B):
        rows = torch.arange(b * ROIS, b * ROIS + ROIS, device="cuda")
        labels[rows[:: ROIS // n_pos_per_image][:n_pos_per_image]] = 1 + (rows[:n_pos_per_image] % (CLASSES - 1))
        props.append(BoxList(rois[rows, 1:], (IMG_W, IMG_H), mode="xyxy"))
        gt = rois[rows[:: ROIS // 8][:8], 1:].clone()
        cx, cy, rx, ry = (gt[:, 0] + gt[:, 2]) / 2, (gt[:, 1] + gt[:, 3]) / 2, (gt[:, 2] - gt[:, 0]) / 3 + 1, (gt[:, 3] - gt[:, 1]) / 3 + 1
        masks = ((((xs[None] - cx[:, None, None]) / rx[:, None, None]) ** 2 + ((ys[None] - cy[:, None, None]) / ry[:, None, None]) ** 2) <= 1).to(torch.uint8)
        t = BoxList(gt, (IMG_W, IMG_H), mode="xyxy")
        t.add_field("labels", torch.arange(1, 9, device="cuda"))
        t.add_field("masks", SegmentationMask(masks, (IMG_W, IMG_H), mode="mask"))
        targets.append(t)
    return rois, labels, props, targets


def maps(tag=True):
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    xs = [torch.randn(B, IMG_H // s, IMG_W // s, C, device="cuda", generator=g) for s in (4, 8, 16, 32)]
    return [ops.amax_compute(x) for x in xs] if tag else xs


def select_row(head, rois, labels, props, targets, reps):
    ev = head.loss_evaluator
    fused = dict(labels=labels, rois=rois)
    us = timed(lambda: ev.select(props, targets, fused=fused), reps)
    return {"stage": "select + targets", "us": round(us, 1)}, ev.select(props, targets, fused=fused)


def pooler_rows(rois, pos_rows, reps):
    from abr_iod_amd import ops
    xs = maps()
    shapes = [tuple(x.shape) for x in xs]
    P_ = pos_rows.numel()
    g = torch.randn(P_, RES, RES, C, device="cuda")
    wide = torch.zeros((rois.shape[0], 8), device="cuda")      # (the row gather moves 16-byte pieces)
    wide[:, :5] = rois
    gathered = ops.mask_gather_rows(wide, pos_rows)[:, :5].contiguous()

    def gather_forward():
        t = ops.mask_gather_rows(wide, pos_rows)[:, :5].contiguous()
        return ops.roi_align_pyramid_forward(xs, t, SCALES, RES, RES, 2, *RULE)

    rows = [("indexed forward", lambda: ops.roi_align_pyramid_forward(xs, rois, SCALES, RES, RES, 2, *RULE, rows=pos_rows)),
            ("gather copy + unindexed forward", gather_forward),
            ("indexed backward", lambda: ops.roi_align_pyramid_backward(g, rois, SCALES, RES, RES, 2, shapes, *RULE, rows=pos_rows)),
            ("unindexed backward on the copy", lambda: ops.roi_align_pyramid_backward(g, gathered, SCALES, RES, RES, 2, shapes, *RULE))]
    out = []
    for name, fn in rows:
        runs = sorted(timed(fn, reps) for _ in range(5))
        out.append({"stage": name, "P": P_, "us_median": round(runs[2], 1), "us_min": round(runs[0], 1), "us_max": round(runs[4], 1)})
    return out


def conv_rows(head, sel, reps):
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(3)
    x = torch.randn(P_MAX, RES, RES, C, device="cuda", generator=g).clamp_(min=0)
    gy = torch.randn(P_MAX, RES, RES, C, device="cuda", generator=g)
    w = torch.randn(C, 3, 3, C, device="cuda", generator=g) * (2.0 / (9 * C)) ** 0.5
    bias = torch.zeros(C, device="cuda")
    wt, dw = ops.conv_dgrad_weights(w), torch.zeros_like(w)
    ops.amax_compute(x)
    ops.amax_compute(gy)
    pred = head.predictor
    flops = 2.0 * P_MAX * RES * RES * 9 * C * C
    rows = []
    for mname, m in (("f32", ops.MATH_F32), ("f16x3", ops.MATH_F16X3), ("bf16x6", ops.MATH_BF16X6)):
        pred.math = m
        logits = pred._run(x)[1]
        for op, fn, fl in (("mask_fcn forward", lambda: ops.conv_forward(x, w, 1, 1, bias=bias, relu=True, math=m, w_version=101), flops),
                           ("mask_fcn dgrad", lambda: ops.conv_forward(gy, wt, 1, 1, math=m, w_version=101), flops),
                           ("mask_fcn wgrad", lambda: ops.conv_wgrad(x, gy, dw, 1, 1, math=m), flops),
                           ("predictor forward", lambda: pred._run(x), 2.0 * P_MAX * RES * RES * C * (4 * C) + 2.0 * P_MAX * M * M * C * CLASSES),
                           ("loss + gradient", lambda: ops.mask_loss(logits, CLASSES, sel["pos_labels"], sel["mask_targets"], n_pos=sel["n_pos"],
                                                                      want_grad=True), None)):
            us = timed(fn, reps)
            rows.append({"op": op, "math": mname, "us": round(us, 1), "TFLOPs": None if fl is None else round(fl / us / 1e6, 1)})
    torch.cuda.synchronize()
    ops.conv_cache_clear()
    return rows


def padding_rows(head, rois, reps):
    """the extractor's forward (pooler + four convs) at n_pos = 32: the padded list of 256 against the 32 rows alone"""
    from abr_iod_amd import ops
    _, labels, _, _ = scene(16)
    pos_rows = ops.mask_compact_pos(labels, P_MAX)[0]
    compact = pos_rows[:32].contiguous()
    xs = [ops.amax_carry(x.permute(0, 3, 1, 2), x) for x in maps()]      # logical NCHW views, the amax tags kept
    fe = head.feature_extractor
    out = []
    with torch.no_grad():
        for mname, m in (("f32", ops.MATH_F32), ("f16x3", ops.MATH_F16X3), ("bf16x6", ops.MATH_BF16X6)):
            fe.math = m
            padded = timed(lambda: fe(xs, rois, rows=pos_rows), reps)
            alone = timed(lambda: fe(xs, rois, rows=compact), reps)
            out.append({"math": mname, "us_256_rows_32_positive": round(padded, 1), "us_32_rows": round(alone, 1),
                        "share_spent_on_padding": round(1.0 - alone / padded, 3)})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from abr_iod_amd.config import cfg as default_cfg
    from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import ROIMaskHead
    torch.cuda.set_device(0)
    cfg = default_cfg.clone()
    cfg.merge_from_list(MASK_CFG)
    head = ROIMaskHead(cfg, C, None).cuda()
    rois, labels, props, targets = scene(P_MAX // B)
    out = {"shape": {"B": B, "image": [IMG_H, IMG_W], "rois_per_image": ROIS, "p_max": P_MAX, "C": C, "res": RES, "layers": list(LAYERS),
                     "classes": CLASSES, "M": M}}
    row, sel = select_row(head, rois, labels, props, targets, a.reps)
    assert int(sel["n_pos"]) == P_MAX
    out["select"] = row
    print("(a) %-40s %9.1f us" % (row["stage"], row["us"]))
    out["pooler"] = pooler_rows(rois, sel["pos_rows"], a.reps)
    print("(b) pooler, P = %d rows of a table of %d, 14 x 14, C = %d (median of 5 x %d calls; min .. max)" % (P_MAX, B * ROIS, C, a.reps))
    for r in out["pooler"]:
        print("    %-40s %9.1f us   (%.1f .. %.1f)" % (r["stage"], r["us_median"], r["us_min"], r["us_max"]))
    out["convs"] = conv_rows(head, sel, a.reps)
    print("(c) [%d,14,14,%d] stages" % (P_MAX, C))
    for r in out["convs"]:
        print("    %-20s %-7s %9.1f us  %s" % (r["op"], r["math"], r["us"], "" if r["TFLOPs"] is None else "%7.1f TFLOP/s" % r["TFLOPs"]))
    out["padding"] = padding_rows(head, rois, a.reps)
    print("(d) extractor forward at n_pos = 32 of %d" % P_MAX)
    for r in out["padding"]:
        print("    %-7s padded %9.1f us   32 rows alone %9.1f us   share spent on padding rows %.1f %%" % (
            r["math"], r["us_256_rows_32_positive"], r["us_32_rows"], 100 * r["share_spent_on_padding"]))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

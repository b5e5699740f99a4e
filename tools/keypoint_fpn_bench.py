"""First measurements of the FPN keypoint head (modeling/roi_heads/keypoint_head/keypoint_head.py on roi_heads/pyramid_extractor.py) at upstream's
sizes (e2e_keypoint_rcnn_R_50_FPN_1x): images of 800 x 1344, maps of 256 channels at strides 4 .. 32, 512 sampled RoIs per image of which at
most 128 are positives (P_max = 128 B), pooler 14 x 14 with sampling ratio 2 over P2..P5, eight 512-wide convs, 17 keypoints, 56 x 56 heat maps.

One training pass of ROIKeypointHead alone -- select + targets, the indexed pooler, the eight convs, the deconvolution, the fused upsampling +
loss, and the whole backward down to the four maps' gradients and every weight gradient -- for B = 2 and B = 4, in the three arithmetics:

  all live   every one of the P_max rows is a kept positive;
  few live   8 kept positives per image, the other rows of the fixed-size list are padding (zero features in, relu(bias) out, valid = 0).

The head always computes P_max rows, so "few live" costs what "all live" costs less whatever the pooler and the loss save; `rows alone` is the
same pass with P_max cut to the live count, i.e. what a head that skipped the padding would pay (nothing here skips it: the number is for a
later change to decide about).  Times are host clock around --reps passes ending in a device synchronise (the weight gradients run on a side
stream), median of 3 windows.

Nothing here is a threshold.  Prints the table, then one JSON line.

    python tools/keypoint_fpn_bench.py --reps 5
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

IMG_H, IMG_W, C, RES, M, K, ROIS, POS = 800, 1344, 256, 14, 56, 17, 512, 128
SCALES = (0.25, 0.125, 0.0625, 0.03125)
LAYERS = (512,) * 8
FEW = 8


def head_cfg(pos_per_image):
    from abr_iod_amd.config import cfg as default_cfg
    cfg = default_cfg.clone()
    cfg.merge_from_list(["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.KEYPOINT_ON", True, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", ROIS,
                         "MODEL.ROI_HEADS.POSITIVE_FRACTION", pos_per_image / ROIS, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
                         "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", RES, "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", SCALES,
                         "MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", M,
                         "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", LAYERS, "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", K])
    return cfg


def scene(B, live_per_image):
    """the sampled set as the fused sampler leaves it: a [512 B,5] table (sides log-uniform 16 .. 900 px: every level), per image 8 person
    boxes with keypoints inside them; `live_per_image` rows of each image are positives lying exactly on one of its person boxes"""
    from abr_iod_amd.engine.synthetic import _box_keypoints
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    g = torch.Generator(device="cuda").manual_seed(1)
    n = B * ROIS
    side = torch.exp(torch.rand(n, 2, device="cuda", generator=g) * 4.0 + 2.8)
    xy = torch.rand(n, 2, device="cuda", generator=g) * torch.tensor([IMG_W - 20.0, IMG_H - 20.0], device="cuda")
    x2y2 = torch.minimum(xy + side, torch.tensor([IMG_W - 1.0, IMG_H - 1.0], device="cuda"))
    img = torch.arange(B, device="cuda").repeat_interleave(ROIS).float()[:, None]
    rois = torch.cat((img, xy, x2y2), 1).contiguous()
    labels = torch.zeros(n, dtype=torch.int64, device="cuda")
    props, targets = [], []
    for b in range(B):
        rows = torch.arange(b * ROIS, b * ROIS + ROIS, device="cuda")
        gt = rois[rows[:: ROIS // 8][:8], 1:].clone()
        pos = rows[:: ROIS // live_per_image][:live_per_image]
        rois[pos, 1:] = gt[torch.arange(live_per_image, device="cuda") % 8]
        labels[pos] = 1
        props.append(BoxList(rois[rows, 1:], (IMG_W, IMG_H), mode="xyxy"))
        t = BoxList(gt, (IMG_W, IMG_H), mode="xyxy")
        t.add_field("labels", torch.ones(8, dtype=torch.int64, device="cuda"))
        t.add_field("keypoints", PersonKeypoints(_box_keypoints(gt.cpu(), K).cuda(), (IMG_W, IMG_H)))
        targets.append(t)
    return props, targets, dict(labels=labels, rois=rois)


def maps(B):
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(2)
    out = []
    for s in (4, 8, 16, 32):
        x = ops.amax_compute(torch.randn(B, IMG_H // s, IMG_W // s, C, device="cuda", generator=g))
        out.append(ops.amax_carry(x.permute(0, 3, 1, 2), x).requires_grad_(True))      # logical NCHW views, the amax tags kept
    return out


def one_pass(head, xs, props, targets, fused):
    for p in head.parameters():
        if p.grad is not None:
            p.grad.zero_()
    for x in xs:
        x.grad = None
    head(xs, props, targets, fused=fused)[2]["loss_kp"].backward()


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        runs.append((time.perf_counter() - t0) / reps * 1e3)   # ms
    return sorted(runs)


def measure(B, pos_per_image, live_per_image, math, reps):
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    torch.manual_seed(0)
    head = build_roi_keypoint_head(head_cfg(pos_per_image), C).cuda().train()
    head.feature_extractor.math = head.predictor.math = math
    bump_param_version()
    props, targets, fused = scene(B, live_per_image)
    xs = maps(B)
    runs = timed(lambda: one_pass(head, xs, props, targets, fused), reps)
    sel = head.last_selection
    n_pos, p_max = int(sel["n_pos"]), sel["pos_rows"].numel()
    assert n_pos == B * live_per_image and p_max == B * pos_per_image, (n_pos, p_max)
    del head, xs
    torch.cuda.synchronize()
    ops.conv_cache_clear()
    torch.cuda.empty_cache()
    return {"B": B, "p_max": p_max, "live": n_pos, "ms_median": round(runs[1], 2), "ms_min": round(runs[0], 2), "ms_max": round(runs[2], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 4])
    a = ap.parse_args()
    from abr_iod_amd import ops
    torch.cuda.set_device(0)
    out = {"shape": {"image": [IMG_H, IMG_W], "rois_per_image": ROIS, "positives_per_image": POS, "C": C, "res": RES, "layers": list(LAYERS),
                     "keypoints": K, "M": M, "few": FEW}, "rows": []}
    conv_flops = lambda p: 3 * 2.0 * p * RES * RES * 9 * (C * 512 + 7 * 512 * 512)      # noqa: E731  forward + dgrad + wgrad of the eight convs
    print("ROIKeypointHead forward + backward, %d x %d images, C = %d, 8 x 512-wide convs, pooler %d, K = %d" % (IMG_H, IMG_W, C, RES, K))
    print("%-7s %2s %-10s %6s %5s %10s %20s %12s" % ("math", "B", "case", "P_max", "live", "ms median", "(min .. max)", "conv TFLOP/s"))
    for mname, m in (("f16x3", ops.MATH_F16X3), ("bf16x6", ops.MATH_BF16X6), ("f32", ops.MATH_F32)):
        for B in a.batches:
            for case, pos, live in (("all live", POS, POS), ("few live", POS, FEW), ("rows alone", FEW, FEW)):
                r = measure(B, pos, live, m, a.reps)
                r.update(math=mname, case=case, conv_tflops=round(conv_flops(r["p_max"]) / r["ms_median"] / 1e9, 1))
                out["rows"].append(r)
                print("%-7s %2d %-10s %6d %5d %10.2f %20s %12.1f" % (mname, B, case, r["p_max"], r["live"], r["ms_median"],
                                                                  "(%.2f .. %.2f)" % (r["ms_min"], r["ms_max"]), r["conv_tflops"]), flush=True)
    by = {(r["math"], r["B"], r["case"]): r["ms_median"] for r in out["rows"]}
    out["padding"] = []
    for (mname, B, case), ms in by.items():
        if case == "few live":
            alone = by[(mname, B, "rows alone")]
            out["padding"].append({"math": mname, "B": B, "ms_few_live": ms, "ms_rows_alone": alone, "share_spent_on_padding": round(1.0 - alone / ms, 3)})
            print("%-7s B = %d: %d live of %d rows: %.2f ms, the live rows alone %.2f ms: %.1f %% of the pass goes to padding rows" % (
                mname, B, B * FEW, B * POS, ms, alone, 100 * (1.0 - alone / ms)))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

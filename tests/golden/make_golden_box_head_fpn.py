#!/usr/bin/env python3
"""FPN box head golden FROM THE REFERENCE (in-container only): the reference's own FPN2MLPFeatureExtractor
(modeling/roi_heads/box_head/roi_box_feature_extractors.py:59-101) and FPNPredictor (roi_box_predictors.py:36-132) called directly on the
CPU -- not through its ROIBoxHead, which unpacks two values from an extractor that returns one -- over the feature maps and RoI set of
tests/golden/pooler_fpn.npz (B = 2, C = 8, four maps, ~60 RoIs with level-boundary and no-level rows), resolution 7, sampling ratio 2,
MLP_HEAD_DIM 32, NUM_CLASSES 5.  The parameters are drawn here (the reference's own init leaves every bias zero and the predictor's weights
at 1e-2 / 1e-3, which would hide a dropped bias or a swapped layer).

tests/golden/box_head_fpn.npz: w_/b_ of fc6, fc7, cls_score, bbox_pred (reference layout), x [K,32], cls [K,5], bbox [K,20], the cotangents
g_cls / g_bbox, and every gradient for loss = <cls, g_cls> + <bbox, g_bbox> the reference can compute on the CPU: gw_/gb_ of the four layers
and g_pooled [K,C,7,7], the gradient at the pooler's output.  The maps' own gradients are NOT stored: the reference's ROIAlign backward is
"Not implemented on the CPU" (its csrc has the CUDA kernel only), so the tests take g_pooled through tests/pooler_ref.py's float64 transpose.
tests/golden/box_head_fpn_state_dict_shapes.json: {"overrides": [...], "shapes": {key: shape}} of the reference's
build_detection_model(cfg).state_dict() for a box-only R-50-FPN configuration (tiny widths)."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import box_head_fpn_ref as HR  # noqa: E402
import pooler_ref as P  # noqa: E402

HEAD = ["MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", HR.RES, "MODEL.ROI_BOX_HEAD.POOLER_SCALES", P.SCALES,
        "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", HR.SAMPLING, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", HR.DIM,
        "MODEL.ROI_BOX_HEAD.NUM_CLASSES", HR.NUM_CLASSES]
TINY = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8,
        "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16]
DETECTOR = ["MODEL.DEVICE", "cpu", "MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.RPN.USE_FPN", True,
            "MODEL.RPN.ANCHOR_STRIDE", (4, 8, 16, 32, 64), "MODEL.RPN.ANCHOR_SIZES", (32, 64, 128, 256, 512), "MODEL.ROI_HEADS.USE_FPN", True,
            "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor", "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor",
            "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_BOX_HEAD.POOLER_SCALES", P.SCALES,
            "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21] + TINY


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.box_head.roi_box_feature_extractors import FPN2MLPFeatureExtractor
    from maskrcnn_benchmark.modeling.roi_heads.box_head.roi_box_predictors import FPNPredictor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    pg = np.load(os.path.join(HERE, "pooler_fpn.npz"))
    B, C = int(pg["B"]), int(pg["C"])
    maps = [tuple(int(v) for v in m) for m in pg["maps"]]
    img_h, img_w = (int(v) for v in pg["image"])
    rois = pg["rois"]
    feats = P.make_feats(int(pg["seed"]), B, C, maps)

    cfg = rh.default_cfg(overrides=HEAD)
    fe = FPN2MLPFeatureExtractor(cfg, C)
    pred = FPNPredictor(cfg, fe.out_channels)
    gen = torch.Generator().manual_seed(HR.GOLDEN_SEED)
    layers = {"fc6": fe.fc6, "fc7": fe.fc7, "cls_score": pred.cls_score, "bbox_pred": pred.bbox_pred}
    with torch.no_grad():
        for name, lin in layers.items():
            bound = (3.0 / lin.in_features) ** 0.5
            lin.weight.copy_((torch.rand(lin.weight.shape, generator=gen) * 2 - 1) * bound)
            lin.bias.copy_((torch.rand(lin.bias.shape, generator=gen) * 2 - 1) * 0.3)

    boxes = [BoxList(torch.from_numpy(rois[rois[:, 0] == b, 1:].copy()), (img_w, img_h), mode="xyxy") for b in range(B)]
    xs = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))) for f in feats]
    kept = {}

    def leaf(_module, _inputs, output):      # the pooler's result as a leaf: its .grad is the gradient the maps' backward would start from
        kept["pooled"] = output.detach().requires_grad_(True)
        return kept["pooled"]

    fe.pooler.register_forward_hook(leaf)
    x = fe(xs, boxes)
    cls, bbox = pred(x)
    g_cls, g_bbox = HR.cotangents(len(rois))
    ((cls * torch.from_numpy(g_cls)).sum() + (bbox * torch.from_numpy(g_bbox)).sum()).backward()
    out = dict(x=x.detach().numpy(), cls=cls.detach().numpy(), bbox=bbox.detach().numpy(), g_cls=g_cls, g_bbox=g_bbox,
               seed=np.int64(HR.GOLDEN_SEED))
    out["g_pooled"] = kept["pooled"].grad.numpy()
    for name, lin in layers.items():
        out["w_" + name], out["b_" + name] = lin.weight.detach().numpy(), lin.bias.detach().numpy()
        out["gw_" + name], out["gb_" + name] = lin.weight.grad.numpy(), lin.bias.grad.numpy()
    np.savez_compressed(os.path.join(HERE, "box_head_fpn.npz"), **out)
    print("rows", len(rois), "x", out["x"].shape, "active fc7 units", float((out["x"] > 0).mean()))

    model = build_detection_model(rh.default_cfg(overrides=DETECTOR))
    with open(os.path.join(HERE, "box_head_fpn_state_dict_shapes.json"), "w") as f:
        shapes = [(k, list(v.shape)) for k, v in model.state_dict().items()]      # one key per line
        f.write('{"overrides": %s,\n "shapes": {\n' % json.dumps([list(v) if isinstance(v, tuple) else v for v in DETECTOR]))
        for i, (k, shape) in enumerate(shapes):
            f.write("  %s: %s%s\n" % (json.dumps(k), json.dumps(shape), "," if i < len(shapes) - 1 else ""))
        f.write(" }}\n")


if __name__ == "__main__":
    main()

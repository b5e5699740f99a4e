#!/usr/bin/env python3
"""FPN mask head golden FROM THE REFERENCE (run by hand where the reference tree exists; see ref_harness.py): the reference's own
MaskRCNNFPNFeatureExtractor (modeling/roi_heads/mask_head/roi_mask_feature_extractors.py:16-65), MaskRCNNC4Predictor, MaskRCNNLossComputation
and MaskPostProcessor called directly on the CPU -- not through its ROIMaskHead, whose forward indexes [0] into this extractor's single
tensor -- over the maps and the RoI table of tests/golden/pooler_fpn.npz and the positives, ground truth and masks of
tests/mask_head_fpn_ref.py's fixture.  Pooler 14 x 14, sampling ratio 2, four levels; CONV_LAYERS (8, 8); NUM_CLASSES 3.  Weights AND biases
are drawn here (the reference's init leaves every bias zero, which would hide a dropped bias).

tests/golden/mask_head_fpn.npz: w_/b_ of mask_fcn1, mask_fcn2, conv5_mask, mask_fcn_logits (reference layout), logits [n_pos,3,28,28],
labels_pos, the mask targets (packed bits), loss, prob (the post-processor's [n_pos,1,28,28]), gw_/gb_ of the four layers and g_pooled
[n_pos,8,14,14], the gradient at the pooler's output (the reference's ROIAlign backward is not implemented on the CPU: the tests take g_pooled
through tests/pooler_ref.py's float64 transpose).
tests/golden/mask_head_fpn_state_dict_shapes.json: {"overrides": [...], "shapes": {key: shape}} of the reference's
build_detection_model(cfg).state_dict() for the tiny R-50-FPN + mask configuration.  The files hold data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the float64 model reads the oracle package)
import ref_harness as rh  # noqa: E402
import mask_head_fpn_ref as MR  # noqa: E402
from make_golden_box_head_fpn import DETECTOR  # noqa: E402

HEAD = ["MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", MR.NUM_CLASSES] + MR.MASK_CFG


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import MaskPostProcessor
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import MaskRCNNLossComputation
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.roi_mask_feature_extractors import MaskRCNNFPNFeatureExtractor
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.roi_mask_predictors import MaskRCNNC4Predictor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

    fx = MR.fixture()
    MR.check_fixture(fx)
    img_h, img_w = fx["image"]
    cfg = rh.default_cfg(overrides=HEAD)
    fe = MaskRCNNFPNFeatureExtractor(cfg, fx["C"])
    pred = MaskRCNNC4Predictor(cfg, fe.out_channels)
    layers = {"mask_fcn1": fe.mask_fcn1, "mask_fcn2": fe.mask_fcn2, "conv5_mask": pred.conv5_mask, "mask_fcn_logits": pred.mask_fcn_logits}
    assert fe.blocks == ["mask_fcn1", "mask_fcn2"] and tuple(layers) == MR.PARAMS
    gen = torch.Generator().manual_seed(MR.GOLDEN_SEED)
    with torch.no_grad():
        for lay in layers.values():
            fan = lay.weight[0].numel() if not isinstance(lay, torch.nn.ConvTranspose2d) else lay.weight.shape[0] * 4
            lay.weight.copy_(torch.randn(lay.weight.shape, generator=gen) * (2.0 / fan) ** 0.5)
            lay.bias.copy_((torch.rand(lay.bias.shape, generator=gen) * 2 - 1) * 0.3)

    rois, rows = fx["rois"], fx["pos_rows"][: fx["n_pos"]]
    pos_props, tgts = [], []
    for b in range(fx["B"]):
        pos_props.append(BoxList(torch.from_numpy(rois[[r for r in rows if rois[r, 0] == b], 1:].copy()), (img_w, img_h), mode="xyxy"))
        t = BoxList(torch.from_numpy(fx["gt_boxes"][b].copy()), (img_w, img_h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(fx["gt_labels"][b].copy()))
        t.add_field("masks", SegmentationMask(torch.from_numpy(fx["gt_masks"][b].copy()), (img_w, img_h), mode="mask"))
        tgts.append(t)
    xs = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))) for f in fx["feats"]]
    kept = {}

    def leaf(_module, _inputs, output):      # the pooler's result as a leaf: its .grad is the gradient the maps' backward would start from
        kept["pooled"] = output.detach().requires_grad_(True)
        return kept["pooled"]

    fe.pooler.register_forward_hook(leaf)
    logits = pred(fe(xs, pos_props))
    ev = MaskRCNNLossComputation(Matcher(0.5, 0.5, allow_low_quality_matches=False), MR.M)
    labels, mask_targets = ev.prepare_targets(pos_props, tgts)
    labels, mask_targets = torch.cat(labels), torch.cat(mask_targets)
    assert torch.equal(labels, torch.from_numpy(fx["labels"][rows])), "a positive did not match its own ground-truth box"
    assert bool(((mask_targets == 0) | (mask_targets == 1)).all()) and 0.05 < float(mask_targets.mean()) < 0.95
    loss = ev(pos_props, logits, tgts)
    loss.backward()
    for p, lab in zip(pos_props, labels.split([len(p) for p in pos_props])):
        p.add_field("labels", lab)
        p.add_field("scores", torch.ones(len(p)))
    with torch.no_grad():
        prob = torch.cat([r.get_field("mask") for r in MaskPostProcessor(None)(logits.detach(), pos_props)])
    out = dict(seed=np.int64(MR.GOLDEN_SEED), n_pos=np.int64(len(rows)), pos_rows=fx["pos_rows"], labels_pos=labels.numpy(),
               targets_bits=np.packbits(mask_targets.numpy().astype(np.uint8)), logits=logits.detach().numpy(), loss=np.float64(loss.double().item()),
               prob=prob.numpy(), g_pooled=kept["pooled"].grad.numpy())
    for name, lay in layers.items():
        out["w_" + name], out["b_" + name] = lay.weight.detach().numpy(), lay.bias.detach().numpy()
        out["gw_" + name], out["gb_" + name] = lay.weight.grad.numpy(), lay.bias.grad.numpy()
    path = os.path.join(HERE, "mask_head_fpn.npz")
    np.savez_compressed(path, **out)
    print("positives", len(rows), "logits", out["logits"].shape, "loss", float(out["loss"]), "bytes", os.path.getsize(path),
          "of", os.path.getsize(os.path.join(HERE, "box_head_fpn.npz")))

    det = [v for v in DETECTOR] + MR.MASK_CFG
    model = build_detection_model(rh.default_cfg(overrides=det))
    with open(os.path.join(HERE, "mask_head_fpn_state_dict_shapes.json"), "w") as f:
        shapes = [(k, list(v.shape)) for k, v in model.state_dict().items()]      # one key per line
        f.write('{"overrides": %s,\n "shapes": {\n' % json.dumps([list(v) if isinstance(v, tuple) else v for v in det]))
        for i, (k, shape) in enumerate(shapes):
            f.write("  %s: %s%s\n" % (json.dumps(k), json.dumps(shape), "," if i < len(shapes) - 1 else ""))
        f.write(" }}\n")


if __name__ == "__main__":
    main()

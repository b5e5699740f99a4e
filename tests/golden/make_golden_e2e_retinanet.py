#!/usr/bin/env python3
"""Whole-RetinaNet-detector golden FROM THE REFERENCE (in-container only; see ref_harness.py): one training forward of the reference's own tiny
R-50-FPN-RETINANET detector (build_detection_model, MODEL.DEVICE cpu) on the two-image batch of tests/e2e_retinanet_common.py, once with
MODEL.RETINANET.USE_C5 True and once with False.

The reference's model cannot be run whole: GeneralizedRCNN.forward hands its RetinaNetModule four arguments where it takes three, its ResNet
hands its FPN a pair the FPN cannot take through nn.Sequential, and RetinaNetLossComputation.__call__ unpacks two lists from a prepare_targets
that returns four (make_golden_retinanet_loss.py).  So the model's own pieces are called in the detector's order: backbone.body, backbone.fpn,
rpn.head, rpn.anchor_generator, and the loss evaluator built from the model's configuration with the two steps of make_golden_retinanet_loss.py
around those lines (a subclass that drops prepare_targets' last two lists; gamma and alpha handed to sigmoid_focal_loss_cpu as one-element
tuples).  No arithmetic is touched.

Weights are NOT stored: both sides regenerate them (tests/e2e_retinanet_common.py::build on the CPU -- this package's seeded initialisation,
enriched and perturbed) and this script loads that state dict into the REFERENCE's model with the reference's load_state_dict (strict).

Stored, data only:
    tests/golden/e2e_retinanet_tiny.npz   image_seed, enrich_seed, anchor_sizes and, per variant v in (c5, p5): v_losses [2] = (cls, reg),
        v_n_pos, v_label_hist [5, C + 2] (the labels -1, 0, 1 .. C counted per level), and e2e_retinanet_common.spot's subsample of P3..P7
        (v_p<l>_spot) and of every level's logits and deltas (v_cls<l>_spot, v_reg<l>_spot), each with its max |value| (.._absmax)
    tests/golden/retinanet_state_dict_shapes.json   per variant the reference's state-dict keys and shapes, and the overrides

    python tests/golden/make_golden_e2e_retinanet.py
"""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, ROOT)
import ref_harness as rh  # noqa: E402

rh.setup()

import e2e_retinanet_common as E  # noqa: E402
from maskrcnn_benchmark.layers import SigmoidFocalLoss  # noqa: E402
from maskrcnn_benchmark.modeling.detector import build_detection_model  # noqa: E402
from maskrcnn_benchmark.modeling.rpn.retinanet.loss import RetinaNetLossComputation, generate_retinanet_labels  # noqa: E402
from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.boxlist_ops import cat_boxlist  # noqa: E402
from maskrcnn_benchmark.structures.image_list import ImageList  # noqa: E402


class Loss(RetinaNetLossComputation):
    def prepare_targets(self, anchors, targets):
        return super().prepare_targets(anchors, targets)[:2]


def run(use_c5, out, shapes):
    v = E.variant(use_c5)
    _, _, sd = E.build("cpu", use_c5)
    cfg = rh.default_cfg(None, E.overrides(use_c5, "cpu"))
    model = build_detection_model(cfg)
    own = model.state_dict()
    assert sorted(own) == sorted(sd), (sorted(set(own) ^ set(sd)))
    for k, t in sd.items():
        assert own[k].shape == t.shape, (k, own[k].shape, t.shape)
    model.load_state_dict(sd, strict=True)
    model.train()
    shapes[v] = {k: list(t.shape) for k, t in own.items()}

    images = ImageList(E.make_images(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    targets = []
    for (h, w), b, l in zip(E.IMAGE_SIZES, gts, gt_labels):
        t = BoxList(torch.from_numpy(b.copy()), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l.copy()))
        targets.append(t)
    ref = model.rpn.loss_evaluator
    r = cfg.MODEL.RETINANET
    ev = Loss(ref.proposal_matcher, ref.box_coder, generate_retinanet_labels, SigmoidFocalLoss((r.LOSS_GAMMA,), (r.LOSS_ALPHA,)),
              bbox_reg_beta=ref.bbox_reg_beta, regress_norm=ref.regress_norm)
    with torch.no_grad():
        cs, _ = model.backbone.body(images.tensors)
        feats = list(model.backbone.fpn(cs))
        assert [tuple(f.shape[-2:]) for f in feats] == list(E.MAPS)
        box_cls, box_reg = model.rpn.head(feats)
        anchors = model.rpn.anchor_generator(images, feats)
        labels, _ = ev.prepare_targets([cat_boxlist(a) for a in anchors], targets)
        loss_cls, loss_reg = ev(anchors, box_cls, box_reg, targets)
    labels = torch.stack(labels).numpy().astype(np.int64)
    # the fixture's conditions, on the reference's own labels
    hist = E.level_histogram(labels)
    assert (hist[:, 2:].sum(1) >= 1).all() and hist[:, 0].sum() >= 1, hist
    assert all((lab > 0).any() for lab in labels)
    out[v + "_losses"] = np.array([float(loss_cls), float(loss_reg)], np.float64)
    out[v + "_n_pos"] = np.array(int((labels > 0).sum()))
    out[v + "_label_hist"] = hist.astype(np.int32)
    for l in range(5):
        for name, t in (("p", feats[l]), ("cls", box_cls[l]), ("reg", box_reg[l])):
            out["%s_%s%d_spot" % (v, name, l)] = E.spot(t, l, E.CSTEP[name]).numpy().copy()
            out["%s_%s%d_absmax" % (v, name, l)] = np.array(float(t.abs().max()))
    print(v, "losses", out[v + "_losses"], "n_pos", int(out[v + "_n_pos"]), "labels per level", hist.tolist())


def main():
    torch.set_num_threads(8)
    out = {"image_seed": np.array(E.IMAGE_SEED), "enrich_seed": np.array(E.ENRICH_SEED), "anchor_sizes": np.array(E.ANCHOR_SIZES)}
    shapes = {}
    for use_c5 in (True, False):
        run(use_c5, out, shapes)
    path = os.path.join(HERE, "e2e_retinanet_tiny.npz")
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, "retinanet_state_dict_shapes.json"), "w") as f:
        json.dump({"overrides": {v: [list(x) if isinstance(x, tuple) else x for x in E.overrides(v == "c5")] for v in shapes}, "shapes": shapes}, f,
                  indent=1)
    print("file KB", os.path.getsize(path) / 1e3, "e2e_fpn_tiny.npz", os.path.getsize(os.path.join(HERE, "e2e_fpn_tiny.npz")) / 1e3)
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "e2e_fpn_tiny.npz"))


if __name__ == "__main__":
    main()

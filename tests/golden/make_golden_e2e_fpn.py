#!/usr/bin/env python3
"""Whole-FPN-detector golden FROM THE REFERENCE (in-container only): one training forward of the reference's own tiny R-50-FPN detector
(build_detection_model, MODEL.DEVICE cpu) on the two-image batch of tests/e2e_fpn_common.py.  Its ROIBoxHead.forward cannot run this head (it
unpacks two values from an extractor that returns one: see make_golden_box_head_fpn.py) and its ResNet hands its FPN a pair the FPN cannot
take, so the pieces are called in the detector's order: backbone (body, then fpn), rpn(images, features, targets) in train mode,
the box loss evaluator's subsample, feature_extractor, predictor, the loss evaluator's __call__.

Weights are NOT stored: both sides regenerate them (tests/e2e_fpn_common.py::build on the CPU -- this package's seeded initialisation, enriched
and perturbed) and this script loads that state dict into the REFERENCE's model with the reference's load_state_dict.

Conditions (checked here, stored as `cond_*`, checked again by tests/test_detector_fpn_ref.py):
  * among the box head's sampled RoIs each of the levels 0..3 holds at least 4 rows; positives and negatives both occur
  * each of the 5 RPN levels holds at least one sampled anchor; every ground-truth box has a positive anchor

Stored (tests/golden/e2e_fpn_tiny.npz, data only): the image seed, ground truth, the RPN sampler's draws (flat indices per image), the proposal
lists the box head sampled from (post-NMS + GT), the box-head draws with labels and regression targets, the four losses, the class logits and
box regression, and a fixed strided subsample (e2e_fpn_common.spot) of P2..P6 and of every level's RPN logits with each tensor's max |value|.

    python tests/golden/make_golden_e2e_fpn.py
"""
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

import e2e_fpn_common as E  # noqa: E402
import pooler_ref as P  # noqa: E402
import rpn_fpn_loss_ref as LR  # noqa: E402
from e2e_common import CONFIGS  # noqa: E402
from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler  # noqa: E402
from maskrcnn_benchmark.modeling.detector import build_detection_model  # noqa: E402
from maskrcnn_benchmark.structures.bounding_box import BoxList  # noqa: E402
from maskrcnn_benchmark.structures.image_list import ImageList  # noqa: E402


def main():
    torch.set_num_threads(8)
    _, dist_type, _, _, _, _, _, n_old = CONFIGS[E.CONFIG]
    from abr_iod_amd.engine.synthetic import VOC_CLASSES
    _, _, _, _, _, sd_t = E.build("cpu", need_source=False)
    cfg = rh.default_cfg(None, E.overrides("cpu") + ["DIST.TYPE", dist_type, "MODEL.ROI_BOX_HEAD.NAME_OLD_CLASSES", VOC_CLASSES[:n_old],
                                                      "MODEL.ROI_BOX_HEAD.NAME_NEW_CLASSES", VOC_CLASSES[n_old:]])
    model = build_detection_model(cfg)
    own = model.state_dict()
    missing = [k for k in own if k not in sd_t]
    assert not missing, missing
    for k, v in sd_t.items():
        assert own[k].shape == v.shape, (k, own[k].shape, v.shape)
    model.load_state_dict(sd_t, strict=True)
    model.train()

    images = ImageList(E.make_images(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    targets = []
    for (h, w), b, l in zip(E.IMAGE_SIZES, gts, gt_labels):
        t = BoxList(torch.from_numpy(b.copy()), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l.copy()))
        targets.append(t)

    draws = []
    orig = BalancedPositiveNegativeSampler.__call__

    def rec(self, matched_idxs, *a, **k):
        pos, neg = orig(self, matched_idxs, *a, **k)
        draws.append((pos, neg))
        return pos, neg
    BalancedPositiveNegativeSampler.__call__ = rec
    torch.manual_seed(11)
    try:
        with torch.no_grad():
            # (the reference's ResNet returns (outputs, backbone_features), which its own FPN cannot take through nn.Sequential: call the two)
            cs, _ = model.backbone.body(images.tensors)
            feats = list(model.backbone.fpn(cs))
            assert len(feats) == 5
            (proposals, rpn_losses), anchors, (objs, regs) = model.rpn(images, feats, targets)
            box = model.roi_heads.box
            pre = [p.bbox.clone().numpy() for p in proposals]
            sampled = box.loss_evaluator.subsample(proposals, targets)
            x = box.feature_extractor(feats, sampled)
            if isinstance(x, tuple):
                x = x[0]
            logits, boxreg = box.predictor(x)
            lc, lb = box.loss_evaluator([logits], [boxreg])
    finally:
        BalancedPositiveNegativeSampler.__call__ = orig
    assert len(draws) == 2, len(draws)
    (rpn_pos, rpn_neg), (head_pos, head_neg) = draws

    out = {"image_seed": np.array(E.IMAGE_SEED), "enrich_seed": np.array(E.ENRICH_SEED), "straddle": np.array(E.STRADDLE)}
    _, _, _, offs = E.anchors_np(E.IMAGE_SIZES[0])
    ok_gt, ok_rpn_levels, both, roi_levels = True, True, True, np.zeros(4, np.int64)
    for i in range(2):
        pos = torch.nonzero(rpn_pos[i]).squeeze(1).numpy()
        neg = torch.nonzero(rpn_neg[i]).squeeze(1).numpy()
        assert len(rpn_pos[i]) == offs[-1]
        out[f"rpn_pos{i}"], out[f"rpn_neg{i}"] = pos.astype(np.int32), neg.astype(np.int32)
        sel = torch.nonzero(head_pos[i] | head_neg[i]).squeeze(1).numpy()
        out[f"head_sel{i}"] = sel.astype(np.int32)
        out[f"props{i}"] = pre[i]
        assert np.array_equal(sampled[i].bbox.numpy(), pre[i][sel])
        out[f"det_labels{i}"] = sampled[i].get_field("labels").numpy().astype(np.int16)
        out[f"det_reg_targets{i}"] = sampled[i].get_field("regression_targets").numpy()
        out[f"gt{i}"], out[f"gt_labels{i}"] = gts[i], gt_labels[i]
        # ---- conditions
        lv = P.levels(np.concatenate([np.zeros((len(sel), 1), np.float32), pre[i][sel]], 1))
        roi_levels += np.bincount(lv, minlength=4)
        both &= bool((out[f"det_labels{i}"] > 0).any() and (out[f"det_labels{i}"] == 0).any())
        samp_lv = np.searchsorted(offs, np.concatenate([pos, neg]), side="right") - 1
        ok_rpn_levels &= bool((np.bincount(samp_lv, minlength=5) >= 1).all())
        _, boxes, vis, _ = E.anchors_np(E.IMAGE_SIZES[i])
        t = LR.prepare_targets(boxes, vis, gts[i])
        ok_gt &= all(bool(((t["matches"] == g) & (t["labels"] == 1)).any()) for g in range(len(gts[i])))
        print("image", i, "RoIs per level", np.bincount(lv, minlength=4).tolist(), "sampled anchors per level", np.bincount(samp_lv, minlength=5).tolist(),
              "of", np.bincount(P.levels(np.concatenate([np.zeros((len(pre[i]), 1), np.float32), pre[i]], 1)), minlength=4).tolist(),
              "positives", int((out[f"det_labels{i}"] > 0).sum()), "rpn pos/neg", len(pos), len(neg), "proposals", len(pre[i]))
    ok_levels = bool((roi_levels >= 4).all())      # over the batch's 128 sampled RoIs
    out["cond_roi_levels"], out["cond_pos_and_neg"] = np.array(ok_levels), np.array(both)
    out["cond_rpn_levels"], out["cond_gt_positive_anchor"] = np.array(ok_rpn_levels), np.array(ok_gt)
    assert ok_levels and both and ok_rpn_levels and ok_gt, (ok_levels, both, ok_rpn_levels, ok_gt)

    for l in range(5):
        out[f"p{l + 2}_spot"], out[f"p{l + 2}_absmax"] = E.spot(feats[l], l).numpy(), np.array(float(feats[l].abs().max()))
        out[f"rpn_obj{l}_spot"] = objs[l][:, :, ::max(1, 8 >> l), ::max(1, 8 >> l)].numpy()
        out[f"rpn_obj{l}_absmax"] = np.array(float(objs[l].abs().max()))
    out["det_logits"], out["det_boxreg"] = logits.numpy(), boxreg.numpy()
    out["loss_classifier"], out["loss_box_reg"] = np.array(float(lc)), np.array(float(lb))
    out["loss_objectness"], out["loss_rpn_box_reg"] = np.array(float(rpn_losses["loss_objectness"])), np.array(float(rpn_losses["loss_rpn_box_reg"]))
    path = os.path.join(HERE, "e2e_fpn_tiny.npz")
    np.savez_compressed(path, **out)
    print({k: float(out[k]) for k in out if k.startswith("loss")}, "file KB", os.path.getsize(path) / 1e3)


if __name__ == "__main__":
    main()

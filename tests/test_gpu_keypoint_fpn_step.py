"""GPU: two training steps of the tiny R-50-FPN detector with MODEL.KEYPOINT_ON (upstream's keypoint settings at CONV_LAYERS (8, 8):
tests/keypoint_fpn_ref.py::KEYPOINT_CFG), on the two images and ground truth of tests/e2e_fpn_common.py -- the image size
tests/test_gpu_mask_head_fpn.py's step test uses -- through model(images, targets) and FusedSGD.step, without and with MODEL.MASK_ON:
every loss is finite, loss_kp among them, every keypoint-head parameter lies in the flat buffer and moves, the other losses of the first step
equal those of a KEYPOINT_ON False run on the same batch, weights and seed bit for bit (tests/test_gpu_keypoint_step.py's rule), and loss_kp
equals the head alone on the detector's own pyramid and sampled set bit for bit."""
import math
import random

import numpy as np
import pytest
import torch

import e2e_fpn_common as E
import keypoint_fpn_ref as KR
import mask_head_fpn_ref as MR
import pooler_ref as P

pytestmark = pytest.mark.gpu

MASK_SEED = 11


def _batch(mask_on):
    from abr_iod_amd.engine.synthetic import _box_keypoints
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    images = ImageList(E.make_images().cuda(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    targets = []
    for i, ((h, w), b, l) in enumerate(zip(E.IMAGE_SIZES, gts, gt_labels)):
        t = BoxList(torch.from_numpy(b).cuda(), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l).cuda())
        t.add_field("keypoints", PersonKeypoints(_box_keypoints(torch.from_numpy(b), 17).cuda(), (w, h)))
        if mask_on:
            t.add_field("masks", SegmentationMask(torch.from_numpy(MR.ellipse_masks(MASK_SEED + i, b, h, w)).cuda(), (w, h), mode="mask"))
        targets.append(t)
    return images, targets


def _build(mask_on, keypoint_on, sd=None):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict
    extra = (MR.MASK_CFG if mask_on else []) + (KR.KEYPOINT_CFG if keypoint_on else [])
    cfg = make_cfgs("15-5", overrides=E.overrides("cuda") + extra)[1]
    _, mt = build_models(None, cfg, seed=0, need_source=False)
    if sd is None:
        sd = E.enrich(E.cpu_sd(mt))
    missing = load_reference_state_dict(mt, sd, strict=False)       # the KEYPOINT_ON False run's weights; the keypoint head keeps its own
    assert all(k.startswith("roi_heads.keypoint.") for k in missing) and bool(missing) == keypoint_on
    return cfg, mt, sd


def _two_steps(cfg, mt, images, targets):
    from abr_iod_amd.solver.build import make_optimizer
    opt = make_optimizer(cfg, mt)
    mt.train()
    seen, head_alone = [], None
    for step in range(2):
        torch.manual_seed(11)
        random.seed(11)
        mt.flat.zero_grad()
        out = mt(images, targets)
        loss_dict, feats = out[0], out[1]
        if step == 0 and "keypoint" in mt.roi_heads:
            ev = mt.roi_heads.box.loss_evaluator
            with torch.no_grad():
                alone = mt.roi_heads.keypoint(feats, ev._proposals, targets, fused=getattr(ev, "_fused_targets", None))
            sel = mt.roi_heads.keypoint.last_selection
            head_alone = dict(loss=alone[2]["loss_kp"].detach().clone(), n_pos=int(sel["n_pos"]), pos_rows=sel["pos_rows"].cpu().numpy(),
                              table=sel["table"].cpu().numpy(), n_maps=len(feats))
        sum(loss_dict.values()).backward()
        opt.step()
        torch.cuda.synchronize()
        seen.append({k: v.detach().clone() for k, v in loss_dict.items()})
    return seen, head_alone


@pytest.mark.parametrize("mask_on", [False, True], ids=["keypoint", "mask+keypoint"])
def test_fpn_keypoint_train_steps(mask_on):
    images, targets = _batch(mask_on)
    cfg0, off, sd = _build(mask_on, False)
    seen_off, _ = _two_steps(cfg0, off, images, targets)
    del off
    cfg, mt, _ = _build(mask_on, True, sd)
    assert list(mt.roi_heads.keys()) == ["box"] + (["mask"] if mask_on else []) + ["keypoint"]
    kp_names = [n for n, _ in mt.named_parameters() if n.startswith("roi_heads.keypoint.")]
    assert len(kp_names) == 6, kp_names       # two conv_fcn layers and kps_score_lowres, weight + bias each
    before = {n: mt.get_parameter(n).detach().clone() for n in kp_names}
    seen, alone = _two_steps(cfg, mt, images, targets)
    want = {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg", "loss_kp"} | ({"loss_mask"} if mask_on else set())
    for ld in seen:
        assert set(ld) == want and all(math.isfinite(float(v)) for v in ld.values()), ld
    print({k: float(v) for k, v in seen[0].items()}, {k: float(v) for k, v in seen[1].items()})
    assert float(seen[0]["loss_kp"]) > 0
    flat = mt.flat.params
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for n, v in before.items():
        p = mt.get_parameter(n)
        assert lo <= p.data_ptr() < hi, n + " lies outside the flat parameter buffer"
        assert bool(torch.isfinite(p).all()) and not torch.equal(p.detach(), v), n + " did not move"
    # KEYPOINT_ON False on the same batch, weights and seed: the other losses of the first step are the same numbers
    assert set(seen[0]) - set(seen_off[0]) == {"loss_kp"}
    for k, v in seen_off[0].items():
        assert torch.equal(seen[0][k], v), (k, float(seen[0][k]), float(v))
    # the head alone on the detector's own pyramid (P6 dropped by the extractor) and sampled set: the same loss_kp, bit for bit
    assert alone["n_maps"] == 5 and torch.equal(alone["loss"], seen[0]["loss_kp"])
    rows = alone["pos_rows"]
    live = rows[rows >= 0]
    assert alone["n_pos"] == len(live) >= 4 and (rows[len(live):] == -1).all()
    lv = P.levels(alone["table"][live])
    print("live", len(live), "of", len(rows), "per level", np.bincount(lv, minlength=4).tolist())
    assert len(set(lv.tolist())) >= 3, lv.tolist()

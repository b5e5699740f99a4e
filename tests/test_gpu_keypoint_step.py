"""GPU: two training steps with MODEL.KEYPOINT_ON, at the smallest image tests/test_gpu_mask_head.py's step test uses, for the finetune trainer
and the incremental trainer, on the joint head pass and on the two head passes: loss_kp is in the dict, every loss is finite, the new
parameters lie in the flat buffer and move, a second run from the same seed reproduces the losses bit for bit, and the other losses of the
first step equal those of a KEYPOINT_ON False run on the same batch (first-step losses do not depend on any learning rate)."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu


SMALL = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 600, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 300,
         "MODEL.RPN.POST_NMS_TOP_N_TEST", 150, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 48, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64]
KP_ON = ["MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False, "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 6,
         "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 24, "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", (32, 32), "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", (0.0625,)]


def _build(name, box_res, keypoint_on, seed=0):
    from e2e_common import CONFIGS, clamp_targets, needs_source
    from abr_iod_amd.engine.synthetic import _box_keypoints, build_models, make_cfgs, synthetic_batch
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    task, dist_type, feat, alpha, beta, gamma, label_range, n_old = CONFIGS[name]
    extra = SMALL + ["MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", box_res] + (KP_ON if keypoint_on else [])
    cfg_s, cfg_t = make_cfgs(task, dist_type=dist_type, feat=feat, alpha=alpha, beta=beta, gamma=gamma, overrides=extra)
    torch.manual_seed(seed)
    random.seed(seed)
    ms, mt = build_models(cfg_s, cfg_t, seed=seed, need_source=needs_source(name))
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=label_range)
    clamp_targets(targets, 224, 160)
    for t in targets:      # keypoints inside the (clamped) GT boxes
        t.add_field("keypoints", PersonKeypoints(_box_keypoints(t.bbox.cpu(), 17).cuda(), (224, 160)))
    return ms, mt, cfg_t, images, targets


def _two_steps(name, box_res, keypoint_on):
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    ms, mt, cfg, images, targets = _build(name, box_res, keypoint_on)
    kp_names = [n for n, _ in mt.named_parameters() if "roi_heads.keypoint" in n]
    before = {n: mt.get_parameter(n).detach().clone() for n in kp_names}
    opt = make_optimizer(cfg, mt)
    sch = make_lr_scheduler(cfg, opt)
    seen = []
    for _ in range(2):
        torch.manual_seed(11)
        random.seed(11)
        ld, _ = train_step(ms, mt, images, targets, opt, sch, cfg, next_images=images)
        torch.cuda.synchronize()
        seen.append({k: float(v) for k, v in ld.items()})
    return mt, before, seen


@pytest.mark.parametrize("name,box_res", [("finetune", 7), ("15-5", 7), ("15-5", 8)], ids=["finetune-joint", "incremental-joint", "incremental-two-pass"])
def test_keypoint_train_steps(name, box_res):
    """(an even box pooler makes the trainer take the two head passes instead of the joint one.  8, not the Mask R-CNN setting 14: beyond 8
    bins per axis ROIAlign's backward leaves its atomic-free gather form for the per-RoI atomics, whose sums are not reproducible from run to
    run -- seen here as last-bit differences in every loss of the second step -- with or without this head)"""
    mt, before, seen = _two_steps(name, box_res, True)
    assert mt.roi_heads.joint_supported == (box_res == 7)
    assert len(before) == 6, sorted(before)       # two conv_fcn layers and kps_score_lowres, weight + bias each
    for ld in seen:
        assert "loss_kp" in ld and all(math.isfinite(v) for v in ld.values()), ld
    assert seen[0]["loss_kp"] > 0
    flat = mt.flat.params
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * 4
    for n, v in before.items():
        p = mt.get_parameter(n)
        assert lo <= p.data_ptr() < hi, f"{n} lies outside the flat parameter buffer"
        assert not torch.equal(p.detach(), v), f"{n} did not move"
    # the same seed reproduces the losses bit for bit
    _, _, again = _two_steps(name, box_res, True)
    assert again == seen, (again, seen)
    # KEYPOINT_ON False on the same batch: the other losses of the first step are the same numbers
    _, none, off = _two_steps(name, box_res, False)
    assert not none
    for k, v in off[0].items():
        assert seen[0][k] == v, (k, seen[0][k], v)
    assert set(seen[0]) - set(off[0]) == {"loss_kp"}

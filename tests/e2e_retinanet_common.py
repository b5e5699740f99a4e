"""Shared by the whole-RetinaNet-detector tests (tests/test_detector_retinanet_ref.py on the CPU, tests/test_gpu_e2e_retinanet.py on the GPU)
and the generator of their fixture (tests/golden/make_golden_e2e_retinanet.py): the tiny R-50-FPN-RETINANET configuration in both
MODEL.RETINANET.USE_C5 variants, the two-image batch, the ground truth, and the weights.

Weights are never stored: every side rebuilds them from the package's seeded CPU initialisation (build_detection_model under
torch.manual_seed(0), engine/synthetic.py::randomize_frozen_bn for the FrozenBN statistics) exported through `reference_state_dict`, then
`enrich` (non-zero biases from a CPU generator, the head's weights grown) and `e2e_common.perturb_trainable`.

The batch is tests/test_gpu_retinanet_loss.py's tiny pyramid, already the edge case: a 128 x 192 canvas holding one 128 x 192 image and one
112 x 160 image (zero padded), maps 16 x 24, 8 x 12, 4 x 6, 2 x 3 and 1 x 2 -- P7 is a stride-2 3 x 3 conv onto a 1 x 2 map.

MODEL.RETINANET.ANCHOR_SIZES is (16, 32, 64, 96, 128), not that test's (16, .., 256): a 256-anchor (362 x 181 at the least) overlaps nothing
that fits a 128 x 192 image by more than a 128-anchor of P6 does, so with those sizes no P7 anchor is ever positive and the head's coarsest
level would receive a gradient from background anchors only."""
import json
import os

import numpy as np
import torch

import retinanet_loss_ref as RL
import retinanet_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 128, 192
IMAGE_SIZES = R.IMAGE_SIZES                   # ((128, 192), (112, 160)), (h, w)
MAPS, STRIDES = R.MAPS, R.STRIDES
ANCHOR_SIZES = (16, 32, 64, 96, 128)
A, C = 9, 3                                   # 27 logits in rows of 28: cls_logits keeps its pad row
NUM_CONVS = 2
IMAGE_SEED, ENRICH_SEED = 37, 20      # (the enrich seed: see NEAR_ZERO below)
# integer boxes; the conditions tests/test_detector_retinanet_ref.py::test_fixture_conditions asserts were searched for with them
GT_BOXES = (((122.0, 35.0, 138.0, 63.0), (62.0, 39.0, 97.0, 100.0), (34.0, 47.0, 131.0, 124.0), (2.0, 1.0, 172.0, 124.0)),
            ((40.0, 53.0, 75.0, 87.0), (58.0, 1.0, 113.0, 74.0), (12.0, 2.0, 154.0, 110.0)))
GT_LABELS = ((1, 3, 2, 1), (3, 2, 2))
# The reference initialises the head at std 0.01 with the prior-probability bias -log(99): its logits stay within a few hundredths of -4.6, the
# focal gradient that reaches the pyramid is tiny, and what returns from P7 through p7, the ReLU mask and p6 into C5 would move no parameter
# gradient by more than rounding does.  The towers and the two output convs are grown until the logits spread over a few units (the regression
# deltas stay small: smooth-L1's two branches both occur) and every mutation of tests/detector_retinanet_ref.py is visible at
# 10 x GRAD_MAX_REL (tests/test_detector_retinanet_ref.py::test_fixture_sees_composition_bugs).
TOWER_GAIN, CLS_GAIN, REG_GAIN = 12.0, 12.0, 4.0
# No tower ReLU input and no P6 element of the float64 model lies within NEAR_ZERO of zero, before the optimiser step and -- within
# NEAR_ZERO_STEPPED, on `stepped_sd`'s weights -- after it: such an element changes sign between the arithmetics and takes a whole gradient
# path with it.  With enrich seed 11 the step moved one input of the cls tower's first conv on P5 to 8.7e-7: under f32 its mask flipped and
# fpn_layer4's gradients, which only P5's 48 pixels feed, moved by 6.7e-2 (flipping that one mask in the float64 model reproduces every figure).
# Seed 20 keeps all four states (two variants, before and after) 4.4e-5 clear.
NEAR_ZERO, NEAR_ZERO_STEPPED = 1e-6, 1e-5
BASE = ["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", "R-50-FPN-RETINANET", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16,
        "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16,
        "MODEL.RETINANET.NUM_CLASSES", C + 1, "MODEL.RETINANET.NUM_CONVS", NUM_CONVS, "MODEL.RETINANET.ANCHOR_SIZES", ANCHOR_SIZES,
        "MODEL.RETINANET.PRE_NMS_TOP_N", 60, "TEST.DETECTIONS_PER_IMG", 40]

# Gradient bounds of tests/test_gpu_e2e_retinanet.py: 3 x the worst value measured against the float64 model over both USE_C5 variants, the
# three arithmetics, both backward passes of the suite and four runs (profiles/e2e_retinanet_parity.txt: max-rel 3.050e-6 under f16x3 with P5
# after the step, l2-rel 1.360e-6 under f32 with C5 before it; the four runs agree to the last digit), the convention of tests/e2e_fpn_common.py
# (ReLU sign flips are discontinuous).  They are 15 times tighter than the FPN detector's: these maps are small, and no ReLU of this fixture
# flipped.  A flip shows as 1e-4 and more (NEAR_ZERO above has a measured case).  The sensitivity test asks every mutation for 10 x GRAD_MAX_REL.
GRAD_MAX_REL, GRAD_REL_L2 = 9.2e-6, 4.1e-6


def variant(use_c5):
    return "c5" if use_c5 else "p5"


def overrides(use_c5, device=None):
    out = BASE + ["MODEL.RETINANET.USE_C5", bool(use_c5)]
    if device is not None:
        out += ["MODEL.DEVICE", device]
    return out


def shapes_json():
    with open(os.path.join(HERE, "golden", "retinanet_state_dict_shapes.json")) as f:
        return json.load(f)


def make_images():
    """[2,3,H,W] float32 on the CPU: uint8-valued pixels minus the pixel mean; the second image zero outside its 112 x 160 (to_image_list's pad)"""
    g = torch.Generator().manual_seed(IMAGE_SEED)
    mean = torch.tensor([102.9801, 115.9465, 122.7717]).view(1, 3, 1, 1)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g).float() - mean
    for i, (h, w) in enumerate(IMAGE_SIZES):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    return img


def gt_arrays():
    return [np.array(b, np.float32) for b in GT_BOXES], [np.array(l, np.int64) for l in GT_LABELS]


def anchors_np():
    """per level the [H*W*A,4] anchors from the oracle's C restatement (one grid for the batch: RetinaNet discards nothing by visibility)"""
    return R.pyramid_anchors(MAPS, STRIDES, ANCHOR_SIZES, R.RATIOS, IMAGE_SIZES[0])


def batch_targets(anchors=None):
    """retinanet_loss_ref.batch_targets of the fixture's ground truth on the levels' concatenated anchors"""
    gts, labs = gt_arrays()
    return RL.batch_targets(np.concatenate(anchors_np()) if anchors is None else anchors, gts, labs)


def level_histogram(labels):
    """[L, C + 2] counts of the labels -1, 0, 1 .. C per level over the batch"""
    offs = np.concatenate([[0], np.cumsum([h * w * A for h, w in MAPS])])
    return np.stack([np.bincount(np.asarray(labels)[:, offs[l]:offs[l + 1]].reshape(-1) + 1, minlength=C + 2) for l in range(len(MAPS))])


def enrich(sd, seed=ENRICH_SEED):
    """in place on a reference-layout state dict of CPU tensors, in the dict's order: 0.1 N(0,1) added to every conv bias (cls_logits keeps its
    prior around it), the head's weights grown by TOWER_GAIN / CLS_GAIN / REG_GAIN.  Asserts the FrozenBN statistics are not the identity."""
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        mod = k.split(".")[-2]
        if "anchor_generator" in k or mod.startswith("bn") or k.split(".")[-3:-1] == ["downsample", "1"]:
            continue
        if k.endswith(".bias"):
            v.add_(0.1 * torch.randn(v.shape, generator=g))
        elif k.startswith("rpn.head."):
            v.mul_(CLS_GAIN if "cls_logits" in k else (REG_GAIN if "bbox_pred" in k else TOWER_GAIN))
    rv = sd["backbone.body.layer4.2.bn3.running_var"]
    assert float((rv - 1).abs().max()) > 0.1 and float(sd["backbone.body.layer4.2.bn3.running_mean"].abs().max()) > 0
    return sd


def cpu_sd(model):
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    return {k: v.detach().cpu().clone() for k, v in reference_state_dict(model).items()}


def build(device, use_c5):
    """(cfg, model, sd): the model built on `device` and LOADED with the fixture's weights (sd: reference layout, CPU float32)"""
    from abr_iod_amd.config import cfg as default_cfg
    from abr_iod_amd.engine.synthetic import randomize_frozen_bn
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict
    from detector_retinanet_ref import trainable_keys
    from e2e_common import perturb_trainable
    cfg = default_cfg.clone()
    cfg.merge_from_list(overrides(use_c5, device))
    torch.manual_seed(0)
    model = build_detection_model(cfg)
    with torch.no_grad():
        randomize_frozen_bn(model, 1)
    sd = enrich(cpu_sd(model))
    perturb_trainable(sd, trainable_keys(sd))
    assert load_reference_state_dict(model, sd) == []
    model.train()
    return cfg, model, sd


# The optimiser step of tests/test_gpu_e2e_retinanet.py: STEP_REL of the weights' norm long, bias learning-rate factor 2, no weight decay on a
# bias, and a weight decay that moves a weight by LR_TIMES_WD of itself whatever learning rate the step works out to (a tensor decayed that must
# not be, or the reverse, leaves the update rule's tolerance by three orders of magnitude).
STEP_REL, MOMENTUM, BIAS_LR_FACTOR, BIAS_WD, LR_TIMES_WD = 0.02, 0.9, 2.0, 0.0, 1e-3


def step_lr(p_norm, g_norm):
    return STEP_REL * float(p_norm) / float(g_norm)


def rule(key, lr):
    """the reference's per-tensor rule (solver/build.py:7-21): a key containing "bias" gets lr x BIAS_LR_FACTOR and weight decay BIAS_WD"""
    return (lr * BIAS_LR_FACTOR, BIAS_WD) if "bias" in key else (lr, LR_TIMES_WD / lr)


def stepped_sd(sd, grads):
    """the state dict after that step from zero momentum, p - lr_k (g + wd_k p) evaluated in float64 from float64 gradients and rounded to
    fp32: what the GPU's step leaves, up to its roundings.  The CPU test checks the fixture's conditions on these weights too: the GPU test
    compares a second backward pass after the step, and a ReLU input that the step moved next to zero flips there as it would here."""
    keys = list(grads)
    lr = step_lr(torch.cat([sd[k].double().reshape(-1) for k in keys]).norm(), torch.cat([grads[k].reshape(-1) for k in keys]).norm())
    out = {k: v.clone() for k, v in sd.items()}
    for k in keys:
        lr_k, wd_k = rule(k, lr)
        p = sd[k].double()
        out[k] = (p - lr_k * (grads[k] + wd_k * p)).float()
    return out, lr


# the fixed subsample the fixture stores of every pyramid map and of every level's logits and deltas: the two fine levels every cstep-th
# channel (4 for the 27 logits: anchors and classes both vary along it), level 0 every second row and column; the coarse levels whole
def spot(t, level, cstep):
    if level >= 2:
        return t
    st = 2 if level == 0 else 1
    return t[:, ::cstep, ::st, ::st]


CSTEP = dict(p=3, cls=4, reg=5)

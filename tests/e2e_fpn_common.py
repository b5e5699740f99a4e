"""Shared by the whole-FPN-detector tests (tests/test_detector_fpn_ref.py on the CPU, tests/test_gpu_e2e_fpn.py on the GPU) and the generator
of their fixture (tests/golden/make_golden_e2e_fpn.py): the tiny R-50-FPN configuration, the two-image batch, the ground truth, and the weights.

Weights are never stored: every side rebuilds them from the package's seeded CPU initialisation (engine/synthetic.py::build_models(seed=0),
which also draws the FrozenBN statistics from a CPU generator) exported through `reference_state_dict`, then `enrich` (non-zero biases and
predictor weights of ordinary size, from a CPU generator: the reference's zero biases and 1e-2 / 1e-3 predictor weights would hide a dropped
bias) and `e2e_common.perturb_trainable` on the target (target != source, so that ID and ARD have gradients).

The batch: a 512 x 704 canvas holding one 512 x 704 image and one 480 x 600 image (zero padded), so the second image's anchor visibility and
proposal clipping differ from the canvas.  Four ground-truth boxes per image with sqrt(area) near 60, 150, 300 and above 450: the level rule
(canonical scale 224) sends RoIs around them to P2, P3, P4 and P5.

MODEL.RPN.STRADDLE_THRESH is 128, not the default 0: the P6 anchors (728 x 360, 512 x 512, 360 x 728 at stride 64) do not fit inside a
512 x 704 image, so with 0 no P6 anchor is ever visible or sampled and the fifth RPN level would receive no loss gradient at all; with 128 they
are, and the visibility mask still depends on the image size (the second image's differs)."""
import json
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
CONFIG = "15-5"
H, W = 512, 704
IMAGE_SIZES = ((512, 704), (480, 600))        # (h, w)
IMAGE_SEED, ENRICH_SEED = 31, 7
GT_BOXES = (((40.0, 30.0, 105.0, 85.0), (150.0, 40.0, 320.0, 170.0), (300.0, 180.0, 640.0, 450.0), (96.0, 0.0, 607.0, 479.0)),
            ((500.0, 400.0, 560.0, 455.0), (30.0, 300.0, 190.0, 440.0), (200.0, 20.0, 520.0, 300.0), (32.0, 0.0, 543.0, 479.0)))
GT_LABELS = ((16, 18, 20, 17), (19, 16, 17, 20))
STRIDES = (4, 8, 16, 32, 64)
MAPS = tuple((H // s, W // s) for s in STRIDES)
ANCHOR_SIZES = (32, 64, 128, 256, 512)
STRADDLE = 128
# eval: at 0.05 the float64 run keeps more than DETECTIONS_PER_IMG = 100 candidates per image (the k-th value cut runs) and none of its decisions
# lies within the margins tests/test_gpu_e2e_fpn.py::test_fpn_eval_detections_vs_float64 excludes (0.1 leaves ~30 detections and no cut)
SCORE_THRESH = 0.05
# `enrich` scales the neck's output convs per level.  A freshly initialised shared RPN head scores every level alike, so the cross-level cut
# (top 300 of the batch by objectness) keeps what the 67 584 P2 anchors' extreme tail offers and next to nothing of the 1 056 P5 anchors: the
# box head would then sample no RoI large enough for P4 / P5.  Growing the coarse levels' outputs grows their logits' spread with them.
LEVEL_GAIN = (1.0, 4.0, 16.0, 64.0)
# ... and shrinking the RPN regression weights keeps the proposals near their anchors: a 512-anchor whose wild deltas are clipped to the whole image
# is the same box as every other one and NMS leaves a single P5-sized proposal.
RPN_REG_GAIN = 0.02
# The reference initialises the RPN head at std 0.01: its logits stay within +-0.3 and its loss sends the maps a gradient some 200 times smaller
# than the box head's, so a composition bug on the RPN's side of a map (P6's gradient returning into P5) would move no parameter gradient by
# more than rounding does.  The head's conv and logit weights are grown until the coarse levels' logits reach a few units, and fc6 -- which
# reads P4 / P5 values in the hundreds -- is shrunk, so that both heads send the pyramid gradients of the same order.
RPN_CONV_GAIN, RPN_CLS_GAIN, FC6_GAIN = 5.0, 4.0, 1.0 / 16
EXTRA = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 600, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 200, "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 300,
         "MODEL.RPN.PRE_NMS_TOP_N_TEST", 600, "MODEL.RPN.POST_NMS_TOP_N_TEST", 200, "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 300,
         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 256, "MODEL.RPN.STRADDLE_THRESH", STRADDLE,
         "MODEL.ROI_HEADS.SCORE_THRESH", SCORE_THRESH]

# Gradient bounds of tests/test_gpu_e2e_fpn.py: 3 x the worst value measured against the float64 model over the three arithmetics, both
# backward passes of the suite and four runs (profiles/e2e_fpn_parity.txt: max-rel 4.44e-5, l2-rel 2.64e-5), the convention of
# tests/test_gpu_e2e.py (ReLU sign flips are discontinuous).  The sensitivity test asks every mutation for 10 x GRAD_MAX_REL.
GRAD_MAX_REL, GRAD_REL_L2 = 1.4e-4, 8e-5


def shapes_json():
    with open(os.path.join(HERE, "golden", "box_head_fpn_state_dict_shapes.json")) as f:
        return json.load(f)


def overrides(device=None):
    """the shapes JSON's tiny R-50-FPN overrides (its MODEL.DEVICE dropped) + EXTRA"""
    o = shapes_json()["overrides"]
    out = []
    for k, v in zip(o[0::2], o[1::2]):
        if k != "MODEL.DEVICE":
            out += [k, tuple(v) if isinstance(v, list) else v]
    out += EXTRA
    if device is not None:
        out += ["MODEL.DEVICE", device]
    return out


def make_images():
    """[2,3,H,W] float32 on the CPU: uint8-valued pixels minus the pixel mean; the second image zero outside its 480 x 600 (to_image_list's pad)"""
    g = torch.Generator().manual_seed(IMAGE_SEED)
    mean = torch.tensor([102.9801, 115.9465, 122.7717]).view(1, 3, 1, 1)
    img = torch.randint(0, 256, (2, 3, H, W), generator=g).float() - mean
    for i, (h, w) in enumerate(IMAGE_SIZES):
        img[i, :, h:, :] = 0
        img[i, :, :, w:] = 0
    return img


def gt_arrays():
    return [np.array(b, np.float32) for b in GT_BOXES], [np.array(l, np.int64) for l in GT_LABELS]


def enrich(sd, seed=ENRICH_SEED):
    """in place on a reference-layout state dict of CPU tensors, in the dict's order: every conv / linear bias ~ 0.1 N(0,1); the predictor's two
    weights ~ U(+-sqrt(3 / fan_in)).  Asserts the FrozenBN statistics are not the identity (build_models draws them)."""
    g = torch.Generator().manual_seed(seed)
    for k, v in sd.items():
        mod = k.split(".")[-2]
        if "anchor_generator" in k or mod.startswith("bn") or k.split(".")[-3:-1] == ["downsample", "1"]:
            continue
        if k.endswith(".bias"):
            v.copy_(0.1 * torch.randn(v.shape, generator=g))
        gain = {"rpn.head.bbox_pred.weight": RPN_REG_GAIN, "rpn.head.conv.weight": RPN_CONV_GAIN, "rpn.head.cls_logits.weight": RPN_CLS_GAIN,
                "roi_heads.box.feature_extractor.fc6.weight": FC6_GAIN}.get(k)
        if gain is not None:
            v.mul_(gain)
        if k.startswith("backbone.fpn.fpn_layer"):
            v.mul_(LEVEL_GAIN[int(k.split(".")[2][len("fpn_layer"):]) - 1])
        elif k.startswith("roi_heads.box.predictor.") and k.endswith(".weight"):
            v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) * (3.0 / v.shape[1]) ** 0.5)
    rv = sd["backbone.body.layer4.2.bn3.running_var"]
    assert float((rv - 1).abs().max()) > 0.1 and float(sd["backbone.body.layer4.2.bn3.running_mean"].abs().max()) > 0
    return sd


def cpu_sd(model):
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    return {k: v.detach().cpu().clone() for k, v in reference_state_dict(model).items()}


def state_dicts(ms, mt):
    """(source, target) reference-layout state dicts (CPU float32) of freshly built models: see the module docstring"""
    from detector_fpn_ref import trainable_keys
    from e2e_common import perturb_trainable
    sd_t = enrich(cpu_sd(mt))
    perturb_trainable(sd_t, trainable_keys(sd_t))
    return (enrich(cpu_sd(ms)) if ms is not None else None), sd_t


def build(device, need_source=True):
    """(cfg_s, cfg_t, ms, mt, sd_s, sd_t): the models built on `device` and LOADED with the fixture's weights"""
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict
    from e2e_common import CONFIGS
    task, dist_type, feat, alpha, beta, gamma, _, _ = CONFIGS[CONFIG]
    cfg_s, cfg_t = make_cfgs(task, dist_type=dist_type, feat=feat, alpha=alpha, beta=beta, gamma=gamma, overrides=overrides(device))
    ms, mt = build_models(cfg_s, cfg_t, seed=0, need_source=need_source)
    sd_s, sd_t = state_dicts(ms, mt)
    assert load_reference_state_dict(mt, sd_t) == []
    if ms is not None:
        assert load_reference_state_dict(ms, sd_s) == []
    return cfg_s, cfg_t, ms, mt, sd_s, sd_t


def anchors_np(image_hw):
    """(per-level list of ([n_l,4] anchors, [n_l] visibility), concatenated boxes, concatenated visibility, offsets) from the oracle's C restatement"""
    from oracle import ops as O
    per = []
    for (h, w), st, s in zip(MAPS, STRIDES, ANCHOR_SIZES):
        per.append(O.grid_anchors(O.cell_anchors(stride=st, sizes=(s,), ratios=(0.5, 1.0, 2.0)), h, w, st, image_hw, STRADDLE))
    offs = np.concatenate([[0], np.cumsum([len(a) for a, _ in per])]).astype(np.int64)
    return per, np.concatenate([a for a, _ in per]), np.concatenate([np.asarray(v).astype(bool) for _, v in per]), offs


def box_targets(gt, gt_labels, boxes, weights=(10.0, 10.0, 5.0, 5.0)):
    """box_head/loss.py:56-84 through the oracle: (labels int64 [n] (0 background, -1 ignored), regression targets [n,4], matches)"""
    from oracle import ops as O
    m = O.matcher(O.box_iou(np.asarray(gt, np.float32), np.asarray(boxes, np.float32)), 0.5, 0.5, False)
    lab = np.asarray(gt_labels, np.int64)[np.clip(m, 0, None)]
    lab[m == -1] = 0
    lab[m == -2] = -1
    tgt = O.box_encode(np.asarray(gt, np.float32)[np.clip(m, 0, None)], np.asarray(boxes, np.float32), weights)
    return lab, tgt, m


# the fixed strided subsample the fixture stores of every pyramid map and of every level's RPN logits: (channel step, row step, column step)
def spot(t, level):
    st = max(1, 8 >> level)
    return t[:, ::5, ::st, ::st]

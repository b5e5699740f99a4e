"""CPU: the FPN mask head's construction, checkpoint keys and refusals, and the float64 model of tests/mask_head_fpn_ref.py against the
reference's own MaskRCNNFPNFeatureExtractor + MaskRCNNC4Predictor + loss + post-processor (tests/golden/mask_head_fpn.npz).  No kernels.

Bound of the float64 model against the float32 reference: 1e-4 relative to the largest magnitude of the compared tensor, the bound
tests/test_detector_fpn_ref.py uses for the same purpose."""
import json
import os

import numpy as np
import pytest
import torch

import mask_head_fpn_ref as MR
from abr_iod_amd.engine.synthetic import make_cfgs
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.modeling.roi_heads.mask_head.fpn_mask_head import MaskRCNNFPNFeatureExtractor
from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import MaskRCNNC4Predictor
from abr_iod_amd.utils.checkpoint import load_reference_state_dict, reference_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = os.path.join(HERE, "golden", "mask_head_fpn_state_dict_shapes.json")
TOL = 1e-4


def _overrides(extra=()):
    with open(SHAPES) as f:
        gold = json.load(f)
    ov = [tuple(v) if isinstance(v, list) else v for v in gold["overrides"]]
    return ov + list(extra), gold["shapes"]


def _cfg(extra=()):
    return make_cfgs("15-5", overrides=_overrides(extra)[0])[1]


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= TOL * max(ref, 1e-30), (what, err, ref)
    return err / max(ref, 1e-30)


# ------------------------------------------------------------------------------------------------ the detector on the CPU
def test_fpn_mask_detector_builds_with_the_reference_keys_and_round_trips():
    torch.manual_seed(0)
    ov, shapes = _overrides()
    assert ov[-len(MR.MASK_CFG):] == MR.MASK_CFG
    m = build_detection_model(_cfg())
    mask = m.roi_heads.mask
    fe = mask.feature_extractor
    assert mask.unshared and isinstance(fe, MaskRCNNFPNFeatureExtractor) and isinstance(mask.predictor, MaskRCNNC4Predictor)
    assert fe is not m.roi_heads.box.feature_extractor and fe.blocks == ["mask_fcn1", "mask_fcn2"] and fe.out_channels == 8
    assert [n for n, _ in fe.named_parameters()] == ["mask_fcn1.weight", "mask_fcn1.bias", "mask_fcn2.weight", "mask_fcn2.bias"]
    assert tuple(fe.mask_fcn1.weight.shape) == (8, 3, 3, 16) and tuple(fe.mask_fcn2.weight.shape) == (8, 3, 3, 8)      # OHWI in memory
    std = (2.0 / (9 * 8)) ** 0.5                                              # make_conv3x3: kaiming normal, fan_out, relu; bias 0
    assert 0.8 * std < float(fe.mask_fcn1.weight.detach().std()) < 1.2 * std and float(fe.mask_fcn1.bias.detach().abs().max()) == 0
    assert len(fe.pooler.poolers) == 4 and fe.pooler.geometry()[:3] == ((14, 14), MR.P.SCALES, 2)
    assert not m.roi_heads.box.keep_joint_head_features
    sd = reference_state_dict(m)
    assert sorted(sd) == sorted(shapes)
    for k, shape in shapes.items():
        assert list(sd[k].shape) == shape, k
    assert not any(k.startswith("roi_heads.mask.feature_extractor.head.") for k in sd)
    assert not any(k.startswith("roi_heads.mask.feature_extractor.fc") for k in sd)
    with torch.no_grad():
        for p in mask.parameters():
            p.uniform_(-1, 1)
    sd = reference_state_dict(m)
    torch.manual_seed(1)
    b = build_detection_model(_cfg())
    load_reference_state_dict(b, sd)
    after = reference_state_dict(b)
    for k in sd:
        assert torch.equal(after[k], sd[k]), k
    w = sd["roi_heads.mask.feature_extractor.mask_fcn1.weight"]
    assert tuple(w.shape) == (8, 16, 3, 3)                                    # the reference's OIHW at the boundary, both ways
    assert torch.equal(b.roi_heads.mask.feature_extractor.mask_fcn1.weight.detach(), w.permute(0, 2, 3, 1))


def test_set_conv_math_and_prep_entries_reach_the_extractor():
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    m = build_detection_model(_cfg())
    fe = m.roi_heads.mask.feature_extractor
    set_conv_math(m.roi_heads, ops.MATH_BF16X6)
    assert fe.math == ops.MATH_BF16X6 and m.roi_heads.mask.predictor.math == ops.MATH_BF16X6
    assert fe.prep_entries() == []           # CPU weights: nothing to prepare; on the device one entry per trainable conv (the GPU suite)


REFUSALS = [
    (["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "ResNet50Conv5ROIFeatureExtractor"],
     r"MODEL\.MASK_ON True.*R-50-FPN.*FEATURE_EXTRACTOR = 'ResNet50Conv5ROIFeatureExtractor'.*MaskRCNNFPNFeatureExtractor"),
    (["MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNConv1x1Predictor"], r"ROI_MASK_HEAD\.PREDICTOR = 'MaskRCNNConv1x1Predictor'"),
    (["MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", True], r"ROI_MASK_HEAD\.SHARE_BOX_FEATURE_EXTRACTOR = True"),
    (["MODEL.ROI_MASK_HEAD.USE_GN", True], r"ROI_MASK_HEAD\.USE_GN = True"),
    (["MODEL.ROI_MASK_HEAD.DILATION", 2], r"ROI_MASK_HEAD\.DILATION = 2"),
    (["MODEL.ROI_MASK_HEAD.CONV_LAYERS", (8, 6)], r"ROI_MASK_HEAD\.CONV_LAYERS = \(8, 6\)"),
    (["MODEL.ROI_MASK_HEAD.CONV_LAYERS", ()], r"ROI_MASK_HEAD\.CONV_LAYERS = \(\)"),
    (["MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.125, 0.0625)], r"ROI_MASK_HEAD\.POOLER_SCALES = \(0\.125, 0\.0625\)"),
    (["MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.25, 0.125, 0.0625, 0.03125, 0.015625)], r"ROI_MASK_HEAD\.POOLER_SCALES = \(0\.25, .*0\.015625\)"),
    (["MODEL.ROI_MASK_HEAD.POOLER_SCALES", ()], r"ROI_MASK_HEAD\.POOLER_SCALES = \(\)"),
    (["MODEL.KEYPOINT_ON", True], r"MODEL\.KEYPOINT_ON True.*R-50-FPN"),
]


@pytest.mark.parametrize("extra, message", REFUSALS)
def test_refusals_on_an_fpn_body_name_key_and_value(extra, message):
    with pytest.raises(NotImplementedError, match=message):
        build_detection_model(_cfg(extra))


def test_resolution_must_be_twice_the_pooler():
    with pytest.raises(ValueError, match=r"ROI_MASK_HEAD\.RESOLUTION = 14 .*set RESOLUTION to 28"):
        build_detection_model(_cfg(["MODEL.ROI_MASK_HEAD.RESOLUTION", 14]))
    m = build_detection_model(_cfg(["MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_MASK_HEAD.RESOLUTION", 14,
                                    "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.25, 0.125)]))
    assert m.roi_heads.mask.feature_extractor.n_levels == 2


def test_default_mask_settings_on_an_fpn_body_name_the_extractor_to_set():
    """MASK_ON with the C4 defaults (the C4 extractor, shared) on R-50-FPN: refused as before, now naming what to set"""
    ov, _ = _overrides()
    box_only = ov[:-len(MR.MASK_CFG)]
    with pytest.raises(NotImplementedError, match=r"^MODEL\.MASK_ON True on MODEL\.BACKBONE\.CONV_BODY 'R-50-FPN'.*'MaskRCNNFPNFeatureExtractor'"):
        build_detection_model(make_cfgs("15-5", overrides=box_only + ["MODEL.MASK_ON", True])[1])


def test_fpn_extractor_on_a_c4_body_is_refused():
    c4 = ["MODEL.DEVICE", "cpu", "MODEL.MASK_ON", True, "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32,
          "MODEL.RESNETS.WIDTH_PER_GROUP", 8]
    with pytest.raises(NotImplementedError, match=r"ROI_MASK_HEAD\.FEATURE_EXTRACTOR = 'MaskRCNNFPNFeatureExtractor'.*'R-50-C4'"):
        build_detection_model(make_cfgs("15-5", overrides=c4 + ["MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor"])[1])


# ------------------------------------------------------------------------------------------------ the float64 model
def test_fixture_conditions():
    fx = MR.fixture()
    MR.check_fixture(fx)
    g = np.load(MR.GOLD)
    assert os.path.getsize(MR.GOLD) <= os.path.getsize(os.path.join(HERE, "golden", "box_head_fpn.npz"))
    assert int(g["seed"]) == MR.GOLDEN_SEED and int(g["n_pos"]) == fx["n_pos"] and np.array_equal(g["pos_rows"], fx["pos_rows"])
    assert np.array_equal(g["labels_pos"], fx["labels"][fx["pos_rows"][: fx["n_pos"]]])
    from mask_ref import compact_ref
    rows, labs, _, n = compact_ref(fx["labels"], MR.P_MAX)
    assert np.array_equal(rows, fx["pos_rows"]) and n == fx["n_pos"] and np.array_equal(labs[:n], g["labels_pos"])


def test_float64_model_reproduces_the_reference_golden():
    fx, g = MR.fixture(), np.load(MR.GOLD)
    p = MR.params64(g)
    out = MR.model(fx, p)
    targets = MR.unpack_targets(g)
    assert targets.shape == (fx["n_pos"], MR.M, MR.M) and 0.05 < targets.mean() < 0.95
    _close(out["logits"].detach().numpy(), g["logits"], "logits")
    loss = MR.loss_of(out["logits"], g["labels_pos"], targets)
    assert abs(float(loss.detach()) - float(g["loss"])) <= TOL * abs(float(g["loss"]))
    loss.backward()
    for n in MR.PARAMS:
        _close(p[n][0].grad.numpy(), g["gw_" + n], "d %s.weight" % n)
        _close(p[n][1].grad.numpy(), g["gb_" + n], "d %s.bias" % n)
    _close(out["pooled"].grad.numpy(), g["g_pooled"], "d pooled")
    assert all(m.grad is not None and float(m.grad.abs().max()) > 0 for m in out["maps"][:3])       # the positives reach three levels
    assert float(out["maps"][3].grad.abs().max()) == 0
    # the post-processor: sigmoid of the label's channel
    idx = np.arange(fx["n_pos"])
    prob = 1.0 / (1.0 + np.exp(-out["logits"].detach().numpy()[idx, g["labels_pos"]]))
    _close(prob[:, None], g["prob"], "prob")
    for a in out["acts"]:
        assert 0.2 < float((a > 0).double().mean()) < 0.8       # both ReLU masks matter

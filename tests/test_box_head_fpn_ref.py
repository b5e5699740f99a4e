"""CPU: the float64 restatement of the FPN box head (tests/box_head_fpn_ref.py) against the reference's own FPN2MLPFeatureExtractor + FPNPredictor
(tests/golden/box_head_fpn.npz), and the FPN detector's construction, checkpoint keys, configuration keys and refusals.  No kernels involved.

Bounds: fpn_ref.conv_rule_ok with one CONV_TOL_* allowance per contraction between the pooled tensor and the compared one -- three for the
logits, two for x; a gradient counts the contractions of its backward path (predictor 1, fc7 2, fc6 and the pooled gradient 3)."""
import json
import os

import numpy as np
import pytest
import torch

import box_head_fpn_ref as HR
import fpn_ref as R
from abr_iod_amd.config import cfg as default_cfg
from abr_iod_amd.engine.synthetic import make_cfgs
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.modeling.roi_heads.box_head import fpn_box_head
from abr_iod_amd.utils.checkpoint import load_reference_state_dict, reference_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "box_head_fpn.npz")
POOLED = os.path.join(HERE, "golden", "pooler_fpn.npz")
SHAPES = os.path.join(HERE, "golden", "box_head_fpn_state_dict_shapes.json")
FWD_DEPTH = {"x": 2, "cls": 3, "bbox": 3}
GRAD_DEPTH = {"cls_score": 1, "bbox_pred": 1, "fc7": 2, "fc6": 3, "pooled": 3}


def _rule(got, want, tol, what):
    ok, err, lim = R.conv_rule_ok(np.asarray(got), np.asarray(want, np.float64), tol)
    assert ok, (what, err, lim)


# ------------------------------------------------------------------------------------------------ the restatement
def test_restatement_against_the_reference_golden():
    g, pooled = np.load(GOLD), np.load(POOLED)["out"]
    assert os.path.getsize(GOLD) < 512 * 1024 and int(g["seed"]) == HR.GOLDEN_SEED
    K, C = pooled.shape[:2]
    assert pooled.shape[2:] == (HR.RES, HR.RES) and g["w_fc6"].shape == (HR.DIM, C * HR.RES ** 2) and g["cls"].shape == (K, HR.NUM_CLASSES)
    p = HR.params64(g)
    fw = HR.forward(pooled, p)
    for key, name in (("x", "h7"), ("cls", "cls"), ("bbox", "bbox")):
        _rule(g[key], fw[name], FWD_DEPTH[key] * R.CONV_TOL_FWD, key)
    assert 0.2 < float((fw["h7"] > 0).mean()) < 0.8 and 0.2 < float((fw["h6"] > 0).mean()) < 0.8      # both ReLU masks matter
    g_cls, g_bbox = HR.cotangents(K)
    assert np.array_equal(g_cls, g["g_cls"]) and np.array_equal(g_bbox, g["g_bbox"])
    bw = HR.backward(fw, p, g_cls, g_bbox, pooled.shape)
    for name in HR.PARAMS:
        _rule(g["gw_" + name], bw["gw_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "d %s.weight" % name)
        _rule(g["gb_" + name], bw["gb_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "d %s.bias" % name)
    _rule(g["g_pooled"], bw["g_pooled"], GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "d pooled")


def test_restatement_backward_is_the_derivative():
    """directional finite difference of <cls, g_cls> + <bbox, g_bbox> in float64 (away from the ReLU kinks: a 1e-7 step)"""
    g, pooled = np.load(GOLD), np.load(POOLED)["out"].astype(np.float64)
    p = HR.params64(g)
    g_cls, g_bbox = HR.cotangents(pooled.shape[0])
    rng = np.random.default_rng(5)
    d_pooled = rng.standard_normal(pooled.shape)
    d_p = {n: (rng.standard_normal(w.shape), rng.standard_normal(b.shape)) for n, (w, b) in p.items()}

    def loss(t):
        q = {n: (w + t * d_p[n][0], b + t * d_p[n][1]) for n, (w, b) in p.items()}
        fw = HR.forward(pooled + t * d_pooled, q)
        return float((fw["cls"] * g_cls).sum() + (fw["bbox"] * g_bbox).sum())

    bw = HR.backward(HR.forward(pooled, p), p, g_cls, g_bbox, pooled.shape)
    want = float((bw["g_pooled"] * d_pooled).sum()) + sum(float((bw["gw_" + n] * d_p[n][0]).sum() + (bw["gb_" + n] * d_p[n][1]).sum()) for n in p)
    h = 1e-7
    got = (loss(h) - loss(-h)) / (2 * h)
    assert abs(got - want) <= 1e-5 * max(1.0, abs(want)), (got, want)


def test_fc6_layout_conversion_round_trips():
    w = np.random.default_rng(0).standard_normal((4, 8 * 49)).astype(np.float32)
    o = HR.fc6_to_ohwi(w, 8)
    assert o.shape == (4, 1, 1, 392) and np.array_equal(HR.fc6_from_ohwi(o, 8), w)
    # column (c, h, w) of the reference is column (h, w, c) of the stored weight
    assert o[2, 0, 0, (3 * 7 + 5) * 8 + 6] == w[2, 6 * 49 + 3 * 7 + 5]
    fc = fpn_box_head._FC(8, 7, 4)
    fc.load_oihw(torch.from_numpy(w))
    assert np.array_equal(fc.weight.detach().numpy(), o) and np.array_equal(fc.oihw().numpy(), w)
    assert tuple(fpn_box_head._FC(32, 1, 32).oihw().shape) == (32, 32)


# ------------------------------------------------------------------------------------------------ the detector on the CPU
def _overrides(extra=()):
    with open(SHAPES) as f:
        gold = json.load(f)
    ov = [tuple(v) if isinstance(v, list) else v for v in gold["overrides"]]
    return ov + list(extra), gold["shapes"]


def _cfg(extra=()):
    return make_cfgs("15-5", overrides=_overrides(extra)[0])[1]


def test_new_config_keys_have_the_reference_defaults():
    assert default_cfg.MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM == 1024 and default_cfg.MODEL.ROI_BOX_HEAD.USE_GN is False
    for key in ("FC_FREEZE", "CLS_FREEZE", "BBS_FREEZE", "CLS_OFFSET", "BBS_OFFSET"):
        assert default_cfg.MODEL.ROI_HEADS[key] is False, key


def test_fpn_detector_builds_with_the_reference_keys_and_round_trips():
    torch.manual_seed(0)
    m = build_detection_model(_cfg())
    box = m.roi_heads.box
    assert isinstance(box.feature_extractor, fpn_box_head.FPN2MLPFeatureExtractor) and isinstance(box.predictor, fpn_box_head.FPNPredictor)
    assert box.feature_extractor.out_channels == 32 and m.roi_heads.joint_supported
    assert [n for n, _ in box.feature_extractor.named_parameters()] == ["fc6.weight", "fc6.bias", "fc7.weight", "fc7.bias"]
    fc6 = box.feature_extractor.fc6
    assert tuple(fc6.weight.shape) == (32, 1, 1, 49 * 16)                        # the bytes of an OHWI [32,7,7,16] conv weight
    bound = (3.0 / (16 * 49)) ** 0.5                                             # kaiming_uniform_(a=1): sqrt(6 / (2 fan_in))
    assert 0.9 * bound < float(fc6.weight.detach().abs().max()) <= bound and float(fc6.bias.detach().abs().max()) == 0
    assert 0 < float(box.predictor.bbox_pred.weight.detach().std()) < 0.002 < float(box.predictor.cls_score.weight.detach().std()) < 0.02
    sd = reference_state_dict(m)
    _, shapes = _overrides()
    assert sorted(sd) == sorted(shapes)
    for k, shape in shapes.items():
        assert list(sd[k].shape) == shape, k
    with torch.no_grad():
        for p in box.parameters():
            p.uniform_(-1, 1)
    sd = reference_state_dict(m)
    torch.manual_seed(1)
    b = build_detection_model(_cfg())
    load_reference_state_dict(b, sd)
    after = reference_state_dict(b)
    for k in sd:
        assert torch.equal(after[k], sd[k]), k
    w = sd["roi_heads.box.feature_extractor.fc6.weight"].numpy()
    assert np.array_equal(b.roi_heads.box.feature_extractor.fc6.weight.detach().numpy(), HR.fc6_to_ohwi(w, 16))


def test_freeze_keys_freeze_the_reference_sets():
    names = {"FC_FREEZE": ("feature_extractor.fc6.", "feature_extractor.fc7."), "CLS_FREEZE": ("predictor.cls_score.",),
             "BBS_FREEZE": ("predictor.bbox_pred.",)}
    for key, prefixes in names.items():
        m = build_detection_model(_cfg(["MODEL.ROI_HEADS." + key, True]))
        frozen = {n for n, p in m.roi_heads.box.named_parameters() if not p.requires_grad}
        assert frozen == {n for n, _ in m.roi_heads.box.named_parameters() if n.startswith(prefixes)}, key


REFUSALS = [
    (["MODEL.ROI_BOX_HEAD.USE_GN", True], r"MODEL\.ROI_BOX_HEAD\.USE_GN True"),
    (["MODEL.ROI_HEADS.CLS_OFFSET", True], r"MODEL\.ROI_HEADS\.CLS_OFFSET True"),
    (["MODEL.ROI_HEADS.BBS_OFFSET", True], r"MODEL\.ROI_HEADS\.BBS_OFFSET True"),
    (["MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPNXconv1fcFeatureExtractor"], r"MODEL\.ROI_BOX_HEAD\.FEATURE_EXTRACTOR 'FPNXconv1fcFeatureExtractor'"),
    (["MODEL.MASK_ON", True], r"MODEL\.MASK_ON True.*R-50-FPN"),
    (["MODEL.KEYPOINT_ON", True], r"MODEL\.KEYPOINT_ON True.*R-50-FPN"),
    (["MODEL.ROI_BOX_HEAD.PREDICTOR", "FastRCNNPredictor"], r"MODEL\.ROI_BOX_HEAD\.PREDICTOR 'FastRCNNPredictor'"),
    (["MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "ResNet50Conv5ROIFeatureExtractor"], r"'ResNet50Conv5ROIFeatureExtractor' on MODEL\.BACKBONE\.CONV_BODY 'R-50-FPN'"),
]


@pytest.mark.parametrize("extra, message", REFUSALS)
def test_refusals_on_an_fpn_body_name_key_and_value(extra, message):
    with pytest.raises(NotImplementedError, match=message):
        build_detection_model(_cfg(extra))


def test_fpn_head_on_a_c4_body_is_refused():
    c4 = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8]
    with pytest.raises(NotImplementedError, match=r"FEATURE_EXTRACTOR 'FPN2MLPFeatureExtractor' on MODEL\.BACKBONE\.CONV_BODY 'R-50-C4'"):
        build_detection_model(make_cfgs("15-5", overrides=c4 + ["MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor"])[1])
    with pytest.raises(NotImplementedError, match=r"PREDICTOR 'FPNPredictor' with MODEL\.ROI_BOX_HEAD\.FEATURE_EXTRACTOR 'ResNet50Conv5ROIFeatureExtractor'"):
        build_detection_model(make_cfgs("15-5", overrides=c4 + ["MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor"])[1])


def test_incremental_train_step_refuses_an_fpn_body():
    from abr_iod_amd.engine.trainer import train_step
    with pytest.raises(NotImplementedError, match=r"MODEL\.BACKBONE\.CONV_BODY 'R-50-FPN'.*train_step"):
        train_step(None, None, None, None, None, None, _cfg())

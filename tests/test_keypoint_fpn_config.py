"""CPU: the FPN keypoint head's construction, checkpoint keys and refusals, and the float64 model of tests/keypoint_fpn_ref.py against the
reference's own KeypointRCNNFeatureExtractor (four pooler scales) + KeypointRCNNPredictor + loss (tests/golden/keypoint_head_fpn.npz).  No
kernels.

Bound of the float64 model against the float32 reference: 1e-4 relative to the largest magnitude of the compared tensor, the bound
tests/test_mask_head_fpn_config.py uses for the same purpose."""
import json
import os

import numpy as np
import pytest
import torch

import keypoint_fpn_ref as KR
import pooler_ref as P
from abr_iod_amd.engine.synthetic import make_cfgs
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import KeypointRCNNFeatureExtractor, KeypointRCNNPredictor
from abr_iod_amd.modeling.roi_heads.mask_head.fpn_mask_head import MaskRCNNFPNFeatureExtractor
from abr_iod_amd.modeling.roi_heads.pyramid_extractor import PyramidConvExtractor
from abr_iod_amd.utils.checkpoint import load_reference_state_dict, reference_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
MASK_SHAPES = os.path.join(HERE, "golden", "mask_head_fpn_state_dict_shapes.json")
TOL = 1e-4
KP = "MODEL.ROI_KEYPOINT_HEAD."


def _overrides(extra=()):
    with open(KR.SHAPES) as f:
        gold = json.load(f)
    ov = [tuple(v) if isinstance(v, list) else v for v in gold["overrides"]]
    return ov + list(extra), gold["shapes"]


def _cfg(extra=()):
    return make_cfgs("15-5", overrides=_overrides(extra)[0])[1]


def _mask_gold():
    with open(MASK_SHAPES) as f:
        gold = json.load(f)
    return [tuple(v) if isinstance(v, list) else v for v in gold["overrides"]], gold["shapes"]


def _close(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err, ref = float(np.abs(got - want).max()), float(np.abs(want).max())
    assert err <= TOL * max(ref, 1e-30), (what, err, ref)


# ------------------------------------------------------------------------------------------------ the detector on the CPU
def test_fpn_keypoint_detector_builds_with_the_reference_keys_and_round_trips():
    torch.manual_seed(0)
    ov, shapes = _overrides()
    mask_ov, _ = _mask_gold()
    assert ov[-len(KR.KEYPOINT_CFG):] == KR.KEYPOINT_CFG
    assert ov[:-len(KR.KEYPOINT_CFG)] == mask_ov[:len(ov) - len(KR.KEYPOINT_CFG)]      # the mask golden's widths, the keypoint keys for the mask keys
    m = build_detection_model(_cfg())
    assert list(m.roi_heads.keys()) == ["box", "keypoint"]
    head = m.roi_heads.keypoint
    fe = head.feature_extractor
    assert isinstance(fe, KeypointRCNNFeatureExtractor) and isinstance(fe, PyramidConvExtractor) and fe.pyramid
    assert isinstance(head.predictor, KeypointRCNNPredictor) and fe.in_channels == m.backbone.out_channels == 16
    assert fe.blocks == ["conv_fcn1", "conv_fcn2"] and fe.out_channels == 8 and fe.n_levels == 4
    assert [n for n, _ in fe.named_parameters()] == ["conv_fcn1.weight", "conv_fcn1.bias", "conv_fcn2.weight", "conv_fcn2.bias"]
    assert tuple(fe.conv_fcn1.weight.shape) == (8, 3, 3, 16) and tuple(fe.conv_fcn2.weight.shape) == (8, 3, 3, 8)      # OHWI in memory
    r = KR.DET_RES
    assert len(fe.pooler.poolers) == 4 and fe.pooler.geometry()[:3] == ((r, r), P.SCALES, 2)
    assert head.loss_evaluator.discretization_size == 4 * r
    sd = reference_state_dict(m)
    assert sorted(sd) == sorted(shapes)
    for k, shape in shapes.items():
        assert list(sd[k].shape) == shape, k
    kp = [k for k in sd if k.startswith("roi_heads.keypoint.")]
    assert len(kp) == 6 and tuple(sd["roi_heads.keypoint.predictor.kps_score_lowres.weight"].shape) == (8, 17, 4, 4)
    with torch.no_grad():
        for p in head.parameters():
            p.uniform_(-1, 1)
        dc = head.predictor.kps_score_lowres
        dc.load_oihw(dc.oihw().clone())      # (keeps the padding planes of the deconvolution's GEMM weight zero)
        dc.bias[dc.num_keypoints:] = 0
    sd = reference_state_dict(m)
    torch.manual_seed(1)
    b = build_detection_model(_cfg())
    load_reference_state_dict(b, sd)
    after = reference_state_dict(b)
    assert sorted(after) == sorted(sd)
    for k in sd:
        assert torch.equal(after[k], sd[k]), k
    w = sd["roi_heads.keypoint.feature_extractor.conv_fcn1.weight"]
    assert tuple(w.shape) == (8, 16, 3, 3)                                    # the reference's OIHW at the boundary, both ways
    assert torch.equal(b.roi_heads.keypoint.feature_extractor.conv_fcn1.weight.detach(), w.permute(0, 2, 3, 1))
    dc = b.roi_heads.keypoint.predictor.kps_score_lowres
    assert dc.kp == 20 and torch.all(dc.weight.detach().view(4, 4, 20, 8)[:, :, 17:] == 0) and torch.all(dc.bias.detach()[17:] == 0)


def test_upstream_sizes_give_the_reference_shapes():
    """e2e_keypoint_rcnn_R_50_FPN_1x's head: 256 channels in, eight 512-wide convs, pooler 14 -> 56 x 56 heat maps (3136 <= the decode's 4096)"""
    from abr_iod_amd.config import cfg as base
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    c = base.clone()
    c.merge_from_list(["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.KEYPOINT_ON", True, KP + "SHARE_BOX_FEATURE_EXTRACTOR", False,
                       KP + "POOLER_SCALES", P.SCALES, KP + "POOLER_SAMPLING_RATIO", 2, KP + "RESOLUTION", 56])
    assert c.MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION == 14 and tuple(c.MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS) == (512,) * 8
    head = build_roi_keypoint_head(c, 256)
    sd = reference_state_dict(head)
    assert tuple(sd["feature_extractor.conv_fcn1.weight"].shape) == (512, 256, 3, 3)
    assert tuple(sd["feature_extractor.conv_fcn8.weight"].shape) == (512, 512, 3, 3)
    assert tuple(sd["predictor.kps_score_lowres.weight"].shape) == (512, 17, 4, 4) and len(sd) == 18


def test_two_scales_build_a_two_level_pooler():
    m = build_detection_model(_cfg([KP + "POOLER_SCALES", (0.25, 0.125)]))
    fe = m.roi_heads.keypoint.feature_extractor
    assert fe.n_levels == 2 and len(fe.pooler.poolers) == 2 and fe.pooler.geometry()[1] == (0.25, 0.125)


def test_set_conv_math_and_prep_entries_reach_the_extractor():
    from abr_iod_amd import ops
    from abr_iod_amd.modeling._flat import flatten_parameters
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    m = build_detection_model(_cfg())
    head = m.roi_heads.keypoint
    fe = head.feature_extractor
    set_conv_math(m.roi_heads, ops.MATH_BF16X6)
    assert fe.math == ops.MATH_BF16X6 and head.predictor.math == ops.MATH_BF16X6
    assert fe.prep_entries() == []           # CPU weights: nothing to prepare; on the device one entry per trainable conv (the GPU suite)
    flat = flatten_parameters(m)
    lo, hi = flat.params.data_ptr(), flat.params.data_ptr() + flat.params.numel() * 4
    for n, p in head.named_parameters():
        assert lo <= p.data_ptr() < hi and p.grad is not None, n + " lies outside the flat buffers"


def test_the_c4_form_is_unchanged():
    from abr_iod_amd.config import cfg as base
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    c = base.clone()
    c.merge_from_list(["MODEL.KEYPOINT_ON", True, KP + "SHARE_BOX_FEATURE_EXTRACTOR", False, KP + "RESOLUTION", 56])
    fe = build_roi_keypoint_head(c, 1024).feature_extractor
    assert not fe.pyramid and fe.spatial_scale == 0.0625 and fe.sampling_ratio == 0 and not hasattr(fe, "pooler")
    assert fe.blocks == ["conv_fcn%d" % i for i in range(1, 9)]
    with pytest.raises(RuntimeError, match="rows"):
        fe([torch.zeros(1, 1024, 4, 4)], torch.zeros(1, 5), rows=torch.zeros(1, dtype=torch.int64))


# ------------------------------------------------------------------------------------------------ refusals
def _box_only():
    ov, _ = _overrides()
    return ov[:-len(KR.KEYPOINT_CFG)]


def test_keypoint_defaults_on_an_fpn_body_name_what_to_set():
    """KEYPOINT_ON with the defaults (the shared extractor, the single scale 1/16) on R-50-FPN: refused as before, now naming what to set"""
    with pytest.raises(NotImplementedError, match=r"^MODEL\.KEYPOINT_ON True on MODEL\.BACKBONE\.CONV_BODY 'R-50-FPN'.*SHARE_BOX_FEATURE_EXTRACTOR = True"
                                                  r".*SHARE_BOX_FEATURE_EXTRACTOR to False.*\(0\.25, 0\.125, 0\.0625, 0\.03125\)"):
        build_detection_model(make_cfgs("15-5", overrides=_box_only() + ["MODEL.KEYPOINT_ON", True])[1])
    # unshared, still the C4 scale
    with pytest.raises(NotImplementedError, match=r"^MODEL\.KEYPOINT_ON True on MODEL\.BACKBONE\.CONV_BODY 'R-50-FPN'.*POOLER_SCALES = \(0\.0625,\)"
                                                  r".*\(0\.25, 0\.125, 0\.0625, 0\.03125\)"):
        build_detection_model(make_cfgs("15-5", overrides=_box_only() + ["MODEL.KEYPOINT_ON", True, KP + "SHARE_BOX_FEATURE_EXTRACTOR", False,
                                                                        KP + "RESOLUTION", 56])[1])


REFUSALS = [
    ([KP + "POOLER_SCALES", (0.25, 0.125, 0.0625, 0.03125, 0.015625)], r"ROI_KEYPOINT_HEAD\.POOLER_SCALES = \(0\.25, .*0\.015625\)"),
    ([KP + "POOLER_SCALES", ()], r"ROI_KEYPOINT_HEAD\.POOLER_SCALES = \(\)"),
    ([KP + "POOLER_SCALES", (0.125, 0.0625)], r"ROI_KEYPOINT_HEAD\.POOLER_SCALES = \(0\.125, 0\.0625\)"),
    ([KP + "POOLER_SCALES", (0.0625,)], r"ROI_KEYPOINT_HEAD\.POOLER_SCALES = \(0\.0625,\)"),
    ([KP + "SHARE_BOX_FEATURE_EXTRACTOR", True], r"ROI_KEYPOINT_HEAD\.SHARE_BOX_FEATURE_EXTRACTOR = True"),
    ([KP + "CONV_LAYERS", (8, 6)], r"ROI_KEYPOINT_HEAD\.CONV_LAYERS = \(8, 6\)"),
    ([KP + "CONV_LAYERS", ()], r"ROI_KEYPOINT_HEAD\.CONV_LAYERS = \(\)"),
    ([KP + "POOLER_RESOLUTION", 17, KP + "RESOLUTION", 68], r"ROI_KEYPOINT_HEAD\.POOLER_RESOLUTION = 17"),
    ([KP + "FEATURE_EXTRACTOR", "KeypointRCNNFPNFeatureExtractor"], r"ROI_KEYPOINT_HEAD\.FEATURE_EXTRACTOR = 'KeypointRCNNFPNFeatureExtractor'"),
    ([KP + "PREDICTOR", "Other"], r"ROI_KEYPOINT_HEAD\.PREDICTOR = 'Other'"),
]


@pytest.mark.parametrize("extra, message", REFUSALS)
def test_refusals_on_an_fpn_body_name_key_and_value(extra, message):
    with pytest.raises(NotImplementedError, match=message):
        build_detection_model(_cfg(extra))


def test_resolution_must_be_four_times_the_pooler():
    with pytest.raises(ValueError, match=r"ROI_KEYPOINT_HEAD\.RESOLUTION = 28 .*set RESOLUTION to 56"):
        build_detection_model(_cfg([KP + "RESOLUTION", 28]))
    with pytest.raises(ValueError, match=r"set RESOLUTION to 28"):
        build_detection_model(_cfg([KP + "POOLER_RESOLUTION", 7]))
    m = build_detection_model(_cfg([KP + "POOLER_RESOLUTION", 16, KP + "RESOLUTION", 64]))       # 64 x 64 = 4096: the decode's largest map
    assert m.roi_heads.keypoint.feature_extractor.resolution == 16


def test_multi_scale_keypoint_scales_on_a_c4_body_are_refused():
    c4 = ["MODEL.DEVICE", "cpu", "MODEL.KEYPOINT_ON", True, KP + "SHARE_BOX_FEATURE_EXTRACTOR", False, KP + "RESOLUTION", 56,
          "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8]
    with pytest.raises(NotImplementedError, match=r"ROI_KEYPOINT_HEAD\.POOLER_SCALES = \(0\.25, 0\.125, 0\.0625, 0\.03125\).*C4"):
        build_detection_model(make_cfgs("15-5", overrides=c4 + [KP + "POOLER_SCALES", P.SCALES])[1])
    m = build_detection_model(make_cfgs("15-5", overrides=c4)[1])
    assert not m.roi_heads.keypoint.feature_extractor.pyramid


# ------------------------------------------------------------------------------------------------ mask and keypoint together
def test_mask_and_keypoint_heads_together():
    mask_ov, mask_shapes = _mask_gold()
    m = build_detection_model(make_cfgs("15-5", overrides=mask_ov + KR.KEYPOINT_CFG)[1])
    assert list(m.roi_heads.keys()) == ["box", "mask", "keypoint"]
    mfe, kfe = m.roi_heads.mask.feature_extractor, m.roi_heads.keypoint.feature_extractor
    assert isinstance(mfe, MaskRCNNFPNFeatureExtractor) and isinstance(kfe, KeypointRCNNFeatureExtractor)
    assert mfe is not kfe and mfe.pooler is not kfe.pooler and mfe is not m.roi_heads.box.feature_extractor
    assert mfe.blocks == ["mask_fcn1", "mask_fcn2"] and kfe.blocks == ["conv_fcn1", "conv_fcn2"]
    assert not {id(p) for p in mfe.parameters()} & {id(p) for p in kfe.parameters()}
    sd = reference_state_dict(m)
    _, kp_shapes = _overrides()
    for k, shape in mask_shapes.items():       # the mask detector's keys, unchanged
        assert list(sd[k].shape) == shape, k
    extra = sorted(set(sd) - set(mask_shapes))
    assert extra == sorted(k for k in kp_shapes if k.startswith("roi_heads.keypoint."))
    assert all(list(sd[k].shape) == kp_shapes[k] for k in extra)


# ------------------------------------------------------------------------------------------------ the float64 model
def test_scene_conditions_and_the_recorded_selection():
    g = np.load(KR.GOLD)
    assert os.path.getsize(KR.GOLD) <= os.path.getsize(os.path.join(HERE, "golden", "mask_head_fpn.npz"))
    assert int(g["seed"]) == KR.GOLDEN_SEED
    for K in KR.KS:
        sc = KR.scene(K)
        KR.check_scene(sc)
        sel = sc["sel"]
        n = sel["n_pos"]
        rows = sel["pos_rows"][:n]
        assert np.array_equal(g["kept_rows"], rows), "the reference's subsample kept other rows"
        assert np.array_equal(g["levels"], sc["lv"][rows]), "the reference's LevelMapper disagrees"
        v = sel["valid"][:n] > 0
        assert np.array_equal(g["valid%d" % K] > 0, v) and np.array_equal(g["heat%d" % K][v], sel["targets"][:n][v])


@pytest.mark.parametrize("K", KR.KS)
def test_float64_model_reproduces_the_reference_golden(K):
    sc, g = KR.scene(K), np.load(KR.GOLD)
    p = KR.params64(g, K)
    out = KR.model(sc, p)
    _close(out["pooled"].detach().numpy(), g["pooled"], "pooled")
    _close(out["acts"][-1].detach().numpy(), g["features"], "conv stack")
    ref = g["logits%d" % K]
    _close(out["logits"].detach().numpy()[: len(ref)], ref, "logits")
    loss, want = out["loss"], float(g["loss%d" % K])
    assert abs(float(loss.detach()) - want) <= TOL * abs(want)
    loss.backward()
    for n in KR.BLOCKS + ("kps_score_lowres",):
        key = n if n in KR.BLOCKS else n
        gw, gb = g["gw%d_%s" % (K, key)], g["gb%d_%s" % (K, key)]
        _close(p[n][0].grad.numpy(), gw, "d %s.weight" % n)
        if n == "kps_score_lowres":      # softmax - onehot sums to zero over a plane: this gradient is zero up to rounding, on both sides
            assert float(np.abs(gb).max()) <= 1e-6 and float(p[n][1].grad.abs().max()) <= 1e-12
        else:
            _close(p[n][1].grad.numpy(), gb, "d %s.bias" % n)
    assert all(m.grad is not None and float(m.grad.abs().max()) > 0 for m in out["maps"])       # the live positives reach all four levels
    for a in out["acts"]:
        assert 0.2 < float((a > 0).double().mean()) < 0.8       # both ReLU masks matter

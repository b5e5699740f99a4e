"""CPU: the RetinaNet restatement (tests/retinanet_ref.py) against the golden the reference's own code wrote (tests/golden/retinanet.npz), the
assumptions the golden's exact comparisons stand on, the configuration node, the anchors of the config path, the build and refusal matrix and
the state-dict names of the RetinaNet bodies and head."""
import json
import os

import numpy as np
import pytest
import torch

import retinanet_ref as R
import rpn_fpn_ref as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.RES2_OUT_CHANNELS", 16, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16, "MODEL.RESNETS.STEM_OUT_CHANNELS", 8,
        "MODEL.RESNETS.WIDTH_PER_GROUP", 4]
RETINA = ["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", "R-50-FPN-RETINANET", "MODEL.RETINANET.NUM_CLASSES", R.C + 1,
          "MODEL.RETINANET.NUM_CONVS", 2, "MODEL.RETINANET.ANCHOR_SIZES", R.SIZES]


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLDEN, "retinanet.npz"))


@pytest.fixture(scope="module")
def golden_run(g):
    L = len(R.MAPS)
    cls, reg = R.golden_arrays([g["cls_%d" % l] for l in range(L)], [g["reg_%d" % l] for l in range(L)])
    anchors = [g["anchors_%d" % l] for l in range(L)]
    return cls, reg, anchors


def _cfg(extra=()):
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(TINY + list(extra))
    return c


def test_restatement_reproduces_the_golden(g, golden_run):
    cls, reg, anchors = golden_run
    for cap in R.CAPS:
        res = R.detect_ref(cls, reg, anchors, R.A, R.C, R.IMAGE_SIZES, R.TH, R.PRE, R.NMS_TH, cap)
        for i, d in enumerate(res):
            want_b, want_s, want_l = R.canonical(g["boxes_%d_%d" % (cap, i)], g["scores_%d_%d" % (cap, i)], g["labels_%d_%d" % (cap, i)])
            assert len(np.unique(want_s)) == len(want_s)        # (what makes the canonical order well defined)
            assert np.array_equal(d["labels"], want_l), (cap, i)                       # class by class: labels, order and count
            assert np.array_equal(d["scores"].view(np.uint32), want_s.view(np.uint32)), (cap, i)   # the same members, in the same order, to the bit
            np.testing.assert_allclose(d["boxes"], want_b, rtol=1e-5, atol=2e-4)


def test_oracle_anchors_equal_the_golden(g):
    for l, a in enumerate(R.pyramid_anchors()):
        assert np.array_equal(a.view(np.uint32), g["anchors_%d" % l].view(np.uint32)), l


def test_golden_conditions_and_score_spacing(golden_run):
    """what the exact comparisons stand on: the seed loop's conditions hold for the stored inputs; every candidate's score differs from the next
    by more than twice the score tolerance of the GPU tests (rtol 3e-7), so no ranking or cut hangs on how a sigmoid was rounded"""
    cls, reg, anchors = golden_run
    bad, res = R.golden_conditions(cls, reg, anchors)
    assert not bad, bad
    for i in range(len(R.IMAGE_SIZES)):
        sc = np.sort(np.concatenate([s["scores"] for s in res[1000][i]["segments"]]).astype(np.float64))
        assert len(sc) > 30 and np.all(np.diff(sc) > 6e-7 * sc[1:]), i
    allsc = np.concatenate([F.torch_sigmoid(np.ascontiguousarray(c).reshape(1, -1))[0] for c in cls]).astype(np.float64)
    passing = np.sort(allsc[allsc > R.TH])
    assert np.all(np.diff(passing) > 6e-7 * passing[1:])          # across the whole batch: no two candidates share a logit
    assert np.abs(allsc - R.TH).min() > 1e-6


def test_config_defaults_equal_the_reference():
    from abr_iod_amd.config import cfg
    want = json.load(open(os.path.join(GOLDEN, "retinanet_defaults.json")))
    det = want.pop("TEST.DETECTIONS_PER_IMG")
    got = {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in cfg.MODEL.RETINANET.items()}
    assert got == want
    for k, v in want.items():
        assert type(got[k]) is type(v), k
    assert cfg.TEST.DETECTIONS_PER_IMG == det and cfg.MODEL.RETINANET_ON is False


def test_config_path_cell_anchors_equal_the_golden(g):
    from abr_iod_amd.modeling.rpn.retinanet import make_anchor_generator_retinanet, retinanet_anchor_sizes
    c = _cfg(RETINA)
    assert retinanet_anchor_sizes(c) == R.level_sizes()
    ag = make_anchor_generator_retinanet(c)
    assert ag.num_anchors_per_location() == [R.A] * len(R.MAPS) and tuple(ag.strides) == R.STRIDES
    for l in range(len(R.MAPS)):
        assert np.array_equal(ag.level_cell_anchors(l).numpy().view(np.uint32), g["cell_%d" % l].view(np.uint32)), l
    # the default sizes too: fractional sizes go through generate_anchors as the reference's numpy code takes them
    from abr_iod_amd.config import cfg
    from oracle import ops as O
    ag = make_anchor_generator_retinanet(cfg)
    for l, (st, s) in enumerate(zip(cfg.MODEL.RETINANET.ANCHOR_STRIDES, retinanet_anchor_sizes(cfg))):
        assert np.array_equal(ag.level_cell_anchors(l).numpy().view(np.uint32), O.cell_anchors(st, s, cfg.MODEL.RETINANET.ASPECT_RATIOS).view(np.uint32)), l


def test_build_and_refusal_matrix():
    from abr_iod_amd.modeling.backbone import fpn as fpn_module
    from abr_iod_amd.modeling.backbone import resnet
    from abr_iod_amd.modeling.backbone.backbone import build_backbone
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetModule
    from abr_iod_amd.modeling.rpn.rpn import build_rpn
    assert resnet.FPN_BODIES == ("R-50-FPN", "R-101-FPN", "R-152-FPN") and set(resnet.RETINANET_BODIES) == {"R-50-FPN-RETINANET", "R-101-FPN-RETINANET"}
    for body, blocks in (("R-50-FPN-RETINANET", [3, 4, 6, 3]), ("R-101-FPN-RETINANET", [3, 4, 23, 3])):
        c = _cfg(RETINA + ["MODEL.BACKBONE.CONV_BODY", body])
        assert [s.block_count for s in resnet.stage_specs(body, True)] == blocks
        # without RETINANET_ON the bodies stay refused, with the text the C4 list and the key are matched by
        off = _cfg(["MODEL.BACKBONE.CONV_BODY", body])
        for build in (build_detection_model, build_backbone, resnet.ResNet):
            with pytest.raises(NotImplementedError, match=r"R-101-C4, R-50-C4.*MODEL\.RETINANET_ON"):
                build(off)
        with pytest.raises(NotImplementedError, match="CONV_BODY"):
            build_backbone(off)
        if body.startswith("R-50"):
            for use_c5 in (True, False):
                b = build_backbone(_cfg(RETINA + ["MODEL.RETINANET.USE_C5", use_c5]))
                top = b.fpn.top_blocks
                assert isinstance(top, fpn_module.LastLevelP6P7) and top.use_P5 == (not use_c5)
                assert top.p6.in_channels == (128 if use_c5 else 16) and b.fpn.inner_blocks == ["fpn_inner2", "fpn_inner3", "fpn_inner4"]
                ids = [id(p) for p in b.fpn._param_list()]
                assert id(top.p6.weight) in ids and id(top.p7.bias) in ids and len(ids) == 16
            assert build_roi_heads(c, 16) == [] and isinstance(build_rpn(c, 16), RetinaNetModule)
    # RETINANET_ON on any other body: both keys named
    for body in ("R-50-C4", "R-50-FPN", "R-50-C5"):
        on = _cfg(["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", body, "MODEL.RPN.USE_FPN", True])
        for build in (build_detection_model, build_backbone, lambda cc: build_roi_heads(cc, 16)):
            with pytest.raises(NotImplementedError, match=r"MODEL\.RETINANET_ON.*MODEL\.BACKBONE\.CONV_BODY"):
                build(on)
    # freezes and the refused conv blocks behave as on the FPN bodies
    for key in ("MODEL.FPN.USE_GN", "MODEL.FPN.USE_RELU"):
        with pytest.raises(NotImplementedError, match=key.replace(".", r"\.")):
            build_backbone(_cfg(RETINA + [key, True]))
    b = build_backbone(_cfg(RETINA + ["MODEL.BACKBONE.FPN_FREEZE", True]))
    assert not any(p.requires_grad for n, p in b.named_parameters() if "fpn" in n) and any(p.requires_grad for p in b.parameters())
    assert not any(p.requires_grad for p in build_backbone(_cfg(RETINA + ["MODEL.BACKBONE.ALL_FREEZE", True])).parameters())
    # any other top block keeps its refusal
    with pytest.raises(NotImplementedError, match="top_blocks"):
        fpn_module.FPN([16, 32], 16, top_blocks=torch.nn.Identity())


def test_detector_entry_points_refuse_what_retinanet_lacks():
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    m = build_detection_model(_cfg(RETINA))
    assert m.roi_heads == [] and m.retinanet
    x = [torch.zeros(3, 64, 64)]
    m.train()
    for call in (lambda: m(x), lambda: m(x, targets=[None]), lambda: m.forward_begin(x, [None])):
        with pytest.raises(NotImplementedError, match="the RetinaNet loss is not built"):
            call()
    with pytest.raises(NotImplementedError, match="the RetinaNet loss is not built"):
        m.rpn(None, [torch.zeros(1, 16, 8, 8)] * 5)
    m.eval()
    for call in (lambda: m.generate_soften_proposal(x), lambda: m.generate_feature_logits_by_targets(x), lambda: m.forward_joint(x, [None], None),
                 lambda: m(x, features=[1], proposals=[1])):
        with pytest.raises(NotImplementedError, match="RetinaNet"):
            call()


def test_state_dict_names_and_checkpoint_round_trip(g, tmp_path):
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.utils.checkpoint import Checkpointer, reference_state_dict
    m = build_detection_model(_cfg(RETINA + ["MODEL.RESNETS.RES2_OUT_CHANNELS", 8]))     # C5 has 64 channels, the pyramid 16: the golden's shapes
    sd = reference_state_dict(m)
    names, shapes = [str(n) for n in g["sd_names"]], g["sd_shapes"]
    for n, s in zip(names, shapes):
        key = ("backbone." if n.startswith("fpn.") else "rpn.") + n
        assert key in sd, key
        assert tuple(sd[key].shape) == tuple(int(v) for v in s if v), key
    ours = sorted(k for k in sd if k.startswith("backbone.fpn.top_blocks.") or k.startswith("rpn.head."))
    assert ours == sorted(("backbone." if n.startswith("fpn.") else "rpn.") + n for n in names)
    prior = m.rpn.head.cls_logits.bias.detach()
    assert torch.allclose(prior[: R.A * R.C], torch.full((R.A * R.C,), -float(np.log(99.0)))) and not m.rpn.head.bbox_pred.bias.any()
    Checkpointer(m, save_dir=str(tmp_path), save_to_disk=True).save("retina")
    m2 = build_detection_model(_cfg(RETINA + ["MODEL.RESNETS.RES2_OUT_CHANNELS", 8]))
    Checkpointer(m2, save_dir=str(tmp_path)).load()
    sd2 = reference_state_dict(m2)
    assert set(sd) == set(sd2) and all(torch.equal(sd[k], sd2[k]) for k in sd)
    assert torch.equal(m.rpn.head.cls_logits.weight, m2.rpn.head.cls_logits.weight)        # the padded storage too

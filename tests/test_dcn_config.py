"""CPU: MODEL.RESNETS.STAGE_WITH_DCN / WITH_MODULATED_DCN / DEFORMABLE_GROUPS build the reference's deformable body
(modeling/backbone/resnet.py:105-125, :289-312; layers/misc.py:114-190): which blocks get a DFConv2d, the state-dict keys and shapes of
the reference's own model (tests/golden/dcn_state_dict_shapes.json, written by tests/golden/make_golden_dcn.py), the checkpoint round
trip, the refused v2 + groups quirk and the optimiser groups of the offset bias.  No kernels involved."""
import json
import os

import pytest
import torch

from abr_iod_amd.config import cfg as default_cfg
from abr_iod_amd.engine.synthetic import make_cfgs
from abr_iod_amd.modeling.backbone.resnet import DFConv2d
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.solver.build import make_optimizer
from abr_iod_amd.utils.checkpoint import Checkpointer, reference_state_dict

TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32,
        "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 128]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dcn_state_dict_shapes.json")


def _gold():
    with open(GOLD) as f:
        return json.load(f)


def _target(extra=()):
    """the 21-class target detector of the 15-5 task (the model the golden was taken from)"""
    return make_cfgs("15-5", overrides=TINY + [str(v) if isinstance(v, tuple) else v for v in extra])[1]


def test_config_has_reference_defaults():
    r = default_cfg.MODEL.RESNETS
    assert tuple(r.STAGE_WITH_DCN) == (False, False, False, False)
    assert r.WITH_MODULATED_DCN is False and r.DEFORMABLE_GROUPS == 1


def test_yaml_selects_stages(tmp_path):
    y = tmp_path / "dcn.yaml"
    y.write_text("MODEL:\n  RESNETS:\n    STAGE_WITH_DCN: [False, True, True, True]\n    WITH_MODULATED_DCN: True\n")
    cfg = _target()
    cfg.merge_from_file(str(y))
    assert tuple(cfg.MODEL.RESNETS.STAGE_WITH_DCN) == (False, True, True, True)
    model = build_detection_model(cfg)
    body = model.backbone.body
    for name, want in (("layer1", False), ("layer2", True), ("layer3", True)):
        for blk in getattr(body, name):
            assert isinstance(blk.conv2, DFConv2d) == want, name
            if want:
                C = blk.conv1.out_channels
                assert blk.conv2.modulated and tuple(blk.conv2.offset.oihw().shape) == (27, C, 3, 3)
                assert tuple(blk.conv2.conv.oihw().shape) == (C, C, 3, 3)
                assert torch.count_nonzero(blk.conv2.offset.bias) == 0
    # STAGE_WITH_DCN[3] has no effect on the C4 layer4 head (roi_box_feature_extractors.py:27-36)
    assert not any(isinstance(m, DFConv2d) for m in model.roi_heads.modules())
    names = [n for n, _ in model.named_parameters() if ".offset." in n]
    assert len(names) == 2 * (4 + 6) and all(n.startswith(("backbone.body.layer2.", "backbone.body.layer3.")) for n in names)


@pytest.mark.parametrize("case", ["default", "v1_FTTF", "v2_TTTT", "v1_dg2_FTFF"])
def test_state_dict_matches_reference(case):
    g = _gold()[case]
    extra = [tuple(v) if isinstance(v, list) else v for v in g["overrides"]]
    model = build_detection_model(_target(extra))
    sd = reference_state_dict(model)
    want = g["shapes"]
    assert set(sd) == set(want)
    for k, v in sd.items():
        assert list(v.shape) == want[k], k


def test_default_parameter_list_unchanged():
    """the default cfg builds exactly the reference's plain body: the same parameter names (and count) as its state_dict"""
    model = build_detection_model(_target())
    want = _gold()["default"]["shapes"]
    names = [n for n, _ in model.named_parameters()]
    assert not any(".offset." in n or ".conv2.conv." in n for n in names)
    assert set(names) <= set(want)
    assert len(names) == sum(1 for k in want if not k.endswith(("running_mean", "running_var", "cell_anchors.0")) and
                             not (".bn" in k or "downsample.1" in k))


def test_checkpoint_round_trip(tmp_path):
    extra = ["MODEL.RESNETS.STAGE_WITH_DCN", (True, True, False, False), "MODEL.RESNETS.DEFORMABLE_GROUPS", 2]
    torch.manual_seed(0)
    a = build_detection_model(_target(extra))
    with torch.no_grad():   # non-zero offset biases, so that a mix-up between real and padding entries shows
        for m in a.modules():
            if isinstance(m, DFConv2d):
                m.offset.bias[: m.offset.out_channels].uniform_(-1, 1)
    d = str(tmp_path)
    Checkpointer(a, save_dir=d, save_to_disk=True).save("dcn")
    data = torch.load(os.path.join(d, "dcn.pth"), weights_only=False)
    k = "backbone.body.layer1.0.conv2.offset.weight"
    assert tuple(data["model"][k].shape) == (36, 8, 3, 3)
    assert tuple(data["model"]["backbone.body.layer1.0.conv2.offset.bias"].shape) == (36,)
    assert tuple(data["model"]["backbone.body.layer2.3.conv2.conv.weight"].shape) == (16, 16, 3, 3)
    torch.manual_seed(1)
    b = build_detection_model(_target(extra))
    Checkpointer(b).load(os.path.join(d, "dcn.pth"))
    sa, sb = reference_state_dict(a), reference_state_dict(b)
    assert set(sa) == set(sb)
    for key in sa:
        assert torch.equal(sa[key], sb[key]), key
    # the storage behind the state dict: padding rows stay zero, the contraction weight is the OHWI tensor read as [Cout][9 Cin]
    blk = b.backbone.body.layer1[0]
    assert torch.count_nonzero(blk.conv2.offset.weight[36:]) == 0 and torch.count_nonzero(blk.conv2.offset.bias[36:]) == 0
    w = sa["backbone.body.layer1.0.conv2.conv.weight"]
    assert torch.equal(blk.conv2.conv.weight.detach().view(8, 3, 3, 8), w.permute(0, 2, 3, 1))


def test_modulated_with_groups_is_refused():
    cfg = _target(["MODEL.RESNETS.STAGE_WITH_DCN", (False, True, False, False), "MODEL.RESNETS.WITH_MODULATED_DCN", True,
                   "MODEL.RESNETS.DEFORMABLE_GROUPS", 2])
    with pytest.raises(NotImplementedError, match="18 offset and 9 mask"):
        build_detection_model(cfg)


def test_offset_bias_optimiser_group():
    cfg = _target(["MODEL.RESNETS.STAGE_WITH_DCN", (False, True, True, False)])
    model = build_detection_model(cfg)
    opt = make_optimizer(cfg, model)
    groups = {g["name"]: g for g in opt.param_groups}
    base, wd = cfg.SOLVER.BASE_LR, cfg.SOLVER.WEIGHT_DECAY
    seen = 0
    for name, g in groups.items():
        if ".offset." not in name:
            continue
        seen += 1
        if name.endswith("bias"):
            assert g["lr"] == pytest.approx(base * cfg.SOLVER.BIAS_LR_FACTOR) and g["weight_decay"] == cfg.SOLVER.WEIGHT_DECAY_BIAS, name
        else:
            assert g["lr"] == pytest.approx(base) and g["weight_decay"] == wd, name
    assert seen == 2 * (4 + 6)
    # the reference-format optimiser state speaks of the reference's shapes
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == len(names)

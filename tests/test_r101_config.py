"""CPU: MODEL.BACKBONE.CONV_BODY "R-101-C4" builds the reference's ResNet-101 C4 body (ResNet101StagesTo4: layer3 has 23 blocks,
modeling/backbone/resnet.py:60-64, :443-453).  Checked against the keys, shapes, dtypes and requires_grad of the reference's own model
(tests/golden/r101_state_dict_shapes.json, written by tests/golden/make_golden_r101.py), the optimiser's per-tensor groups and gradient
buckets at the new depth, the Caffe2 blob names of res4_0..res4_22, the checkpoint files, and the refusal of every other body.
No kernels involved."""
import json
import os
import pickle

import numpy as np
import pytest
import torch

from abr_iod_amd import ops
from abr_iod_amd.engine.synthetic import build_models, make_cfgs
from abr_iod_amd.engine.trainer import frozen_prefix_shareable
from abr_iod_amd.modeling.backbone import resnet
from abr_iod_amd.modeling.backbone.backbone import build_backbone
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.solver.build import make_optimizer
from abr_iod_amd.solver.grad_reducer import BUCKET_ORDER, make_buckets
from abr_iod_amd.utils.checkpoint import (Checkpointer, DetectronCheckpointer, align_keys, c2_blob_to_key, load_state_dict,
                                          reference_state_dict)

R101 = ["MODEL.DEVICE", "cpu", "MODEL.BACKBONE.CONV_BODY", "R-101-C4"]
TINY = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8,
        "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 128]
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "r101_state_dict_shapes.json")


def _gold():
    with open(GOLD) as f:
        return json.load(f)["entries"]


def _cfgs(extra=(), tiny=False):
    return make_cfgs("15-5", overrides=R101 + (TINY if tiny else []) + [str(v) if isinstance(v, tuple) else v for v in extra])


def _target(extra=(), tiny=False):
    return build_detection_model(_cfgs(extra, tiny)[1])


@pytest.fixture(scope="module")
def full():
    """the full-width 21-class R-101-C4 target at the default FREEZE_CONV_BODY_AT 2 (the model the golden was taken from)"""
    torch.manual_seed(0)
    return _target()


def test_stage_table():
    assert [s.block_count for s in resnet.stage_specs("R-50-C4")] == [3, 4, 6]
    assert [s.block_count for s in resnet.stage_specs("R-101-C4")] == [3, 4, 23]
    assert [s.return_features for s in resnet.stage_specs("R-101-C4")] == [False, False, True]


def test_state_dict_matches_reference(full):
    gold = _gold()
    sd = reference_state_dict(full)
    assert set(sd) == {k for k, _, _, _ in gold}
    for k, shape, dtype, _ in gold:
        assert list(sd[k].shape) == shape and str(sd[k].dtype) == "torch." + dtype, k
    # the parameters in the reference's order (the order of its optimiser's per-tensor groups) with its requires_grad
    want = [(k, rg) for k, _, _, rg in gold if rg is not None]
    assert [(n, p.requires_grad) for n, p in full.named_parameters()] == want
    assert len(full.backbone.body.layer3) == 23 and len(full.roi_heads.box.feature_extractor.head.layer4) == 3


def test_trainable_count_and_optimiser_groups(full):
    names = [n for n, p in full.named_parameters() if p.requires_grad]
    assert len(names) == 103
    assert sum(n.startswith("backbone.body.layer3.") for n in names) == 23 * 3 + 1
    opt = make_optimizer(_cfgs()[1], full)
    assert len(opt.param_groups) == len(full.flat.segments)
    sd = opt.state_dict()
    assert len(sd["param_groups"]) == 103 and not sd["state"]
    # every trainable tensor lies inside the flat buffer's trainable region, in one segment of its own
    seen = set()
    for name, p, off, _ in opt._reference_params():
        g = opt._group_of(off)
        assert off + p.numel() <= g["range"][1] <= full.flat.n_trainable, name
        seen.add(g["range"])
    assert len(seen) == len(opt.param_groups)


def test_gradient_buckets_keep_order_and_layout(full):
    buckets = make_buckets(full.flat.segments)
    assert tuple(buckets) == BUCKET_ORDER
    size = {b: sum(e - a for a, e in r) for b, r in buckets.items()}
    assert 27.0e6 < size["backbone"] < 27.5e6                    # layer2 + the 23 blocks of layer3
    assert 15.0e6 < size["roi_heads"] < 15.3e6 and 9.4e6 < size["rpn"] < 9.6e6   # the heads' buckets do not change
    assert sum(size.values()) == full.flat.n_trainable
    for b, rs in buckets.items():
        assert all(r0[1] < r1[0] for r0, r1 in zip(rs, rs[1:])), b          # ascending, adjacent ranges merged
    segs = {n: (a, e) for n, a, e, _ in full.flat.segments}
    assert all(any(a <= segs[n][0] and segs[n][1] <= e for a, e in buckets["backbone"]) for n in segs if n.startswith("backbone.body.layer3."))


@pytest.mark.parametrize("freeze,count,frozen", [(0, 114, None), (1, 113, []), (2, 103, ["layer1"]), (3, 90, ["layer1", "layer2"]),
                                                 (4, 20, ["layer1", "layer2", "layer3"])])
def test_freeze_rule_at_23_blocks(freeze, count, frozen):
    m = _target(["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze], tiny=True)
    body = m.backbone.body
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert len(names) == count
    stages = ["backbone.body.stem."] + ["backbone.body.layer%d." % i for i in range(1, 4)]
    assert not any(n.startswith(tuple(stages[:freeze])) for n in names)
    assert body.frozen_stage_names() == frozen
    assert body._trains("layer3") == (freeze < 4)


def test_frozen_prefix_sharing_between_source_and_target():
    cfg_s, cfg_t = _cfgs(tiny=True)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    assert mt.backbone.body.frozen_stage_names() == ["layer1"] == ms.backbone.body.frozen_stage_names()
    assert frozen_prefix_shareable(ms, mt)
    # a frozen layer1 tensor that differs between the two models makes the prefix a different function
    with torch.no_grad():
        ms.backbone.body.layer1[2].conv3.weight.add_(1.0)
    resnet.bump_param_version()
    assert not frozen_prefix_shareable(ms, mt)


def test_deformable_layer3_has_23_dfconvs():
    extra = ["MODEL.RESNETS.STAGE_WITH_DCN", (False, False, True, False), "MODEL.RESNETS.WITH_MODULATED_DCN", True]
    m = _target(extra, tiny=True)
    l3 = m.backbone.body.layer3
    assert len(l3) == 23 and all(isinstance(b.conv2, resnet.DFConv2d) and b.conv2.modulated for b in l3)
    assert not any(isinstance(b.conv2, resnet.DFConv2d) for b in m.backbone.body.layer2)
    names = [n for n, p in m.named_parameters() if p.requires_grad]
    assert sum(".conv2.offset." in n for n in names) == 2 * 23 and len(names) == 103 + 2 * 23
    opt = make_optimizer(_cfgs(extra, tiny=True)[1], m)
    assert len(opt.param_groups) == len(m.flat.segments) and len(opt.state_dict()["param_groups"]) == len(names)


@pytest.mark.parametrize("dtype,math", [("float16", ops.MATH_F16), ("bfloat16", ops.MATH_BF16)])
def test_dtype_reaches_every_block(dtype, math):
    m = _target(["DTYPE", dtype], tiny=True)
    for name in ("layer1", "layer2", "layer3"):
        assert all(b.math == math for b in getattr(m.backbone.body, name)), name
    assert resnet.set_conv_math(m.backbone, ops.MATH_F32) == 3 + 4 + 23


def test_c2_blob_names_at_depth():
    cases = {"res4_22_branch2c_bn_s": "layer3.22.bn3.weight", "res4_22_branch2c_bn_b": "layer3.22.bn3.bias",
             "res4_22_branch2c_w": "layer3.22.conv3.weight", "res4_22_branch2a_w": "layer3.22.conv1.weight",
             "res4_22_branch2b_bn_s": "layer3.22.bn2.weight", "res4_21_branch2c_bn_s": "layer3.21.bn3.weight",
             "res4_10_branch2b_w": "layer3.10.conv2.weight", "res4_0_branch1_w": "layer3.0.downsample.0.weight",
             "res4_0_branch1_bn_s": "layer3.0.downsample.1.weight", "res5_0_branch2a_w": "layer4.0.conv1.weight",
             "res4_22_branch2c_w_momentum": None}
    for blob, key in cases.items():
        assert c2_blob_to_key(blob) == key, blob


def _c2_blobs(specs):
    """every weight blob name of the stages (res2..res4) of a Detectron ResNet body"""
    out = []
    for spec in specs:
        for i in range(spec.block_count):
            for br in (["1"] if i == 0 else []) + ["2a", "2b", "2c"]:
                pre = "res%d_%d_branch%s" % (spec.index + 1, i, br)
                out += [pre + "_w", pre + "_bn_s", pre + "_bn_b"]
    return out


def test_c2_pkl_loads_every_r101_body_tensor(tmp_path):
    cfg_s, cfg_t = _cfgs(tiny=True)
    mt = build_detection_model(cfg_t)
    ref = reference_state_dict(mt)
    rng = np.random.RandomState(0)
    blobs, want = {}, {}
    for blob in _c2_blobs(resnet.stage_specs("R-101-C4")):
        key = "backbone.body." + c2_blob_to_key(blob)
        blobs[blob] = rng.randn(*ref[key].shape).astype(np.float32)
        want[key] = blobs[blob]
    assert sum(k.startswith("backbone.body.layer3.") for k in want) == 23 * 9 + 3
    f = str(tmp_path / "R-101.pkl")
    with open(f, "wb") as fh:
        pickle.dump({"blobs": blobs}, fh)
    DetectronCheckpointer(cfg_t, mt).load(f)
    after = reference_state_dict(mt)
    for key, v in want.items():
        assert np.array_equal(after[key].numpy(), v), key
    # every conv weight and FrozenBN weight / bias of layer1..layer3 comes from the file
    body = {k for k in ref if k.startswith("backbone.body.layer") and k.endswith((".weight", ".bias"))}
    assert body == set(want)


def test_unsupported_bodies_are_refused():
    for body in ("R-50-C5", "R-101-C5", "R-50-FPN", "R-101-FPN", "R-152-FPN", "R-50-FPN-RETINANET", "R-101-FPN-RETINANET", "FBNet"):
        _, cfg = make_cfgs("15-5", overrides=["MODEL.DEVICE", "cpu", "MODEL.BACKBONE.CONV_BODY", body] + TINY)
        for build in (build_detection_model, build_backbone, resnet.ResNet):
            with pytest.raises(NotImplementedError, match="R-101-C4, R-50-C4"):
                build(cfg)


def test_reference_layout_round_trip(full, tmp_path):
    """a file written by ours holds the reference model's keys, shapes and dtypes (what its Checkpointer needs: torch.load, longest-suffix
    alignment, load_state_dict) and reads back into a fresh model bit for bit"""
    gold = _gold()
    d = str(tmp_path)
    with torch.no_grad():
        full.backbone.body.layer3[22].conv3.weight.uniform_(-1, 1)
    Checkpointer(full, save_dir=d, save_to_disk=True).save("model_final", trim=True)
    loaded = torch.load(os.path.join(d, "model_final.pth"), weights_only=False)["model"]
    keys = [k for k, _, _, _ in gold]
    assert align_keys(keys, list(loaded)) == {k: k for k in keys}
    for k, shape, dtype, _ in gold:
        assert list(loaded[k].shape) == shape and str(loaded[k].dtype) == "torch." + dtype, k
    torch.manual_seed(1)
    b = _target()
    Checkpointer(b).load(os.path.join(d, "model_final.pth"))
    sa, sb = reference_state_dict(full), reference_state_dict(b)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_incremental_weight_surgery(tmp_path):
    """the source (16 classes) -> target (21 classes) surgery of build_models and of loading a trimmed source checkpoint"""
    cfg_s, cfg_t = _cfgs(tiny=True)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    ss, st = reference_state_dict(ms), reference_state_dict(mt)
    for k, v in ss.items():
        w = st[k]
        assert torch.equal(v, w if v.shape == w.shape else w[: v.shape[0]]), k
    d = str(tmp_path)
    Checkpointer(ms, save_dir=d, save_to_disk=True).save("model_trimmed", trim=True)
    torch.manual_seed(3)
    fresh = build_detection_model(cfg_t)
    before = reference_state_dict(fresh)
    load_state_dict(fresh, torch.load(os.path.join(d, "model_trimmed.pth"), weights_only=False)["model"])
    after = reference_state_dict(fresh)
    for k, v in ss.items():
        if after[k].shape == v.shape:
            assert torch.equal(after[k], v), k
        else:   # grown head: the stored rows first, the new classes' rows untouched
            assert torch.equal(after[k][: v.shape[0]], v) and torch.equal(after[k][v.shape[0]:], before[k][v.shape[0]:]), k
    assert torch.equal(after["backbone.body.layer3.22.conv2.weight"], ss["backbone.body.layer3.22.conv2.weight"])

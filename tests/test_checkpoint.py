"""F3: checkpoint files in the reference's format -- CPU only, no kernels involved.
Reference behaviour restated from utils/checkpoint.py:13-142 and utils/model_serialization.py:10-91."""
import os
import pickle

import numpy as np
import pytest
import torch

from abr_iod_amd.engine.synthetic import make_cfgs
from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
from abr_iod_amd.utils.checkpoint import (Checkpointer, DetectronCheckpointer, align_keys, c2_blob_to_key, load_state_dict,
                                          reference_state_dict)

TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32,
        "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 128]


def _models():
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, gamma=1.0, overrides=TINY)
    return cfg_s, cfg_t, build_detection_model(cfg_s), build_detection_model(cfg_t)


def _sd(g, prefix):
    return {k[len(prefix):]: torch.from_numpy(g[k]) for k in g.files if k.startswith(prefix)}


def test_align_keys_longest_suffix_wins():
    m = align_keys(["backbone.body.stem.conv1.weight", "backbone.body.layer1.0.conv1.weight", "rpn.head.conv.bias"],
                   ["conv1.weight", "layer1.0.conv1.weight", "unused.bias"])
    assert m == {"backbone.body.stem.conv1.weight": "conv1.weight", "backbone.body.layer1.0.conv1.weight": "layer1.0.conv1.weight"}


def test_c2_blob_names():
    cases = {"conv1_w": "conv1.weight", "res_conv1_bn_s": "bn1.weight", "res_conv1_bn_b": "bn1.bias",
             "res2_0_branch1_w": "layer1.0.downsample.0.weight", "res2_0_branch1_bn_s": "layer1.0.downsample.1.weight",
             "res3_3_branch2b_w": "layer2.3.conv2.weight", "res4_5_branch2c_bn_b": "layer3.5.bn3.bias",
             "res5_2_branch2a_bn_s": "layer4.2.bn1.weight", "conv_rpn_w": "rpn.head.conv.weight",
             "rpn_cls_logits_b": "rpn.head.cls_logits.bias", "rpn_bbox_pred_w": "rpn.head.bbox_pred.weight",
             "cls_score_w": "cls_score.weight", "bbox_pred_b": "bbox_pred.bias", "pred_w": "fc1000.weight",
             "conv1_w_momentum": None, "lr": None}
    for blob, key in cases.items():
        assert c2_blob_to_key(blob) == key, blob


def test_model_file_round_trip_and_grown_head(gold, tmp_path):
    g = gold("e2e_tiny")
    sd_t, sd_s = _sd(g, "T/"), _sd(g, "S/")
    cfg_s, cfg_t, ms, mt = _models()
    # a reference-written file: {"model": state_dict} with DistributedDataParallel's "module." prefix
    f = str(tmp_path / "ref_source.pth")
    torch.save({"model": {"module." + k: v for k, v in sd_s.items()}, "iteration": 7}, f)
    extra = Checkpointer(ms).load(f)
    assert extra == {"iteration": 7}
    back = reference_state_dict(ms)
    assert set(back) == set(sd_s)            # every key of the reference's state_dict, cell-anchor buffers included
    for k, v in sd_s.items():
        assert torch.equal(back[k], v), k
    # weight surgery: the 16-class source file into the 21-class target -> first 16 / 64 rows copied, the rest untouched
    before = reference_state_dict(mt)
    Checkpointer(mt).load(f)
    after = reference_state_dict(mt)
    for k in ("roi_heads.box.predictor.cls_score.weight", "roi_heads.box.predictor.cls_score.bias",
              "roi_heads.box.predictor.bbox_pred.weight", "roi_heads.box.predictor.bbox_pred.bias"):
        n = sd_s[k].shape[0]
        assert after[k].shape[0] > n
        assert torch.equal(after[k][:n], sd_s[k]) and torch.equal(after[k][n:], before[k][n:]), k
    assert torch.equal(after["backbone.body.layer2.0.conv1.weight"], sd_s["backbone.body.layer2.0.conv1.weight"])
    # our file, our loader, trimmed: model only and last_checkpoint not tagged
    d = str(tmp_path / "out")
    os.makedirs(d)
    Checkpointer(mt, save_dir=d, save_to_disk=True).save("model_trimmed", trim=True)
    assert sorted(os.listdir(d)) == ["model_trimmed.pth"]
    data = torch.load(os.path.join(d, "model_trimmed.pth"), weights_only=False)
    assert list(data.keys()) == ["model"]
    assert set(sd_t) == set(data["model"].keys())
    for k, v in data["model"].items():
        assert v.shape == sd_t[k].shape and v.device.type == "cpu", k


def test_pretrained_backbone_suffix_matching(tmp_path):
    """ImageNet-style file with bare `layerN...` keys lands in backbone.body.* and in the C5 head (layer4)."""
    cfg_s, cfg_t, ms, mt = _models()
    ref = reference_state_dict(mt)
    gen = torch.Generator().manual_seed(0)
    loaded = {}
    for k, v in ref.items():
        for pre in ("backbone.body.stem.", "backbone.body.", "roi_heads.box.feature_extractor.head."):
            if k.startswith(pre):
                loaded[k[len(pre):]] = torch.randn(v.shape, generator=gen)
                break
    f = str(tmp_path / "imagenet.pth")
    torch.save(loaded, f)  # bare state_dict, no "model" key (utils/checkpoint.py:139-141)
    DetectronCheckpointer(cfg_t, mt).load(f)
    after = reference_state_dict(mt)
    assert torch.equal(after["backbone.body.stem.conv1.weight"], loaded["conv1.weight"])
    assert torch.equal(after["backbone.body.layer3.5.conv2.weight"], loaded["layer3.5.conv2.weight"])
    assert torch.equal(after["roi_heads.box.feature_extractor.head.layer4.2.bn3.bias"], loaded["layer4.2.bn3.bias"])
    assert torch.equal(after["rpn.head.conv.weight"], ref["rpn.head.conv.weight"])  # no match -> untouched
    with pytest.raises(FileNotFoundError):
        DetectronCheckpointer(cfg_t, mt).load("catalog://ImageNetPretrained/MSRA/R-50")


def test_c2_pkl_loads(tmp_path):
    cfg_s, cfg_t, ms, mt = _models()
    ref = reference_state_dict(mt)
    w = np.random.RandomState(0).randn(*ref["backbone.body.layer1.0.conv1.weight"].shape).astype(np.float32)
    s = np.random.RandomState(1).rand(ref["backbone.body.layer1.0.bn1.weight"].shape[0]).astype(np.float32)
    f = str(tmp_path / "R-50.pkl")
    with open(f, "wb") as fh:
        pickle.dump({"blobs": {"res2_0_branch2a_w": w, "res2_0_branch2a_bn_s": s, "res2_0_branch2a_w_momentum": w * 0}}, fh)
    DetectronCheckpointer(cfg_t, mt).load(f)
    after = reference_state_dict(mt)
    assert np.array_equal(after["backbone.body.layer1.0.conv1.weight"].numpy(), w)
    assert np.array_equal(after["backbone.body.layer1.0.bn1.weight"].numpy(), s)


def test_resume_with_torch_sgd_state(tmp_path):
    """"optimizer" is torch.optim.SGD's state_dict built the reference's way (solver/build.py:7-21); a full checkpoint
    round-trips through last_checkpoint and the momentum buffers come back in OIHW layout."""
    cfg_s, cfg_t, ms, mt = _models()
    opt = make_optimizer(cfg_t, mt)
    sched = make_lr_scheduler(cfg_t, opt)
    # what the reference would have written after a few steps on the same architecture
    ref_sd = reference_state_dict(mt)
    names = [n for n, p in mt.named_parameters() if p.requires_grad]
    tensors = [torch.nn.Parameter(ref_sd[n].clone()) for n in names]
    groups = [{"params": [t], "lr": cfg_t.SOLVER.BASE_LR * (cfg_t.SOLVER.BIAS_LR_FACTOR if "bias" in n else 1),
               "weight_decay": cfg_t.SOLVER.WEIGHT_DECAY_BIAS if "bias" in n else cfg_t.SOLVER.WEIGHT_DECAY}
              for n, t in zip(names, tensors)]
    topt = torch.optim.SGD(groups, cfg_t.SOLVER.BASE_LR, momentum=cfg_t.SOLVER.MOMENTUM)
    gen = torch.Generator().manual_seed(1)
    for _ in range(2):
        for t in tensors:
            t.grad = torch.randn(t.shape, generator=gen)
        topt.step()
    d = str(tmp_path / "run")
    os.makedirs(d)
    model_sd = dict(ref_sd)
    model_sd.update({n: t.detach() for n, t in zip(names, tensors)})
    torch.save({"model": model_sd, "optimizer": topt.state_dict(), "scheduler": {"last_epoch": 1234}, "iteration": 1234},
               os.path.join(d, "model_last.pth"))
    with open(os.path.join(d, "last_checkpoint"), "w") as fh:
        fh.write(os.path.join(d, "model_last.pth"))
    ck = Checkpointer(mt, opt, sched, save_dir=d, save_to_disk=True)
    extra = ck.load("ignored-because-last_checkpoint-wins.pth")
    assert extra == {"iteration": 1234} and sched.last_epoch == 1234
    out = opt.state_dict()
    tsd = topt.state_dict()
    assert len(out["param_groups"]) == len(tsd["param_groups"]) == len(names)
    for i, n in enumerate(names):
        assert out["param_groups"][i]["params"] == [i]
        for k in ("lr", "weight_decay", "momentum", "dampening", "nesterov"):
            assert out["param_groups"][i][k] == tsd["param_groups"][i][k], (n, k)
        assert torch.equal(out["state"][i]["momentum_buffer"], tsd["state"][i]["momentum_buffer"]), n
    # save -> fresh objects -> load gives the same thing; torch's own SGD accepts our optimizer state
    ck.save("model_0001235", iteration=1235)
    assert ck.get_checkpoint_file().endswith("model_0001235.pth")
    cfg_s2, cfg_t2, _, mt2 = _models()
    opt2 = make_optimizer(cfg_t2, mt2)
    sched2 = make_lr_scheduler(cfg_t2, opt2)
    extra2 = Checkpointer(mt2, opt2, sched2, save_dir=d).load()
    assert extra2 == {"iteration": 1235} and sched2.last_epoch == 1234
    a, b = reference_state_dict(mt), reference_state_dict(mt2)
    assert all(torch.equal(a[k], b[k]) for k in a)
    assert torch.equal(opt.momentum_buffer, opt2.momentum_buffer)
    topt.load_state_dict(torch.load(ck.get_checkpoint_file(), weights_only=False)["optimizer"])


def test_reference_checkpointer_reads_our_file(gold, tmp_path):
    """Interop pin: a file written by ours loads into the REFERENCE's model the way the reference's Checkpointer._load_file /
    _load_model do it (torch.load + utils/model_serialization.py:72-91: strip "module.", longest-suffix alignment, then
    model.load_state_dict), and the model's state_dict then equals what we exported.  The reference model's state_dict --
    every key, shape and dtype, the target at these widths -- is the one tests/golden/e2e_tiny.npz stores (T/), written by the
    reference itself (tests/golden/make_golden_e2e.py)."""
    rm_sd = _sd(gold("e2e_tiny"), "T/")
    cfg_s, cfg_t, ms, mt = _models()
    d = str(tmp_path / "ours")
    os.makedirs(d)
    Checkpointer(mt, save_dir=d, save_to_disk=True).save("model_final", trim=True)
    loaded = torch.load(os.path.join(d, "model_final.pth"), weights_only=False)["model"]
    ours = reference_state_dict(mt)
    assert set(rm_sd) == set(ours)
    # every key of the reference's model takes the file's tensor of the same name (none keeps its initial value)
    amap = align_keys(list(rm_sd), list(loaded))
    assert amap == {k: k for k in rm_sd}
    for k, v in rm_sd.items():
        got = loaded[amap[k]]
        assert got.shape == v.shape and got.dtype == v.dtype, k      # what load_state_dict's copy_ needs
        assert torch.equal(got, ours[k]), k

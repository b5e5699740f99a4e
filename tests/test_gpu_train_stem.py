"""MODEL.BACKBONE.FREEZE_CONV_BODY_AT below the default 2: the stem (0) and layer1 (0, 1) train.  One step of the tiny-image setup of
test_gpu_e2e.py::test_train_step_losses_and_grads_vs_oracle against the torch-CPU oracle with the same trainable set, the trainable parameter
names for every FREEZE value against the reference's _freeze_backbone rule, and one full train_step at FREEZE 0."""
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

BASE_TRAINABLE = ("backbone.body.layer2", "backbone.body.layer3", "rpn.", "roi_heads.")
SMALL = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 600, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 300,
         "MODEL.RPN.POST_NMS_TOP_N_TEST", 150, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 48, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64]


def _close(a, b, tol=1e-4):
    return abs(a - b) <= tol * max(1.0, abs(b))


def _build(name, math, freeze, seed=0):
    import os
    from e2e_common import CONFIGS, clamp_targets, needs_source
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs, synthetic_batch
    task, dist_type, feat, alpha, beta, gamma, label_range, n_old = CONFIGS[name]
    os.environ["ABR_CONV_MATH"] = math
    try:
        cfg_s, cfg_t = make_cfgs(task, dist_type=dist_type, feat=feat, alpha=alpha, beta=beta, gamma=gamma,
                                 overrides=SMALL + ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze])
        torch.manual_seed(seed)
        random.seed(seed)
        ms, mt = build_models(cfg_s, cfg_t, seed=seed, need_source=needs_source(name))
    finally:
        os.environ.pop("ABR_CONV_MATH", None)   # read at model construction only
    with torch.no_grad():  # make target != source so that the ARD / ID gradients are non-trivial
        g = torch.Generator(device="cuda").manual_seed(5)
        n = mt.flat.n_trainable
        mt.flat.params[:n].mul_(1.0 + 0.05 * torch.randn(n, device="cuda", generator=g))
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=label_range)
    clamp_targets(targets, 224, 160)
    return dict(cfg_s=cfg_s, cfg_t=cfg_t, ms=ms, mt=mt, images=images, targets=targets, n_old=n_old, dist_type=dist_type)


def _prefixes(freeze):
    extra = ("backbone.body.stem",) if freeze < 1 else ()
    return extra + (("backbone.body.layer1",) if freeze < 2 else ()) + BASE_TRAINABLE


CASES = [(0, "15-5", "f16x3"), (0, "15-5", "bf16x6"), (0, "15-5", "f32"), (0, "finetune", "f16x3"), (1, "15-5", "f16x3"), (1, "finetune", "f16x3")]


@pytest.mark.parametrize("case", CASES, ids=["freeze{}-{}-{}".format(*c) for c in CASES])
def test_freeze_losses_and_grads_vs_oracle(case):
    from abr_iod_amd.distillation.distillation import calculate_attentive_roi_feature_distillation, calculate_roi_distillation_losses
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import convert_to_roi_format
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    from oracle import torch_ref as R
    from oracle.model_ref import RefModel

    freeze, name, math = case
    S = _build(name, math, freeze)
    ms, mt, images, targets, cfg = S["ms"], S["mt"], S["images"], S["targets"], S["cfg_t"]
    n_old, dist_type = S["n_old"], S["dist_type"]
    k_old, k_all = n_old + 1, mt.roi_heads.box.predictor.num_classes
    distill = ms is not None
    sd_t = reference_state_dict(mt)
    sd_s = reference_state_dict(ms) if distill else None
    mt.flat.zero_grad()
    if distill:
        with torch.no_grad():
            soften_result, _, soften_proposal, feat_s, _, _, _, raf_s = ms.generate_soften_proposal(images)
    loss_dict, feat_t, _, anchors, rpn_out, props, raf_det, _ = mt(images, targets)
    assert feat_t[0].requires_grad
    total = sum(loss_dict.values())
    gpu = {k: float(v) for k, v in loss_dict.items()}
    if distill:
        target_result, _, raf_t = mt.forward(images, targets, features=feat_t, proposals=soften_proposal)
        l_id = calculate_roi_distillation_losses(soften_result, target_result, dist=dist_type)
        l_ard = calculate_attentive_roi_feature_distillation(raf_s, raf_t, gamma=cfg.DIST.GAMMA)
        total = total + cfg.DIST.ALPHA * l_id + cfg.DIST.BETA * l_ard
        gpu["id"], gpu["ard"] = float(l_id), float(l_ard)
    total.backward()
    torch.cuda.synchronize()

    ref_t = RefModel(sd_t, trainable_prefixes=_prefixes(freeze))
    img = images.cpu()
    if distill:
        ref_s = RefModel(sd_s, trainable_prefixes=())
        with torch.no_grad():
            fs = ref_s.backbone(img)
    ft = ref_t.backbone(img)
    np.testing.assert_allclose(feat_t[0].detach().cpu().numpy(), ft.detach().numpy(), rtol=0, atol=1e-4 * float(ft.abs().max()))
    obj, reg = ref_t.rpn_head(ft)
    ev = mt.rpn.loss_evaluator
    labels, reg_t = ev.last_targets
    pos_idx, samp_idx = ev.last_sampled
    n = labels[0].numel()
    pos_idx, samp_idx = pos_idx.cpu(), samp_idx.cpu()
    pos_idx, samp_idx = pos_idx[pos_idx >= 0], samp_idx[samp_idx >= 0]
    posm = torch.zeros(2 * n, dtype=torch.bool); posm[pos_idx] = True
    negm = torch.zeros(2 * n, dtype=torch.bool); negm[samp_idx] = True; negm &= ~posm
    lo, lb = R.rpn_loss(obj, reg, torch.stack([l.cpu() for l in labels]), torch.stack([t.cpu() for t in reg_t]), posm.view(2, n), negm.view(2, n))
    det_props = mt.roi_heads.box.loss_evaluator._proposals
    rois = convert_to_roi_format(det_props).cpu()
    labels_h = torch.cat([p.get_field("labels") for p in det_props]).cpu()
    rt_h = torch.cat([p.get_field("regression_targets") for p in det_props]).cpu()
    _, logits, boxreg = ref_t.box_head(ft, rois)
    lc, lbox = R.box_head_loss(logits, boxreg, labels_h, rt_h, dist_type, n_old)
    total_r = lc + lbox + lo + lb
    ref = dict(loss_classifier=float(lc), loss_box_reg=float(lbox), loss_objectness=float(lo), loss_rpn_box_reg=float(lb))
    if distill:
        rois64 = convert_to_roi_format(soften_proposal).cpu()
        with torch.no_grad():
            pooled_s, zs, bs = ref_s.box_head(fs, rois64)
        pooled_t, zt, bt = ref_t.box_head(ft, rois64)
        l_id_r = R.roi_distillation_loss(zs, bs.view(-1, k_old, 4), zt, bt.view(-1, k_all, 4), dist_type)
        l_ard_r = R.ard_loss(pooled_s, pooled_t, cfg.DIST.GAMMA)
        total_r = total_r + cfg.DIST.ALPHA * l_id_r + cfg.DIST.BETA * l_ard_r
        ref["id"], ref["ard"] = float(l_id_r), float(l_ard_r)
    total_r.backward()
    print("GPU   ", gpu)
    print("oracle", ref)
    for k in ref:
        assert _close(gpu[k], ref[k]), f"{k}: gpu {gpu[k]} vs oracle {ref[k]}"

    convs = {id(m.weight): m for m in mt.modules() if isinstance(m, Conv2d)}
    rgrads = ref_t.grads()
    report = []
    for pname, p in mt.named_parameters():
        if not p.requires_grad:
            continue
        g = p.grad
        if id(p) in convs:
            if convs[id(p)].in_channels != g.shape[-1]:   # the stem's padded input channel: its gradient is exactly 0
                assert torch.all(g[..., convs[id(p)].in_channels:] == 0), pname
            g = g[..., : convs[id(p)].in_channels].permute(0, 3, 1, 2)
        g = g.detach().cpu()
        r = rgrads[pname]
        rel = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-12)
        rel_l2 = float((g - r).norm() / max(float(r.norm()), 1e-12))
        report.append((pname, rel, rel_l2))
    for pname, rel, rel_l2 in report:
        print(f"  {pname:70s} max-rel {rel:.2e}  l2-rel {rel_l2:.2e}")
    assert len(report) == len(rgrads) == (63 if freeze == 0 else 62), (len(report), len(rgrads))
    assert any(n_.startswith("backbone.body.layer1.") for n_, _, _ in report)
    assert any(n_ == "backbone.body.stem.conv1.weight" for n_, _, _ in report) == (freeze == 0)
    for pname, rel, rel_l2 in report:
        assert rel <= 3.5e-3 and rel_l2 <= 1e-3, f"grad {pname}: max-rel {rel}, l2-rel {rel_l2}"
    if freeze == 0:
        assert float(mt.backbone.body.stem.conv1.weight.grad.abs().max()) > 0


def test_trainable_names_follow_the_reference_freeze_rule():
    """resnet.py:134-143 of the reference: stage 0 is the stem, stage i layer{i}; every stage below FREEZE_CONV_BODY_AT is frozen."""
    from abr_iod_amd.engine.synthetic import make_cfgs
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    names = {}
    for freeze in range(5):
        _, cfg_t = make_cfgs("15-5", overrides=SMALL + ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze])
        m = build_detection_model(cfg_t)
        names[freeze] = {n for n, p in m.named_parameters() if p.requires_grad}
        all_names = {n for n, _ in m.named_parameters()}
        del m
    convs = {n for n in all_names if n.endswith("conv1.weight") or n.endswith("conv2.weight") or n.endswith("conv3.weight") or "downsample.0" in n}
    everything = {n for n in all_names if not n.startswith("backbone.body.") or n in convs}
    for freeze in range(5):
        frozen = ["backbone.body.stem."] + ["backbone.body.layer%d." % i for i in range(1, 4)]
        want = {n for n in everything if not any(n.startswith(pre) for pre in frozen[:freeze])}
        assert names[freeze] == want, (freeze, sorted(names[freeze] ^ want)[:8])
    assert len(names[2]) == 52 and len(names[1]) == 62 and len(names[0]) == 63


def _train_one(freeze, seed=0, next_images=True):
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    S = _build("15-5", "f16x3", freeze, seed=seed)
    ms, mt, cfg = S["ms"], S["mt"], S["cfg_t"]
    opt = make_optimizer(cfg, mt)
    sch = make_lr_scheduler(cfg, opt)
    named = [(n, p) for n, p in mt.named_parameters()]
    before = {n: p.detach().clone() for n, p in named}
    lrs = {g["name"]: g["lr"] for g in opt.param_groups}
    torch.manual_seed(11)
    random.seed(11)
    train_step(ms, mt, S["images"], S["targets"], opt, sch, cfg, next_images=S["images"] if next_images else None)
    torch.cuda.synchronize()
    return S, mt, opt, named, before, lrs


def test_train_step_freeze0_sgd_determinism_checkpoint(tmp_path):
    from abr_iod_amd.utils.checkpoint import Checkpointer, reference_state_dict
    S, mt, opt, named, before, lrs = _train_one(0)
    cfg = S["cfg_t"]
    stem_w = mt.backbone.body.stem.conv1.weight
    assert torch.all(stem_w.detach()[..., 3] == 0), "the padded stem channel moved"
    moved = 0
    for n, p in named:
        if not (n.startswith("backbone.body.stem.") or n.startswith("backbone.body.layer1.")) or not p.requires_grad:
            continue
        # torch.optim.SGD (momentum, weight decay, dampening 0) from a zero momentum buffer given the same gradient
        r = before[n].clone().requires_grad_(True)
        wd = cfg.SOLVER.WEIGHT_DECAY_BIAS if "bias" in n else cfg.SOLVER.WEIGHT_DECAY
        topt = torch.optim.SGD([r], lr=lrs[n], momentum=cfg.SOLVER.MOMENTUM, weight_decay=wd)
        r.grad = p.grad.detach().clone()
        topt.step()
        assert torch.allclose(p.detach(), r.detach(), rtol=1e-6, atol=1e-7), n
        moved += int(not torch.equal(p.detach(), before[n]))
    assert moved == 11, moved   # the stem conv and layer1's ten convs all learn
    for n, p in named:
        if not p.requires_grad:
            assert torch.equal(p.detach(), before[n]), n
    # the same step from the same state: bit-identical
    _, mt2, _, named2, _, _ = _train_one(0)
    for (n, p), (_, q) in zip(named, named2):
        assert torch.equal(p.detach(), q.detach()), n
    # the checkpoint carries the trained stem in the reference's layout
    sd = reference_state_dict(mt)
    w = sd["backbone.body.stem.conv1.weight"]
    assert tuple(w.shape) == (64, 3, 7, 7)
    assert torch.equal(w.cpu(), stem_w.detach()[..., :3].permute(0, 3, 1, 2).cpu())
    ck = Checkpointer(mt, None, None, str(tmp_path), save_to_disk=True)
    ck.save("model_stem")
    saved = torch.load(str(tmp_path / "model_stem.pth"), weights_only=False)["model"]
    assert tuple(saved["backbone.body.stem.conv1.weight"].shape) == (64, 3, 7, 7)
    ck2 = Checkpointer(mt2, None, None, str(tmp_path), save_to_disk=False)
    ck2.load(str(tmp_path / "model_stem.pth"))
    assert torch.equal(mt2.backbone.body.stem.conv1.weight.detach(), stem_w.detach())


@pytest.mark.parametrize("freeze", [3, 4])
def test_train_step_deeper_freeze_keeps_frozen_stages(freeze):
    S, mt, opt, named, before, lrs = _train_one(freeze)
    frozen = ["backbone.body.stem."] + ["backbone.body.layer%d." % i for i in range(1, 4)]
    n_frozen = 0
    for n, p in named:
        if any(n.startswith(pre) for pre in frozen[:freeze]):
            assert not p.requires_grad, n
            assert torch.equal(p.detach(), before[n]), n
            n_frozen += 1
    assert n_frozen > 0
    assert any(not torch.equal(p.detach(), before[n]) for n, p in named if p.requires_grad)

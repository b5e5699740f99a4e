"""GPU: the R-101-C4 body (MODEL.BACKBONE.CONV_BODY "R-101-C4", 23 layer3 blocks) in a training step.  One step of the tiny-image setup of
test_gpu_train_stem.py against the torch-CPU oracle with 23 layer3 blocks (every loss, every trainable gradient) at FREEZE_CONV_BODY_AT 2
and 1 and in each arithmetic; a deformable layer3 (STAGE_WITH_DCN (F, F, T, F)) step; the eval forward against the oracle's backbone and
PostProcessor; and full-size steps of BASELINE.json configs[2] (15-5, ID + ARD, B = 4, 600x1000)."""
import math
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

R101 = ["MODEL.BACKBONE.CONV_BODY", "R-101-C4"]
SMALL = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 600, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 300,
         "MODEL.RPN.POST_NMS_TOP_N_TEST", 150, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 48, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64]
BASE_TRAINABLE = ("backbone.body.layer2", "backbone.body.layer3", "rpn.", "roi_heads.")


def _ref_model():
    from oracle.model_ref import RefModel

    class R101RefModel(RefModel):
        BLOCKS = {"layer1": 3, "layer2": 4, "layer3": 23}

    return R101RefModel


def _close(a, b, tol=1e-4):
    return abs(a - b) <= tol * max(1.0, abs(b))


def _build(name, math_, freeze, extra=(), seed=0):
    from e2e_common import CONFIGS, clamp_targets, needs_source
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs, synthetic_batch
    task, dist_type, feat, alpha, beta, gamma, label_range, n_old = CONFIGS[name]
    os.environ["ABR_CONV_MATH"] = math_
    try:
        cfg_s, cfg_t = make_cfgs(task, dist_type=dist_type, feat=feat, alpha=alpha, beta=beta, gamma=gamma,
                                 overrides=R101 + SMALL + ["MODEL.BACKBONE.FREEZE_CONV_BODY_AT", freeze] + list(extra))
        torch.manual_seed(seed)
        random.seed(seed)
        ms, mt = build_models(cfg_s, cfg_t, seed=seed, need_source=needs_source(name))
    finally:
        os.environ.pop("ABR_CONV_MATH", None)   # read at model construction only
    assert len(mt.backbone.body.layer3) == 23
    with torch.no_grad():  # make target != source so that the ARD / ID gradients are non-trivial
        g = torch.Generator(device="cuda").manual_seed(5)
        n = mt.flat.n_trainable
        mt.flat.params[:n].mul_(1.0 + 0.05 * torch.randn(n, device="cuda", generator=g))
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=label_range)
    clamp_targets(targets, 224, 160)
    return dict(cfg_s=cfg_s, cfg_t=cfg_t, ms=ms, mt=mt, images=images, targets=targets, n_old=n_old, dist_type=dist_type)


def _prefixes(freeze):
    return (("backbone.body.layer1",) if freeze < 2 else ()) + BASE_TRAINABLE


CASES = [(2, "f16x3"), (2, "bf16x6"), (2, "f32"), (1, "f16x3")]


@pytest.mark.parametrize("case", CASES, ids=["freeze{}-{}".format(*c) for c in CASES])
def test_r101_losses_and_grads_vs_oracle(case):
    from abr_iod_amd.distillation.distillation import calculate_attentive_roi_feature_distillation, calculate_roi_distillation_losses
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import convert_to_roi_format
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    from oracle import torch_ref as R

    freeze, math_ = case
    S = _build("15-5", math_, freeze)
    ms, mt, images, targets, cfg = S["ms"], S["mt"], S["images"], S["targets"], S["cfg_t"]
    n_old, dist_type = S["n_old"], S["dist_type"]
    k_old, k_all = n_old + 1, mt.roi_heads.box.predictor.num_classes
    sd_t, sd_s = reference_state_dict(mt), reference_state_dict(ms)
    mt.flat.zero_grad()
    with torch.no_grad():
        soften_result, _, soften_proposal, feat_s, _, _, _, raf_s = ms.generate_soften_proposal(images)
    loss_dict, feat_t, _, anchors, rpn_out, props, raf_det, _ = mt(images, targets)
    total = sum(loss_dict.values())
    gpu = {k: float(v) for k, v in loss_dict.items()}
    target_result, _, raf_t = mt.forward(images, targets, features=feat_t, proposals=soften_proposal)
    l_id = calculate_roi_distillation_losses(soften_result, target_result, dist=dist_type)
    l_ard = calculate_attentive_roi_feature_distillation(raf_s, raf_t, gamma=cfg.DIST.GAMMA)
    total = total + cfg.DIST.ALPHA * l_id + cfg.DIST.BETA * l_ard
    gpu["id"], gpu["ard"] = float(l_id), float(l_ard)
    total.backward()
    torch.cuda.synchronize()

    Ref = _ref_model()
    ref_t = Ref(sd_t, trainable_prefixes=_prefixes(freeze))
    ref_s = Ref(sd_s, trainable_prefixes=())
    img = images.cpu()
    with torch.no_grad():
        fs = ref_s.backbone(img)
    np.testing.assert_allclose(feat_s[0].cpu().numpy(), fs.numpy(), rtol=0, atol=1e-4 * float(fs.abs().max()))
    ft = ref_t.backbone(img)
    np.testing.assert_allclose(feat_t[0].detach().cpu().numpy(), ft.detach().numpy(), rtol=0, atol=1e-4 * float(ft.abs().max()))
    obj, reg = ref_t.rpn_head(ft)
    ev = mt.rpn.loss_evaluator
    labels, reg_t = ev.last_targets
    pos_idx, samp_idx = ev.last_sampled
    n = labels[0].numel()
    pos_idx, samp_idx = pos_idx.cpu(), samp_idx.cpu()
    pos_idx, samp_idx = pos_idx[pos_idx >= 0], samp_idx[samp_idx >= 0]
    posm = torch.zeros(2 * n, dtype=torch.bool)
    posm[pos_idx] = True
    negm = torch.zeros(2 * n, dtype=torch.bool)
    negm[samp_idx] = True
    negm &= ~posm
    lo, lb = R.rpn_loss(obj, reg, torch.stack([l.cpu() for l in labels]), torch.stack([t.cpu() for t in reg_t]), posm.view(2, n), negm.view(2, n))
    det_props = mt.roi_heads.box.loss_evaluator._proposals
    rois = convert_to_roi_format(det_props).cpu()
    labels_h = torch.cat([p.get_field("labels") for p in det_props]).cpu()
    rt_h = torch.cat([p.get_field("regression_targets") for p in det_props]).cpu()
    _, logits, boxreg = ref_t.box_head(ft, rois)
    lc, lbox = R.box_head_loss(logits, boxreg, labels_h, rt_h, dist_type, n_old)
    rois64 = convert_to_roi_format(soften_proposal).cpu()
    with torch.no_grad():
        pooled_s, zs, bs = ref_s.box_head(fs, rois64)
    pooled_t, zt, bt = ref_t.box_head(ft, rois64)
    l_id_r = R.roi_distillation_loss(zs, bs.view(-1, k_old, 4), zt, bt.view(-1, k_all, 4), dist_type)
    l_ard_r = R.ard_loss(pooled_s, pooled_t, cfg.DIST.GAMMA)
    total_r = lc + lbox + lo + lb + cfg.DIST.ALPHA * l_id_r + cfg.DIST.BETA * l_ard_r
    ref = dict(loss_classifier=float(lc), loss_box_reg=float(lbox), loss_objectness=float(lo), loss_rpn_box_reg=float(lb),
               id=float(l_id_r), ard=float(l_ard_r))
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
            g = g[..., : convs[id(p)].in_channels].permute(0, 3, 1, 2)
        g = g.detach().cpu()
        r = rgrads[pname]
        rel = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-12)
        rel_l2 = float((g - r).norm() / max(float(r.norm()), 1e-12))
        report.append((pname, rel, rel_l2))
    for pname, rel, rel_l2 in report:
        print(f"  {pname:70s} max-rel {rel:.2e}  l2-rel {rel_l2:.2e}")
    assert len(report) == len(rgrads) == (103 if freeze == 2 else 113), (len(report), len(rgrads))
    assert any(n_.startswith("backbone.body.layer3.22.") for n_, _, _ in report)
    assert any(n_.startswith("backbone.body.layer1.") for n_, _, _ in report) == (freeze < 2)
    for pname, rel, rel_l2 in report:
        assert rel <= 3.5e-3 and rel_l2 <= 1e-3, f"grad {pname}: max-rel {rel}, l2-rel {rel_l2}"


def test_r101_deformable_layer3_step():
    """STAGE_WITH_DCN (F, F, T, F): 23 deformable conv2s in one stage node; one train_step moves every offset conv, finite losses"""
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    S = _build("15-5", "f16x3", 2, extra=["MODEL.RESNETS.STAGE_WITH_DCN", "(False, False, True, False)", "MODEL.RESNETS.WITH_MODULATED_DCN", True])
    ms, mt, cfg = S["ms"], S["mt"], S["cfg_t"]
    offs = {n: p.detach().clone() for n, p in mt.named_parameters() if ".conv2.offset." in n}
    assert len(offs) == 2 * 23 and all(n.startswith("backbone.body.layer3.") for n in offs)
    opt = make_optimizer(cfg, mt)
    sch = make_lr_scheduler(cfg, opt)
    for _ in range(2):
        ld, _ = train_step(ms, mt, S["images"], S["targets"], opt, sch, cfg, next_images=S["images"])
        torch.cuda.synchronize()
        assert all(math.isfinite(float(v)) for v in ld.values()), ld
    moved = [n for n, v in offs.items() if not torch.equal(mt.get_parameter(n).detach(), v)]
    assert sorted(moved) == sorted(offs)


def test_r101_eval_forward_matches_oracle():
    """model.eval()(images): the C4 features equal the oracle's 23-block backbone, and the detections equal the oracle's PostProcessor
    applied to the model's own logits for the RPN's test-time proposals"""
    from abr_iod_amd.structures.image_list import to_image_list
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    from oracle import torch_ref as R
    S = _build("15-5", "f16x3", 2)
    mt, images = S["mt"], S["images"]
    mt.eval()
    with torch.no_grad():
        result, features, bg = mt(images)
        (props, _), _, _ = mt.rpn(to_image_list(images), features, None)
        logits, reg, _, _ = mt.roi_heads.box.calculate_soften_label(features, props)
    ref = _ref_model()(reference_state_dict(mt), trainable_prefixes=())
    with torch.no_grad():
        ft = ref.backbone(images.cpu())
    np.testing.assert_allclose(features[0].cpu().numpy(), ft.numpy(), rtol=0, atol=1e-4 * float(ft.abs().max()))
    assert len(result) == 2 and all(len(r) <= 100 for r in result)
    want, want_bg = R.post_process(logits.cpu(), reg.reshape(len(logits), -1).cpu(), [p.bbox.cpu().numpy() for p in props],
                                   [p.size for p in props])
    for r, (b, s, l) in zip(result, want):
        assert np.array_equal(r.get_field("labels").cpu().numpy(), l)
        np.testing.assert_allclose(r.get_field("scores").cpu().numpy(), s, rtol=1e-5)
        np.testing.assert_allclose(r.bbox.cpu().numpy(), b, rtol=1e-5, atol=2e-4)
    np.testing.assert_allclose(bg.get_field("scores").cpu().numpy(), want_bg[1], rtol=1e-5)
    mt.train()


def test_r101_full_size_steps():
    """configs[2] at B = 4, 600x1000 with the frozen-prefix prefetch: finite losses, the last layer3 block learns, layer1 stays put"""
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs, synthetic_batch
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=4, overrides=R101)
    random.seed(0)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    opt = make_optimizer(cfg_t, mt)
    sch = make_lr_scheduler(cfg_t, opt)
    assert len(opt.param_groups) == len(mt.flat.segments) and sum(p.requires_grad for p in mt.parameters()) == 103
    batches = [synthetic_batch(4, 600, 1000, seed=42 + 1009 * j, label_range=(16, 21), max_boxes=mb) for j, mb in enumerate((5, 3))]
    l3 = mt.backbone.body.layer3[22].conv3.weight.detach().clone()
    l1 = mt.backbone.body.layer1[2].conv3.weight.detach().clone()
    for i in range(3):
        im, tg = batches[i % 2]
        ld, _ = train_step(ms, mt, im, tg, opt, sch, cfg_t, next_images=batches[(i + 1) % 2][0])
        vals = {k: float(v.detach()) for k, v in ld.items()}
        assert all(math.isfinite(v) for v in vals.values()), (i, vals)
    torch.cuda.synchronize()
    assert not torch.equal(mt.backbone.body.layer3[22].conv3.weight.detach(), l3)
    assert torch.equal(mt.backbone.body.layer1[2].conv3.weight.detach(), l1)

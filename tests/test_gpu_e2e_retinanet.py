"""GPU: the whole R-50-FPN-RETINANET detector (tiny widths, NUM_CONVS 2, 3 foreground classes) against the float64 model
tests/detector_retinanet_ref.py on IDENTICAL weights, images and ground truth, in the three fp32-accurate arithmetics and both
MODEL.RETINANET.USE_C5 variants (P6 reads C5, or P5).

  * test_retinanet_train_step_losses_and_grads_vs_float64: model(batch, targets), sum(losses).backward().  Exact: the anchors, the labels
    (retinanet_loss_ref.batch_targets on the model's own anchors), n_pos.  Values: the regression targets within their bound, P3..P7 and every
    level's logits and deltas within 1e-4 of max |ref|, the two losses by retinanet_loss_ref.check_losses against the float64 model's, the
    gradient of each of the 70 trainable tensors within e2e_retinanet_common.GRAD_MAX_REL / GRAD_REL_L2; the pad row of cls_logits exactly 0.
  * test_retinanet_step_follows_the_update_rule: one FusedSGD step from zero momentum is p - lr_k (g + wd_k p) per tensor, lr_k and wd_k by
    the reference's rule (a key containing "bias": lr x 2, no weight decay), within 4 eps (|p| + lr_k (|g| + wd_k |p|)): the update is three
    roundings.  Frozen tensors keep their bits.
  * test_retinanet_step_then_forward_vs_float64: the first test's comparison on the weights after that step (derived weight copies).

What the pieces' own tests cannot see and these can: P6's and P7's gradients returning through p7, the ReLU mask and p6 into C5 (added to the
lateral's) or into P5 and the top-down chain, the head's parameter gradients accumulated over five levels, the pyramid starting at C3, the
order of levels, cells and anchors between the head's outputs and the targets, which tensors train, and what the optimiser does to the
names RetinaNet adds (tests/test_detector_retinanet_ref.py shows the inputs react to each)."""
import os

import numpy as np
import pytest
import torch

import detector_retinanet_ref as D
import e2e_retinanet_common as E
import retinanet_loss_ref as RL

pytestmark = pytest.mark.gpu

MATHS = ("bf16x6", "f16x3", "f32")
N_TRAINABLE = 70
EPS32 = float(np.finfo(np.float32).eps)

def N(t):
    return t.detach().cpu().numpy()


def _near(got, want, what):
    want = np.asarray(want, np.float64)
    err, lim = float(np.abs(np.asarray(got, np.float64) - want).max()), 1e-4 * float(np.abs(want).max())
    print("%-28s err %.3e  limit %.3e" % (what, err, lim))
    assert err <= lim, (what, err, lim)


@pytest.fixture(scope="module", params=[(m, c5) for m in MATHS for c5 in (True, False)], ids=lambda p: "%s-%s" % (p[0], E.variant(p[1])))
def S(request):
    from abr_iod_amd import ops
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    math, use_c5 = request.param
    os.environ["ABR_CONV_MATH"] = math
    try:
        cfg, mt, sd = E.build("cuda", use_c5)
    finally:
        os.environ.pop("ABR_CONV_MATH", None)   # read at model construction only
    want = {"bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f32": ops.MATH_F32}[math]
    assert all(m.math == want for m in mt.modules() if hasattr(m, "math"))
    assert mt.backbone.fpn.top_blocks.use_P5 == (not use_c5) and mt.rpn.head.ld_cls == 28 and mt.rpn.head.num_classes == E.C
    cpu_images = E.make_images()
    images = ImageList(cpu_images.cuda(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    targets = []
    for (h, w), b, l in zip(E.IMAGE_SIZES, gts, gt_labels):
        t = BoxList(torch.from_numpy(b).cuda(), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l).cuda())
        targets.append(t)
    return dict(math=math, use_c5=use_c5, v=E.variant(use_c5), cfg=cfg, mt=mt, sd=sd, images=images, cpu_images=cpu_images, targets=targets,
                gts=gts, gt_labels=gt_labels, stepped=False)


def _gpu_step(S):
    """model(batch, targets), sum(losses).backward() -> what the comparison needs, everything read back"""
    from abr_iod_amd import ops
    mt = S["mt"]
    mt.train()
    mt.flat.zero_grad()
    out = mt(S["images"], S["targets"])
    assert len(out) == 8 and out[5] is None and out[6] is None and out[7] is None
    losses, feats, anchors, (box_cls, box_reg) = out[0], out[1], out[3], out[4]
    assert set(losses) == {"loss_retina_cls", "loss_retina_reg"} and len(feats) == 5 and len(anchors) == 2
    sum(losses.values()).backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    ev = mt.rpn.loss_evaluator
    return dict(losses={k: float(v) for k, v in losses.items()}, feats=[N(f) for f in feats], logits=[N(c) for c in box_cls],
                deltas=[N(r) for r in box_reg], anchors=[[N(a.bbox) for a in per] for per in anchors],
                labels=np.stack([N(l) for l in ev.last_targets[0]]).astype(np.int64), targets=np.stack([N(t) for t in ev.last_targets[1]]),
                n_pos=int(ev.last_n_pos.item()))


def _gpu_grads(mt, ref_grads):
    """{reference key: the GPU's gradient in the reference's layout}: OHWI -> OIHW for conv weights, padded input channels and the pad row of
    cls_logits dropped (the row is asserted to be exactly zero first).  The tensors that carry a gradient on the GPU are the float64 model's
    trainable set; a frozen tensor has no gradient or an all-zero one."""
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    convs = {id(m.weight): m for m in mt.modules() if isinstance(m, Conv2d)}
    out = {}
    for name, p in mt.named_parameters():
        if not p.requires_grad:
            assert not D.is_trainable(name), name + " is frozen on the GPU"
            assert p.grad is None or not p.grad.any(), name + " is frozen and has a gradient"
            continue
        assert D.is_trainable(name), name + " trains on the GPU"
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
        g, r = p.grad.detach(), ref_grads[name]
        if id(p) in convs:
            conv = convs[id(p)]
            assert not g[conv.out_channels:].any(), name + ": a pad row has a gradient"
            g = g[: conv.out_channels, ..., : conv.in_channels].permute(0, 3, 1, 2)
        elif g.dim() == 1 and g.numel() > r.numel():      # (a bias computed wider than it is stores only its real entries)
            assert not g[r.numel():].any(), name + ": a pad entry has a gradient"
            g = g[: r.numel()]
        out[name] = g.cpu().double().reshape(r.shape)
    return out


def _compare(S, gpu, tag):
    """the float64 model on the model's CURRENT weights: exact checks, value checks, every gradient -> report rows"""
    mt = S["mt"]
    sd = E.cpu_sd(mt)
    # ---------------- exact: anchors, labels, n_pos; the regression targets within their bound
    want_anchors = E.anchors_np()
    for per in gpu["anchors"]:
        assert len(per) == 5 and all(np.array_equal(a, w) for a, w in zip(per, want_anchors)), "the model's anchors"
    tg = RL.batch_targets(np.concatenate(gpu["anchors"][0]), S["gts"], S["gt_labels"])
    assert RL.threshold_margin(tg["per_image"]) >= 1e-4
    assert np.array_equal(gpu["labels"], tg["labels"]), "anchor labels"
    assert gpu["n_pos"] == tg["n_pos"] == int((gpu["labels"] > 0).sum()) > 0 and (gpu["labels"] == -1).any()
    assert np.all(np.abs(gpu["targets"] - tg["targets"]) <= tg["target_bound"]), "regression targets"
    # ---------------- the float64 model
    ref = D.DetectorRetinaNetRef(sd)
    out = D.step(ref, S["cpu_images"], tg["labels"], tg["targets"], not S["use_c5"])
    near = min(min(float(t.detach().abs().min()) for t in out["pre"]), float(out["ps"][3].detach().abs().min()))
    print("closest tower ReLU input / P6 element to zero in the float64 model: %.3e" % near)
    assert near > E.NEAR_ZERO, "the FIXTURE puts a ReLU input within %.1e of zero on these weights: its sign is the arithmetic's to choose" % E.NEAR_ZERO
    for l in range(5):
        _near(gpu["feats"][l], out["ps"][l].detach().numpy(), "P%d" % (l + 3))
        _near(gpu["logits"][l], out["logits"][l].detach().numpy(), "logits, level %d" % l)
        _near(gpu["deltas"][l], out["deltas"][l].detach().numpy(), "deltas, level %d" % l)
    rows = lambda ts: [t.detach().permute(0, 2, 3, 1).reshape(t.shape[0], -1, t.shape[1]).numpy() for t in ts]      # noqa: E731
    want = RL.losses(rows(out["logits"]), rows(out["deltas"]), E.A, E.C, tg["labels"], tg["targets"])
    assert abs(want["cls"] - out["losses"]["loss_retina_cls"]) <= 1e-12 * want["cls"] and abs(want["reg"] - out["losses"]["loss_retina_reg"]) <= 1e-12 * want["reg"]
    print("GPU    ", gpu["losses"])
    print("float64", out["losses"])
    RL.check_losses(gpu["losses"]["loss_retina_cls"], gpu["losses"]["loss_retina_reg"], want, "%s %s %s" % (S["math"], S["v"], tag))
    # ---------------- gradients of every trainable tensor
    head = mt.rpn.head
    assert tuple(head.cls_logits.weight.grad.shape) == (28, 3, 3, 16) and not head.cls_logits.weight.grad[27].any() and not head.cls_logits.bias.grad[27].any()
    rgrads = ref.grads()
    ggrads = _gpu_grads(mt, rgrads)
    assert sorted(ggrads) == sorted(rgrads) == sorted(D.trainable_keys(E.shapes_json()["shapes"][S["v"]]))
    assert len(ggrads) == N_TRAINABLE
    report = []
    for name, r in rgrads.items():
        g = ggrads[name]
        rel = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300)
        rel_l2 = float((g - r).norm()) / max(float(r.norm()), 1e-300)
        report.append((name, rel, rel_l2))
        print("PARITY %-7s %-9s %-62s max-rel %.2e  l2-rel %.2e" % (S["math"], S["v"] + "/" + tag, name, rel, rel_l2))
    print("PARITY-WORST %s %s max-rel %.3e l2-rel %.3e" % (S["math"], S["v"] + "/" + tag, max(r[1] for r in report), max(r[2] for r in report)))
    for name, rel, rel_l2 in report:
        assert rel <= E.GRAD_MAX_REL and rel_l2 <= E.GRAD_REL_L2, f"grad {name}: max-rel {rel}, l2-rel {rel_l2}"
    return report


def test_retinanet_train_step_losses_and_grads_vs_float64(S):
    assert not S["stepped"], "this test needs the fixture's weights: it runs before the step"
    sd_now = E.cpu_sd(S["mt"])
    assert all(torch.equal(sd_now[k], v) for k, v in S["sd"].items()), "the loaded weights do not round-trip"
    _compare(S, _gpu_step(S), "step1")


def _step(S):
    """one FusedSGD step from zero momentum, e2e_retinanet_common.STEP_REL of the weights' norm long, checked against the update rule tensor by
    tensor"""
    from abr_iod_amd.solver.build import FusedSGD
    mt = S["mt"]
    _gpu_step(S)                                     # gradients of the current weights (and every derived copy built)
    n = mt.flat.n_trainable
    lr = E.step_lr(mt.flat.params[:n].norm(), mt.flat.grads.norm())      # (the pad entries of both buffers are zero)
    opt = FusedSGD(mt, lr, E.MOMENTUM, E.rule("weight", lr)[1], E.BIAS_LR_FACTOR, E.BIAS_WD)
    before = {name: (p.detach().clone(), p.grad.detach().clone() if p.requires_grad else None) for name, p in mt.named_parameters()}
    buffers = {name: b.detach().clone() for name, b in mt.named_buffers()}
    flat_before = mt.flat.params[:n].clone()
    opt.step()
    torch.cuda.synchronize()
    S["stepped"] = True
    n_checked, worst = 0, 0.0
    for name, p in mt.named_parameters():
        p0, g0 = before[name]
        if not p.requires_grad:
            assert not D.is_trainable(name) and torch.equal(p.detach(), p0), name + " is frozen and changed"
            continue
        assert D.is_trainable(name), name
        lr_k, wd_k = E.rule(name, lr)      # a key containing "bias": lr x 2 and no weight decay
        p64, g64 = p0.double(), g0.double()
        want = p64 - lr_k * (g64 + wd_k * p64)
        tol = 4 * EPS32 * (p64.abs() + lr_k * (g64.abs() + wd_k * p64.abs()))
        err = (p.detach().double() - want).abs()
        over = float((err - tol).max())
        worst = max(worst, float((err / tol.clamp(min=1e-300)).max()))
        assert over <= 0, "%s after the step: off the update rule by %.3e more than the bound allows" % (name, over)
        assert not torch.equal(p.detach(), p0), name + " did not move"
        n_checked += 1
    moved = float((mt.flat.params[:n] - flat_before).norm() / flat_before.norm())
    print("relative step", moved, "lr", lr, "worst error / bound", worst)
    assert n_checked == N_TRAINABLE and 1e-2 <= moved <= 1e-1, (n_checked, moved)      # large enough to matter to the next forward
    for name, b in mt.named_buffers():
        assert torch.equal(b, buffers[name]), name + " (a buffer) changed"
    head = mt.rpn.head
    assert not head.cls_logits.weight[27].any() and not head.cls_logits.bias[27].any()


def test_retinanet_step_follows_the_update_rule(S):
    assert not S["stepped"]
    _step(S)


# (last: it needs the weights after the step)
def test_retinanet_step_then_forward_vs_float64(S):
    """forward / backward again on the stepped weights: everything derived from the weights (dgrad copies, the library's cached planes) must
    have followed, or the comparison with the float64 model on the NEW weights fails"""
    if not S["stepped"]:
        _step(S)
    sd_now = E.cpu_sd(S["mt"])
    moved = [k for k in D.trainable_keys(S["sd"]) if not torch.equal(sd_now[k], S["sd"][k])]
    assert len(moved) == N_TRAINABLE
    _compare(S, _gpu_step(S), "step2")
    S["mt"].flat.zero_grad()

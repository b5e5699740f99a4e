"""GPU: the RPN loss over a feature pyramid (csrc/rpn_pyramid_loss.hip: abr_rpn_pyramid_loss / _backward; AnchorGenerator.pyramid,
RPNLossComputation and RPNModule.train() over L > 1 levels in modeling/rpn/rpn.py) against the float64 restatement of tests/rpn_fpn_loss_ref.py
and the golden the reference's own code wrote (tests/golden/rpn_fpn_loss.npz).

Bounds are the ones tests/test_gpu_loss_kernels.py uses for the same formulas: losses TOL x (sum of |addends|) / denominator, BCE gradient
8 EPS scale, smooth-L1 gradient 4 EPS scale 10 (rpn_fpn_loss_ref.check_losses / check_grads); everything outside the sampled entries is exactly 0."""
import numpy as np
import pytest
import torch

import rpn_fpn_loss_ref as LR

pytestmark = pytest.mark.gpu

HI, LO, BATCH, FRACTION = 0.7, 0.3, 256, 0.5


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------- kernels
SHAPES = {1: [(5, 7)], 2: [(6, 5), (1, 1)], 5: [(7, 9), (4, 5), (3, 3), (2, 1), (1, 1)],
          8: [(9, 8), (5, 6), (4, 4), (3, 3), (3, 2), (2, 1), (1, 2), (1, 1)]}


def hand_built(seed, L, A, N=3, max_pos=12, batch=24):
    """head outputs (|logit| up to 80, decoys in the pad columns) and a sample that holds, as positives of image 0 and image N - 1, the first
    anchor (a = 0) and the last one (a = A - 1) of EVERY level (the 1 x 1 level included), random further positives and negatives, and an image
    (1) without positives -> dict"""
    rng = np.random.default_rng(seed)
    Cf = (5 * A + 3) // 4 * 4
    nlocs = [h * w for h, w in SHAPES[L]]
    offs = LR.level_offsets(nlocs, A)
    n = int(offs[-1])
    ys = []
    for nloc in nlocs:
        y = np.zeros((N, nloc, Cf), np.float32)
        y[:, :, :A] = (rng.standard_normal((N, nloc, A)) * 4).astype(np.float32)
        y[:, :, A:5 * A] = rng.standard_normal((N, nloc, 4 * A)).astype(np.float32) * 0.3
        y[:, :, 5 * A:] = np.float32(np.nan)          # pad columns are never read
        ys.append(y)
    edges = sorted({int(o) for o in offs[:-1]} | {int(o) - 1 for o in offs[1:]})      # first and last anchor of every level
    tgt = (rng.standard_normal((N, n, 4)) * 0.3).astype(np.float32)
    labels = np.full((N, n), -1, np.float32)
    pos = np.full((N, max(max_pos, len(edges))), -1, np.int64)
    neg = np.full((N, batch), -1, np.int64)
    counts = np.zeros((N, 2), np.int32)
    for i in range(N):
        rest = np.setdiff1d(np.arange(n), edges)
        rng.shuffle(rest)
        p = np.array([], np.int64)
        if i != 1:
            extra = rest[: min(pos.shape[1] - len(edges), max(n // 4 - len(edges), 0), 3 + i)]
            p = np.sort(np.concatenate([edges, extra])).astype(np.int64)
            rest = rest[len(extra):]
        q = np.sort(rest[: min(batch - 2 * i, len(rest))]).astype(np.int64)
        pos[i, :len(p)], neg[i, :len(q)], counts[i] = p + i * n, q + i * n, (len(p), len(q))
        labels[i, p], labels[i, q] = 1, 0
    # extreme logits at sampled entries: a confident right and a confident wrong answer of each sign
    flat_s = np.concatenate([pos[pos >= 0], neg[neg >= 0]])
    i_, l_, loc_, a_ = LR.decode_index(flat_s, n, offs, A)
    for k, v in zip(rng.choice(len(flat_s), 4, replace=False), (80.0, -80.0, 79.5, -33.25)):
        ys[l_[k]][i_[k], loc_[k], a_[k]] = v
    return dict(ys=ys, A=A, Cf=Cf, N=N, n=n, offs=offs, nlocs=nlocs, labels=labels, tgt=tgt, pos=pos, neg=neg, counts=counts,
                shapes=[(N, h, w, Cf) for h, w in SHAPES[L]])


def run_kernels(c, g_obj=1.0, g_box=1.0, want_grad=True):
    from abr_iod_amd import ops
    ys = [cuda(y) for y in c["ys"]]
    pos, neg = cuda(c["pos"]), cuda(c["neg"])
    losses, rec = ops.rpn_pyramid_loss(ys, c["A"], cuda(c["labels"]), cuda(c["tgt"]), pos, neg, cuda(c["counts"]), want_grad=want_grad)
    if not want_grad:
        assert rec is None
        return losses, None
    grads = ops.rpn_pyramid_loss_backward(c["shapes"], c["A"], rec, pos.shape[1], neg.shape[1], torch.tensor(g_obj, device="cuda"),
                                          torch.tensor(g_box, device="cuda"), ys[0].device)
    return losses, grads


def reference(c, g_obj=1.0, g_box=1.0):
    ys = [np.nan_to_num(y, nan=0.0) for y in c["ys"]]
    pos = c["pos"].reshape(-1)
    return LR.losses(ys, c["A"], c["labels"], c["tgt"], pos, np.concatenate([pos, c["neg"].reshape(-1)]), denom=int(c["counts"].sum()),
                     g_obj=g_obj, g_box=g_box)


def as_np(grads):
    return [g.cpu().numpy().reshape(g.shape[0], -1, g.shape[-1]) for g in grads]


@pytest.mark.parametrize("L,A", [(1, 3), (2, 1), (2, 15), (5, 3), (5, 15), (8, 1), (8, 3)])
def test_kernels_against_the_restatement(L, A):
    c = hand_built(100 * L + A, L, A)
    assert c["Cf"] == {1: 8, 3: 16, 15: 76}[A] and c["counts"][1, 0] == 0 and (L == 1 or c["nlocs"][-1] == 1)
    for g_obj, g_box in ((1.0, 1.0), (0.7, -2.0)):
        losses, grads = run_kernels(c, g_obj, g_box)
        ref = reference(c, g_obj, g_box)
        what = "L=%d A=%d upstream (%g, %g)" % (L, A, g_obj, g_box)
        print(what, "losses", losses.tolist(), "float64", ref["obj"], ref["box"])
        LR.check_losses(losses[0].item(), losses[1].item(), ref, what)
        LR.check_grads(as_np(grads), ref, A, what)
        # one allocation, the levels back to back
        base = grads[0].data_ptr()
        for g, shp in zip(grads, c["shapes"]):
            assert g.data_ptr() == base and tuple(g.shape) == shp and g.is_contiguous()
            base += g.numel() * 4
    no_grad, _ = run_kernels(c, want_grad=False)
    assert torch.equal(no_grad, run_kernels(c)[0])


def test_all_padding_gives_zero_loss_and_zero_gradient():
    c = hand_built(7, 5, 3)
    c["pos"][:], c["neg"][:], c["counts"][:] = -1, -1, 0
    losses, grads = run_kernels(c, 0.7, -2.0)
    assert losses.tolist() == [0.0, 0.0]                                   # (denominator max(0, 1) = 1: no 0 / 0)
    assert all(not g.any() for g in grads)
    # one sampled negative alone: the denominator is 1 and the loss is that anchor's term
    c["neg"][2, 0], c["counts"][2, 1] = 2 * c["n"] + c["offs"][3], 1
    c["labels"][2, c["offs"][3]] = 0
    losses, grads = run_kernels(c)
    ref = reference(c)
    assert ref["denom"] == 1
    LR.check_losses(losses[0].item(), losses[1].item(), ref, "one negative")
    LR.check_grads(as_np(grads), ref, 3, "one negative")
    assert sum(int((g != 0).sum()) for g in grads) == 1 and losses[1].item() == 0.0


def test_out_of_range_indices_are_skipped_like_padding():
    c = hand_built(8, 2, 3)
    ref = reference(c)
    assert c["neg"][2, -1] == -1 and c["pos"][1, 0] == -1                 # (both slots are padding: the sample itself is unchanged)
    c["neg"][2, -1] = c["N"] * c["n"] + 5
    c["pos"][1, 0] = 1 << 40
    losses, grads = run_kernels(c)
    LR.check_losses(losses[0].item(), losses[1].item(), ref, "out of range")
    LR.check_grads(as_np(grads), ref, 3, "out of range")


def test_single_level_agrees_with_the_single_level_route():
    """L = 1: the existing _RPNLossFn (bce_logits_gather + smooth_l1_rows + scale_ + add_) on the same sample, both within the bounds"""
    from abr_iod_amd.modeling.rpn.rpn import _RPNLossFn
    c = hand_built(11, 1, 3)
    ref = reference(c, 0.7, -2.0)
    (h, w), N, Cf = SHAPES[1][0], c["N"], c["Cf"]
    fused = cuda(np.nan_to_num(c["ys"][0])).view(N, h, w, Cf).permute(0, 3, 1, 2).requires_grad_(True)
    pos = cuda(c["pos"]).reshape(-1)
    samp = torch.cat([pos, cuda(c["neg"]).reshape(-1)])
    denom = torch.tensor([float(c["counts"].sum())], device="cuda")
    lo, lb = _RPNLossFn.apply(fused, 3, cuda(c["labels"]).view(-1), cuda(c["tgt"]).view(-1, 4), pos, samp, denom, None)
    (0.7 * lo - 2.0 * lb).backward()
    LR.check_losses(lo.item(), lb.item(), ref, "single-level route")
    LR.check_grads([fused.grad.permute(0, 2, 3, 1).reshape(N, h * w, Cf).cpu().numpy()], ref, 3, "single-level route")
    losses, grads = run_kernels(c, 0.7, -2.0)
    LR.check_losses(losses[0].item(), losses[1].item(), ref, "pyramid route, L = 1")
    LR.check_grads(as_np(grads), ref, 3, "pyramid route, L = 1")


def test_results_do_not_depend_on_the_run_or_the_stream():
    c = hand_built(12, 5, 3)
    l0, g0 = run_kernels(c, 0.7, -2.0)
    l1, g1 = run_kernels(c, 0.7, -2.0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        l2, g2 = run_kernels(c, 0.7, -2.0)
    side.synchronize()
    torch.cuda.synchronize()
    for l, g in ((l1, g1), (l2, g2)):
        assert torch.equal(l0, l) and all(torch.equal(a, b) for a, b in zip(g0, g))


def test_wrapper_refuses_malformed_arguments():
    from abr_iod_amd import ops
    c = hand_built(13, 2, 3)
    ys = [cuda(np.nan_to_num(y)) for y in c["ys"]]
    args = (cuda(c["labels"]), cuda(c["tgt"]), cuda(c["pos"]), cuda(c["neg"]), cuda(c["counts"]))
    with pytest.raises(RuntimeError, match="levels"):
        ops.rpn_pyramid_loss(ys * 5, 3, *args)
    with pytest.raises(RuntimeError, match="labels"):
        ops.rpn_pyramid_loss(ys, 3, args[0][:, :-1].contiguous(), *args[1:])
    with pytest.raises(RuntimeError, match="rpn_pyramid_loss"):
        ops.rpn_pyramid_loss([y[:, :, :14].contiguous() for y in ys], 3, *args)         # Cf = 14 < 5 A: the library's own check


# ---------------------------------------------------------------------------------------------------------------------------- golden
@pytest.fixture(scope="module", params=[t for t, _ in LR.CASES])
def case(gold, request):
    c = LR.golden_case(gold("rpn_fpn_loss"), gold("rpn_fpn"), request.param)
    c["straddle"] = dict(LR.CASES)[request.param]
    c["targets64"] = [LR.prepare_targets(c["boxes"], c["vis_cat"][i], c["gt"][i], HI, LO) for i in range(len(c["gt"]))]
    tgt = np.stack([r["targets"] for r in c["targets64"]])
    c["ref"] = LR.losses(c["ys"], c["A"], c["labels"], tgt, c["pos"], c["samp"])
    return c


def evaluator():
    from abr_iod_amd.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.matcher import Matcher
    from abr_iod_amd.modeling.rpn.rpn import RPNLossComputation
    return RPNLossComputation(Matcher(HI, LO, allow_low_quality_matches=True), BalancedPositiveNegativeSampler(BATCH, FRACTION),
                              BoxCoder(weights=(1.0, 1.0, 1.0, 1.0)))


def golden_setup(c):
    """the library's own anchors for the golden's geometry, the head outputs as leaf tensors, the targets"""
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    N = len(LR.IMAGE_SIZES)
    ag = AnchorGenerator(sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(4, 8, 16, 32, 64),
                         straddle_thresh=c["straddle"]).cuda()
    fused = [cuda(y).view(N, H, W, -1).permute(0, 3, 1, 2).requires_grad_(True) for y, (H, W) in zip(c["ys"], LR.MAPS)]
    anchors = ag(ImageList(torch.zeros(N, 3, 128, 192, device="cuda"), list(LR.IMAGE_SIZES)), fused)
    targets = [BoxList(cuda(g), (w, h), mode="xyxy") for g, (h, w) in zip(c["gt"], LR.IMAGE_SIZES)]
    return ag, fused, anchors, targets


def level_grads(fused):
    return [f.grad.permute(0, 2, 3, 1).reshape(f.shape[0], -1, f.shape[1]).cpu().numpy() for f in fused]


def test_anchor_pyramid_is_the_reference_concatenation_and_cached(case):
    ag, fused, anchors, _ = golden_setup(case)
    grids = [f.shape[-2:] for f in fused]
    for i, hw in enumerate(LR.IMAGE_SIZES):
        boxes, vis, offs = ag.pyramid(grids, hw)
        assert np.array_equal(boxes.cpu().numpy(), case["boxes"]) and list(offs) == case["offs"].tolist()
        assert vis.dtype == torch.uint8 and np.array_equal(vis.cpu().numpy(), case["vis_cat"][i])
        again = ag.pyramid(grids, hw)
        assert again[0] is boxes and again[1] is vis and anchors[i][0]._pyramid[0] is boxes      # built once, shared by the images
    assert ag.pyramid(grids, LR.IMAGE_SIZES[0])[0] is ag.pyramid(grids, LR.IMAGE_SIZES[1])[0]


def test_golden_through_the_loss_computation(case):
    _, fused, anchors, targets = golden_setup(case)
    ev = evaluator()
    sampled = (cuda(case["pos"]), cuda(case["samp"]))
    lo, lb = ev(anchors, None, None, targets, fused=fused, sampled=sampled)
    (lo + lb).backward()
    labels, tgts = ev.last_targets
    ref, A = case["ref"], case["A"]
    for i, r in enumerate(case["targets64"]):
        assert np.array_equal(labels[i].cpu().numpy(), case["labels"][i]), i                       # labels: exact
        assert np.all(np.abs(tgts[i].cpu().numpy() - r["targets"]) <= r["target_bound"]), i
    pa = case["pos_all"]
    got_t = torch.stack(tgts).reshape(-1, 4).cpu().numpy()[pa]
    bound = np.concatenate([r["target_bound"] for r in case["targets64"]]).reshape(-1, 4)[pa]
    assert np.all(np.abs(got_t - case["tgt_pos_all"]) <= 2 * bound)                                 # both within `bound` of float64
    print(case["straddle"], "losses", lo.item(), lb.item(), "golden", case["loss_objectness"], case["loss_rpn_box_reg"], "float64", ref["obj"], ref["box"])
    LR.check_losses(lo.item(), lb.item(), ref, "vs restatement")
    assert abs(lo.item() - case["loss_objectness"]) <= 2 * LR.TOL * ref["obj_addends"]              # (the golden is within TOL of float64 too)
    assert abs(lb.item() - case["loss_rpn_box_reg"]) <= 2 * LR.TOL * ref["box_addends"]
    grads = level_grads(fused)
    LR.check_grads(grads, ref, A, "vs restatement")
    d_obj, d_reg = LR.sampled_grads(grads, A, case["n"], case["offs"], case["pos"], case["samp"])
    assert np.all(np.abs(d_obj - case["d_obj"]) <= 2 * 8 * LR.EPS * ref["obj_scale"])
    assert np.all(np.abs(d_reg - case["d_reg"]) <= 2 * 4 * LR.EPS * ref["box_scale"] * 10)
    # introspection: the sample as flat lists, padding -1
    got_pos, got_samp = (t.cpu().numpy() for t in ev.last_sampled)
    assert sorted(got_pos[got_pos >= 0].tolist()) == sorted(case["pos"].tolist())
    assert sorted(got_samp[got_samp >= 0].tolist()) == sorted(case["samp"].tolist())
    # the reference's signature (lists of L objectness / regression tensors) gives the same bits; inject_sampled works like sampled=
    _, fused2, anchors2, _ = golden_setup(case)
    ev.inject_sampled = sampled
    lo2, lb2 = ev(anchors2, [f[:, :A] for f in fused2], [f[:, A:5 * A] for f in fused2], targets)
    (lo2 + lb2).backward()
    assert torch.equal(lo2, lo) and torch.equal(lb2, lb)
    for a, b in zip(fused, fused2):
        assert torch.equal(a.grad, b.grad)


def test_unpinned_sampler(case):
    _, fused, anchors, targets = golden_setup(case)
    ev = evaluator()
    torch.manual_seed(5)
    lo, lb = ev(anchors, None, None, targets, fused=fused)
    pos, samp = (t.cpu().numpy() for t in ev.last_sampled)
    pos, samp = pos[pos >= 0], samp[samp >= 0]
    n, lab = case["n"], case["labels"].reshape(-1)
    assert len(np.unique(samp)) == len(samp) and set(pos.tolist()) <= set(samp.tolist())
    neg = np.setdiff1d(samp, pos)
    for i in range(len(case["gt"])):
        li = case["labels"][i]
        n_pos = min(int((li == 1).sum()), int(BATCH * FRACTION))
        n_neg = min(int((li == 0).sum()), BATCH - n_pos)
        assert int((pos // n == i).sum()) == n_pos and int((neg // n == i).sum()) == n_neg, i
    assert np.all(lab[pos] == 1) and np.all(lab[neg] == 0)
    tgt = np.stack([r["targets"] for r in case["targets64"]])
    LR.check_losses(lo.item(), lb.item(), LR.losses(case["ys"], case["A"], case["labels"], tgt, pos, samp), "unpinned sampler")


# ---------------------------------------------------------------------------------------------------------------------------- module
def fpn_cfg(straddle=-1):
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.MODEL.RPN.USE_FPN = True
    c.MODEL.RPN.ANCHOR_STRIDE, c.MODEL.RPN.ANCHOR_SIZES = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512)
    c.MODEL.RPN.STRADDLE_THRESH = straddle
    c.MODEL.RPN.PRE_NMS_TOP_N_TRAIN, c.MODEL.RPN.POST_NMS_TOP_N_TRAIN, c.MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN = 200, 60, 100
    return c


def module_inputs(gold, C=64):
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    g = gold("rpn_fpn_loss")
    N = len(LR.IMAGE_SIZES)
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(N, C, H, W, generator=gen).cuda() for H, W in LR.MAPS]
    images = ImageList(torch.zeros(N, 3, 128, 192, device="cuda"), list(LR.IMAGE_SIZES))
    gts = [g["gt_%d" % i] for i in range(N)]
    targets = [BoxList(cuda(b), (w, h), mode="xyxy") for b, (h, w) in zip(gts, LR.IMAGE_SIZES)]
    return feats, images, targets, gts


def head_grads(head):
    torch.cuda.synchronize()
    return [t.detach().double().cpu().numpy().copy() for t in (head.fused_weight_grad, head.fused_bias_grad, head.conv.weight.grad, head.conv.bias.grad)]


def zero_head_grads(head):
    for t in (head.fused_weight_grad, head.fused_bias_grad, head.conv.weight.grad, head.conv.bias.grad):
        if t is not None:
            t.zero_()


def test_rpn_module_trains_over_five_maps(gold):
    """RPNModule.train() over a pyramid: two finite losses, proposals with the ground truth appended, rpn_output as lists of five; the shared
    head's gradients are the SUM over the levels of what each level's dense gradient gives through the single-map backward (conv_wgrad and
    bias_grad accumulate into the fused buffers), at the bound the conv tests give a weight gradient (fpn_ref.conv_rule_ok, CONV_TOL_GRAD:
    tests/conv_ref.py holds the float64 formulas, the constant lives with the rule)."""
    import fpn_ref
    from abr_iod_amd.modeling.rpn.rpn import RPNModule
    torch.manual_seed(0)
    m = RPNModule(fpn_cfg(), 64).cuda().train()
    with torch.no_grad():
        for conv in (m.head.cls_logits, m.head.bbox_pred):
            conv.weight.mul_(20)
    feats, images, targets, gts = module_inputs(gold)
    (boxes, losses), anchors, (obj, reg) = m(images, feats, targets)
    assert set(losses) == {"loss_objectness", "loss_rpn_box_reg"} and all(bool(torch.isfinite(v)) for v in losses.values())
    assert len(obj) == len(reg) == 5 and len(anchors) == 2 and all(len(a) == 5 for a in anchors)
    A = m.head.num_anchors
    for o, r, (H, W) in zip(obj, reg, LR.MAPS):
        assert tuple(o.shape) == (2, A, H, W) and tuple(r.shape) == (2, 4 * A, H, W)
    assert len(boxes) == 2
    for b, gt in zip(boxes, gts):
        bb, sc = b.bbox.cpu().numpy(), b.get_field("objectness").cpu().numpy()
        assert len(gt) < len(bb) <= 100 + len(gt) and np.array_equal(bb[-len(gt):], gt) and np.all(sc[-len(gt):] == 1)
    zero_head_grads(m.head)
    (1000.0 * (losses["loss_objectness"] + losses["loss_rpn_box_reg"])).backward()
    multi = head_grads(m.head)
    assert all(np.isfinite(g).all() and np.abs(g).max() > 0 for g in multi)
    # the levels' dense gradients for the SAME sample, then one single-map backward per level
    sampled = m.loss_evaluator.last_sampled
    leaves = [m.head.forward_fused(f).detach().requires_grad_(True) for f in feats]
    lo, lb = m.loss_evaluator(anchors, None, None, targets, fused=leaves, sampled=sampled)
    # (the injected lists are padded to another width, so the sums run in another order: the values agree to rounding, the gradients exactly)
    assert abs(lo.item() - losses["loss_objectness"].item()) <= 1e-5 * abs(lo.item()) and abs(lb.item() - losses["loss_rpn_box_reg"].item()) <= 1e-5 * abs(lb.item())
    (1000.0 * (lo + lb)).backward()
    total = None
    for f, leaf in zip(feats, leaves):
        zero_head_grads(m.head)
        m.head.forward_fused(f).backward(leaf.grad)
        one = head_grads(m.head)
        total = one if total is None else [t + o for t, o in zip(total, one)]
    for name, got, want in zip(("fused weight", "fused bias", "conv weight", "conv bias"), multi, total):
        ok, err, lim = fpn_ref.conv_rule_ok(got, want, fpn_ref.CONV_TOL_GRAD)
        print("%-14s max |want| %.3e  err %.3e  limit %.3e" % (name, np.abs(want).max(), err, lim))
        assert ok, (name, err, lim)


def test_rpn_module_without_targets_raises_both_classes(gold):
    from abr_iod_amd.modeling.rpn.rpn import MissingTargets, RPNModule
    m = RPNModule(fpn_cfg(), 64).cuda().train()
    feats, images, _, _ = module_inputs(gold)
    assert issubclass(MissingTargets, ValueError) and issubclass(MissingTargets, NotImplementedError)
    with pytest.raises(ValueError, match="multi-level RPN loss.*needs targets"):
        m(images, feats, targets=None)
    with pytest.raises(NotImplementedError, match="multi-level RPN loss"):
        m(images, feats)


def test_single_map_keeps_the_single_level_route(gold):
    """one map: RPNModule.train() computes exactly what _RPNLossFn over ops.rpn_targets_batched gives for the injected sample (the route of every
    C4 configuration), through the fused tensor or through a list of one"""
    from abr_iod_amd import ops
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.rpn.rpn import RPNModule, _RPNLossFn
    c = cfg.clone()
    c.MODEL.RPN.PRE_NMS_TOP_N_TRAIN, c.MODEL.RPN.POST_NMS_TOP_N_TRAIN = 200, 60
    torch.manual_seed(0)
    m = RPNModule(c, 64).cuda().train()
    feats, images, targets, _ = module_inputs(gold)
    feat = feats[2]                                     # 8 x 12 at stride 16
    A = m.head.num_anchors
    n = 8 * 12 * A
    gen = torch.Generator().manual_seed(1)
    picks = torch.cat([torch.randperm(n, generator=gen)[:40] + i * n for i in range(2)]).sort().values.cuda()
    m.loss_evaluator.inject_sampled = (picks[::4].contiguous(), picks)
    (_, losses), anchors, _ = m(images, [feat], targets)
    fused = m.head.forward_fused(feat)
    lab, tgt, _keep = ops.rpn_targets_batched(anchors[0][0].bbox, [a[0]._visibility_u8 for a in anchors], [t.bbox for t in targets],
                                              m.loss_evaluator.proposal_matcher.high_threshold, m.loss_evaluator.proposal_matcher.low_threshold,
                                              m.loss_evaluator.box_coder.weights)
    lo, lb = _RPNLossFn.apply(fused, A, lab.view(-1), tgt.view(-1, 4), picks[::4].contiguous(), picks, None, None)
    assert torch.equal(lo, losses["loss_objectness"]) and torch.equal(lb, losses["loss_rpn_box_reg"])
    lo1, lb1 = m.loss_evaluator(anchors, None, None, targets, fused=[fused])
    assert torch.equal(lo1, lo) and torch.equal(lb1, lb)
    assert not hasattr(anchors[0][0], "_pyramid")


# ---------------------------------------------------------------------------------------------------------------------------- end to end
class _Model(torch.nn.Module):
    """backbone + RPN as a model FusedSGD can own (flat parameter storage like GeneralizedRCNN's)"""

    def __init__(self, backbone, rpn):
        super().__init__()
        self.backbone, self.rpn = backbone, rpn
        self.flat = None

    def flatten_parameters(self):
        from abr_iod_amd.modeling._flat import flatten_parameters
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        self.flat = flatten_parameters(self)
        bump_param_version()
        return self.flat


def test_backbone_fpn_rpn_trains_end_to_end(gold):
    """build_backbone("R-50-FPN") -> RPNModule.train() -> sum of the two losses -> backward(): every trainable parameter of the neck and of the
    head gets a finite, non-zero gradient, a FusedSGD step moves each of them, and a second step's losses are finite"""
    from abr_iod_amd.modeling.backbone.backbone import build_backbone
    from abr_iod_amd.modeling.rpn.rpn import RPNModule
    from abr_iod_amd.solver.build import FusedSGD
    from abr_iod_amd.structures.image_list import ImageList
    c = fpn_cfg()
    c.MODEL.BACKBONE.CONV_BODY = "R-50-FPN"
    c.MODEL.RESNETS.BACKBONE_OUT_CHANNELS = 256
    torch.manual_seed(0)
    backbone = build_backbone(c).cuda()
    model = _Model(backbone, RPNModule(c, backbone.out_channels).cuda()).train()
    opt = FusedSGD(model, 0.01, 0.9, 1e-4, 2.0, 0.0)
    _, _, targets, _ = module_inputs(gold)
    gen = torch.Generator().manual_seed(4)
    image = torch.randn(2, 3, 128, 192, generator=gen).cuda()
    images = ImageList(image, list(LR.IMAGE_SIZES))
    watched = {n: p for n, p in model.named_parameters() if p.requires_grad and (n.startswith("backbone.fpn.") or n.startswith("rpn.head."))}
    assert len(watched) >= 16 + 6

    def step():
        opt.zero_grad()
        feats, _ = model.backbone(image)
        assert [tuple(f.shape[-2:]) for f in feats] == list(LR.MAPS)
        (boxes, losses), _, _ = model.rpn(images, list(feats), targets)
        total = losses["loss_objectness"] + losses["loss_rpn_box_reg"]
        total.backward()
        torch.cuda.synchronize()
        return losses

    before = {n: p.detach().cpu().clone() for n, p in watched.items()}
    losses = step()
    assert all(bool(torch.isfinite(v)) for v in losses.values())
    for n, p in watched.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    opt.step()
    torch.cuda.synchronize()
    for n, p in watched.items():
        now = p.detach().cpu()
        assert bool(torch.isfinite(now).all()) and bool((now != before[n]).any()), n
    losses = step()
    assert all(bool(torch.isfinite(v)) for v in losses.values())

"""GPU: the mask head's kernels against tests/golden/mask_head.npz (recorded from the reference's project_masks_on_boxes,
MaskRCNNLossComputation, MaskRCNNC4Predictor, MaskPostProcessor and Masker) and against float64 on the CPU, and one training step of the tiny
160x224 setup with MODEL.MASK_ON against the torch-CPU oracle with a mask branch (tests/mask_ref.py)."""
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24
W, H = 97, 61


def _gold():
    return np.load(os.path.join(GOLD, "mask_head.npz"))


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ targets
@pytest.mark.parametrize("tag", ["u8", "f32"])
@pytest.mark.parametrize("M", [8, 14, 28])
def test_mask_targets_vs_reference(tag, M):
    """bit-exact for uint8 masks, <= 1e-6 absolute for float32 masks: corners ending in .5 (even / odd), boxes outside the image on each side,
    narrower than a pixel, crops smaller and larger than M.  Measured: uint8 0 mismatching pixels at M = 8, 14, 28; float32 at most 1.2e-7.
    (Exactness needed the reference run's operation order -- source index as one fused multiply-add, tap weights multiplied first, taps
    accumulated by a chain of fused multiply-adds: with the nested (1 - l) a + l b form 21 / 198 uint8 pixels differed at M = 14 / 28, some of
    them interior pixels that the reference itself truncates to 0.)"""
    from abr_iod_amd import ops
    g = _gold()
    boxes, inst, want = g["t_boxes"], g["t_masks_" + tag], g["t_%s_M%d" % (tag, M)]
    n = len(boxes)
    masks = [_cuda(inst[i:i + 1]) for i in range(n)]          # one image per box: box i crops instance i
    gts = [_cuda(boxes[i:i + 1]) for i in range(n)]
    rois = torch.cat((torch.arange(n, dtype=torch.float32).view(-1, 1), torch.from_numpy(boxes)), 1).cuda()
    rows = torch.arange(n, device="cuda")
    got = ops.mask_targets(masks, gts, rois, rows, M).cpu().numpy()
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    print("mask targets", tag, M, "max abs err", err.max(), "mismatching pixels", int((err > 0).sum()))
    if tag == "u8":
        assert np.array_equal(got, want)
    else:
        assert err.max() <= 1e-6
    # a padding row gives zeros
    pad = ops.mask_targets(masks, gts, rois, torch.tensor([-1, 0], device="cuda"), M).cpu().numpy()
    assert not pad[0].any() and np.array_equal(pad[1], got[0])


def _loss_fixture():
    g = _gold()
    labels = torch.from_numpy(g["l_labels"])
    props = [g["l_props0"], g["l_props1"]]
    rois = torch.cat([torch.cat((torch.full((len(p), 1), float(i)), torch.from_numpy(p)), 1) for i, p in enumerate(props)]).cuda()
    masks = [_cuda(g["l_masks0"]), _cuda(g["l_masks1"])]
    gts = [_cuda(g["l_gt0"]), _cuda(g["l_gt1"])]
    return g, labels, rois, masks, gts


def test_compaction_matching_and_targets_vs_reference():
    """labels -> compacted positives (ascending, -1 padded, inverse map), each positive matched to its instance by first-maximum IoU,
    targets bit-exact with MaskRCNNLossComputation.prepare_targets"""
    from abr_iod_amd import ops
    g, labels, rois, masks, gts = _loss_fixture()
    K = labels.numel()
    want_rows = (labels > 0).nonzero().flatten()
    P = want_rows.numel()
    for p_max in (P, P + 5, K):
        rows, plab, inv, n_pos = ops.mask_compact_pos(labels.cuda(), p_max)
        assert int(n_pos) == P
        assert torch.equal(rows.cpu()[:P], want_rows) and bool((rows.cpu()[P:] == -1).all()) and bool((plab.cpu()[P:] == -1).all())
        assert torch.equal(plab.cpu()[:P], labels[want_rows])
        want_inv = torch.full((K,), -1, dtype=torch.int64)
        want_inv[want_rows] = torch.arange(P)
        assert torch.equal(inv.cpu(), want_inv)
        t = ops.mask_targets(masks, gts, rois, rows, 14).cpu().numpy()
        assert np.array_equal(t[:P], g["l_targets"]) and not t[P:].any()
    rows, plab, inv, n_pos = ops.mask_compact_pos(labels.cuda(), 3)      # (more positives than slots: the list is cut, nothing out of bounds)
    assert int(n_pos) == 3 and torch.equal(rows.cpu(), want_rows[:3]) and int((inv.cpu() >= 0).sum()) == 3
    x = torch.randn(K, 2, 2, 8, device="cuda")
    rows, _, inv, _ = ops.mask_compact_pos(labels.cuda(), P + 2)
    xg = ops.mask_gather_rows(x, rows)
    assert torch.equal(xg[:P].cpu(), x.cpu()[want_rows]) and not bool(xg[P:].any())
    back = ops.mask_gather_rows(xg, inv).cpu()
    assert torch.equal(back[want_rows], x.cpu()[want_rows]) and not bool(back[labels <= 0].any())


# ------------------------------------------------------------------------------------------------ loss
from mask_loss_check import check_loss as _check_loss  # noqa: E402  (shared with tests/test_gpu_mask_kernels.py)


def test_mask_loss_vs_float64_and_reference():
    g = _gold()
    labels = torch.from_numpy(g["l_labels"])
    lp = labels[labels > 0]
    got = _check_loss(torch.from_numpy(g["l_logits"]), lp, torch.from_numpy(g["l_targets"]), tag="fixture")
    assert abs(got - float(g["l_loss"])) <= 4 * EPS * max(1.0, abs(float(g["l_loss"])))      # (the reference's own fp32 mean)
    # padded rows (label -1) with the device count: same value
    P, K, M, _ = g["l_logits"].shape
    z = torch.cat((torch.from_numpy(g["l_logits"]), torch.randn(3, K, M, M)))
    t = torch.cat((torch.from_numpy(g["l_targets"]), torch.rand(3, M, M)))
    got2 = _check_loss(z, torch.cat((lp, torch.full((3,), -1, dtype=torch.int64))), t, n_pos=P, tag="fixture + padding")
    assert got2 == got


@pytest.mark.parametrize("case", ["|x| up to 80", "P = 0", "P = 1", "label at the last class", "no positives among padded rows", "fractional targets"])
def test_mask_loss_edges(case):
    gen = torch.Generator().manual_seed(11)
    K, M = 21, 14
    if case == "P = 0":
        from abr_iod_amd import ops
        loss, grad = ops.mask_loss(torch.zeros(0, M, M, 24, device="cuda"), K, torch.zeros(0, dtype=torch.int64, device="cuda"),
                                   torch.zeros(0, M, M, device="cuda"), want_grad=True)
        assert float(loss) == 0.0 and grad.numel() == 0
        return
    P = 1 if case == "P = 1" else 7
    x = torch.randn(P, K, M, M, generator=gen) * 3
    labels = torch.randint(1, K, (P,), generator=gen)
    t = (torch.rand(P, M, M, generator=gen) > 0.5).float()
    n_pos = None
    if case == "|x| up to 80":
        x = (torch.rand(P, K, M, M, generator=gen) * 2 - 1) * 80
        x[0, labels[0], 0, :4] = torch.tensor([80.0, -80.0, 0.0, -0.0])
    elif case == "label at the last class":
        labels[:] = K - 1
    elif case == "no positives among padded rows":
        labels[:] = -1
        n_pos = 0
    elif case == "fractional targets":
        t = torch.rand(P, M, M, generator=gen)
    _check_loss(x, labels, t, n_pos=n_pos, tag=case)


# ------------------------------------------------------------------------------------------------ predictor
def _predictor(C, Cm, K, math_name):
    from abr_iod_amd import ops
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import MaskRCNNC4Predictor
    c = cfg.clone()
    c.merge_from_list(["MODEL.ROI_MASK_HEAD.CONV_LAYERS", (Cm,) * 4, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", K])
    pred = MaskRCNNC4Predictor(c, C).cuda()
    pred.math = {"f32": ops.MATH_F32, "f16x3": ops.MATH_F16X3}[math_name]
    return pred


def test_predictor_forward_vs_reference_fixture():
    g = _gold()
    pred = _predictor(64, 16, 5, "f32")
    pred.conv5_mask.load_oihw(_cuda(g["p_conv5_mask.weight"]))
    pred.mask_fcn_logits.load_oihw(_cuda(g["p_mask_fcn_logits.weight"]))
    with torch.no_grad():
        pred.conv5_mask.bias.copy_(_cuda(g["p_conv5_mask.bias"]))
        pred.mask_fcn_logits.bias[:5].copy_(_cuda(g["p_mask_fcn_logits.bias"]))
        got = pred(_cuda(g["p_x"])).cpu().numpy()
    assert got.shape == g["p_logits"].shape
    np.testing.assert_allclose(got, g["p_logits"], rtol=0, atol=64 * EPS * float(np.abs(g["p_logits"]).max()))


def _rel(got, want64, scale):
    ok = scale > 0
    return float(((got.double().cpu() - want64).abs()[ok] / scale[ok]).max())


@pytest.mark.parametrize("shape", [(6, 1024, 64, 21, 4), (6, 2048, 256, 21, 7)], ids=["C1024-h4", "C2048-h7"])
def test_deconv_relu_conv_admitted_per_contraction(shape):
    """Every contraction of the mask branch -- the deconvolution's GEMM (K = C_head), the 1x1 logits conv (K = C_mid), their two input
    gradients (K = K_pad, 4 C_mid) and two weight gradients (K = P M M, P h w) -- against float64 on the CPU, each on the GPU's OWN operands, at
    tests/test_gpu_f16x3_admission.py's rule: with e = max |err| / sum |a||b|, e_f16x3 <= max(2 e_f32, 8 eps) and e_f16x3 <= 32 eps, the fp32
    MFMA route measured beside it.  The passes between them (depth-to-space + bias + ReLU and its backward) are exact elementwise maps and
    are held to equality; the bias gradients are column sums, held to test_gpu_loss_kernels.py's 4 eps of sum |addends|.  C2048-h7 is the
    Mask R-CNN C4 setting's shape (POOLER_RESOLUTION 14 -> 7x7 -> 14x14)."""
    import torch.nn.functional as F
    from abr_iod_amd import ops
    from mask_ref import mask_branch
    P, C, Cm, K, h = shape
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(P, C, h, h, generator=gen).clamp(min=0)        # (layer4's output is a ReLU's)
    gz = torch.randn(P, K, 2 * h, 2 * h, generator=gen)
    b5v, blv = torch.randn(Cm, generator=gen) * 0.1, torch.randn(K, generator=gen) * 0.1
    errs = {}
    ops.x6_range_flags(reset=True)
    for math_name in ("f32", "f16x3"):
        torch.manual_seed(4)       # the same weights in both arithmetics
        pred = _predictor(C, Cm, K, math_name)
        c5, cl, math = pred.conv5_mask, pred.mask_fcn_logits, pred.math
        with torch.no_grad():
            c5.bias.copy_(b5v)
            cl.bias[:K].copy_(blv)
        Kp = cl.weight.shape[0]
        w5, b5 = c5.oihw().cpu().double(), c5.bias.detach().cpu().double()
        wl, bl = cl.oihw().cpu().double(), cl.bias.detach().cpu()[:K].double()
        xh = x.cuda().permute(0, 2, 3, 1).contiguous()
        e = errs[math_name] = {}
        with torch.no_grad():
            # forward: GEMM + depth-to-space + bias + ReLU, then the 1x1 conv on the GPU's t
            t, z = pred._run(xh)
            t64 = F.relu(F.conv_transpose2d(x.double(), w5, b5, stride=2))
            e["deconv GEMM (K = C_head)"] = _rel(t.permute(0, 3, 1, 2), t64, F.conv_transpose2d(x.double().abs(), w5.abs(), b5.abs(), stride=2))
            tg = t.cpu().permute(0, 3, 1, 2).double()
            e["logits conv (K = C_mid)"] = _rel(z[..., :K].permute(0, 3, 1, 2), F.conv2d(tg, wl, bl), F.conv2d(tg.abs(), wl.abs(), bl.abs()))
            assert not bool(z[..., K:].any())
            # backward, stage by stage on the GPU's own operands
            g = torch.zeros(P, 2 * h, 2 * h, Kp)
            g[..., :K] = gz.permute(0, 2, 3, 1)
            g = g.cuda()
            gt = ops.conv_forward(g, cl.dgrad_weight(), 1, 0, math=math)
            e["logits dgrad (K = K_pad)"] = _rel(gt.permute(0, 3, 1, 2), F.conv_transpose2d(gz.double(), wl), F.conv_transpose2d(gz.double().abs(), wl.abs()))
            gy = ops.mask_d2s_bias_relu_backward(gt, t)
            gt_masked = torch.where(t > 0, gt, torch.zeros_like(gt))            # [P,2h,2w,Cm]
            want_gy = gt_masked.view(P, h, 2, h, 2, Cm).permute(0, 1, 3, 2, 4, 5).reshape(P, h, h, 4 * Cm)
            assert torch.equal(gy, want_gy), "depth-to-space backward is an exact map"
            gm = gt_masked.cpu().permute(0, 3, 1, 2).double()
            gx = ops.conv_forward(gy, c5.dgrad_weight(), 1, 0, math=math, w_version=c5.version())
            e["deconv dgrad (K = 4 C_mid)"] = _rel(gx.permute(0, 3, 1, 2), F.conv2d(gm, w5, stride=2), F.conv2d(gm.abs(), w5.abs(), stride=2))
            dw5 = torch.zeros_like(c5.weight)
            ops.conv_wgrad(xh, gy, dw5, 1, 0, math=math)
            gm6 = gm.view(P, Cm, h, 2, h, 2)
            e["deconv wgrad (K = P h w)"] = _rel(c5.ref_layout(dw5), torch.einsum("pchw,pmhywx->cmyx", x.double(), gm6),
                                                  torch.einsum("pchw,pmhywx->cmyx", x.double().abs(), gm6.abs()))
            dwl = torch.zeros_like(cl.weight)
            ops.conv_wgrad(t, g, dwl, 1, 0, math=math)
            e["logits wgrad (K = P M M)"] = _rel(cl.ref_layout(dwl), torch.einsum("pkhw,pmhw->km", gz.double(), tg)[:, :, None, None],
                                                  torch.einsum("pkhw,pmhw->km", gz.double().abs(), tg.abs())[:, :, None, None])
            assert not bool(dwl[K:].any())
            db5, dbl = torch.zeros(Cm, device="cuda"), torch.zeros(Kp, device="cuda")
            ops.bias_grad(gy.view(-1, Cm), db5)
            ops.bias_grad(g, dbl)
            for name, got, rows in (("conv5_mask.bias", db5, gm.permute(0, 2, 3, 1).reshape(-1, Cm)), ("mask_fcn_logits.bias", dbl[:K], gz.double().permute(0, 2, 3, 1).reshape(-1, K))):
                assert bool(((got.double().cpu() - rows.sum(0)).abs() <= 4 * EPS * rows.abs().sum(0) + 1e-30).all()), name + " gradient"
        # the autograd node strings exactly these launches together: its logits are the staged ones, its gradients agree with float64 autograd
        for p_ in pred.parameters():
            p_.grad = torch.zeros_like(p_)
        xg = xh.permute(0, 3, 1, 2).requires_grad_(True)
        zz = pred(xg)
        assert torch.equal(zz.detach(), z[..., :K].permute(0, 3, 1, 2))
        zz.backward(gz.cuda())
        torch.cuda.synchronize()
        assert torch.equal(xg.grad.permute(0, 2, 3, 1), gx)
        x64, w5r, b5r, wlr, blr = (v.clone().requires_grad_(True) for v in (x.double(), w5, b5, wl, bl))
        mask_branch(x64, w5r, b5r, wlr, blr).backward(gz.double())
        for name, got, want in (("conv5_mask.weight", c5.ref_layout(c5.weight.grad), w5r.grad), ("conv5_mask.bias", c5.bias.grad, b5r.grad),
                                ("mask_fcn_logits.weight", cl.ref_layout(cl.weight.grad), wlr.grad), ("mask_fcn_logits.bias", cl.bias.grad[:K], blr.grad),
                                ("input", xg.grad, x64.grad)):
            rel = float((got.double().cpu() - want).abs().max() / want.abs().max())
            assert rel <= 1e-5, (math_name, name, rel)       # (a wiring check; the accuracy is admitted per contraction above)
    for name in errs["f32"]:
        e32, e3 = errs["f32"][name], errs["f16x3"][name]
        print(f"{name}: f32 {e32 / EPS:.2f} ulp   f16x3 {e3 / EPS:.2f} ulp")
    for name in errs["f32"]:
        e32, e3 = errs["f32"][name], errs["f16x3"][name]
        assert e3 <= max(2.0 * e32, 8 * EPS), (name, e3 / EPS, e32 / EPS)
        assert e3 <= 32 * EPS and e32 <= 32 * EPS, (name, e3 / EPS, e32 / EPS)
    assert ops.x6_range_flags(reset=True) == 0


# ------------------------------------------------------------------------------------------------ eval
def test_select_and_paste_vs_reference():
    from abr_iod_amd import ops
    from mask_ref import paste_f64
    g = _gold()
    x = torch.from_numpy(g["e_logits"])
    D, K, M, _ = x.shape
    z = torch.zeros(D, M, M, 8)
    z[..., :K] = x.permute(0, 2, 3, 1)
    prob = ops.mask_select_sigmoid(z.cuda(), K, _cuda(g["e_labels"]))
    assert prob.shape == (D, 1, M, M)
    np.testing.assert_allclose(prob.cpu().numpy(), g["e_prob"], rtol=0, atol=4 * EPS)
    # paste the REFERENCE's probabilities: bit-exact wherever the float64 interpolated value is farther than 1e-6 from the threshold
    ref_prob = torch.from_numpy(g["e_prob"])
    got = ops.mask_paste(ref_prob.cuda(), _cuda(g["e_boxes"]), H, W, 0.5).cpu()
    assert got.dtype == torch.uint8 and got.shape == (D, 1, H, W)
    want = torch.from_numpy(g["e_pasted"])
    excused = 0
    for d in range(D):
        vals, written = paste_f64(ref_prob[d, 0], torch.from_numpy(g["e_boxes"][d]), H, W)
        near = written & ((vals - 0.5).abs() <= 1e-6)
        excused += int(near.sum())
        bad = (got[d, 0] != want[d, 0]) & ~near
        assert not bool(bad.any()), (d, bad.nonzero()[:5].tolist())
    print("paste: excused pixels", excused, "of", D * H * W)
    assert excused <= 1e-3 * D * H * W
    assert bool(want.any()) and int((got != want).sum()) <= excused


# ------------------------------------------------------------------------------------------------ the model
SMALL = ["MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 600, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 100, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 300,
         "MODEL.RPN.POST_NMS_TOP_N_TEST", 150, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 48, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 64]


def _mask_overrides(res):
    """res 7: the voc YAMLs' pooler (7 -> layer4 4x4 -> RESOLUTION 8); res 14: the Mask R-CNN C4 setting (14 -> 7x7 -> RESOLUTION 14)"""
    return ["MODEL.MASK_ON", True, "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", res, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", res,
            "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.0625,), "MODEL.ROI_MASK_HEAD.RESOLUTION", 2 * ((res - 1) // 2 + 1)]


TRAINABLE = ("backbone.body.layer2", "backbone.body.layer3", "rpn.", "roi_heads.")


def _close(a, b, tol=1e-4):
    return abs(a - b) <= tol * max(1.0, abs(b))


def _build(name, math_="f16x3", extra=(), seed=0, res=7):
    from e2e_common import CONFIGS, clamp_targets, needs_source
    from abr_iod_amd.engine.synthetic import _box_masks, build_models, make_cfgs, synthetic_batch
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    task, dist_type, feat, alpha, beta, gamma, label_range, n_old = CONFIGS[name]
    os.environ["ABR_CONV_MATH"] = math_
    try:
        cfg_s, cfg_t = make_cfgs(task, dist_type=dist_type, feat=feat, alpha=alpha, beta=beta, gamma=gamma, overrides=SMALL + _mask_overrides(res) + list(extra))
        torch.manual_seed(seed)
        random.seed(seed)
        ms, mt = build_models(cfg_s, cfg_t, seed=seed, need_source=needs_source(name))
    finally:
        os.environ.pop("ABR_CONV_MATH", None)
    with torch.no_grad():
        g = torch.Generator(device="cuda").manual_seed(5)
        n = mt.flat.n_trainable
        mt.flat.params[:n].mul_(1.0 + 0.05 * torch.randn(n, device="cuda", generator=g))
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=label_range)
    clamp_targets(targets, 224, 160)
    for t in targets:   # uint8 ellipses inside the (clamped) GT boxes
        t.add_field("masks", SegmentationMask(_box_masks(t.bbox.cpu(), 160, 224, "ellipse", torch.uint8).cuda(), (224, 160), mode="mask"))
    return dict(cfg_s=cfg_s, cfg_t=cfg_t, ms=ms, mt=mt, images=images, targets=targets, n_old=n_old, dist_type=dist_type, name=name)


def _ref_mask_targets(det_props, targets, labels_h, M):
    """the reference's per-RoI path on the CPU: IoU argmax -> crop -> resize (the SegmentationMask API, pinned to the reference by
    tests/test_mask_config.py)"""
    from oracle import ops as O  # noqa: F401  (the oracle package is importable here)
    out, off = [], 0
    for p, t in zip(det_props, targets):
        b, gt = p.bbox.cpu(), t.bbox.cpu()
        seg = t.get_field("masks").to("cpu")
        lab = labels_h[off:off + len(b)]
        off += len(b)
        area1 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
        area2 = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
        lt = torch.max(gt[:, None, :2], b[:, :2])
        rb = torch.min(gt[:, None, 2:], b[:, 2:])
        wh = (rb - lt + 1).clamp(min=0)
        inter = wh[..., 0] * wh[..., 1]
        iou = inter / (area1[:, None] + area2 - inter)
        matched = iou.max(0)[1]
        for i in (lab > 0).nonzero().flatten().tolist():
            out.append(seg[int(matched[i])].crop(b[i]).resize((M, M)).get_mask_tensor().float())
    return torch.stack(out) if out else torch.zeros(0, M, M)


@pytest.mark.parametrize("res", [7, 14], ids=["pooler7-M8", "pooler14-M14"])
@pytest.mark.parametrize("name", ["finetune", "15-5"])
def test_mask_step_losses_and_grads_vs_oracle(name, res):
    """all five losses within 1e-4 relative of the oracle with a mask branch, every trainable gradient within test_gpu_r101_step.py's bounds
    (max-rel 3.5e-3, l2-rel 1e-3); soften slot 2 = the predictor on the source head features"""
    from mask_ref import mask_loss as ref_mask_loss, ref_model_with_mask
    from abr_iod_amd.distillation.distillation import calculate_attentive_roi_feature_distillation, calculate_roi_distillation_losses
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import convert_to_roi_format
    from abr_iod_amd.utils.checkpoint import reference_state_dict
    from oracle import torch_ref as R
    S = _build(name, res=res)
    ms, mt, images, targets, cfg = S["ms"], S["mt"], S["images"], S["targets"], S["cfg_t"]
    n_old, dist_type = S["n_old"], S["dist_type"]
    assert cfg.MODEL.ROI_MASK_HEAD.RESOLUTION == (8 if res == 7 else 14) and mt.roi_heads.joint_supported == (res == 7)
    distill = ms is not None
    k_old, k_all = n_old + 1, mt.roi_heads.box.predictor.num_classes
    sd_t = reference_state_dict(mt)
    mt.flat.zero_grad()
    if distill:
        sd_s = reference_state_dict(ms)
        with torch.no_grad():
            soften_result, soft_mask_logits, soften_proposal, feat_s, _, _, _, raf_s = ms.generate_soften_proposal(images)
    loss_dict, feat_t, _, anchors, rpn_out, props, raf_det, _ = mt(images, targets)
    assert sorted(loss_dict) == ["loss_box_reg", "loss_classifier", "loss_mask", "loss_objectness", "loss_rpn_box_reg"]
    total = sum(loss_dict.values())
    gpu = {k: float(v) for k, v in loss_dict.items()}
    if distill:
        target_result, t_mask_logits, raf_t = mt.forward(images, targets, features=feat_t, proposals=soften_proposal)
        l_id = calculate_roi_distillation_losses(soften_result, target_result, dist=dist_type)
        l_ard = calculate_attentive_roi_feature_distillation(raf_s, raf_t, gamma=cfg.DIST.GAMMA)
        total = total + cfg.DIST.ALPHA * l_id + cfg.DIST.BETA * l_ard
        gpu["id"], gpu["ard"] = float(l_id), float(l_ard)
    total.backward()
    torch.cuda.synchronize()

    Ref = ref_model_with_mask()
    ref_t = Ref(sd_t, trainable_prefixes=TRAINABLE)
    img = images.cpu()
    ft = ref_t.backbone(img)
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
    _, x_head = ref_t.head_features(ft, rois, res=res)
    logits, boxreg = ref_t.box_predictor(x_head)
    lc, lbox = R.box_head_loss(logits, boxreg, labels_h, rt_h, dist_type, n_old)
    pos = (labels_h > 0).nonzero().flatten()
    assert len(pos) > 0
    M = cfg.MODEL.ROI_MASK_HEAD.RESOLUTION
    mt_ref = _ref_mask_targets(det_props, targets, labels_h, M)
    sel = mt.roi_heads.mask.last_selection
    assert int(sel["n_pos"]) == len(pos) and torch.equal(sel["pos_rows"].cpu()[:len(pos)], pos)
    assert torch.equal(sel["mask_targets"].cpu()[:len(pos)], mt_ref), "mask targets differ from the per-RoI crop + resize"
    mlog = ref_t.mask_predictor(x_head[pos])
    lm = ref_mask_loss(mlog, labels_h[pos], mt_ref)
    total_r = lc + lbox + lo + lb + lm
    ref = dict(loss_classifier=float(lc), loss_box_reg=float(lbox), loss_objectness=float(lo), loss_rpn_box_reg=float(lb), loss_mask=float(lm))
    if distill:
        ref_s = Ref(sd_s, trainable_prefixes=())
        with torch.no_grad():
            fs = ref_s.backbone(img)
        rois64 = convert_to_roi_format(soften_proposal).cpu()
        with torch.no_grad():
            pooled_s, xs = ref_s.head_features(fs, rois64, res=res)
            zs, bs = ref_s.box_predictor(xs)
            want_soft = ref_s.mask_predictor(xs)
        assert soft_mask_logits is not None and tuple(soft_mask_logits.shape) == tuple(want_soft.shape)
        np.testing.assert_allclose(soft_mask_logits.cpu().numpy(), want_soft.numpy(), rtol=0, atol=1e-4 * float(want_soft.abs().max()))
        pooled_t, xt = ref_t.head_features(ft, rois64, res=res)
        zt, bt = ref_t.box_predictor(xt)
        assert t_mask_logits is not None and tuple(t_mask_logits.shape) == (len(rois64), k_all, M, M)
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
        gq = p.grad
        if id(p) in convs:
            gq = convs[id(p)].ref_layout(gq)
        elif pname.endswith("mask_fcn_logits.bias"):
            gq = gq[:k_all]
        gq = gq.detach().cpu()
        r = rgrads[pname]
        rel = float((gq - r).abs().max()) / max(float(r.abs().max()), 1e-12)
        rel_l2 = float((gq - r).norm() / max(float(r.norm()), 1e-12))
        report.append((pname, rel, rel_l2))
    for pname, rel, rel_l2 in report:
        print(f"  {pname:70s} max-rel {rel:.2e}  l2-rel {rel_l2:.2e}")
    assert len(report) == len(rgrads) == 52 + 4, (len(report), len(rgrads))
    assert sum("roi_heads.mask.predictor" in n_ for n_, _, _ in report) == 4
    for pname, rel, rel_l2 in report:
        assert rel <= 3.5e-3 and rel_l2 <= 1e-3, f"grad {pname}: max-rel {rel}, l2-rel {rel_l2}"


@pytest.mark.parametrize("res", [7, 14], ids=["pooler7-M8", "pooler14-M14"])
def test_mask_train_steps_eval_and_checkpoint_round_trip(res):
    """(pooler 14: the trainer takes the two head passes instead of the joint one, which needs an odd pooler.)  two train_step calls move the new layers with finite losses (loss_mask in the dict); eval returns "mask" equal to the oracle's branch on
    the detections (unpasted and pasted); reference_state_dict round trip; a 16-class load into a 21-class model grows mask_fcn_logits"""
    import math
    from mask_ref import ref_model_with_mask
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import convert_to_roi_format
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict, load_state_dict, reference_state_dict
    S = _build("15-5", res=res)
    ms, mt, cfg, images, targets = S["ms"], S["mt"], S["cfg_t"], S["images"], S["targets"]
    before = {n: p.detach().clone() for n, p in mt.named_parameters() if "roi_heads.mask" in n}
    assert len(before) == 4
    opt = make_optimizer(cfg, mt)
    sch = make_lr_scheduler(cfg, opt)
    seen = []
    for _ in range(2):
        ld, _ = train_step(ms, mt, images, targets, opt, sch, cfg, next_images=images)
        torch.cuda.synchronize()
        assert "loss_mask" in ld and all(math.isfinite(float(v)) for v in ld.values()), ld
        seen.append(float(ld["loss_mask"]))
    assert seen[0] > 0
    assert all(not torch.equal(mt.get_parameter(n).detach(), v) for n, v in before.items())
    # eval
    mt.eval()
    with torch.no_grad():
        result, features, _ = mt(images)
    sd = reference_state_dict(mt)
    ref = ref_model_with_mask()(sd, trainable_prefixes=())
    assert sum(len(r) for r in result) > 0
    rois = convert_to_roi_format(result).cpu()
    labels = torch.cat([r.get_field("labels") for r in result]).cpu()
    with torch.no_grad():
        _, xh = ref.head_features(features[0].cpu().contiguous(), rois, res=res)
        want = ref.mask_predictor(xh).sigmoid()[torch.arange(len(rois)), labels][:, None]
    got = torch.cat([r.get_field("mask") for r in result]).cpu()
    assert got.shape == want.shape
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=0, atol=1e-4)
    mt.roi_heads.mask.post_processor.paste = True
    with torch.no_grad():
        pasted, _, _ = mt(images)
    mt.roi_heads.mask.post_processor.paste = False
    for r in pasted:
        m = r.get_field("mask")
        assert m.dtype == torch.uint8 and tuple(m.shape) == (len(r), 1, 160, 224)
    mt.train()
    # checkpoint round trip and head growth
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    other = build_detection_model(cfg)
    load_reference_state_dict(other, sd)
    back = reference_state_dict(other)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    sd_s = reference_state_dict(ms)
    grown = build_detection_model(cfg)
    load_state_dict(grown, {k: v.cpu() for k, v in sd_s.items()})
    g = reference_state_dict(grown)
    for k in ("roi_heads.mask.predictor.mask_fcn_logits.weight", "roi_heads.mask.predictor.mask_fcn_logits.bias", "roi_heads.box.predictor.cls_score.weight"):
        assert g[k].shape[0] == 21 and torch.equal(g[k][:16], sd_s[k]), k


def test_mask_off_is_unchanged():
    """MASK_ON = False (the default): no mask module, no mask parameter, the soften tuple's third slot stays None"""
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    cfg_s, cfg_t = make_cfgs("15-5", overrides=SMALL)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    assert "mask" not in mt.roi_heads and not any("mask" in n for n, _ in mt.named_parameters())
    assert sum(p.requires_grad for p in mt.parameters()) == 52
    box = mt.roi_heads.box
    assert box.keep_joint_head_features is False and box.last_joint_soft_x is None and mt.roi_heads.joint_supported

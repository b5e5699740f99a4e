"""GPU: the FPN mask head (modeling/roi_heads/mask_head/fpn_mask_head.py + the unshared mode of ROIMaskHead).

MODULE (sections 1-3): ROIMaskHead on the maps, RoI table, positives and masks of tests/mask_head_fpn_ref.py's fixture with the golden's weights,
stage by stage in f32 against the float64 model and the reference's own output (tests/golden/mask_head_fpn.npz).  Bounds: fpn_ref.conv_rule_ok
with one CONV_TOL_* allowance per contraction between the pooled tensor and the compared one (mask_fcn1 1, mask_fcn2 2, the deconvolution 3,
the logits 4; a gradient counts the contractions of its backward path: mask_fcn_logits 1, conv5_mask 2, mask_fcn2 3, mask_fcn1 and the pooled
gradient 4) -- tests/test_gpu_box_head_fpn.py's form.  The pooled rows are bit-equal to the unindexed pooler's; the maps' gradients are
checked against tests/pooler_ref.py's float64 transpose of the GPU's own pooled gradient (roi_align_ref.check, 1e-6 of the sum of |addends|).
f16x3 and bf16x6: every compared tensor within max(2 x the f32 route's own error, 8 eps) of the float64 model, relative to max |expected|.

DETECTOR (sections 4-6): the tiny R-50-FPN + mask configuration on the two images and ground truth of tests/e2e_fpn_common.py with seeded
ellipse masks, one training step against tests/mask_head_fpn_ref.py::MaskDetectorRef in the three arithmetics, eval, the soften entry points."""
import os
import random

import numpy as np
import pytest
import torch
from torch import nn

import detector_fpn_ref as D
import e2e_fpn_common as E
import fpn_ref as R
import mask_head_fpn_ref as MR
import mask_ref
import pooler_ref as P
import rpn_fpn_loss_ref as LR
from abr_iod_amd import ops

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -24
FWD_DEPTH = {"act1": 1, "act2": 2, "logits": 4}
GRAD_DEPTH = {"mask_fcn_logits": 1, "conv5_mask": 2, "mask_fcn2": 3, "mask_fcn1": 4, "pooled": 4}
MATHS = ("bf16x6", "f16x3", "f32")
MASK_SEED = 11


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


class no_sync(object):
    """torch's sync debug mode at "error": any host synchronisation inside raises"""

    def __enter__(self):
        self.before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode(self.before)


def _rule(got, want, tol, what):
    ok, err, lim = R.conv_rule_ok(np.asarray(got), np.asarray(want, np.float64), tol)
    print("%-34s err %.3e  limit %.3e" % (what, err, lim))
    assert ok, (what, err, lim)


@pytest.fixture(scope="module", autouse=True)
def _warm():
    ops.amax_compute(torch.zeros(64, device="cuda"))     # library load
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ 1. module
def _head_cfg():
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", MR.NUM_CLASSES,
                       "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 32, "MODEL.ROI_HEADS.POSITIVE_FRACTION", 0.25] + MR.MASK_CFG)      # p_max = 2 * 8
    return c


class _Head(nn.Module):
    """the golden's extractor + predictor inside ROIMaskHead, as a model FusedSGD can own"""

    def __init__(self, g, math):
        super().__init__()
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import ROIMaskHead
        from abr_iod_amd.utils.checkpoint import load_reference_state_dict
        self.mask = ROIMaskHead(_head_cfg(), 8, None)
        where = {"mask_fcn1": "feature_extractor", "mask_fcn2": "feature_extractor", "conv5_mask": "predictor", "mask_fcn_logits": "predictor"}
        sd = {}
        for n, part in where.items():
            sd["mask.%s.%s.weight" % (part, n)] = torch.from_numpy(g["w_" + n])
            sd["mask.%s.%s.bias" % (part, n)] = torch.from_numpy(g["b_" + n])
        assert load_reference_state_dict(self, sd) == []
        self.cuda()
        self.mask.feature_extractor.math = self.mask.predictor.math = math
        bump_param_version()
        self.flat = None

    def flatten_parameters(self):
        from abr_iod_amd.modeling._flat import flatten_parameters
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        self.flat = flatten_parameters(self)
        bump_param_version()
        return self.flat

    def layers(self):
        fe, pr = self.mask.feature_extractor, self.mask.predictor
        return {"mask_fcn1": fe.mask_fcn1, "mask_fcn2": fe.mask_fcn2, "conv5_mask": pr.conv5_mask, "mask_fcn_logits": pr.mask_fcn_logits}

    def run(self, xs, scene):
        self.mask.train()
        _, _, losses = self.mask(xs, scene["props"], scene["targets"], fused=scene["fused"])
        losses["loss_mask"].backward()
        return losses["loss_mask"]


def _scene(fx):
    """the fixture as ROIMaskHead's training inputs: the sampled set (the whole table: BoxLists for the sizes, the fused table and labels on the
    device) and the ground truth with its masks"""
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    h, w = fx["image"]
    rois = fx["rois"]
    props, targets = [], []
    for b in range(fx["B"]):
        props.append(BoxList(T(np.nan_to_num(rois[rois[:, 0] == b, 1:])), (w, h), mode="xyxy"))
        t = BoxList(T(fx["gt_boxes"][b]), (w, h), mode="xyxy")
        t.add_field("labels", T(fx["gt_labels"][b]))
        t.add_field("masks", SegmentationMask(T(fx["gt_masks"][b]), (w, h), mode="mask"))
        targets.append(t)
    return dict(props=props, targets=targets, fused=dict(labels=T(fx["labels"]), rois=T(rois)))


def _maps(feats, requires_grad=True, tag=False):
    xs = []
    for f in feats:
        t = T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
        if tag:
            ops.amax_carry(t, ops.amax_compute(t.permute(0, 2, 3, 1)))
        xs.append(t.requires_grad_(requires_grad))
    return xs


def _param_grads(head):
    out = {}
    for name, m in head.layers().items():
        out["gw_" + name] = N(m.ref_layout(m.weight.grad))
        out["gb_" + name] = N(m.bias.grad)[: m.out_channels]
    return out


def _run(math, spy=False, tag=False):
    g, fx = np.load(MR.GOLD), MR.fixture()
    head = _Head(g, math)
    xs = _maps(fx["feats"], tag=tag)
    rec, pool_bwd = [], []
    real_w, real_p = ops.conv_wgrad_async, ops.roi_align_pyramid_backward
    if spy:
        def spied_w(x, gy, dw, *a, **k):
            rec.append((N(x), N(gy)))
            return real_w(x, gy, dw, *a, **k)

        def spied_p(grad, rois, *a, **k):
            pool_bwd.append((N(grad), N(k["rows"])))
            return real_p(grad, rois, *a, **k)
        ops.conv_wgrad_async, ops.roi_align_pyramid_backward = spied_w, spied_p
    try:
        loss = head.run(xs, _scene(fx))
        torch.cuda.synchronize()
    finally:
        ops.conv_wgrad_async, ops.roi_align_pyramid_backward = real_w, real_p
    sel = head.mask.last_selection
    out = dict(g=g, fx=fx, head=head, loss=float(loss.detach()), logits=N(head.mask.last_mask_logits), gx=[N(t.grad) for t in xs], rec=rec, pool_bwd=pool_bwd,
               pos_rows=N(sel["pos_rows"]), pos_labels=N(sel["pos_labels"]), n_pos=int(sel["n_pos"]), targets=N(sel["mask_targets"]))
    out.update(_param_grads(head))
    return out


@pytest.fixture(scope="module")
def f32_run():
    """one forward and backward of the golden's head under the fp32 MFMA arithmetic, every operand of every weight gradient kept: shared,
    never modified"""
    return _run(ops.MATH_F32, spy=True)


@pytest.fixture(scope="module")
def model64(f32_run):
    """the float64 model on the golden's weights and targets, back-propagated once: shared, never modified"""
    g, fx = f32_run["g"], f32_run["fx"]
    p = MR.params64(g)
    out = MR.model(fx, p)
    for a in out["acts"]:
        a.retain_grad()
    loss = MR.loss_of(out["logits"], g["labels_pos"], MR.unpack_targets(g))
    loss.backward()
    want = {"logits": out["logits"].detach().numpy(), "act1": out["acts"][0].detach().numpy(), "act2": out["acts"][1].detach().numpy(),
            "pooled": out["pooled"].detach().numpy(), "g_pooled": out["pooled"].grad.numpy(), "loss": float(loss.detach()),
            "gmaps": [m.grad.numpy() for m in out["maps"]]}
    for n in MR.PARAMS:
        want["gw_" + n], want["gb_" + n] = p[n][0].grad.numpy(), p[n][1].grad.numpy()
    return want


def test_selection_and_targets_are_the_fixtures(f32_run):
    r, g, fx = f32_run, f32_run["g"], f32_run["fx"]
    n = fx["n_pos"]
    assert r["n_pos"] == n and np.array_equal(r["pos_rows"], fx["pos_rows"]) and (r["pos_rows"][n:] == -1).all()
    assert np.array_equal(r["pos_labels"][:n], g["labels_pos"])
    assert np.array_equal(r["targets"][:n], MR.unpack_targets(g)), "mask targets differ from the reference's project_masks_on_boxes"


def test_module_stage_by_stage_f32(f32_run, model64):
    r, w, fx = f32_run, model64, f32_run["fx"]
    n, Pm = fx["n_pos"], MR.P_MAX
    (t, g_logits), (xh, g_y), (act1, g2), (pooled, g1) = r["rec"]          # mask_fcn_logits, conv5_mask, mask_fcn2, mask_fcn1: what each wgrad read
    assert pooled.shape == (Pm, 14, 14, 8) and act1.shape == (Pm, 14, 14, 8) and xh.shape == (Pm, 14, 14, 8) and r["logits"].shape == (Pm, 3, 28, 28)
    # the pooled rows: the unindexed pooler's bits on the positives, zeros at the padding, within the float64 bound
    from roi_align_ref import TOL, check
    whole = N(ops.roi_align_pyramid_forward([T(f) for f in fx["feats"]], T(fx["rois"]), P.SCALES, 14, 14, 2, P.K_MIN, P.K_MAX))
    assert np.array_equal(pooled[:n], whole[fx["pos_rows"][:n]]) and not pooled[n:].any()
    rows = fx["pos_rows"][:n]
    want_p, S = P.want_forward(fx["feats"], fx["rois"][rows], fx["lv"][rows], 14, 14, 2)
    check(pooled[:n], want_p, S, "pooled rows")
    nchw = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))      # noqa: E731
    _rule(nchw(act1[:n]), w["act1"], FWD_DEPTH["act1"] * R.CONV_TOL_FWD, "mask_fcn1 + ReLU")
    _rule(nchw(xh[:n]), w["act2"], FWD_DEPTH["act2"] * R.CONV_TOL_FWD, "mask_fcn2 + ReLU")
    _rule(r["logits"][:n], w["logits"], FWD_DEPTH["logits"] * R.CONV_TOL_FWD, "logits")
    assert abs(r["loss"] - w["loss"]) <= 1e-4 * max(1.0, abs(w["loss"])), (r["loss"], w["loss"])
    # padding rows: relu(bias) features in, no loss, exactly zero gradient at every stage
    assert not g_logits[n:].any() and not g_y[n:].any() and not g2[n:].any() and not g1[n:].any()
    for name in MR.PARAMS:
        _rule(r["gw_" + name], w["gw_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "d %s.weight" % name)
        _rule(r["gb_" + name], w["gb_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "d %s.bias" % name)
    (gp, bwd_rows), = r["pool_bwd"]
    assert np.array_equal(bwd_rows, fx["pos_rows"]) and not gp[n:].any()
    _rule(nchw(gp[:n]), w["g_pooled"], GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "d pooled")
    # the maps: the pooler's float64 transpose of the GPU's own pooled gradient
    shapes = [f.shape for f in fx["feats"]]
    for l, (want, S) in enumerate(P.want_backward(gp[:n], fx["rois"][rows], fx["lv"][rows], shapes, 14, 14, 2)):
        check(np.ascontiguousarray(r["gx"][l].transpose(0, 2, 3, 1)), want, S, "d map %d" % l, axes="b,y,x,c", tol=TOL)
        assert (np.abs(r["gx"][l]).max() > 0) == (l < 3)
        _rule(r["gx"][l], w["gmaps"][l], GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "d map %d against the float64 model" % l)


def test_module_against_the_reference_golden_f32(f32_run):
    r, g = f32_run, f32_run["g"]
    n = int(g["n_pos"])
    _rule(r["logits"][:n], g["logits"], FWD_DEPTH["logits"] * R.CONV_TOL_FWD, "golden logits")
    assert abs(r["loss"] - float(g["loss"])) <= 1e-4 * max(1.0, float(g["loss"]))
    for name in MR.PARAMS:
        _rule(r["gw_" + name], g["gw_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "golden d %s.weight" % name)
        _rule(r["gb_" + name], g["gb_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "golden d %s.bias" % name)
    (gp, _), = r["pool_bwd"]
    _rule(np.ascontiguousarray(gp[:n].transpose(0, 3, 1, 2)), g["g_pooled"], GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "golden d pooled")


@pytest.mark.parametrize("math", ["f16x3", "bf16x6"])
def test_other_arithmetics_within_twice_the_fp32_route(math, f32_run, model64):
    """logits, loss and every gradient against the float64 model, error relative to max |expected|: within max(2 x the fp32 MFMA route's own
    error on the same inputs, 8 eps) -- tests/test_gpu_box_head_fpn.py's form.  f16x3 is the default arithmetic."""
    assert ops.DEFAULT_CONV_MATH == "f16x3"
    ops.x6_range_flags(reset=True)
    other = _run({"f16x3": ops.MATH_F16X3, "bf16x6": ops.MATH_BF16X6}[math], tag=True)
    assert ops.x6_range_flags(reset=True) == 0
    n = f32_run["fx"]["n_pos"]
    keys = ["logits", "loss"] + ["g%s_%s" % (k, name) for name in MR.PARAMS for k in "wb"]
    for key in keys:
        w = np.asarray(model64[key], np.float64)
        a, b = np.asarray(f32_run[key], np.float64), np.asarray(other[key], np.float64)
        if key == "logits":
            a, b = a[:n], b[:n]
        scale = float(np.abs(w).max())
        e32, eo = float(np.abs(a - w).max()) / scale, float(np.abs(b - w).max()) / scale
        print("%-20s f32 %.2f eps   %s %.2f eps" % (key, e32 / EPS, math, eo / EPS))
        assert np.isfinite(b).all() and eo <= max(2.0 * e32, 8 * EPS), (key, eo, e32)
    for l in range(4):
        w = model64["gmaps"][l]
        scale = max(float(np.abs(w).max()), 1e-30)
        e32, eo = float(np.abs(f32_run["gx"][l] - w).max()) / scale, float(np.abs(other["gx"][l] - w).max()) / scale
        print("d map %d              f32 %.2f eps   %s %.2f eps" % (l, e32 / EPS, math, eo / EPS))
        assert eo <= max(2.0 * e32, 8 * EPS), (l, eo, e32)


# ------------------------------------------------------------------------------------------------------------------ 2. edges of the module
def test_no_detections_return_empty_fields_without_a_launch(f32_run, monkeypatch):
    from abr_iod_amd.structures.bounding_box import BoxList
    head, fx = f32_run["head"], f32_run["fx"]
    xs = _maps(fx["feats"], requires_grad=False)
    boxes = []
    for _ in range(2):
        b = BoxList(torch.zeros((0, 4), device="cuda"), (192, 128), mode="xyxy")
        b.add_field("labels", torch.zeros((0,), dtype=torch.int64, device="cuda"))
        boxes.append(b)
    called = []
    monkeypatch.setattr(ops.L, "check", lambda *a, **k: called.append(a))
    head.mask.eval()
    try:
        with torch.no_grad():
            x, result, losses = head.mask(xs, boxes)
            soft = head.mask.calculate_soften_label(xs, boxes)
            feats = head.mask.feature_extractor(xs, torch.zeros((0, 5), device="cuda"))
    finally:
        head.mask.train()
    assert called == [] and x is None and losses == {}
    assert all(tuple(r.get_field("mask").shape) == (0, 1, 28, 28) for r in result)
    assert tuple(soft.shape) == (0, 3, 28, 28) and tuple(feats.shape) == (0, 8, 14, 14)


def test_eval_masks_on_given_detections(f32_run, model64):
    """the detections' table through the extractor (no rows list), the predictor and the post-processor: the probabilities of each detection's
    label channel, equal to the float64 model's on the same boxes; pasted with POSTPROCESS_MASKS"""
    from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import MaskPostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    head, fx, g = f32_run["head"], f32_run["fx"], f32_run["g"]
    n = fx["n_pos"]
    rows = fx["pos_rows"][:n]
    h, w = fx["image"]
    boxes = []
    for b in range(2):
        sel = fx["rois"][rows, 0] == b
        bl = BoxList(T(fx["rois"][rows][sel, 1:]), (w, h), mode="xyxy")
        bl.add_field("labels", T(g["labels_pos"][sel]))
        bl.add_field("scores", torch.ones(int(sel.sum()), device="cuda"))
        boxes.append(bl)
    head.mask.eval()
    try:
        with torch.no_grad():
            _, result, _ = head.mask(_maps(fx["feats"], requires_grad=False), boxes)
            head.mask.post_processor = MaskPostProcessor(True, 0.5)
            _, pasted, _ = head.mask(_maps(fx["feats"], requires_grad=False), boxes)
    finally:
        head.mask.post_processor = MaskPostProcessor(False, 0.5)
        head.mask.train()
    prob = np.concatenate([N(r.get_field("mask")) for r in result])
    assert prob.shape == (n, 1, 28, 28) and prob.min() >= 0 and prob.max() <= 1
    want = 1.0 / (1.0 + np.exp(-model64["logits"][np.arange(n), g["labels_pos"]]))
    _rule(prob[:, 0], want, FWD_DEPTH["logits"] * R.CONV_TOL_FWD, "eval probabilities")
    _rule(prob, g["prob"], FWD_DEPTH["logits"] * R.CONV_TOL_FWD, "golden post-processor")
    for r, b in zip(pasted, boxes):
        m = r.get_field("mask")
        assert tuple(m.shape) == (len(b), 1, h, w) and set(np.unique(N(m)).tolist()) <= {0, 1} and bool(m.any())


# ------------------------------------------------------------------------------------------------------------------ 3. optimiser
def test_fused_sgd_moves_mask_fcn_and_refreshes_its_derived_weights(f32_run):
    from abr_iod_amd.modeling.backbone import resnet
    from abr_iod_amd.solver.build import FusedSGD
    g, fx = f32_run["g"], f32_run["fx"]
    head = _Head(g, ops.MATH_F32)
    opt = FusedSGD(head, 0.01, 0.9, 1e-4, 2.0, 0.0)
    fe = head.mask.feature_extractor
    assert [e[0] for e in fe.prep_entries()] == fe.convs() and all(e[2:] == (1, 1, ops.MATH_F32) for e in fe.prep_entries())
    assert fe.mask_fcn1._optimised and fe.mask_fcn2._optimised
    assert all(p.data_ptr() >= head.flat.params.data_ptr() and p.grad is not None for p in head.parameters())
    before = {n: N(p).copy() for n, p in head.named_parameters()}
    scene = _scene(fx)
    opt.zero_grad()
    head.run(_maps(fx["feats"]), scene)
    opt.step()
    torch.cuda.synchronize()
    after = {n: N(p).copy() for n, p in head.named_parameters()}
    assert all(np.isfinite(after[n]).all() and (after[n] != before[n]).any() for n in before)
    assert fe.mask_fcn1._wt_version == fe.mask_fcn2._wt_version == resnet._PARAM_VERSION[0]      # rebuilt by the step's preparation
    # forward and backward on the NEW weights against the float64 model on them: every derived copy followed
    opt.zero_grad()
    xs = _maps(fx["feats"])
    loss = head.run(xs, scene)
    torch.cuda.synchronize()
    p = {n: (m.oihw().cpu().double().requires_grad_(), m.bias.detach().cpu().double()[: m.out_channels].requires_grad_()) for n, m in head.layers().items()}
    out = MR.model(fx, p)
    want = MR.loss_of(out["logits"], g["labels_pos"], MR.unpack_targets(g))
    want.backward()
    n = fx["n_pos"]
    _rule(N(head.mask.last_mask_logits)[:n], out["logits"].detach().numpy(), FWD_DEPTH["logits"] * R.CONV_TOL_FWD, "after a step: logits")
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-4 * max(1.0, float(want.detach()))
    for l in range(3):      # through all four refreshed dgrad copies
        _rule(N(xs[l].grad), out["maps"][l].grad.numpy(), GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "after a step: d map %d" % l)
    assert float(np.abs(N(head.mask.last_mask_logits)[:n] - f32_run["logits"][:n]).max()) > 1e-3      # the new weights really are in use


# ------------------------------------------------------------------------------------------------------------------ 4. detector
def _gt_masks():
    gts, _ = E.gt_arrays()
    return [MR.ellipse_masks(MASK_SEED + i, gts[i], *E.IMAGE_SIZES[i]) for i in range(2)]


@pytest.fixture(scope="module", params=MATHS)
def S(request):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict
    from e2e_common import perturb_trainable
    math = request.param
    os.environ["ABR_CONV_MATH"] = math
    try:
        cfg = make_cfgs("15-5", overrides=E.overrides("cuda") + MR.MASK_CFG)[1]
        _, mt = build_models(None, cfg, seed=0, need_source=False)
    finally:
        os.environ.pop("ABR_CONV_MATH", None)   # read at model construction only
    want = {"bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f32": ops.MATH_F32}[math]
    assert all(m.math == want for m in mt.modules() if hasattr(m, "math")) and mt.roi_heads.mask.feature_extractor.math == want
    sd = E.enrich(E.cpu_sd(mt))
    perturb_trainable(sd, D.trainable_keys(sd))
    assert load_reference_state_dict(mt, sd) == []
    cpu_images = E.make_images()
    images = ImageList(cpu_images.cuda(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    masks = _gt_masks()
    targets = []
    for (h, w), b, l, m in zip(E.IMAGE_SIZES, gts, gt_labels, masks):
        t = BoxList(torch.from_numpy(b).cuda(), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l).cuda())
        t.add_field("masks", SegmentationMask(torch.from_numpy(m).cuda(), (w, h), mode="mask"))
        targets.append(t)
    return dict(math=math, cfg=cfg, mt=mt, images=images, cpu_images=cpu_images, targets=targets, gts=gts, gt_labels=gt_labels, masks=masks)


def _gpu_step(S, sync_free=False):
    """one training step, everything the comparison needs read back; sync_free: the part between the RPN and the losses runs under no_sync"""
    mt, images, targets = S["mt"], S["images"], S["targets"]
    mt.train()
    mt.flat.zero_grad()
    torch.manual_seed(7)
    random.seed(7)
    if sync_free:
        state = mt.forward_begin(images, targets)
        torch.cuda.synchronize()
        with no_sync():       # RPN finish -> box targets -> both poolers -> both heads -> every loss: nothing is read back
            first = mt.forward_finish(state)
        sum(first[0].values()).backward()
        torch.cuda.synchronize()
        return dict(losses={k: float(v) for k, v in first[0].items()}, n_pos=int(mt.roi_heads.mask.last_selection["n_pos"]))
    loss_dict, feats, _, anchors, rpn_out, _, _, _ = mt(images, targets)
    total = sum(loss_dict.values())
    total.backward()
    torch.cuda.synchronize()
    ev, evb = mt.rpn.loss_evaluator, mt.roi_heads.box.loss_evaluator
    det = evb._proposals
    det_rois = np.concatenate([np.concatenate([np.full((len(p), 1), i, np.float32), N(p.bbox)], 1) for i, p in enumerate(det)])
    sel = mt.roi_heads.mask.last_selection
    fe = mt.roi_heads.mask.feature_extractor
    pos_rows = N(sel["pos_rows"])
    live = pos_rows[pos_rows >= 0]
    return dict(losses={k: float(v) for k, v in loss_dict.items()}, total=float(total), feats=feats,
                anchors=[[(N(a.bbox), N(a.get_field("visibility")).astype(bool)) for a in per] for per in anchors],
                rpn_labels=np.stack([N(l) for l in ev.last_targets[0]]), rpn_targets=np.stack([N(t) for t in ev.last_targets[1]]),
                pos_idx=N(ev.last_sampled[0]), samp_idx=N(ev.last_sampled[1]), det_rois=det_rois,
                det_labels=np.concatenate([N(p.get_field("labels")) for p in det]).astype(np.int64),
                det_reg_targets=np.concatenate([N(p.get_field("regression_targets")) for p in det]),
                table=N(sel["rois"]), pos_rows=pos_rows, pos_labels=N(sel["pos_labels"]), n_pos=int(sel["n_pos"]), mask_targets=N(sel["mask_targets"]),
                mask_logits=N(mt.roi_heads.mask.last_mask_logits),
                pos_levels=N(fe.pooler.map_levels(torch.from_numpy(det_rois[live]).cuda())))


def _gpu_grads(mt, ref_grads):
    """{reference key: the GPU's gradient in the reference's layout}"""
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    convs = {id(m.weight): m for m in mt.modules() if isinstance(m, Conv2d)}
    out = {}
    for name, p in mt.named_parameters():
        if not p.requires_grad:
            assert not D.is_trainable(name), name + " is frozen on the GPU"
            continue
        assert D.is_trainable(name), name + " trains on the GPU"
        g, r = p.grad.detach(), ref_grads[name]
        if id(p) in convs:
            g = convs[id(p)].ref_layout(g)
        elif g.dim() == 1 and g.numel() > r.numel():      # (a bias computed wider than it is stores only its real entries)
            g = g[: r.numel()]
        out[name] = g.cpu().double().reshape(r.shape)
    return out


# Gradient bounds, measured, not chosen: 3 x the worst value against the float64 model over the three arithmetics and four runs
# (profiles/mask_head_fpn_parity.txt: max-rel 6.460e-7 on backbone.fpn.fpn_inner1.weight under bf16x6, l2-rel 4.071e-7 on
# roi_heads.box.predictor.bbox_pred.weight; the four runs agreed to every printed digit).  The pyramid backward's atomic order varies from run
# to run and ReLU sign flips are discontinuous: the margin tests/e2e_fpn_common.py takes for the same reason.
GRAD_MAX_REL, GRAD_REL_L2 = 3 * 6.460e-7, 3 * 4.071e-7


def test_mask_detector_train_step_vs_float64(S):
    mt, cfg = S["mt"], S["cfg"]
    gpu = _gpu_step(S)
    # ---------------- exact: the positive set, each positive's level, the mask targets
    labels = gpu["det_labels"]
    R_ = cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE
    p_max = 2 * int(R_ * cfg.MODEL.ROI_HEADS.POSITIVE_FRACTION)
    want_rows, want_labels, _, n_pos = mask_ref.compact_ref(labels, p_max)
    assert np.array_equal(gpu["table"][labels >= 0], gpu["det_rois"][labels >= 0])      # pos_rows index the sampled set's own table
    assert gpu["n_pos"] == n_pos and np.array_equal(gpu["pos_rows"], want_rows) and np.array_equal(gpu["pos_labels"][:n_pos], want_labels[:n_pos])
    rows = want_rows[:n_pos]
    pos_rois = gpu["det_rois"][rows]
    assert n_pos >= 8 and (want_rows[n_pos:] == -1).all()
    assert all((pos_rois[:, 0] == i).any() for i in range(2))
    lv = P.levels(pos_rois)
    assert np.array_equal(gpu["pos_levels"], lv) and len(set(lv.tolist())) >= 3, lv.tolist()
    print("positives", n_pos, "of", p_max, "per level", np.bincount(lv, minlength=4).tolist())
    want_t, matched = mask_ref.targets_ref([torch.from_numpy(m) for m in S["masks"]], S["gts"], gpu["det_rois"], want_rows, MR.M)
    assert np.array_equal(gpu["mask_targets"], want_t.numpy()), "mask targets differ from the per-RoI crop + resize"
    assert 0.05 < float(want_t[:n_pos].mean()) < 0.95
    # ---------------- the float64 model on the GPU's draws
    ref_tgt = []
    for i in range(2):
        boxes = np.concatenate([a for a, _ in gpu["anchors"][i]])
        vis = np.concatenate([v for _, v in gpu["anchors"][i]])
        t = LR.prepare_targets(boxes, vis, S["gts"][i])
        assert np.array_equal(gpu["rpn_labels"][i], t["labels"]), "anchor labels of image %d" % i
        ref_tgt.append(t)
    pos, samp = gpu["pos_idx"][gpu["pos_idx"] >= 0], gpu["samp_idx"][gpu["samp_idx"] >= 0]
    live = labels >= 0
    ref = MR.MaskDetectorRef(E.cpu_sd(mt))
    out = MR.mask_step(ref, S["cpu_images"], pos_rois, want_labels[:n_pos], want_t[:n_pos].numpy(),
                       rpn_labels=np.stack([t["labels"] for t in ref_tgt]), rpn_targets=np.stack([t["targets"] for t in ref_tgt]), pos_idx=pos,
                       samp_idx=samp, det_rois=gpu["det_rois"][live], det_labels=labels[live], det_reg_targets=gpu["det_reg_targets"][live],
                       dist_type=cfg.DIST.TYPE, n_old=15)
    assert np.array_equal(out["mask_levels"], lv)
    print("GPU    ", gpu["losses"], gpu["total"])
    print("float64", out["losses"], out["total"])
    assert set(gpu["losses"]) == set(out["losses"]) and "loss_mask" in out["losses"] and len(out["losses"]) == 5
    for k, v in out["losses"].items():
        assert abs(gpu["losses"][k] - v) <= 1e-4 * max(1.0, abs(v)), f"{k}: gpu {gpu['losses'][k]} vs float64 {v}"
    assert abs(gpu["total"] - out["total"]) <= 1e-4 * max(1.0, abs(out["total"])), (gpu["total"], out["total"])
    err = float(np.abs(gpu["mask_logits"][:n_pos] - out["mask_logits"]).max())
    assert err <= 1e-4 * float(np.abs(out["mask_logits"]).max()), ("mask logits", err)
    # ---------------- gradients of every trainable tensor
    rgrads = ref.grads()
    ggrads = _gpu_grads(mt, rgrads)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mask_head_fpn_state_dict_shapes.json")) as f:
        import json
        keys = D.trainable_keys(json.load(f)["shapes"])
    assert sorted(ggrads) == sorted(rgrads) == sorted(keys) and sum(k.startswith("roi_heads.mask.") for k in keys) == 8
    report = []
    for name, r in rgrads.items():
        g = ggrads[name]
        rel = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300)
        rel_l2 = float((g - r).norm()) / max(float(r.norm()), 1e-300)
        report.append((name, rel, rel_l2))
        print("PARITY %-7s %-62s max-rel %.2e  l2-rel %.2e" % (S["math"], name, rel, rel_l2))
    print("PARITY-WORST %s max-rel %.3e l2-rel %.3e" % (S["math"], max(r[1] for r in report), max(r[2] for r in report)))
    for name, rel, rel_l2 in report:
        assert rel <= GRAD_MAX_REL and rel_l2 <= GRAD_REL_L2, f"grad {name}: max-rel {rel}, l2-rel {rel_l2}"
    mt.flat.zero_grad()


def test_mask_detector_trains_without_a_host_round_trip_between_rpn_and_losses(S):
    mt = S["mt"]
    gpu = _gpu_step(S, sync_free=True)
    assert set(gpu["losses"]) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg", "loss_mask"}
    assert all(np.isfinite(v) for v in gpu["losses"].values()) and gpu["n_pos"] > 0
    for n, p in mt.roi_heads.mask.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
    mt.flat.zero_grad()


# ------------------------------------------------------------------------------------------------------------------ 5. eval
def test_mask_detector_eval_attaches_masks(S):
    from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import MaskPostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    mt = S["mt"]
    mask = mt.roi_heads.mask
    mt.eval()
    try:
        with torch.no_grad():
            result = mt(S["images"])[0]
            mask.post_processor = MaskPostProcessor(True, 0.5)
            pasted = mt(S["images"])[0]
            # an image without a detection among images with some: an empty field
            feats = mt.backbone(S["images"].tensors)[0]
            some = BoxList(result[0].bbox[:3], result[0].size, mode="xyxy")
            some.add_field("labels", result[0].get_field("labels")[:3])
            none = BoxList(result[1].bbox[:0], result[1].size, mode="xyxy")
            none.add_field("labels", result[1].get_field("labels")[:0])
            mask.post_processor = MaskPostProcessor(False, 0.5)
            _, mixed, _ = mask(feats, [some, none])
            torch.cuda.synchronize()
    finally:
        mask.post_processor = MaskPostProcessor(False, 0.5)
        mt.train()
    for det, pst, (h, w) in zip(result, pasted, E.IMAGE_SIZES):
        m = N(det.get_field("mask"))
        assert len(det) > 0 and m.shape == (len(det), 1, 2 * MR.RES, 2 * MR.RES) and np.isfinite(m).all() and m.min() >= 0 and m.max() <= 1
        assert tuple(pst.get_field("mask").shape) == (len(pst), 1, h, w)
    assert tuple(mixed[0].get_field("mask").shape) == (3, 1, 28, 28) and tuple(mixed[1].get_field("mask").shape) == (0, 1, 28, 28)
    assert np.array_equal(N(mixed[0].get_field("mask")), N(result[0].get_field("mask"))[:3])


# ------------------------------------------------------------------------------------------------------------------ 6. soften entry points
def test_soften_entry_points_return_the_float64_mask_logits(S):
    """calculate_soften_label and forward_joint with the unshared head: predictor(extractor(features, proposals)) on the proposals the box
    soften labels use -- this project's definition -- equal to the float64 model's on the same proposals"""
    from abr_iod_amd.structures.bounding_box import BoxList
    mt = S["mt"]
    rng = np.random.default_rng(3)
    props, rois = [], []
    for i, ((h, w), gt) in enumerate(zip(E.IMAGE_SIZES, S["gts"])):
        b = (gt + rng.uniform(-6, 6, gt.shape)).astype(np.float32)
        b[:, 0::2] = np.clip(b[:, 0::2], 0, w - 1)
        b[:, 1::2] = np.clip(b[:, 1::2], 0, h - 1)
        props.append(BoxList(torch.from_numpy(b).cuda(), (w, h), mode="xyxy"))
        rois.append(np.concatenate([np.full((len(b), 1), i, np.float32), b], 1))
    rois = np.concatenate(rois)
    assert len(set(P.levels(rois).tolist())) >= 3
    ref = MR.MaskDetectorRef(E.cpu_sd(mt), trainable=False)
    with torch.no_grad():
        want = ref.mask_head(ref.features(S["cpu_images"]), rois)[0].numpy()
    mt.train()
    torch.manual_seed(9)
    with torch.no_grad():
        first = mt(S["images"], S["targets"])
        (_, _), soft_logits, _ = mt(S["images"], S["targets"], features=first[1], proposals=props)
        torch.manual_seed(9)
        _, ((_, _), joint_logits, _) = mt.forward_joint(S["images"], S["targets"], props)
        empty = mt.roi_heads.mask.calculate_soften_label(first[1], [BoxList(p.bbox[:0], p.size, mode="xyxy") for p in props])
        torch.cuda.synchronize()
    assert tuple(soft_logits.shape) == want.shape == (8, 21, 28, 28) and tuple(empty.shape) == (0, 21, 28, 28)
    for name, got in (("calculate_soften_label", soft_logits), ("forward_joint", joint_logits)):
        err = float(np.abs(N(got) - want).max())
        print("%-24s err %.3e  limit %.3e" % (name, err, 1e-4 * float(np.abs(want).max())))
        assert err <= 1e-4 * float(np.abs(want).max()), (name, err)
    mt.flat.zero_grad()

"""GPU: the FPN keypoint head -- ROIKeypointHead with the pyramid form of KeypointRCNNFeatureExtractor (roi_heads/pyramid_extractor.py) -- alone,
without a backbone, on the scene of tests/keypoint_fpn_ref.py: 2 images of 640 x 512, maps of 16 channels at strides 4 .. 32, pooler 6 -> 24 x 24
heat maps, CONV_LAYERS (16, 16), K = 5 and 17, the golden's weights (tests/golden/keypoint_head_fpn.npz).

Against the float64 model, under f32, bf16x6 and f16x3: fpn_ref.conv_rule_ok with one CONV_TOL_* allowance per contraction between the pooled
tensor and the compared one, counted as tests/test_gpu_mask_head_fpn.py counts them (conv_fcn1 1, conv_fcn2 2, the deconvolution's GEMM and the
logits 3; a gradient counts the contractions of its backward path: kps_score_lowres 1, conv_fcn2 2, conv_fcn1, the pooled gradient and the
maps 3).  loss_kp within 1e-4 * max(1, |ref|).  The selection, every live row's level and the pooled rows are exact.  Against the reference's
own recorded output: tests/test_gpu_keypoint_head.py::test_head_vs_reference_fixture's bounds (64 eps * max |ref| on the logits, 1e-4 on the
loss and the gradients)."""
import numpy as np
import pytest
import torch

import fpn_ref as FR
import keypoint_fpn_ref as KR
import pooler_ref as P
from abr_iod_amd import ops

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
FWD_DEPTH = {"act1": 1, "act2": 2, "logits": 3}
GRAD_DEPTH = {"kps_score_lowres": 1, "conv_fcn2": 2, "conv_fcn1": 3, "pooled": 3}
MATH = {"f32": ops.MATH_F32, "bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3}
LAYERS = KR.BLOCKS + ("kps_score_lowres",)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def _rule(got, want, tol, what):
    ok, err, lim = FR.conv_rule_ok(np.asarray(got), np.asarray(want, np.float64), tol)
    print("%-40s err %.3e  limit %.3e" % (what, err, lim))
    assert ok, (what, err, lim)


@pytest.fixture(scope="module", autouse=True)
def _warm():
    ops.amax_compute(torch.zeros(64, device="cuda"))     # library load
    torch.cuda.synchronize()


def _head(K, g, math):
    """ROIKeypointHead at the scene's sizes with the golden's weights"""
    from abr_iod_amd.config import cfg as base
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    c = base.clone()
    c.merge_from_list(KR.head_cfg_list(K))
    head = build_roi_keypoint_head(c, KR.C)
    dc = head.predictor.kps_score_lowres
    with torch.no_grad():
        for n in KR.BLOCKS:
            conv = getattr(head.feature_extractor, n)
            conv.load_oihw(torch.from_numpy(g["w_" + n]))
            conv.bias.copy_(torch.from_numpy(g["b_" + n]))
        dc.load_oihw(torch.from_numpy(g["w%d_kps_score_lowres" % K]))
        dc.bias.zero_()
        dc.bias[:K].copy_(torch.from_numpy(g["b%d_kps_score_lowres" % K]))
    head.cuda().train()
    head.feature_extractor.math = head.predictor.math = math
    bump_param_version()
    return head


def _inputs(sc, labels=None, fused=True):
    """the scene as ROIKeypointHead's training inputs: the sampled set as BoxLists with "labels" (and, `fused`, as the fused sampler's device
    table), the ground truth with its keypoints"""
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    h, w = sc["image"]
    rois, labels = sc["rois"], sc["labels"] if labels is None else labels
    props, targets = [], []
    for b in range(KR.B):
        on = rois[:, 0] == b
        p = BoxList(T(rois[on, 1:]), (w, h), mode="xyxy")
        p.add_field("labels", T(labels[on]))
        props.append(p)
        t = BoxList(T(sc["gt_boxes"][b]), (w, h), mode="xyxy")
        t.add_field("labels", torch.arange(1, len(sc["gt_boxes"][b]) + 1).cuda())
        t.add_field("keypoints", PersonKeypoints(T(sc["keypoints"][b]), (w, h)))
        targets.append(t)
    return props, targets, (dict(labels=T(labels), rois=T(rois)) if fused else None)


def _maps(feats, requires_grad=True, tag=False):
    xs = []
    for f in feats:
        t = T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
        if tag:
            ops.amax_carry(t, ops.amax_compute(t.permute(0, 2, 3, 1)))
        xs.append(t.requires_grad_(requires_grad))
    return xs


def _run(K, math="f32", spy=False, labels=None, fused=True):
    g, sc = np.load(KR.GOLD), KR.scene(K)
    head = _head(K, g, MATH[math])
    xs = _maps(sc["feats"], tag=math != "f32")
    props, targets, table = _inputs(sc, labels, fused)
    rec, pool_bwd = [], []
    real_w, real_p = ops.conv_wgrad_async, ops.roi_align_pyramid_backward
    if spy:
        def spied_w(x, gy, dw, *a, **k):
            rec.append((N(x), N(gy)))
            return real_w(x, gy, dw, *a, **k)

        def spied_p(grad, rois, *a, **k):
            pool_bwd.append((N(grad), N(rois), N(k["rows"])))
            return real_p(grad, rois, *a, **k)
        ops.conv_wgrad_async, ops.roi_align_pyramid_backward = spied_w, spied_p
    try:
        _, _, losses = head(xs, props, targets, fused=table)
        loss = losses["loss_kp"]
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.conv_wgrad_async, ops.roi_align_pyramid_backward = real_w, real_p
    sel = head.last_selection
    fe, dc = head.feature_extractor, head.predictor.kps_score_lowres
    out = dict(K=K, g=g, sc=sc, head=head, loss=float(loss.detach()), loss_t=loss.detach().clone(), logits=N(head.last_kp_logits),
               gx=[N(t.grad) for t in xs], rec=rec, pool_bwd=pool_bwd, sel={k: N(v) for k, v in sel.items()}, inputs=(props, targets, table))
    for n in KR.BLOCKS:
        conv = getattr(fe, n)
        out["gw_" + n], out["gb_" + n] = N(conv.ref_layout(conv.weight.grad)), N(conv.bias.grad)
    out["gw_kps_score_lowres"], out["gb_kps_score_lowres"] = N(dc.ref_layout(dc.weight.grad)), N(dc.bias.grad)[:K]
    out["pad_w"], out["pad_b"] = N(dc.weight.grad.view(4, 4, dc.kp, KR.LAYERS[-1])[:, :, K:]), N(dc.bias.grad)[K:]
    return out


_RUNS, _MODELS = {}, {}


def _f32_run(K):
    """one forward and backward under the fp32 MFMA arithmetic, every operand of every weight gradient kept: shared, never modified"""
    if K not in _RUNS:
        _RUNS[K] = _run(K, spy=True)
    return _RUNS[K]


def _model64(K):
    """the float64 model on the golden's weights, back-propagated once: shared, never modified"""
    if K not in _MODELS:
        g, sc = np.load(KR.GOLD), KR.scene(K)
        p = KR.params64(g, K)
        out = KR.model(sc, p)
        for a in out["acts"]:
            a.retain_grad()
        out["loss"].backward()
        want = {"logits": out["logits"].detach().numpy(), "act1": out["acts"][0].detach().numpy(), "act2": out["acts"][1].detach().numpy(),
                "pooled": out["pooled"].detach().numpy(), "g_pooled": out["pooled"].grad.numpy(), "loss": float(out["loss"].detach()),
                "gmaps": [m.grad.numpy() for m in out["maps"]]}
        for n in LAYERS:
            want["gw_" + n], want["gb_" + n] = p[n][0].grad.numpy(), p[n][1].grad.numpy()
        _MODELS[K] = want
    return _MODELS[K]


def _against_float64(r, w, what):
    K, n = r["K"], r["sc"]["sel"]["n_pos"]
    _rule(r["logits"][:n], w["logits"], FWD_DEPTH["logits"] * FR.CONV_TOL_FWD, what + " logits")
    print("%s loss_kp %.7f float64 %.7f" % (what, r["loss"], w["loss"]))
    assert abs(r["loss"] - w["loss"]) <= 1e-4 * max(1.0, abs(w["loss"])), (r["loss"], w["loss"])
    for name in LAYERS:
        _rule(r["gw_" + name], w["gw_" + name], GRAD_DEPTH[name] * FR.CONV_TOL_GRAD, "%s d %s.weight" % (what, name))
        _rule(r["gb_" + name], w["gb_" + name], GRAD_DEPTH[name] * FR.CONV_TOL_GRAD, "%s d %s.bias" % (what, name))
    for l in range(4):
        assert float(np.abs(w["gmaps"][l]).max()) > 0
        _rule(r["gx"][l], w["gmaps"][l], GRAD_DEPTH["pooled"] * FR.CONV_TOL_GRAD, "%s d map %d" % (what, l))
    # the padding planes of the deconvolution's GEMM weight and of its bias take exactly zero gradient
    assert r["pad_w"].size == 16 * (ops.kp_pad(K) - K) * KR.LAYERS[-1] and not r["pad_w"].any() and not r["pad_b"].any()


# ------------------------------------------------------------------------------------------------------------------ training
@pytest.mark.parametrize("K", KR.KS)
def test_selection_levels_and_pooled_rows_are_exact(K):
    r = _f32_run(K)
    sc, sel, head = r["sc"], r["sel"], r["head"]
    KR.check_scene(sc)        # every level live, both level boundaries, a dropped instance, a point outside, a dropped image, padding
    want = sc["sel"]
    for key in ("pos_rows", "inv", "targets", "valid"):
        assert np.array_equal(sel[key], want[key]), key
    assert sel["n_pos"].item() == want["n_pos"] and sel["n_valid"].item() == want["n_valid"] > 0
    assert "rois" not in sel and np.array_equal(sel["table"], sc["rois"])       # no gathered table: the rows index the sampled set's own
    n = want["n_pos"]
    rows = want["pos_rows"][:n]
    fe = head.feature_extractor
    lv = N(fe.pooler.map_levels(T(sc["rois"][rows])))
    assert np.array_equal(lv, sc["lv"][rows]) and np.array_equal(lv, r["g"]["levels"]) and np.array_equal(lv, P.levels(sc["rois"][rows]))
    (act2, _), (act1, _), (pooled, g1) = r["rec"]          # kps_score_lowres, conv_fcn2, conv_fcn1: what each weight gradient read
    assert pooled.shape == act1.shape == act2.shape == (KR.P_MAX, KR.RES, KR.RES, 16) and r["logits"].shape == (KR.P_MAX, K, KR.M, KR.M)
    with torch.no_grad():
        by_pooler = N(fe.pooler(_maps(sc["feats"], requires_grad=False), T(sc["rois"]), rows=T(want["pos_rows"])))
    assert np.array_equal(pooled[:n].transpose(0, 3, 1, 2), by_pooler[:n]) and np.abs(by_pooler[:n]).max() > 0
    assert not pooled[n:].any() and not by_pooler[n:].any()
    from roi_align_ref import check
    want_p, S = P.want_forward(sc["feats"], sc["rois"][rows], sc["lv"][rows], KR.RES, KR.RES, KR.SAMPLING)
    check(pooled[:n], want_p, S, "pooled rows")
    # padding rows: relu(bias) features, no gradient at any stage, nothing handed to the pooler's backward
    bias_act = np.maximum(N(fe.conv_fcn1.bias), 0)
    assert np.array_equal(act1[n:], np.broadcast_to(bias_act, act1[n:].shape)) and not g1[n:].any()
    (gp, table, bwd_rows), = r["pool_bwd"]
    assert np.array_equal(bwd_rows, want["pos_rows"]) and np.array_equal(table, sc["rois"]) and not gp[n:].any()


@pytest.mark.parametrize("K", KR.KS)
def test_stage_by_stage_against_float64_f32(K):
    r, w = _f32_run(K), _model64(K)
    n = r["sc"]["sel"]["n_pos"]
    (act2, _), (act1, _), (pooled, _) = r["rec"]
    nchw = lambda a: np.ascontiguousarray(a.transpose(0, 3, 1, 2))      # noqa: E731
    _rule(nchw(act1[:n]), w["act1"], FWD_DEPTH["act1"] * FR.CONV_TOL_FWD, "conv_fcn1 + ReLU")
    _rule(nchw(act2[:n]), w["act2"], FWD_DEPTH["act2"] * FR.CONV_TOL_FWD, "conv_fcn2 + ReLU")
    (gp, _, _), = r["pool_bwd"]
    _rule(nchw(gp[:n]), w["g_pooled"], GRAD_DEPTH["pooled"] * FR.CONV_TOL_GRAD, "d pooled")
    _against_float64(r, w, "f32")
    # the maps: the pooler's float64 transpose of the GPU's own pooled gradient
    from roi_align_ref import TOL, check
    sc = r["sc"]
    rows = sc["sel"]["pos_rows"][:n]
    shapes = [f.shape for f in sc["feats"]]
    for l, (want, S) in enumerate(P.want_backward(gp[:n], sc["rois"][rows], sc["lv"][rows], shapes, KR.RES, KR.RES, KR.SAMPLING)):
        check(np.ascontiguousarray(r["gx"][l].transpose(0, 2, 3, 1)), want, S, "d map %d" % l, axes="b,y,x,c", tol=TOL)


@pytest.mark.parametrize("K", KR.KS)
@pytest.mark.parametrize("math", ["bf16x6", "f16x3"])
def test_other_arithmetics_against_float64(math, K):
    assert ops.DEFAULT_CONV_MATH == "f16x3"
    ops.x6_range_flags(reset=True)
    r = _run(K, math)
    assert ops.x6_range_flags(reset=True) == 0
    assert np.array_equal(r["sel"]["pos_rows"], r["sc"]["sel"]["pos_rows"])
    _against_float64(r, _model64(K), math)


@pytest.mark.parametrize("K", KR.KS)
def test_against_the_reference_fixture(K):
    r, g = _f32_run(K), _f32_run(K)["g"]
    n = r["sc"]["sel"]["n_pos"]
    (act2, _), _, (pooled, _) = r["rec"]
    for got, name in ((pooled, "pooled"), (act2, "features")):
        want = g[name]
        err = float(np.abs(got[:n].transpose(0, 3, 1, 2) - want).max())
        print(name, "max err", err, "bound", 64 * EPS * float(np.abs(want).max()))
        assert err <= 64 * EPS * float(np.abs(want).max()), name
    ref = g["logits%d" % K]
    err = float(np.abs(r["logits"][: len(ref)] - ref).max())
    print("logits: max err", err, "bound", 64 * EPS * float(np.abs(ref).max()))
    assert len(ref) and err <= 64 * EPS * float(np.abs(ref).max())
    want = float(g["loss%d" % K])
    print("loss", r["loss"], "reference", want)
    assert abs(r["loss"] - want) <= 1e-4 * max(1.0, abs(want))
    for name in LAYERS:
        gw = g["gw%d_%s" % (K, name)]
        err = float(np.abs(r["gw_" + name] - gw).max())
        print("grad", name, "weight: max err", err, "of", float(np.abs(gw).max()))
        assert err <= 1e-4 * float(np.abs(gw).max()), name
        gb = g["gb%d_%s" % (K, name)]
        if name == "kps_score_lowres":      # a sum of (softmax - onehot) over whole planes: zero up to rounding, on both sides
            assert float(np.abs(r["gb_" + name]).max()) <= 1e-6 and float(np.abs(gb).max()) <= 1e-6
        else:
            assert float(np.abs(r["gb_" + name] - gb).max()) <= 1e-4 * float(np.abs(gb).max()), name


def test_second_pass_and_the_boxlist_path_reproduce_the_loss_bit_for_bit():
    r = _f32_run(5)
    head, (props, targets, table) = r["head"], r["inputs"]
    xs = _maps(r["sc"]["feats"], requires_grad=False)
    again = head(xs, props, targets, fused=table)[2]["loss_kp"]
    by_boxlists = head(xs, props, targets)[2]["loss_kp"]         # the concatenated table instead of the fused sampler's
    assert torch.equal(again.detach(), r["loss_t"]) and torch.equal(by_boxlists.detach(), r["loss_t"])
    assert np.array_equal(N(head.last_selection["table"]), r["sc"]["rois"])


def test_a_map_no_live_roi_reaches_gets_an_exactly_zero_gradient():
    sc = KR.scene(5)
    labels = sc["labels"].copy()
    labels[sc["lv"] == 3] = 0           # the 448 and the 480 px positives become negatives: nothing is pooled from P5
    r = _run(5, labels=labels)
    rows = r["sel"]["pos_rows"]
    live = rows[rows >= 0]
    assert len(live) == sc["sel"]["n_pos"] - 2 and sorted(set(sc["lv"][live].tolist())) == [0, 1, 2]
    assert all(np.abs(r["gx"][l]).max() > 0 for l in range(3)) and not r["gx"][3].any()
    assert r["loss"] > 0 and np.isfinite(r["loss"])


def test_a_batch_without_a_live_row_gives_zero_loss_and_zero_gradients():
    sc = KR.scene(17)
    labels = sc["labels"].copy()
    labels[sc["rois"][:, 0] == 0] = 0     # only image 1's positives are left, and every one of them is dropped
    assert (labels > 0).sum() >= 2
    r = _run(17, labels=labels, spy=True)
    assert r["sel"]["n_pos"].item() == 0 and r["sel"]["n_valid"].item() == 0 and (r["sel"]["pos_rows"] == -1).all()
    assert r["loss"] == 0.0
    for name in LAYERS:
        assert not r["gw_" + name].any() and not r["gb_" + name].any(), name
    assert not any(gx.any() for gx in r["gx"]) and not r["pad_w"].any() and not r["pad_b"].any()
    assert not r["rec"][-1][0].any()           # the pooled tensor: all padding


# ------------------------------------------------------------------------------------------------------------------ eval
def test_eval_fields_for_zero_one_and_several_detections():
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    K = 17
    r = _f32_run(K)
    head, sc = r["head"], r["sc"]
    h, w = sc["image"]
    xs = _maps(sc["feats"], requires_grad=False)
    # an ordinary box, a degenerate one, one larger than the image; the 448 px boundary box and a small one
    some = [torch.tensor([[10., 20, 100, 140], [50, 60, 51.5, 60.2], [-5, -8, 650, 520]]).cuda(),
            torch.tensor([[180., 40, 627, 487], [300, 300, 330, 340]]).cuda()]
    head.eval()
    try:
        for counts in [(0, 0), (1, 0), (0, 1), (3, 2)]:
            dets = []
            for n, boxes in zip(counts, some):
                b = BoxList(boxes[:n].clone(), (w, h), mode="xyxy")
                b.add_field("scores", torch.ones(n).cuda())
                dets.append(b)
            with torch.no_grad():
                x, out, losses = head(xs, dets)
            assert losses == {} and len(out) == 2 and (x is None) == (sum(counts) == 0)
            for n, res in zip(counts, out):
                kp = res.get_field("keypoints")
                assert isinstance(kp, PersonKeypoints) and tuple(kp.keypoints.shape) == (n, K, 3) and tuple(kp.get_field("logits").shape) == (n, K)
                assert res.has_field("scores") and len(res) == n
                if n:
                    assert torch.all(kp.keypoints[..., 2] == 1) and torch.isfinite(kp.keypoints).all()
                    b = res.bbox
                    bw, bh = (b[:, 2] - b[:, 0]).clamp(min=1)[:, None], (b[:, 3] - b[:, 1]).clamp(min=1)[:, None]
                    assert torch.all(kp.keypoints[..., 0] >= b[:, 0:1]) and torch.all(kp.keypoints[..., 0] <= b[:, 0:1] + bw)
                    assert torch.all(kp.keypoints[..., 1] >= b[:, 1:2]) and torch.all(kp.keypoints[..., 1] <= b[:, 1:2] + bh)
            if sum(counts):
                with torch.no_grad():
                    logits = head.predictor(head.feature_extractor(xs, dets))
                    xy, score = ops.kp_decode(logits, torch.cat([d.bbox for d in dets]))
                assert tuple(x.shape) == (sum(counts), 16, KR.RES, KR.RES) and tuple(logits.shape) == (sum(counts), K, KR.M, KR.M)
                assert torch.equal(torch.cat([o.get_field("keypoints").keypoints for o in out]), xy)
                assert torch.equal(torch.cat([o.get_field("keypoints").get_field("logits") for o in out]), score)
    finally:
        head.train()

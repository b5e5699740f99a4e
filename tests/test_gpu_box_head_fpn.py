"""GPU: the FPN box head.  csrc/box_head_fpn.hip's two entry points (abr_roi_head_targets_table bit for bit against abr_roi_head_targets on
the same candidates and seed; abr_h3_amax_max bit for bit against the levels' words), modeling/roi_heads/box_head/fpn_box_head.py stage by
stage against float64 of the GPU's own input to every stage (fpn_ref.conv_rule_ok at CONV_TOL_FWD / CONV_TOL_GRAD) and end to end against the
reference's FPN2MLPFeatureExtractor + FPNPredictor (tests/golden/box_head_fpn.npz) at one allowance per contraction of the chain, the default
arithmetic (f16x3) at the admission tests' yardstick, the freezes, the optimiser hook-up, and the whole R-50-FPN detector at tiny widths.

The golden holds no gradients of the maps (the reference's ROIAlign backward does not run on the CPU): they are checked against the float64
transpose of tests/pooler_ref.py applied to the GPU's own pooled gradient, which itself is checked against the golden's."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import box_head_fpn_ref as HR
from amax_words import abs_bits, as_float, read_word
import fpn_ref as R
import pooler_ref as P
from abr_iod_amd import ops

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "box_head_fpn.npz")
POOLED = os.path.join(HERE, "golden", "pooler_fpn.npz")
EPS = 2.0 ** -24
FWD_DEPTH = {"x": 2, "cls": 3, "bbox": 3}
GRAD_DEPTH = {"cls_score": 1, "bbox_pred": 1, "fc7": 2, "fc6": 3, "pooled": 3}


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


# ------------------------------------------------------------------------------------------------------------------ 1. targets kernel
WEIGHTS = (10.0, 10.0, 5.0, 5.0)
TENSORS = ("cand", "labels_all", "regt_all", "obj_all", "n_cand", "neg_idx", "counts", "rois", "labels", "reg_targets", "sampled_idx", "n_valid",
           "obj", "pos_rows", "col0")


def _candidates(Nimg, cap, n_gt, seed):
    rng = np.random.default_rng(seed)
    gts, labs = [], []
    for g in n_gt:
        x1, y1 = rng.uniform(0, 60, g), rng.uniform(0, 40, g)
        gts.append(T(np.stack([x1, y1, x1 + rng.uniform(8, 30, g), y1 + rng.uniform(8, 20, g)], 1).astype(np.float32)))
        labs.append(T(rng.integers(1, 5, g).astype(np.int64)))
    rois = np.zeros((Nimg, cap, 4), np.float32)
    for i in range(Nimg):      # a third of the rows are jittered ground truth (positives), the rest anywhere
        base = N(gts[i])[rng.integers(0, n_gt[i], cap)]
        jit = base + rng.uniform(-3, 3, (cap, 4)).astype(np.float32)
        x1, y1 = rng.uniform(0, 70, cap), rng.uniform(0, 45, cap)
        anywhere = np.stack([x1, y1, x1 + rng.uniform(4, 25, cap), y1 + rng.uniform(4, 18, cap)], 1).astype(np.float32)
        rois[i] = np.where((np.arange(cap) % 3 == 0)[:, None], jit, anywhere)
    scores = np.sort(rng.uniform(0, 1, (Nimg, cap)).astype(np.float32), 1)[:, ::-1].copy()
    return T(rois), T(scores), gts, labs


@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("Nimg, cap, n_out, n_gt, Rn, max_pos", [
    (2, 40, [40, 3], [3, 1], 16, 4),     # the second image has fewer candidates than R: padding rows
    (1, 1, [0], [2], 16, 4),             # no proposal at all: the ground-truth rows only
    (2, 40, [40, 3], [3, 1], 16, 0),     # max_pos = 0: negatives only
])
def test_targets_table_equals_keep_path_bit_for_bit(Nimg, cap, n_out, n_gt, Rn, max_pos, agnostic):
    rois, scores, gts, labs = _candidates(Nimg, cap, n_gt, seed=cap + max_pos)
    n_dev = torch.tensor(n_out, dtype=torch.int32).cuda()
    keep = torch.arange(cap, dtype=torch.int32).repeat(Nimg, 1).cuda()      # the identity: candidate j of image i is row j
    args = (gts, labs, 0.5, 0.5, WEIGHTS, Rn, max_pos, 5, agnostic)
    torch.cuda.synchronize()
    with no_sync():
        got = ops.roi_head_targets_table(rois, scores, n_dev, *args, seed=1234)
    want = ops.roi_head_targets(rois, scores, keep, n_dev, *args, seed=1234)
    torch.cuda.synchronize()
    for k in TENSORS:
        a, b = N(got[k]), N(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    if max_pos:      # (with max_pos = 0 the list is never written: one allocated slot per image)
        assert N(got["pos_idx"]).tobytes() == N(want["pos_idx"]).tobytes()
    counts, labels = N(got["counts"]), N(got["labels"]).reshape(Nimg, Rn)
    for i in range(Nimg):
        drawn = int(counts[i].sum())
        if max_pos:      # thresholds 0.5 / 0.5 leave no candidate unlabelled: every candidate is drawn, up to R of them
            assert drawn == min(Rn, n_out[i] + n_gt[i]) and counts[i, 0] > 0
        else:
            assert counts[i, 0] == 0
        assert (labels[i, drawn:] == -1).all() and (labels[i, :drawn] >= 0).all()      # rows past what was drawn are padding
        assert (N(got["rois"]).reshape(Nimg, Rn, 5)[i, :, 0] == i).all()
    assert float(got["n_valid"]) == counts.sum()
    if n_out == [40, 3]:
        assert int((labels[1] == -1).sum()) >= Rn - 4                                     # the short image really ends in padding rows


def test_targets_table_refuses_an_image_without_ground_truth(monkeypatch):
    rois, scores, gts, labs = _candidates(2, 8, [2, 1], seed=0)
    gts[1], labs[1] = gts[1][:0], labs[1][:0]
    called = []
    monkeypatch.setattr(ops.L, "check", lambda *a, **k: called.append(a))
    with pytest.raises(ValueError, match="No ground-truth boxes"):
        ops.roi_head_targets_table(rois, scores, torch.tensor([8, 8], dtype=torch.int32).cuda(), gts, labs, 0.5, 0.5, WEIGHTS, 16, 4, 5)
    assert called == []


# ------------------------------------------------------------------------------------------------------------------ 2. amax bound
def _word(t):
    """the amax bits behind t's tag, read back; the word must carry the tag's epoch"""
    w, e = ops.amax_of(t)
    assert w is not None
    epoch, bits = read_word(w)
    assert epoch == e, "the word does not carry the tag's epoch"
    return bits


@pytest.mark.parametrize("L", [1, 2, 5])
def test_amax_bound_is_the_largest_level_word(L):
    rng = np.random.default_rng(L)
    scales = [0.5, 3.0, 0.01, 7.5, 2.0][:L]
    srcs = [ops.amax_compute(T((s * rng.standard_normal((2, 5 + l, 3, 8))).astype(np.float32))) for l, s in enumerate(scales)]
    dst = torch.zeros(4, 8, device="cuda")
    ops.amax_bound_levels(dst, srcs)
    want = max(_word(s) for s in srcs)
    assert _word(dst) == want == max(abs_bits(s) for s in srcs)
    # one level without a tag: the result has none either
    bare = torch.zeros(4, 8, device="cuda")
    ops.amax_bound_levels(bare, srcs[:-1] + [torch.ones(2, 2, device="cuda")])
    assert ops.amax_of(bare)[0] is None
    assert ops.L.lib().abr_h3_amax_max(None, None, 0, None, 0, ops.L.stream()) != 0       # L = 0: refused before any launch


def _pyramid_inputs():
    pg = np.load(POOLED)
    B, C = int(pg["B"]), int(pg["C"])
    maps = [tuple(int(v) for v in m) for m in pg["maps"]]
    feats = P.make_feats(int(pg["seed"]), B, C, maps)
    return pg, feats, pg["rois"]


def test_pooler_tags_its_output_and_keeps_its_values():
    from abr_iod_amd.modeling.poolers import Pooler
    pg, feats, rois = _pyramid_inputs()
    pooler = Pooler((7, 7), P.SCALES, 2)
    plain = [T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last) for f in feats]
    tagged = [T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last) for f in feats]
    for t in tagged:
        ops.amax_carry(t, ops.amax_compute(t.permute(0, 2, 3, 1)))
        assert ops.amax_of(t)[0] is not None
    a, b = pooler(plain, T(rois)), pooler(tagged, T(rois))
    assert ops.amax_of(a)[0] is None and ops.amax_of(b)[0] is not None
    assert N(a).tobytes() == N(b).tobytes() and np.array_equal(N(b), pg["out"])
    assert as_float(_word(b)) == max(float(np.abs(f).max()) for f in feats) >= float(b.abs().max())
    tagged[2] = plain[2]
    assert ops.amax_of(pooler(tagged, T(rois)))[0] is None


# ------------------------------------------------------------------------------------------------------------------ 3. module
def _head_cfg(extra=()):
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", HR.RES, "MODEL.ROI_BOX_HEAD.POOLER_SCALES",
                       P.SCALES, "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", HR.SAMPLING, "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", HR.DIM,
                       "MODEL.ROI_BOX_HEAD.NUM_CLASSES", HR.NUM_CLASSES] + list(extra))
    return c


class _Head(nn.Module):
    """the golden's extractor + predictor as a model FusedSGD can own"""

    def __init__(self, g, math, extra=()):
        super().__init__()
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        from abr_iod_amd.modeling.roi_heads.box_head.fpn_box_head import FPN2MLPFeatureExtractor, FPNPredictor
        c = _head_cfg(extra)
        self.feature_extractor = FPN2MLPFeatureExtractor(c, 8)
        self.predictor = FPNPredictor(c, self.feature_extractor.out_channels)
        fe, pr = self.feature_extractor, self.predictor
        with torch.no_grad():
            for fc, name in ((fe.fc6, "fc6"), (fe.fc7, "fc7")):
                fc.load_oihw(torch.from_numpy(g["w_" + name]))
                fc.bias.copy_(torch.from_numpy(g["b_" + name]))
            for lin, name in ((pr.cls_score, "cls_score"), (pr.bbox_pred, "bbox_pred")):
                lin.weight.copy_(torch.from_numpy(g["w_" + name]))
                lin.bias.copy_(torch.from_numpy(g["b_" + name]))
        self.cuda()
        fe.math = math
        bump_param_version()
        self.flat = None

    def flatten_parameters(self):
        from abr_iod_amd.modeling._flat import flatten_parameters
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        self.flat = flatten_parameters(self)
        bump_param_version()
        return self.flat

    def run(self, xs, rois, g_cls, g_bbox):
        x, pooled = self.feature_extractor(xs, rois)
        cls, bbox = self.predictor(x)
        if pooled.requires_grad:
            pooled.retain_grad()
        ((cls * g_cls).sum() + (bbox * g_bbox).sum()).backward()
        return x, pooled, cls, bbox


def _maps(feats, requires_grad=True, tag=False):
    xs = []
    for f in feats:
        t = T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last)
        if tag:
            ops.amax_carry(t, ops.amax_compute(t.permute(0, 2, 3, 1)))
        xs.append(t.requires_grad_(requires_grad))
    return xs


def _param_grads(head):
    fe, pr = head.feature_extractor, head.predictor
    out = {}
    for name, m in (("fc6", fe.fc6), ("fc7", fe.fc7)):
        out["gw_" + name] = None if m.weight.grad is None else N(m.ref_layout(m.weight.grad))
        out["gb_" + name] = None if m.bias.grad is None else N(m.bias.grad)
    for name, m in (("cls_score", pr.cls_score), ("bbox_pred", pr.bbox_pred)):
        out["gw_" + name] = None if m.weight.grad is None else N(m.weight.grad)
        out["gb_" + name] = None if m.bias.grad is None else N(m.bias.grad)
    return out


def _run(math, extra=(), spy=False, tag=False):
    g = np.load(GOLD)
    pg, feats, rois = _pyramid_inputs()
    head = _Head(g, math, extra)
    xs = _maps(feats, tag=tag)
    rec = []
    real = ops.conv_wgrad_async
    if spy:
        def spied(x, gy, dw, *a, **k):
            rec.append((N(x), N(gy)))
            return real(x, gy, dw, *a, **k)
        ops.conv_wgrad_async = spied
    try:
        x, pooled, cls, bbox = head.run(xs, T(rois), T(g["g_cls"]), T(g["g_bbox"]))
        torch.cuda.synchronize()
    finally:
        ops.conv_wgrad_async = real
    out = dict(g=g, pg=pg, feats=feats, rois=rois, head=head, x=N(x), pooled=N(pooled), cls=N(cls), bbox=N(bbox), g_pooled=N(pooled.grad),
               gx=[N(t.grad) for t in xs], rec=rec, pooled_tag=ops.amax_of(pooled)[0])
    out.update(_param_grads(head))
    return out


@pytest.fixture(scope="module")
def f32_run():
    """one forward and backward of the golden's head under the fp32 MFMA arithmetic, every operand of every weight gradient kept: shared,
    never modified"""
    return _run(ops.MATH_F32, spy=True)


def test_module_stage_by_stage_f32(f32_run):
    r = f32_run
    p = HR.params64(r["g"])
    K = r["pooled"].shape[0]
    assert r["pooled"].shape == (K, 8, 7, 7) and r["x"].shape == (K, HR.DIM)
    assert np.array_equal(r["pooled"], r["pg"]["out"])                        # the pooler's bits (tests/test_gpu_pooler.py)
    (xr, g), (h6, g7), (flat, g6) = r["rec"]                                  # predictor, fc7, fc6: what each weight gradient read
    assert np.array_equal(flat.reshape(K, 7, 7, 8), r["pooled"].transpose(0, 2, 3, 1)) and np.array_equal(xr.reshape(K, -1), r["x"])
    flat_ref = r["pooled"].astype(np.float64).reshape(K, -1)
    h6, xr, g, g7, g6 = (a.reshape(K, -1).astype(np.float64) for a in (h6, xr, g, g7, g6))
    # forward, every stage on the GPU's own input to it
    _rule(h6, np.maximum(flat_ref @ p["fc6"][0].T + p["fc6"][1], 0), R.CONV_TOL_FWD, "fc6 + ReLU")
    _rule(xr, np.maximum(h6 @ p["fc7"][0].T + p["fc7"][1], 0), R.CONV_TOL_FWD, "fc7 + ReLU")
    _rule(r["cls"], xr @ p["cls_score"][0].T + p["cls_score"][1], R.CONV_TOL_FWD, "cls_score")
    _rule(r["bbox"], xr @ p["bbox_pred"][0].T + p["bbox_pred"][1], R.CONV_TOL_FWD, "bbox_pred")
    # backward
    nc = HR.NUM_CLASSES
    assert np.array_equal(g[:, :nc], r["g"]["g_cls"]) and np.array_equal(g[:, nc:5 * nc], r["g"]["g_bbox"]) and not g[:, 5 * nc:].any()
    _rule(r["gw_cls_score"], g[:, :nc].T @ xr, R.CONV_TOL_GRAD, "d cls_score.weight")
    _rule(r["gw_bbox_pred"], g[:, nc:5 * nc].T @ xr, R.CONV_TOL_GRAD, "d bbox_pred.weight")
    _rule(r["gb_cls_score"], g[:, :nc].sum(0), R.CONV_TOL_GRAD, "d cls_score.bias")
    _rule(r["gb_bbox_pred"], g[:, nc:5 * nc].sum(0), R.CONV_TOL_GRAD, "d bbox_pred.bias")
    _rule(g7, (g[:, :nc] @ p["cls_score"][0] + g[:, nc:5 * nc] @ p["bbox_pred"][0]) * (xr > 0), R.CONV_TOL_GRAD, "d fc7 output (masked)")
    _rule(r["gw_fc7"], g7.T @ h6, R.CONV_TOL_GRAD, "d fc7.weight")
    _rule(r["gb_fc7"], g7.sum(0), R.CONV_TOL_GRAD, "d fc7.bias")
    _rule(g6, (g7 @ p["fc7"][0]) * (h6 > 0), R.CONV_TOL_GRAD, "d fc6 output (masked)")
    _rule(r["gw_fc6"], g6.T @ flat_ref, R.CONV_TOL_GRAD, "d fc6.weight (reference layout)")
    _rule(r["gb_fc6"], g6.sum(0), R.CONV_TOL_GRAD, "d fc6.bias")
    _rule(r["g_pooled"], (g6 @ p["fc6"][0]).reshape(r["pooled"].shape), R.CONV_TOL_GRAD, "d pooled")
    # the maps: the pooler's float64 transpose of the GPU's own pooled gradient
    from roi_align_ref import TOL, check
    gp = np.ascontiguousarray(r["g_pooled"].transpose(0, 2, 3, 1))
    shapes = [f.shape for f in r["feats"]]
    for l, (want, S) in enumerate(P.want_backward(gp, r["rois"], P.levels(r["rois"]), shapes, 7, 7, 2)):
        check(np.ascontiguousarray(r["gx"][l].transpose(0, 2, 3, 1)), want, S, "d map %d" % l, axes="b,y,x,c", tol=TOL)
        assert np.abs(r["gx"][l]).max() > 0


def test_module_against_the_reference_golden_f32(f32_run):
    r, g = f32_run, f32_run["g"]
    for key in ("x", "cls", "bbox"):
        _rule(r[key], g[key], FWD_DEPTH[key] * R.CONV_TOL_FWD, "golden " + key)
    for name in HR.PARAMS:
        _rule(r["gw_" + name], g["gw_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "golden d %s.weight" % name)
        _rule(r["gb_" + name], g["gb_" + name], GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "golden d %s.bias" % name)
    _rule(r["g_pooled"], g["g_pooled"], GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "golden d pooled")


def test_no_rois_returns_empty_without_a_launch(monkeypatch):
    g = np.load(GOLD)
    _, feats, _ = _pyramid_inputs()
    head = _Head(g, ops.MATH_F32)
    xs = _maps(feats, requires_grad=False)
    called = []
    monkeypatch.setattr(ops.L, "check", lambda *a, **k: called.append(a))
    x, pooled = head.feature_extractor(xs, torch.zeros((0, 5), device="cuda"))
    cls, bbox = head.predictor(x)
    assert called == []
    assert tuple(x.shape) == (0, HR.DIM) and tuple(pooled.shape) == (0, 8, 7, 7) and tuple(cls.shape) == (0, 5) and tuple(bbox.shape) == (0, 20)
    y = head.predictor(torch.zeros((0, HR.DIM, 1, 1), device="cuda"))      # [K,D,1,1] is accepted too
    assert tuple(y[0].shape) == (0, 5)


def test_predictor_accepts_both_input_shapes(f32_run):
    head = f32_run["head"]
    x = T(f32_run["x"])
    with torch.no_grad():
        a = head.predictor(x)
        b = head.predictor(x.view(x.shape[0], -1, 1, 1))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and np.array_equal(N(a[0]), f32_run["cls"])
    with pytest.raises(ValueError, match=r"\[K,D\] or \[K,D,1,1\]"):
        head.predictor(torch.zeros((2, HR.DIM, 2, 2), device="cuda"))


# ------------------------------------------------------------------------------------------------------------------ 4. default arithmetic
def test_default_arithmetic_f16x3_within_twice_the_fp32_route(f32_run):
    """logits and gradients against float64 of the whole chain, error relative to max |expected|: f16x3 within max(2 x the fp32 MFMA route's
    own error on the same inputs, 8 eps) -- tests/test_gpu_f16x3_admission.py's yardstick.  The pooled tensor reaches fc6 tagged."""
    assert ops.DEFAULT_CONV_MATH == "f16x3"
    ops.x6_range_flags(reset=True)
    h3 = _run(ops.MATH_F16X3, tag=True)
    assert h3["pooled_tag"] is not None and f32_run["pooled_tag"] is None
    assert ops.x6_range_flags(reset=True) == 0
    g = f32_run["g"]
    p = HR.params64(g)
    fw = HR.forward(f32_run["pooled"], p)
    bw = HR.backward(fw, p, g["g_cls"], g["g_bbox"], f32_run["pooled"].shape)
    want = {"cls": fw["cls"], "bbox": fw["bbox"], "x": fw["h7"], "g_pooled": bw["g_pooled"]}
    for name in HR.PARAMS:
        want["gw_" + name], want["gb_" + name] = bw["gw_" + name], bw["gb_" + name]
    assert np.array_equal(h3["pooled"], f32_run["pooled"])
    for key, w in want.items():
        scale = float(np.abs(w).max())
        e32 = float(np.abs(f32_run[key].astype(np.float64) - w).max()) / scale
        e3 = float(np.abs(h3[key].astype(np.float64) - w).max()) / scale
        print("%-16s f32 %.2f eps   f16x3 %.2f eps" % (key, e32 / EPS, e3 / EPS))
        assert np.isfinite(h3[key]).all() and e3 <= max(2.0 * e32, 8 * EPS), (key, e3, e32)


def test_set_conv_math_reaches_fc6_and_fc7(f32_run):
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    head = _Head(f32_run["g"], ops.MATH_F32)
    assert set_conv_math(head, ops.MATH_F16X3) == 1 and head.feature_extractor.math == ops.MATH_F16X3
    assert [e[4] for e in head.feature_extractor.prep_entries()] == [ops.MATH_F16X3] * 2


# ------------------------------------------------------------------------------------------------------------------ 5. freezes
class _Count(object):
    """counts the weight-gradient and bias-gradient launches, by the gradient buffer they write"""

    def __init__(self, monkeypatch):
        self.wgrads, self.biases = [], []
        real_w, real_b = ops.conv_wgrad_async, ops.bias_grad
        monkeypatch.setattr(ops, "conv_wgrad_async", lambda x, gy, dw, *a, **k: (self.wgrads.append((dw.data_ptr(), tuple(dw.shape))), real_w(x, gy, dw, *a, **k))[1])
        monkeypatch.setattr(ops, "bias_grad", lambda gy, db: (self.biases.append(db.data_ptr()), real_b(gy, db))[1])


@pytest.mark.parametrize("key, frozen, n_wgrad", [("FC_FREEZE", ("fc6", "fc7"), 1), ("CLS_FREEZE", ("cls_score",), 3), ("BBS_FREEZE", ("bbox_pred",), 3)])
def test_a_frozen_layer_launches_no_weight_gradient_and_passes_the_input_gradient(key, frozen, n_wgrad, f32_run, monkeypatch):
    g = f32_run["g"]
    _, feats, rois = _pyramid_inputs()
    head = _Head(g, ops.MATH_F32, ["MODEL.ROI_HEADS." + key, True])
    xs = _maps(feats)
    cnt = _Count(monkeypatch)
    head.run(xs, T(rois), T(g["g_cls"]), T(g["g_bbox"]))
    torch.cuda.synchronize()
    monkeypatch.undo()
    got = _param_grads(head)
    assert len(cnt.wgrads) == n_wgrad and len(cnt.biases) == n_wgrad
    fe, pr = head.feature_extractor, head.predictor
    for name in HR.PARAMS:
        if name in frozen:
            assert got["gw_" + name] is None and got["gb_" + name] is None, name
        else:      # the trainable layers' gradients are what they are without the freeze (each run within the rule of the same float64 value)
            _rule(got["gw_" + name], f32_run["gw_" + name], 2 * GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "%s: d %s.weight" % (key, name))
            _rule(got["gb_" + name], f32_run["gb_" + name], 2 * GRAD_DEPTH[name] * R.CONV_TOL_GRAD, "%s: d %s.bias" % (key, name))
    if key == "FC_FREEZE":
        assert cnt.wgrads[0][1][0] == pr.n_out_pad
    else:
        nc, r4 = pr.num_classes, 4 * pr.num_bbox_reg_classes
        lo, n = (nc, r4) if key == "CLS_FREEZE" else (0, (nc + 3) // 4 * 4)
        assert cnt.wgrads[0] == (pr.fused_weight_grad[lo:lo + n].data_ptr(), (n, 1, 1, HR.DIM))
        frozen_rows = pr._gw2d[:nc] if key == "CLS_FREEZE" else pr._gw2d[nc:nc + r4]
        assert not bool(frozen_rows.any())             # the frozen rows of the fused gradient buffer stay zero
    for l, t in enumerate(xs):
        assert float(t.grad.abs().max()) > 0
        _rule(N(t.grad), f32_run["gx"][l], 2 * GRAD_DEPTH["pooled"] * R.CONV_TOL_GRAD, "%s: d map %d" % (key, l))


# ------------------------------------------------------------------------------------------------------------------ 6. optimiser
def test_fused_sgd_moves_the_head_and_refreshes_its_derived_weights(f32_run):
    from abr_iod_amd.modeling.backbone import resnet
    from abr_iod_amd.solver.build import FusedSGD
    g = f32_run["g"]
    _, feats, rois = _pyramid_inputs()
    head = _Head(g, ops.MATH_F32)
    opt = FusedSGD(head, 0.01, 0.9, 1e-4, 2.0, 0.0)
    fe, pr = head.feature_extractor, head.predictor
    assert fe.fc6._optimised and fe.fc7._optimised
    assert all(p.data_ptr() >= head.flat.params.data_ptr() and p.grad is not None for p in head.parameters())
    before = {n: N(p).copy() for n, p in head.named_parameters()}

    def step_inputs():
        return _maps(feats), T(rois), T(g["g_cls"]), T(g["g_bbox"])

    opt.zero_grad()
    head.run(*step_inputs())
    opt.step()
    torch.cuda.synchronize()
    after = {n: N(p).copy() for n, p in head.named_parameters()}
    assert all(np.isfinite(after[n]).all() and (after[n] != before[n]).any() for n in before)
    assert fe.fc6._wt_version == fe.fc7._wt_version == pr._wt_version == resnet._PARAM_VERSION[0]      # rebuilt by the step's preparation
    opt.zero_grad()
    xs, rois_t, g_cls, g_bbox = step_inputs()
    x, pooled, cls, bbox = head.run(xs, rois_t, g_cls, g_bbox)
    torch.cuda.synchronize()
    p = {"fc6": (fe.fc6.oihw().cpu().numpy().astype(np.float64), after["feature_extractor.fc6.bias"]),
         "fc7": (fe.fc7.oihw().cpu().numpy().astype(np.float64), after["feature_extractor.fc7.bias"]),
         "cls_score": (after["predictor.cls_score.weight"], after["predictor.cls_score.bias"]),
         "bbox_pred": (after["predictor.bbox_pred.weight"], after["predictor.bbox_pred.bias"])}
    fw = HR.forward(N(pooled), p)
    bw = HR.backward(fw, p, g["g_cls"], g["g_bbox"], tuple(pooled.shape))
    _rule(N(cls), fw["cls"], 3 * R.CONV_TOL_FWD, "after a step: cls")
    _rule(N(bbox), fw["bbox"], 3 * R.CONV_TOL_FWD, "after a step: bbox")
    _rule(N(pooled.grad), bw["g_pooled"], 3 * R.CONV_TOL_GRAD, "after a step: d pooled")      # through all three refreshed dgrad copies
    assert float(np.abs(fw["cls"] - f32_run["cls"]).max()) > 1e-3                                # the new weights really are in use


def test_a_frozen_half_of_the_predictor_survives_weight_decay(f32_run):
    """CLS_FREEZE alone: cls_score shares bbox_pred's optimiser segment, whose weight decay (1 % per step here) would shrink it.  The forward
    pass queued RIGHT behind a step must already compute with the original rows -- the restore runs on the weight-preparation stream, so the
    logits, not only the weights after a synchronisation, are what is compared: against float64 of the original cls_score at the conv rule
    (a decayed step would be off by 1 % of the logits, ten times the bound and more)."""
    from abr_iod_amd.solver.build import FusedSGD
    g = f32_run["g"]
    _, feats, rois = _pyramid_inputs()
    head = _Head(g, ops.MATH_F32, ["MODEL.ROI_HEADS.CLS_FREEZE", True])
    opt = FusedSGD(head, 0.01, 0.9, 1.0, 2.0, 1.0)
    pr = head.predictor
    w0, b0, r0 = N(pr.cls_score.weight).copy(), N(pr.cls_score.bias).copy(), N(pr.bbox_pred.weight).copy()
    x = T(f32_run["x"])
    want = f32_run["x"].astype(np.float64) @ w0.astype(np.float64).T + b0
    assert float(np.abs(want).max()) > 0.1      # 1 % of that per decayed step, against a bound of 1e-4
    logits = []
    for _ in range(2):
        opt.zero_grad()
        head.run(_maps(feats), T(rois), T(g["g_cls"]), T(g["g_bbox"]))
        opt.step()
        with torch.no_grad():
            logits.append(head.predictor(x)[0])      # no synchronisation between the step and this call
    torch.cuda.synchronize()
    for i, y in enumerate(logits):
        _rule(N(y), want, R.CONV_TOL_FWD, "cls logits right behind step %d" % (i + 1))
    assert np.array_equal(N(pr.cls_score.weight), w0) and np.array_equal(N(pr.cls_score.bias), b0)
    assert (N(pr.bbox_pred.weight) != r0).any()


# ------------------------------------------------------------------------------------------------------------------ 7. detector
TINY = ["MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8,
        "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16]
FPN_CFG = ["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.RPN.USE_FPN", True, "MODEL.RPN.ANCHOR_STRIDE", (4, 8, 16, 32, 64),
           "MODEL.RPN.ANCHOR_SIZES", (8, 16, 32, 64, 128), "MODEL.ROI_HEADS.USE_FPN", True,
           "MODEL.ROI_BOX_HEAD.FEATURE_EXTRACTOR", "FPN2MLPFeatureExtractor", "MODEL.ROI_BOX_HEAD.PREDICTOR", "FPNPredictor",
           "MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_BOX_HEAD.POOLER_SCALES", P.SCALES, "MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO", 2,
           "MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM", 32, "MODEL.RPN.PRE_NMS_TOP_N_TRAIN", 200, "MODEL.RPN.POST_NMS_TOP_N_TRAIN", 100,
           "MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN", 120, "MODEL.RPN.PRE_NMS_TOP_N_TEST", 300, "MODEL.RPN.POST_NMS_TOP_N_TEST", 200,
           "MODEL.RPN.FPN_POST_NMS_TOP_N_TEST", 400, "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64,
           # every level must see a gradient for "every trainable parameter has one": at 64 x 96 no RoI is large enough for P5, so P5's and P6's
           # come from the RPN loss -- their 24 anchors stay visible (no straddle filter) and the sampler draws 1024 of the 1536 per image
           "MODEL.RPN.STRADDLE_THRESH", -1, "MODEL.RPN.BATCH_SIZE_PER_IMAGE", 1024,
           # eval must return detections for its checks to mean anything: a freshly initialised 21-way softmax scores every class ~0.048,
           # under the default threshold 0.05
           "MODEL.ROI_HEADS.SCORE_THRESH", 0.01]


@pytest.fixture(scope="module")
def detector():
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    cfg = make_cfgs("15-5", overrides=TINY + FPN_CFG)[1]
    _, model = build_models(None, cfg, seed=0, need_source=False)
    gen = torch.Generator().manual_seed(3)
    image = (torch.randn(2, 3, 64, 96, generator=gen) * 40).cuda()
    boxes = [[[4.0, 6.0, 40.0, 50.0], [50.0, 10.0, 90.0, 36.0]], [[10.0, 20.0, 30.0, 60.0], [40.0, 4.0, 84.0, 56.0]]]
    labels = [[16, 18], [17, 20]]
    targets = []
    for b, l in zip(boxes, labels):
        t = BoxList(torch.tensor(b).cuda(), (96, 64), mode="xyxy")
        t.add_field("labels", torch.tensor(l).cuda())
        targets.append(t)
    return cfg, model, ImageList(image, [(64, 96), (64, 96)]), targets


def _conv_close(a, b, tol, what):
    a, b = N(a).astype(np.float64), N(b).astype(np.float64)
    err, lim = float(np.abs(a - b).max()), tol * max(1.0, float(np.abs(b).max()))
    print("%-34s err %.3e  limit %.3e" % (what, err, lim))
    assert err <= lim, (what, err, lim)


def test_detector_trains_without_a_host_round_trip_between_rpn_and_losses(detector):
    from abr_iod_amd.modeling.rpn.rpn import LazyPyramidProposals
    cfg, model, images, targets = detector
    model.train()
    model.flat.zero_grad()      # (p.grad are views of the flat gradient buffer: zero it, never drop them)
    torch.manual_seed(5)
    state = model.forward_begin(images, targets)
    (boxes, _), _, _ = model.rpn.forward_finish(state["rpn"])
    assert isinstance(boxes, LazyPyramidProposals)
    torch.cuda.synchronize()
    with no_sync():       # RPN finish -> targets -> pooler -> MLP -> predictor -> both losses: nothing is read back
        first = model.forward_finish(state)
    losses, feats = first[0], first[1]
    assert set(losses) == {"loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"}
    assert all(bool(torch.isfinite(v)) for v in losses.values()) and len(feats) == 5
    ev = model.roi_heads.box.loss_evaluator
    t = ev._fused_targets
    assert t is not None and tuple(t["rois"].shape) == (128, 5) and tuple(first[6].shape) == (128, 16, 7, 7)
    if ops.uses_amax(model.roi_heads.box.feature_extractor.math):      # the default arithmetic: the neck's outputs are tagged, so the pooled tensor is
        assert model.conv_math == "f16x3" and ops.amax_of(first[6])[0] is not None
    sum(losses.values()).backward()
    torch.cuda.synchronize()
    watched = [n for n, p in model.named_parameters() if p.requires_grad]
    assert any(n.startswith("roi_heads.box.feature_extractor.fc6") for n in watched) and any(n.startswith("backbone.body.layer2") for n in watched)
    for n, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, n
        else:
            assert n.startswith(("backbone.body.stem", "backbone.body.layer1")), n
    # the same draw through the BoxList path (collect + subsample): the same two box losses at the conv rule
    sampled = [t["sampled_idx"][i][t["sampled_idx"][i] >= 0] for i in range(2)]
    assert all(len(s) > 4 for s in sampled)
    ev.inject_sampled_inds = sampled
    try:
        _, _, _, losses2, _ = model.roi_heads(feats, boxes, targets)
    finally:
        ev.inject_sampled_inds = None
    assert ev._fused_targets is None
    for k in ("loss_classifier", "loss_box_reg"):
        _conv_close(losses[k], losses2[k], 3 * R.CONV_TOL_FWD, "BoxList path " + k)
    model.flat.zero_grad()      # (p.grad are views of the flat gradient buffer: zero it, never drop them)


def test_detector_eval_returns_detections_inside_the_image(detector):
    cfg, model, images, targets = detector
    model.eval()
    with torch.no_grad():
        result, feats, background = model(images)
    model.train()
    assert len(result) == 2 and len(feats) == 5
    for det in result:
        assert det.has_field("scores") and det.has_field("labels")
        bb = N(det.bbox)
        assert bb.shape[1] == 4 and np.isfinite(bb).all()
        assert 0 < len(bb) <= cfg.MODEL.ROI_HEADS.DETECTIONS_PER_IMG       # (SCORE_THRESH 0.01 in the fixture: a fresh 21-way softmax sits at 0.048)
        assert (bb[:, 0] >= 0).all() and (bb[:, 1] >= 0).all() and (bb[:, 2] <= 95).all() and (bb[:, 3] <= 63).all()
        assert (bb[:, 2] >= bb[:, 0]).all() and (bb[:, 3] >= bb[:, 1]).all()
        assert (N(det.get_field("labels")) >= 1).all() and (N(det.get_field("scores")) > cfg.MODEL.ROI_HEADS.SCORE_THRESH).all()


def test_detector_soften_entry_points_and_the_joint_pass(detector):
    cfg, model, images, targets = detector
    model.eval()
    with torch.no_grad():
        soft = model.soften_finish(model.soften_begin(images))       # deferred selection: the picks index the selector's table directly
        (scores, bboxes), mask_logits, selected, feats, _, _, _, raf = soft
        picks = model.last_soften_indices
        assert all(hasattr(b, "_roi_table") for b in selected)       # the fused path really ran
        generic = model.generate_soften_proposal(images, selected_indices=picks)     # the BoxList path (collect, sort, index)
        by_targets = model.generate_feature_logits_by_targets(images, targets)
    assert tuple(raf.shape) == (64 * 2, 16, 7, 7) and tuple(scores.shape) == (128, 21) and tuple(bboxes.shape) == (128, 21, 4) and mask_logits is None
    assert all(len(b) == 64 for b in selected)
    for a, b in zip(selected, generic[2]):
        assert torch.equal(a.bbox, b.bbox)
    assert torch.equal(raf, generic[7]) and torch.equal(scores, generic[0][0])
    assert tuple(by_targets[0][0].shape) == (4, 21) and tuple(by_targets[4].shape) == (4, 16, 7, 7)
    model.train()
    # forward + the features= / proposals= call against forward_joint, the same sampler draw
    torch.manual_seed(9)
    first = model(images, targets)
    (t_scores, t_bboxes), _, t_raf = model(images, targets, features=first[1], proposals=selected)
    torch.manual_seed(9)
    joint_first, ((j_scores, j_bboxes), _, j_raf) = model.forward_joint(images, targets, selected)
    for k in first[0]:
        _conv_close(joint_first[0][k], first[0][k], 3 * R.CONV_TOL_FWD, "joint " + k)
    _conv_close(j_scores, t_scores, 3 * R.CONV_TOL_FWD, "joint soften scores")
    _conv_close(j_bboxes, t_bboxes, 3 * R.CONV_TOL_FWD, "joint soften boxes")
    assert torch.equal(j_raf, t_raf) and torch.equal(joint_first[6], first[6]) and tuple(j_raf.shape) == (128, 16, 7, 7)
    sum(joint_first[0].values()).backward()
    torch.cuda.synchronize()
    assert float(model.roi_heads.box.feature_extractor.fc6.weight.grad.abs().max()) > 0
    model.flat.zero_grad()      # (p.grad are views of the flat gradient buffer: zero it, never drop them)

"""GPU: RetinaNet's inference half.  csrc/retinanet.hip (abr_retina_detect) and RetinaNetPostProcessor against the golden the reference's own
code wrote (tests/golden/retinanet.npz) and, at the edges, against the numpy restatement of tests/retinanet_ref.py; LastLevelP6P7 inside the
FPN's autograd node and RetinaNetHead against the float64 restatement and the golden; the tiny R-50-FPN-RETINANET detector in eval.

Comparisons of labels, order and counts are exact: the golden's candidate scores are all different and far apart (test_retinanet_ref.py), the
edge cases draw their logits from multiples of 0.5 (long tie groups, no order hangs on how a sigmoid is rounded), the restatement's tie rules
are the library's documented ones, and the case builder redraws anything whose NMS decision lies within 1e-5 of the threshold.  Scores: rtol
3e-7; boxes: rtol 1e-5 / atol 2e-4 (the figures of test_gpu_rpn_pyramid.py against its golden).  The golden's order inside a class is put into
the library's (descending score) by retinanet_ref.canonical: see that module's docstring."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import fpn_ref as FR
import retinanet_ref as R
import rpn_fpn_ref as F
from oracle import ops as O

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retinanet.npz")
PASSING = np.arange(-2.5, 6.01, 0.5, dtype=np.float32)      # sigmoid > 0.05 with room to spare (sigmoid(-3) = 0.047)
BELOW = np.arange(-6.0, -3.49, 0.5, dtype=np.float32)


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


@pytest.fixture(scope="module")
def golden_run(g):
    L = len(R.MAPS)
    cls, reg = R.golden_arrays([g["cls_%d" % l] for l in range(L)], [g["reg_%d" % l] for l in range(L)])
    return cls, reg, [g["anchors_%d" % l] for l in range(L)]


def run_op(cls, reg, anchors, A, Cn, image_sizes, th, pre, nms, det, min_size=0):
    from abr_iod_amd import ops
    img_hw = torch.tensor([list(s) for s in image_sizes], dtype=torch.int32).cuda()
    boxes, scores, labels, n_out = ops.retina_detect([cuda(c) for c in cls], [cuda(r) for r in reg], [cuda(a) for a in anchors], A, Cn, img_hw, th, pre,
                                                     nms, det, R.WEIGHTS, min_size)
    cap = len(cls) * pre
    assert tuple(boxes.shape) == (len(image_sizes), cap, 4) and tuple(scores.shape) == tuple(labels.shape) == (len(image_sizes), cap)
    assert labels.dtype == torch.int64 and n_out.dtype == torch.int32
    n = n_out.tolist()
    for i in range(len(n)):       # rows past the count are zero
        assert not boxes[i, n[i]:].any() and not scores[i, n[i]:].any() and not labels[i, n[i]:].any(), i
    return [dict(boxes=N(boxes[i, :n[i]]), scores=N(scores[i, :n[i]]), labels=N(labels[i, :n[i]])) for i in range(len(n))]


def check(got, want, tag):
    assert len(got["labels"]) == len(want["labels"]), (tag, len(got["labels"]), len(want["labels"]))
    assert np.array_equal(got["labels"], want["labels"]), tag
    np.testing.assert_allclose(got["scores"], want["scores"], rtol=3e-7, atol=0, err_msg=str(tag))
    np.testing.assert_allclose(got["boxes"], want["boxes"], rtol=1e-5, atol=2e-4, err_msg=str(tag))


# ----------------------------------------------------------------------------------------------------------------- against the golden
@pytest.mark.parametrize("cap", R.CAPS)
def test_op_against_the_golden(g, golden_run, cap):
    cls, reg, anchors = golden_run
    got = run_op(cls, reg, anchors, R.A, R.C, R.IMAGE_SIZES, R.TH, R.PRE, R.NMS_TH, cap)
    for i, d in enumerate(got):
        wb, ws, wl = R.canonical(g["boxes_%d_%d" % (cap, i)], g["scores_%d_%d" % (cap, i)], g["labels_%d_%d" % (cap, i)])
        check(d, dict(boxes=wb, scores=ws, labels=wl), (cap, i))
    assert [len(d["labels"]) for d in got] == ([30, 30] if cap == 30 else [len(g["labels_1000_%d" % i]) for i in range(2)])


@pytest.mark.parametrize("cap", R.CAPS)
def test_postprocessor_against_the_golden(g, golden_run, cap):
    """through RetinaNetPostProcessor with the reference's signature (NCHW maps, per-image anchor BoxLists) -> BoxLists"""
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetPostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    cls, reg, anchors = golden_run
    n = len(R.IMAGE_SIZES)
    grids = [cuda(a) for a in anchors]
    boxlists = [[BoxList(a, (w, h), mode="xyxy") for a in grids] for h, w in R.IMAGE_SIZES]
    box_cls = [cuda(c.reshape(n, H, W, R.A * R.C)).permute(0, 3, 1, 2) for c, (H, W) in zip(cls, R.MAPS)]
    box_reg = [cuda(r.reshape(n, H, W, R.A * 4).transpose(0, 3, 1, 2)) for r, (H, W) in zip(reg, R.MAPS)]      # (one NCHW-contiguous input too)
    pp = RetinaNetPostProcessor(R.TH, R.PRE, R.NMS_TH, cap, 0, R.C + 1)
    res = pp(boxlists, box_cls, box_reg)
    assert len(res) == n
    for i, b in enumerate(res):
        assert b.size == (R.IMAGE_SIZES[i][1], R.IMAGE_SIZES[i][0]) and b.mode == "xyxy" and sorted(b.fields()) == ["labels", "scores"]
        assert b.get_field("labels").dtype == torch.int64 and b.get_field("scores").dtype == torch.float32
        wb, ws, wl = R.canonical(g["boxes_%d_%d" % (cap, i)], g["scores_%d_%d" % (cap, i)], g["labels_%d_%d" % (cap, i)])
        check(dict(boxes=N(b.bbox), scores=N(b.get_field("scores")), labels=N(b.get_field("labels"))), dict(boxes=wb, scores=ws, labels=wl), (cap, i))
    with pytest.raises(NotImplementedError, match="one feature level"):
        pp([bl[:1] for bl in boxlists], box_cls[:1], box_reg[:1])
    big = RetinaNetPostProcessor(R.TH, 2000, R.NMS_TH, cap, 0, R.C + 1)
    with pytest.raises(ValueError, match="PRE_NMS_TOP_N"):
        big(boxlists, box_cls, box_reg)


# ----------------------------------------------------------------------------------------------------------------- edges, against the restatement
def build_case(seed, image_sizes, maps, strides, ratios, scales, Cn, counts, nms, ld_extra=0):
    """tie-heavy head outputs: counts[l][i] logits of segment (l, i) (None: all of them) come from PASSING, the rest from BELOW; deltas are
    multiples of 1/16; `ld_extra` pad columns behind the logits hold +100.  Redrawn until no equal-label IoU lies within 1e-5 of `nms`."""
    n, A = len(image_sizes), len(ratios) * len(scales)
    anchors = [O.grid_anchors(O.cell_anchors(st, tuple(st * 2.0 * s for s in scales), ratios), H, W, st, image_sizes[0])[0] for (H, W), st in zip(maps, strides)]
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        cls, reg = [], []
        for l, (H, W) in enumerate(maps):
            nloc, AC = H * W, A * Cn
            c = rng.choice(BELOW, size=(n, nloc, AC + ld_extra)).astype(np.float32)
            for i in range(n):
                k = nloc * AC if counts[l][i] is None else counts[l][i]
                at = rng.choice(nloc * AC, size=k, replace=False)
                c[i, at // AC, at % AC] = rng.choice(PASSING, size=k)
            c[:, :, AC:] = 100.0
            cls.append(c)
            reg.append((rng.integers(-16, 17, size=(n, nloc, 4 * A)) / 16.0).astype(np.float32))
        probe = R.detect_ref(cls, reg, anchors, A, Cn, image_sizes, R.TH, 1 << 20, nms, 0)
        if not any(np.any(np.abs(R.same_label_ious(d["segments"]) - nms) < 1e-5) for d in probe):
            return cls, reg, anchors, A
    raise RuntimeError("no draw without a near-threshold NMS decision")


SIZES2 = ((64, 96), (56, 80))
MAPS5, STRIDES5 = ((8, 12), (4, 6), (2, 3), (1, 2), (1, 1)), (8, 16, 32, 64, 128)
RAT3, SC3 = (0.5, 1.0, 2.0), (1.0, 2 ** (1 / 3.0), 2 ** (2 / 3.0))
CASES = {
    # name: (image sizes, maps, strides, ratios, scales, C, counts per level and image, pre, det, pad columns)
    "five levels, exactly pre and pre + 1": (SIZES2, MAPS5, STRIDES5, RAT3, SC3, 4, ((70, 71), (71, 70), (40, 0), (None, 5), (None, None)), 70, 40, 0),
    "one image, one level": (SIZES2[:1], MAPS5[:1], STRIDES5[:1], RAT3, SC3, 4, ((300,),), 128, 0, 0),
    "fewer logits than pre": (SIZES2, MAPS5[3:], STRIDES5[3:], RAT3, SC3, 3, ((None, None), (None, 7)), 100, 4, 0),
    "one class": (SIZES2, MAPS5[1:4], STRIDES5[1:4], RAT3, SC3, 1, ((90, 60), (None, 20), (10, None)), 64, 12, 0),
    "27 columns in ld = 28": (SIZES2, MAPS5[:3], STRIDES5[:3], RAT3, SC3, 3, ((200, 120), (65, 64), (None, 0)), 64, 50, 1),
    "one anchor per location": (SIZES2, MAPS5[:2], STRIDES5[:2], (1.0,), (1.0,), 5, ((33, 200), (None, 1)), 40, 1000, 3),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_edges_against_the_restatement(name):
    sizes, maps, strides, ratios, scales, Cn, counts, pre, det, pad = CASES[name]
    cls, reg, anchors, A = build_case(len(name), sizes, maps, strides, ratios, scales, Cn, counts, 0.4, pad)
    want = R.detect_ref(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det)
    got = run_op(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det)
    for i in range(len(sizes)):
        check(got[i], want[i], (name, i))
    # the case exercises what it is there for
    assert any(len(np.unique(s["scores"])) < len(s["scores"]) for d in want for s in d["segments"] if len(s["scores"]) > 20), name    # ties in a segment
    if det and det < 1000:
        assert any(d["n_nms"] > det for d in want), name
    # min_size > 0 drops rows before NMS: a second configuration of the same inputs
    want = R.detect_ref(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det, min_size=24)
    got = run_op(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det, min_size=24)
    for i in range(len(sizes)):
        check(got[i], want[i], (name, "min_size", i))


def _planted(spots, maps, A, Cn, n=1, reg_spots=()):
    """all logits -6 but the planted (level, image, loc, a, c, logit); all deltas 0 but reg_spots (level, image, loc, a, 4 deltas)"""
    cls = [np.full((n, H * W, A * Cn), -6.0, np.float32) for H, W in maps]
    reg = [np.zeros((n, H * W, 4 * A), np.float32) for H, W in maps]
    for l, i, loc, a, c, v in spots:
        cls[l][i, loc, a * Cn + c] = v
    for l, i, loc, a, d in reg_spots:
        reg[l][i, loc, 4 * a:4 * a + 4] = d
    return cls, reg


def test_planted_ties_duplicates_and_the_clamp():
    """two equal scores exactly at the detections cut (both kept); one box under two labels (both kept) and under one label from two levels
    (one kept: the earlier level wins the tie); equal scores across levels; a delta above the log(1000 / 16) clamp"""
    sizes, maps, A, Cn = ((200, 300),), ((4, 6), (4, 6)), 1, 3
    far = np.array([[x, y, x + 19, y + 19] for y in range(0, 160, 40) for x in range(0, 240, 40)], np.float32)       # 24 disjoint 20 x 20 boxes
    anchors = [far, far.copy()]
    spots = [(0, 0, 0, 0, 0, 3.0), (0, 0, 1, 0, 0, 2.0), (1, 0, 2, 0, 0, 2.0), (0, 0, 3, 0, 0, 1.0),      # class 1: scores 3, 2, 2 (two levels), 1
             (0, 0, 5, 0, 1, 2.5), (0, 0, 5, 0, 2, 0.5),                                                    # one box under labels 2 and 3
             (0, 0, 7, 0, 1, 1.5), (1, 0, 7, 0, 1, 1.5)]                                                    # one box, label 2, both levels, equal scores
    cls, reg = _planted(spots, maps, A, Cn, reg_spots=[(0, 0, 3, 0, (0.0, 0.0, 30.0, 25.0))])
    for det, n_want in ((0, 7), (4, 4), (3, 4), (2, 2)):       # the 3rd largest score is 2.0 twice: the cut at 3 keeps four
        want = R.detect_ref(cls, reg, anchors, A, Cn, sizes, R.TH, 50, 0.4, det)
        got = run_op(cls, reg, anchors, A, Cn, sizes, R.TH, 50, 0.4, det)
        check(got[0], want[0], det)
        assert len(got[0]["labels"]) == n_want, det
    got = run_op(cls, reg, anchors, A, Cn, sizes, R.TH, 50, 0.4, 0)[0]
    assert got["labels"].tolist() == [1, 1, 1, 1, 2, 2, 3]
    assert np.array_equal(got["boxes"][4], got["boxes"][6]) and np.array_equal(got["boxes"][4], far[5])       # labels 2 and 3 share the box
    assert np.array_equal(got["boxes"][5], far[7])                                                            # ... and the duplicate left one
    clamped = got["boxes"][3]                                                                                 # 20 * 62.5 wide, clipped to the image
    assert clamped.tolist() == [0.0, 0.0, 299.0, 199.0]


def test_no_candidate_anywhere_and_an_empty_batch():
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetPostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    maps, A, Cn = MAPS5[:2], 9, 4
    cls, reg, anchors, _ = build_case(3, SIZES2, maps, STRIDES5[:2], RAT3, SC3, Cn, ((0, 0), (0, 0)), 0.4)
    got = run_op(cls, reg, anchors, A, Cn, SIZES2, R.TH, 100, 0.4, 100)
    assert all(len(d["labels"]) == 0 for d in got)
    pp = RetinaNetPostProcessor(R.TH, 100, 0.4, 100, 0, Cn + 1)
    grids = [cuda(a) for a in anchors]      # one grid per level for the batch, as AnchorGenerator hands them out
    boxlists = [[BoxList(a, (w, h), mode="xyxy") for a in grids] for h, w in SIZES2]
    res = pp.forward_nhwc(boxlists, [cuda(c.reshape(2, H, W, -1)) for c, (H, W) in zip(cls, maps)], [cuda(r.reshape(2, H, W, -1)) for r, (H, W) in zip(reg, maps)], A)
    for b in res:
        assert len(b) == 0 and tuple(b.bbox.shape) == (0, 4) and b.get_field("labels").dtype == torch.int64 and b.get_field("scores").dtype == torch.float32
    # N == 0: nothing is launched, empty tables come back
    img_hw = torch.zeros((0, 2), dtype=torch.int32, device="cuda")
    out = ops.retina_detect([cuda(c[:0]) for c in cls], [cuda(r[:0]) for r in reg], [cuda(a) for a in anchors], A, Cn, img_hw, R.TH, 100, 0.4, 100)
    assert tuple(out[0].shape) == (0, 200, 4) and tuple(out[3].shape) == (0,)


def test_a_smaller_pyramid_after_a_larger_one():
    """no call depends on what an earlier one left in the per-stream scratch"""
    big = CASES["five levels, exactly pre and pre + 1"]
    cls, reg, anchors, A = build_case(11, big[0], big[1], big[2], big[3], big[4], big[5], big[6], 0.4)
    run_op(cls, reg, anchors, A, big[5], big[0], R.TH, 1600, 0.4, 0)
    sizes, maps, strides, ratios, scales, Cn, counts, pre, det, pad = CASES["one class"]
    cls, reg, anchors, A = build_case(12, sizes, maps, strides, ratios, scales, Cn, counts, 0.4)
    for _ in range(2):
        want = R.detect_ref(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det)
        got = run_op(cls, reg, anchors, A, Cn, sizes, R.TH, pre, 0.4, det)
        for i in range(len(sizes)):
            check(got[i], want[i], i)


def test_over_limit_arguments_are_errors_before_any_launch(golden_run):
    from abr_iod_amd import _lib, ops
    cls, reg, anchors = golden_run
    assert ops.retina_max_candidates() == 8192 and ops.rpn_pyramid_max_k() == 2048
    img_hw = torch.tensor([list(s) for s in R.IMAGE_SIZES], dtype=torch.int32).cuda()
    args = ([cuda(c) for c in cls], [cuda(r) for r in reg], [cuda(a) for a in anchors], R.A, R.C, img_hw, R.TH)
    with pytest.raises(RuntimeError, match="PRE_NMS_TOP_N"):
        ops.retina_detect(*args, 2049, R.NMS_TH, 100)
    with pytest.raises(RuntimeError, match="PRE_NMS_TOP_N"):
        ops.retina_detect(*args, 1639, R.NMS_TH, 100)           # 5 x 1639 > 8192
    ops.retina_detect(*args, 1638, R.NMS_TH, 100)               # ... and 5 x 1638 fits, as the defaults' 5 x 1000 do
    with pytest.raises(RuntimeError, match="levels"):
        ops.retina_detect(args[0] * 2, args[1] * 2, args[2] * 2, *args[3:], 100, R.NMS_TH, 100)
    # the library itself: every limit is an error before anything is launched (the outputs keep their sentinel)
    L, lib = len(cls), _lib.lib()
    n_out = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    boxes = torch.full((2, 8, 4), -7.0, device="cuda")
    vp, ci = C.c_void_p * L, C.c_int * L
    tables = (vp(*[t.data_ptr() for t in args[0]]), ci(*[t.shape[2] for t in args[0]]), vp(*[t.data_ptr() for t in args[1]]), ci(*[t.shape[2] for t in args[1]]),
              vp(*[t.data_ptr() for t in args[2]]), ci(*[t.shape[1] for t in args[0]]))

    def call(pre, cap, A=R.A, Cn=R.C):
        return lib.abr_retina_detect(*tables, L, 2, A, Cn, img_hw.data_ptr(), R.TH, pre, R.NMS_TH, 100, 10.0, 10.0, 5.0, 5.0, 0.0, cap, boxes.data_ptr(),
                                     boxes.data_ptr(), boxes.data_ptr(), n_out.data_ptr(), None)
    for pre, cap, A, Cn in ((2049, 5 * 2049, R.A, R.C), (1639, 5 * 1639, R.A, R.C), (100, 499, R.A, R.C), (100, 500, R.A + 1, R.C), (0, 0, R.A, R.C),
                            (100, 500, R.A, 1 << 19)):
        assert call(pre, cap, A, Cn) == -1 and b"retina_detect" in lib.abr_last_error(), (pre, cap, A, Cn)
    torch.cuda.synchronize()
    assert n_out.tolist() == [-7, -7] and bool((boxes == -7).all())


# ----------------------------------------------------------------------------------------------------------------- neck
def _rule(got, want, tol, what):
    ok, err, lim = FR.conv_rule_ok(np.asarray(got), np.asarray(want, np.float64), tol)
    print("%-34s err %.3e  limit %.3e" % (what, err, lim))
    assert ok, (what, err, lim)


def _neck(g, cin, seed=5):
    """an FPN over C3..C5 (8, 12, cin channels; 16 out) with the golden's LastLevelP6P7 weights loaded, and its input maps"""
    from abr_iod_amd.modeling.backbone import fpn as fpn_module
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    torch.manual_seed(seed)
    chans = [0, 8, 12, cin if cin != 16 else 20]
    top_in = cin
    f = fpn_module.FPN(chans, 16, top_blocks=fpn_module.LastLevelP6P7(top_in, 16)).cuda()
    assert f.top_blocks.use_P5 == (cin == 16)
    with torch.no_grad():
        f.top_blocks.p6.load_oihw(cuda(g["p6p7_%d_w6" % cin]))
        f.top_blocks.p7.load_oihw(cuda(g["p6p7_%d_w7" % cin]))
        f.top_blocks.p6.bias.copy_(cuda(g["p6p7_%d_b6" % cin]))
        f.top_blocks.p7.bias.copy_(cuda(g["p6p7_%d_b7" % cin]))
        for n, p in f.named_parameters():
            if "top_blocks" not in n and n.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.3)
    bump_param_version()
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((2, c, 36 >> l, 44 >> l)).astype(np.float32) for l, c in enumerate(chans[1:])]     # C5 is 9 x 11, as the golden's
    return f, xs


def _neck64(f, xs, gs):
    """the whole neck with LastLevelP6P7 in float64 (torch on the CPU) and the loss sum <P_l, g_l> over the outputs with a gradient ->
    (outputs, input gradients, {parameter name: gradient})"""
    import torch.nn.functional as Fn
    prm = {n: torch.tensor(N(p).astype(np.float64), requires_grad=True) for n, p in f.named_parameters()}

    def conv(name, t, **kw):
        return Fn.conv2d(t, prm[name + ".weight"].permute(0, 3, 1, 2), prm[name + ".bias"], **kw)       # OHWI -> OIHW
    xt = [torch.tensor(x.astype(np.float64), requires_grad=True) for x in xs]
    last = conv("fpn_inner4", xt[2])
    ps = [conv("fpn_layer4", last, padding=1)]
    for l in (1, 0):
        last = conv("fpn_inner%d" % (l + 2), xt[l]) + Fn.interpolate(last, scale_factor=2, mode="nearest")
        ps.insert(0, conv("fpn_layer%d" % (l + 2), last, padding=1))
    p6 = conv("top_blocks.p6", ps[2] if f.top_blocks.use_P5 else xt[2], stride=2, padding=1)
    ps += [p6, conv("top_blocks.p7", Fn.relu(p6), stride=2, padding=1)]
    if any(gg is not None for gg in gs):
        sum((p * torch.tensor(gg.astype(np.float64))).sum() for p, gg in zip(ps, gs) if gg is not None).backward()
    zero = lambda t: t.grad.numpy() if t.grad is not None else np.zeros(tuple(t.shape))      # noqa: E731
    return [p.detach().numpy() for p in ps], [zero(x) for x in xt], {n: zero(p) for n, p in prm.items()}


@pytest.mark.parametrize("cin", [64, 16])
def test_p6p7_forward(g, cin):
    f, xs = _neck(g, cin)
    # the top block alone, on the golden's input, against the reference's output and the float64 restatement
    x = g["p6p7_%d_%s" % (cin, "p5" if cin == 16 else "c5")]
    with torch.no_grad():
        p6, p7 = f.top_blocks(cuda(g["p6p7_%d_c5" % cin]), cuda(g["p6p7_%d_p5" % cin]))
    w6, w7 = (g["p6p7_%d_%s" % (cin, k)] for k in ("w6", "w7"))
    r6, r7 = R.p6p7_ref(w6, g["p6p7_%d_b6" % cin], w7, g["p6p7_%d_b7" % cin], x)
    assert tuple(p6.shape) == (2, 16, 5, 6) and tuple(p7.shape) == (2, 16, 3, 3)
    for got, want, gold, depth, what in ((p6, r6, g["p6p7_%d_p6" % cin], 1, "P6"), (p7, r7, g["p6p7_%d_p7" % cin], 2, "P7")):
        _rule(N(got), want, depth * FR.CONV_TOL_FWD, "%s (cin %d) float64" % (what, cin))
        _rule(N(got), gold.astype(np.float64), depth * FR.CONV_TOL_FWD, "%s (cin %d) golden" % (what, cin))
    # inside the FPN: five outputs, with and without the autograd node
    with torch.no_grad():
        plain = f([cuda(x) for x in xs])
    node = f([cuda(x).requires_grad_(True) for x in xs])
    assert [tuple(p.shape) for p in plain] == [(2, 16, 36, 44), (2, 16, 18, 22), (2, 16, 9, 11), (2, 16, 5, 6), (2, 16, 3, 3)]
    assert all(torch.equal(a, b) for a, b in zip(plain, node)) and all(p.requires_grad for p in node)
    want, _, _ = _neck64(f, xs, [None] * 5)
    for l in range(5):
        depth = {64: (2, 2, 2, 1, 2), 16: (2, 2, 2, 3, 4)}[cin][l]      # contractions between the input maps and the output
        _rule(N(plain[l]), want[l], depth * FR.CONV_TOL_FWD, "P%d inside the FPN (cin %d)" % (l + 3, cin))


@pytest.mark.parametrize("which", ["P6 and P7", "P7 only", "P6 only", "all five", "P3 only"])
@pytest.mark.parametrize("cin", [64, 16])
def test_p6p7_backward_inside_the_fpn_node(g, cin, which):
    """_FPNFn's backward with the new top block against float64: every parameter gradient and every input gradient; an output without a
    gradient costs nothing (its convs' gradients stay untouched)"""
    f, xs = _neck(g, cin)
    rng = np.random.default_rng(17)
    on = {"P6 and P7": (3, 4), "P7 only": (4,), "P6 only": (3,), "all five": (0, 1, 2, 3, 4), "P3 only": (0,)}[which]
    xt = [cuda(x).requires_grad_(True) for x in xs]
    ps = f(xt)
    gs = [rng.standard_normal(tuple(p.shape)).astype(np.float32) if l in on else None for l, p in enumerate(ps)]
    f.zero_grad()
    sum((p * cuda(gg)).sum() for p, gg in zip(ps, gs) if gg is not None).backward()
    torch.cuda.synchronize()
    _, gx64, gp64 = _neck64(f, xs, gs)
    depth = 4 * FR.CONV_TOL_GRAD        # at most four contractions between an output gradient and anything compared (p7, p6, fpn_layer4, fpn_inner4)
    for n, p in f.named_parameters():
        want = gp64[n]
        if not want.any():
            assert p.grad is None or not p.grad.any(), (n, "no gradient arrives here")
        else:
            _rule(N(p.grad), want, depth, "d %s (%s, cin %d)" % (n, which, cin))
    for l, x in enumerate(xt):
        if not gx64[l].any():
            assert x.grad is None or not x.grad.any(), l
        else:
            _rule(N(x.grad), gx64[l], depth, "d C%d (%s, cin %d)" % (l + 3, which, cin))
    top = f.top_blocks
    if which == "P3 only":
        assert all(p.grad is None or not p.grad.any() for p in top.parameters())
    if which == "P6 only":
        assert top.p7.weight.grad is None or not top.p7.weight.grad.any()
    if which == "P7 only":
        assert top.p6.weight.grad.any() and top.p7.weight.grad.any()


# ----------------------------------------------------------------------------------------------------------------- head
def _head(g, num_classes=R.C + 1):
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetHead
    c = cfg.clone()
    c.merge_from_list(["MODEL.RETINANET.NUM_CLASSES", num_classes, "MODEL.RETINANET.NUM_CONVS", 2])
    head = RetinaNetHead(c, 16).cuda()
    sd = {str(k)[len("head_"):]: g[k] for k in g.files if k.startswith("head_") and k.endswith(("weight", "bias"))}
    with torch.no_grad():
        for name, conv in [("cls_tower.0", head.cls_tower[0]), ("cls_tower.2", head.cls_tower[2]), ("bbox_tower.0", head.bbox_tower[0]),
                           ("bbox_tower.2", head.bbox_tower[2]), ("cls_logits", head.cls_logits), ("bbox_pred", head.bbox_pred)]:
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            if name == "cls_logits":
                w, b = w[: conv.out_channels], b[: conv.out_channels]
            conv.weight[: conv.out_channels].copy_(cuda(w).permute(0, 2, 3, 1))
            conv.bias[: conv.out_channels].copy_(cuda(b))
    bump_param_version()
    return head, sd


def test_head_forward_on_two_levels(g):
    head, sd = _head(g)
    assert (head.ld_cls, head.ld_reg, head.num_anchors, head.num_classes) == (36, 36, 9, 4)
    xs = [g["head_x_%d" % l] for l in range(2)]
    with torch.no_grad():
        logits, deltas = head([cuda(x) for x in xs])
        nhwc = [head.forward_nhwc(cuda(x)) for x in xs]
    want_l, want_d = R.head_ref(sd, xs, 2)
    tol = 3 * FR.CONV_TOL_FWD       # three contractions: the conv-stack rule of the FPN mask head's test
    for l in range(2):
        assert tuple(logits[l].shape) == tuple(g["head_cls_%d" % l].shape) and tuple(deltas[l].shape) == tuple(g["head_reg_%d" % l].shape)
        _rule(N(logits[l]), want_l[l], tol, "logits %d float64" % l)
        _rule(N(deltas[l]), want_d[l], tol, "deltas %d float64" % l)
        _rule(N(logits[l]), g["head_cls_%d" % l].astype(np.float64), tol, "logits %d golden" % l)
        _rule(N(deltas[l]), g["head_reg_%d" % l].astype(np.float64), tol, "deltas %d golden" % l)
        # the NHWC rows are the reference's permute_and_flatten order: column a * C + c
        assert torch.equal(nhwc[l][0].permute(0, 3, 1, 2)[:, :36], logits[l]) and torch.equal(nhwc[l][1].permute(0, 3, 1, 2), deltas[l])
    with pytest.raises(NotImplementedError, match="backward is not built"):
        head([cuda(xs[0])])
    # 27 logits in ld = 28: the pad column is computed from zero rows
    head3, _ = _head(g, num_classes=4)
    assert head3.ld_cls == 28 and tuple(head3.cls_logits.weight.shape) == (28, 3, 3, 16)
    with torch.no_grad():
        cls3, _ = head3.forward_nhwc(cuda(xs[0]))
        l3, _ = head3([cuda(xs[0])])
    assert tuple(cls3.shape) == (2, 6, 8, 28) and not cls3[..., 27].any() and tuple(l3[0].shape) == (2, 27, 6, 8)
    _rule(N(l3[0]), want_l[0][:, :27], tol, "27 of the 36 logit rows")
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    from abr_iod_amd import ops
    assert set_conv_math(head, ops.MATH_F16X3) >= 1 and head.math == ops.MATH_F16X3


# ----------------------------------------------------------------------------------------------------------------- whole model
@pytest.fixture(scope="module")
def tiny():
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.structures.image_list import to_image_list
    c = cfg.clone()
    c.merge_from_list(["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", "R-50-FPN-RETINANET", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16,
                       "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16,
                       "MODEL.RETINANET.NUM_CLASSES", R.C + 1, "MODEL.RETINANET.NUM_CONVS", 2, "MODEL.RETINANET.ANCHOR_SIZES", R.SIZES,
                       "MODEL.RETINANET.PRE_NMS_TOP_N", 60, "TEST.DETECTIONS_PER_IMG", 40])
    torch.manual_seed(0)
    model = build_detection_model(c)
    head = model.rpn.head
    with torch.no_grad():      # a head whose logits spread over several units: the fresh one (std 0.01, bias -4.6) passes nothing
        for conv in (head.cls_tower[0], head.cls_tower[2], head.bbox_tower[0], head.bbox_tower[2]):
            conv.weight.mul_(12.0)
        head.cls_logits.weight.mul_(40.0)
        head.cls_logits.bias[:36].fill_(-2.0)
        head.bbox_pred.weight.mul_(10.0)
    bump_param_version()
    model.eval()
    gen = torch.Generator().manual_seed(3)
    images = [torch.randn(3, 128, 192, generator=gen).cuda() * 40, torch.randn(3, 112, 160, generator=gen).cuda() * 40]
    batch = to_image_list(images, 64)
    return c, model, batch


def test_tiny_detector_in_eval(tiny):
    c, model, batch = tiny
    model.eval()
    with torch.no_grad():
        dets, feats, background = model(batch)
        (boxes, losses), anchors, (box_cls, box_reg) = model.rpn(batch, feats)
    assert background is None and losses == {} and len(dets) == 2
    assert [tuple(f.shape) for f in feats] == [(2, 16) + m for m in R.MAPS]
    assert [tuple(t.shape) for t in box_cls] == [(2, 36) + m for m in R.MAPS] and [tuple(t.shape) for t in box_reg] == [(2, 36) + m for m in R.MAPS]
    cls = [N(t.permute(0, 2, 3, 1)).reshape(2, -1, 36) for t in box_cls]
    reg = [N(t.permute(0, 2, 3, 1)).reshape(2, -1, 36) for t in box_reg]
    grids = [N(anchors[0][l].bbox) for l in range(5)]
    for l, a in enumerate(R.pyramid_anchors()):            # the generator's grid on the device = the golden's anchors, to the bit
        assert np.array_equal(grids[l].view(np.uint32), a.view(np.uint32)), l
    want = R.detect_ref(cls, reg, grids, R.A, R.C, R.IMAGE_SIZES, c.MODEL.RETINANET.INFERENCE_TH, 60, c.MODEL.RETINANET.NMS_TH, 40)
    print("candidates per segment", [[s["n_cand"] for s in w["segments"]] for w in want], "after NMS", [w["n_nms"] for w in want])
    assert all(w["n_nms"] > 40 for w in want) and any(s["n_cand"] > 60 for w in want for s in w["segments"])       # both cuts are active
    for i, (b, b2) in enumerate(zip(dets, boxes)):
        assert b.size == (R.IMAGE_SIZES[i][1], R.IMAGE_SIZES[i][0]) and sorted(b.fields()) == ["labels", "scores"]
        got = dict(boxes=N(b.bbox), scores=N(b.get_field("scores")), labels=N(b.get_field("labels")))
        check(got, want[i], i)
        assert torch.equal(b.bbox, b2.bbox) and torch.equal(b.get_field("labels"), b2.get_field("labels"))
    model.train()
    with pytest.raises(NotImplementedError, match="the RetinaNet loss is not built"):
        model(batch, targets=[None, None])
    with pytest.raises(NotImplementedError, match="the RetinaNet loss is not built"):
        model(batch)


def test_inference_loop_runs_a_retinanet_model(tiny):
    """engine/inference.py over a (two-batch) data loader: no background results, no mask packing, BoxLists on the host keyed by image id"""
    from abr_iod_amd.engine.inference import compute_on_dataset
    c, model, batch = tiny
    with torch.no_grad():
        model.eval()
        want = model(batch)[0]
    class Loader(list):
        dataset = None      # (asked for an image's size only where an output carries pasted masks: none does)
    results, background = compute_on_dataset(model, Loader([(batch, None, [7, 9]), (batch, None, [11, 12])]), torch.device("cuda"), pack_masks=True)
    assert sorted(results) == [7, 9, 11, 12] and background == {7: None, 11: None}
    for k, i in ((7, 0), (9, 1), (11, 0), (12, 1)):
        b = results[k]
        assert b.bbox.device.type == "cpu" and sorted(b.fields()) == ["labels", "scores"] and len(b) == len(want[i]) > 0
        assert torch.equal(b.bbox, want[i].bbox.cpu()) and torch.equal(b.get_field("labels"), want[i].get_field("labels").cpu())

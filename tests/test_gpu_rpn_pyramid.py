"""GPU: RPN proposal selection over a feature pyramid (csrc/rpn_pyramid.hip: abr_rpn_pyramid_topk / _decode / _select; the multi-level
AnchorGenerator, RPNPostProcessor and RPNModule of modeling/rpn/rpn.py) against the single-level operators it must equal bit for bit, the numpy
restatement of tests/rpn_fpn_ref.py and the golden the reference's own code wrote (tests/golden/rpn_fpn.npz).

Index comparisons are exact: the logits come from ranking_ref's small value sets (no order hangs on an expf rounding), the restatement's tie
rule is the library's documented one, and the set builders redraw anything whose NMS or MIN_SIZE decision lies near its threshold."""
import numpy as np
import pytest
import torch

import ranking_ref as R
import rpn_fpn_ref as F

pytestmark = pytest.mark.gpu


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------------------------------------------------------------------- ranking
def pyramid_logits(seed, N, A, ld, nlocs, sets):
    rng = np.random.default_rng(seed)
    return [R.embed(rng, R.draw(rng, s, (N, nloc * A)), A, ld) for nloc, s in zip(nlocs, sets)]


def topk_pyramid_exact(ys_np, A, pre, tag):
    """one pyramid call, every level checked index for index against ranking_ref.topk_ref and bit for bit against ops.topk_sigmoid"""
    from abr_iod_amd import ops
    ys = [cuda(y) for y in ys_np]
    sc, idx = ops.rpn_pyramid_topk(ys, [A] * len(ys), pre)
    N = ys[0].shape[0]
    ks = [min(pre, y.shape[1] * A) for y in ys]
    assert tuple(sc.shape) == tuple(idx.shape) == (N, len(ys), max(ks)) and idx.dtype == torch.int64
    for l, (y_np, y, k) in enumerate(zip(ys_np, ys, ks)):
        ref_i, _ = R.topk_ref(y_np, A, k)
        assert torch.equal(idx[:, l, :k].cpu(), torch.from_numpy(ref_i)), (tag, l)
        want_s = torch.sigmoid(y[:, :, :A].reshape(N, -1)).gather(1, cuda(ref_i))
        assert torch.allclose(sc[:, l, :k], want_s, rtol=2e-7, atol=0), (tag, l)
        one_s, one_i = ops.topk_sigmoid(y, A, k)
        assert torch.equal(sc[:, l, :k], one_s) and torch.equal(idx[:, l, :k], one_i), (tag, l)
        assert not sc[:, l, k:].any() and not idx[:, l, k:].any(), (tag, l)          # entries past k_l are zero
    return sc, idx


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A,ld", [(3, 16), (1, 1)])
def test_pyramid_topk_equals_the_reference_order_per_level(N, A, ld):
    """levels with n > k and n no multiple of 64, n < pre (all taken), n = 6 and a single location; every value set, the all-equal one
    included (the cut then falls on the index bits alone)"""
    nlocs = [701, 50, 6 // A if A > 1 else 6, 1]
    sets = ["halves", "one_bin", "specials", "const"]
    for r in range(4):
        rot = sets[r:] + sets[:r]
        topk_pyramid_exact(pyramid_logits(10 * N + r, N, A, ld, nlocs, rot), A, 200, (N, A, r))


def test_pyramid_topk_at_its_cap_and_beyond():
    from abr_iod_amd import ops
    cap = ops.rpn_pyramid_max_k()
    assert cap == 2048
    ys = pyramid_logits(5, 2, 3, 16, [1700, 300], ["const", "halves"])       # 5100 equal keys cut at 2048, and a level taken whole
    topk_pyramid_exact(ys, 3, cap, "cap")
    with pytest.raises(RuntimeError, match="in-LDS sort"):
        ops.rpn_pyramid_topk([cuda(y) for y in ys], [3, 3], cap + 1)


def test_pyramid_topk_single_level_equals_topk_sigmoid():
    from abr_iod_amd import ops
    rng = np.random.default_rng(3)
    y = cuda(R.embed(rng, R.draw(rng, "halves", (2, 1200 * 3)), 3, 16))
    sc, idx = ops.rpn_pyramid_topk([y], [3], 500)
    one_s, one_i = ops.topk_sigmoid(y, 3, 500)
    assert torch.equal(sc[:, 0], one_s) and torch.equal(idx[:, 0], one_i)


def test_pyramid_topk_scratch_survives_changing_pyramids():
    """a larger pyramid, a smaller one, another batch size, the larger one again on one stream: every call checked"""
    big = pyramid_logits(1, 3, 3, 16, [2000, 500, 120, 30, 8], ["halves", "one_bin", "const", "specials", "halves"])
    small = pyramid_logits(2, 1, 3, 16, [40, 3], ["const", "halves"])
    mid = pyramid_logits(3, 2, 1, 1, [900, 77, 5], ["one_bin", "halves", "const"])
    for tag, ys, A, pre in (("big", big, 3, 1000), ("small", small, 3, 1000), ("mid", mid, 1, 300), ("small2", small, 3, 7), ("big2", big, 3, 1000)):
        topk_pyramid_exact(ys, A, pre, tag)


# ---------------------------------------------------------------------------------------------------------------------------- decode
def decode_case(seed, image_sizes, min_size, maps=((12, 18), (6, 9), (3, 5), (1, 2)), A=3, pre=150):
    ys, anchors, levels = F.tie_heavy_inputs(seed, maps, A, image_sizes, pre, 40, 0.7, min_size)
    return ys, anchors, levels, A, pre


def run_decode(ys_np, anchors_np, A, pre, image_sizes, min_size):
    from abr_iod_amd import ops
    ys, anchors = [cuda(y) for y in ys_np], [cuda(a) for a in anchors_np]
    sc, idx = ops.rpn_pyramid_topk(ys, [A] * len(ys), pre)
    img_hw = torch.tensor(image_sizes, dtype=torch.int32, device="cuda")
    props, sc2, counts = ops.rpn_pyramid_decode(ys, [A] * len(ys), anchors, idx, sc, img_hw, pre, (1.0, 1.0, 1.0, 1.0), min_size)
    singles = [ops.rpn_decode_clip(y, A, a, idx[:, l, :min(pre, y.shape[1] * A)].contiguous(), img_hw, (1.0, 1.0, 1.0, 1.0), A=A)
               for l, (y, a) in enumerate(zip(ys, anchors))]
    return sc, idx, props, sc2, counts, singles


def test_pyramid_decode_without_min_size_equals_rpn_decode_clip():
    sizes = ((48, 72), (40, 64), (48, 70))
    ys, anchors, _, A, pre = decode_case(11, sizes, 0)
    sc, idx, props, sc2, counts, singles = run_decode(ys, anchors, A, pre, sizes, 0)
    L = len(ys)
    for l, one in enumerate(singles):
        k = one.shape[1]
        for i in range(len(sizes)):
            assert torch.equal(props[i * L + l, :k], one[i]) and torch.equal(sc2[i * L + l, :k], sc[i, l, :k]), (i, l)
            assert int(counts[i * L + l]) == k
            assert not props[i * L + l, k:].any()


def test_pyramid_decode_min_size_compacts_in_rank_order():
    """MIN_SIZE = 8: the survivors of every segment are the restatement's, in rank order, without holes; the last image is smaller than
    MIN_SIZE, so every one of its segments ends empty"""
    sizes = ((48, 72), (40, 64), (6, 7))
    ys, anchors, levels, A, pre = decode_case(12, sizes, 8)
    sc, idx, props, sc2, counts, singles = run_decode(ys, anchors, A, pre, sizes, 8)
    L, dropped = len(ys), 0
    for l in range(L):
        for i in range(len(sizes)):
            alive = torch.from_numpy(levels[l][i]["alive"]).cuda()
            c, seg = int(counts[i * L + l]), i * L + l
            assert c == len(alive), (i, l)
            assert torch.equal(props[seg, :c], singles[l][i][alive]) and torch.equal(sc2[seg, :c], sc[i, l][alive]), (i, l)
            assert not props[seg, c:].any() and not sc2[seg, c:].any()
            np.testing.assert_allclose(props[seg, :c].cpu().numpy(), levels[l][i]["boxes"], rtol=1e-5, atol=2e-4)
            dropped += singles[l].shape[1] - c
    assert all(int(counts[2 * L + l]) == 0 for l in range(L)) and int(counts[:2 * L].min()) > 0
    assert dropped > sum(s.shape[1] for s in singles)          # more than the empty image's rows: the other images lost boxes too


def test_pyramid_decode_min_size_edge_is_inclusive():
    """zero deltas decode an integer anchor to itself: a side equal to MIN_SIZE stays, MIN_SIZE - 1 goes (either side)"""
    from abr_iod_amd import ops
    anchors = torch.tensor([[0, 0, 7, 7], [0, 0, 6, 6], [10, 10, 17, 16], [20, 20, 27, 27], [30, 30, 36, 37], [40, 40, 48, 47]],
                           dtype=torch.float32, device="cuda")
    y = torch.zeros((1, 6, 5), device="cuda")
    y[0, :, 0] = torch.tensor([5.0, 4.0, 3.0, 2.0, 1.0, 0.0])                      # rank order = anchor order
    sc, idx = ops.rpn_pyramid_topk([y], [1], 6)
    props, sc2, counts = ops.rpn_pyramid_decode([y], [1], [anchors], idx, sc, torch.tensor([[64, 64]], dtype=torch.int32, device="cuda"), 6,
                                                (1.0, 1.0, 1.0, 1.0), 8)
    assert int(counts[0]) == 3
    assert torch.equal(props[0, :3], anchors[[0, 3, 5]]) and torch.equal(sc2[0, :3], sc[0, 0, [0, 3, 5]])


# ---------------------------------------------------------------------------------------------------------------------------- selection
def synthetic_candidates(seed, N, L, post, k_max, n_keep, values):
    """props / scores [N*L,k_max,..], keep = the first post entries of a permutation per segment, n_keep as given; scores from `values`"""
    rng = np.random.default_rng(seed)
    S = N * L
    props = rng.random((S, k_max, 4)).astype(np.float32)
    scores = np.asarray(values, np.float32)[rng.integers(0, len(values), (S, k_max))]
    keep = np.stack([np.sort(rng.permutation(k_max)[:post]) for _ in range(S)]).astype(np.int32)
    return props, scores, keep, np.asarray(n_keep, np.int32).reshape(S)


def select_exact(props, scores, keep, n_keep, N, L, fpn, tag):
    from abr_iod_amd import ops
    post = keep.shape[1]
    cs = [np.concatenate([scores[i * L + l][keep[i * L + l, :n_keep[i * L + l]]] for l in range(L)]) for i in range(N)]
    cp = [np.concatenate([l * post + np.arange(n_keep[i * L + l]) for l in range(L)]).astype(np.int64) for i in range(N)]
    t = [cuda(x) for x in (props, scores, keep, n_keep)]
    for per_batch in (False, True):
        want = F.select_ref(cs, cp, L * post, fpn, per_batch)
        rois, sc, src, n_out = ops.rpn_pyramid_select(*t, N, fpn, per_batch)
        again = ops.rpn_pyramid_select(*t, N, fpn, per_batch)
        for a, b in zip((rois, sc, src, n_out), again):
            assert torch.equal(a, b), (tag, per_batch)                             # deterministic, padding included
        assert n_out.tolist() == [len(w) for w in want], (tag, per_batch, n_out.tolist(), [len(w) for w in want])
        for i, w in enumerate(want):
            got = src[i, :len(w)].cpu().numpy()
            assert np.array_equal(got, w), (tag, per_batch, i)
            seg, row = i * L + w // post, keep[i * L + w // post, w % post]
            assert np.array_equal(rois[i, :len(w)].cpu().numpy(), props[seg, row]) and np.array_equal(sc[i, :len(w)].cpu().numpy(), scores[seg, row])
            assert bool((src[i, len(w):] == -1).all()) and not rois[i, len(w):].any()
    return want


QUARTERS = [0.0, 0.25, 0.5, 0.75, 1.0, -0.5]


@pytest.mark.parametrize("total_minus_fpn", [-5, 0, 1])
def test_select_around_the_cut(total_minus_fpn):
    """fewer candidates than fpn_post_n, exactly as many, one more (per image in mode 0, over the batch in mode 1)"""
    N, L, post = 2, 3, 16
    n_keep = [16, 7, 0, 3, 16, 11]                                               # 23 and 30 candidates
    props, scores, keep, nk = synthetic_candidates(1, N, L, post, 40, n_keep, QUARTERS)
    for fpn in (23 - total_minus_fpn, 30 - total_minus_fpn, 53 - total_minus_fpn):
        select_exact(props, scores, keep, nk, N, L, fpn, (total_minus_fpn, fpn))


def test_select_cut_inside_tie_groups():
    """one score everywhere: the cut falls inside a tie group that spans the levels (mode 0) and the images (mode 1); then two values, the
    low one everywhere in image 1, which therefore receives nothing in mode 1; then an image without candidates"""
    N, L, post = 3, 2, 32
    props, scores, keep, nk = synthetic_candidates(2, N, L, post, 50, [20, 32, 32, 9, 4, 32], [0.5])
    for fpn in (25, 45, 70, 100):
        want = select_exact(props, scores, keep, nk, N, L, fpn, ("const", fpn))
    scores[2:4] = np.float32(0.25)
    want = select_exact(props, scores, keep, nk, N, L, 60, "starved")
    nk[2:4] = 0
    select_exact(props, scores, keep, nk, N, L, 40, "empty image")
    select_exact(props, scores, keep, np.zeros_like(nk), N, L, 40, "no candidates at all")
    assert want is not None


def test_select_beyond_the_lds_sort_size():
    """N = 4, L = 5, post = 1024: 20 480 candidates, more than one in-LDS sort holds"""
    N, L, post = 4, 5, 1024
    rng = np.random.default_rng(7)
    n_keep = rng.integers(900, 1025, N * L)
    n_keep[3] = 1024
    vals = (np.arange(0, 64) / 64.0).tolist()
    props, scores, keep, nk = synthetic_candidates(3, N, L, post, 1024, n_keep, vals)
    select_exact(props, scores, keep, nk, N, L, 2000, "large")


# ---------------------------------------------------------------------------------------------------------------------------- selector
def golden_case(gold):
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator
    from abr_iod_amd.structures.image_list import ImageList
    g = gold("rpn_fpn")
    L, N, A = len(F.MAPS), len(F.IMAGE_SIZES), len(F.RATIOS)
    ys = F.golden_fused([g["obj_%d" % l] for l in range(L)], [g["reg_%d" % l] for l in range(L)])
    fused = [cuda(y.reshape(N, H, W, 5 * A)).permute(0, 3, 1, 2) for y, (H, W) in zip(ys, F.MAPS)]      # logical NCHW, channels-last memory
    ag = AnchorGenerator(sizes=F.SIZES, aspect_ratios=F.RATIOS, anchor_strides=F.STRIDES, straddle_thresh=0).cuda()
    anchors = ag(ImageList(torch.zeros(N, 3, 128, 192, device="cuda"), list(F.IMAGE_SIZES)), fused)
    return g, ys, fused, anchors


def test_anchor_generator_five_levels_equals_the_reference(gold):
    g, _, _, anchors = golden_case(gold)
    assert len(anchors) == len(F.IMAGE_SIZES) and all(len(a) == len(F.MAPS) for a in anchors)
    for i in range(len(F.IMAGE_SIZES)):
        for l in range(len(F.MAPS)):
            bl = anchors[i][l]
            assert bl.size == (F.IMAGE_SIZES[i][1], F.IMAGE_SIZES[i][0])
            assert np.array_equal(bl.bbox.cpu().numpy(), g["anchors_%d" % l]), (i, l)
            assert np.array_equal(bl.get_field("visibility").cpu().numpy(), g["vis_%d_%d" % (i, l)].astype(bool)), (i, l)
            assert np.array_equal(bl._visibility_u8.cpu().numpy(), g["vis_%d_%d" % (i, l)]), (i, l)


def selector(train, per_batch, min_size, pre=F.PRE, post=F.POST, fpn=F.FPN_POST):
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.rpn.rpn import RPNPostProcessor
    pp = RPNPostProcessor(pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=F.NMS_THRESH, min_size=min_size, box_coder=BoxCoder((1., 1., 1., 1.)),
                          fpn_post_nms_top_n=fpn, fpn_post_nms_per_batch=per_batch)
    pp.train(train)
    return pp


@pytest.mark.parametrize("ms", [0, F.MIN_SIZE])
@pytest.mark.parametrize("mode,train,per_batch", [("train_batch", True, True), ("train_image", True, False), ("test", False, True)])
def test_selector_reproduces_the_reference_golden(gold, mode, train, per_batch, ms):
    from abr_iod_amd.structures.bounding_box import BoxList
    g, _, fused, anchors = golden_case(gold)
    A = len(F.RATIOS)
    targets = [BoxList(cuda(g["gt_%d" % i]), (w, h)) for i, (h, w) in enumerate(F.IMAGE_SIZES)]
    res = selector(train, per_batch, ms)(anchors, [f[:, :A] for f in fused], [f[:, A:] for f in fused], targets if train else None)
    for i, b in enumerate(res):
        wb, ws = g["boxes_%s_%d_%d" % (mode, ms, i)], g["scores_%s_%d_%d" % (mode, ms, i)]
        assert tuple(b.bbox.shape) == wb.shape, (mode, ms, i, b.bbox.shape, wb.shape)
        np.testing.assert_allclose(b.get_field("objectness").cpu().numpy(), ws, rtol=3e-7, atol=0)      # same order: scores line up one by one
        np.testing.assert_allclose(b.bbox.cpu().numpy(), wb, rtol=1e-5, atol=2e-4)


def tie_case(seed, min_size, pre=120, post=30):
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator
    from abr_iod_amd.structures.image_list import ImageList
    maps, A, sizes = ((14, 20), (7, 10), (4, 5), (2, 3)), 3, ((56, 80), (50, 76), (56, 66))
    ys, anchors_np, levels = F.tie_heavy_inputs(seed, maps, A, sizes, pre, post, F.NMS_THRESH, min_size)
    fused = [cuda(y.reshape(len(sizes), H, W, -1)).permute(0, 3, 1, 2) for y, (H, W) in zip(ys, maps)]
    ag = AnchorGenerator(sizes=F.SIZES[:4], aspect_ratios=F.RATIOS, anchor_strides=F.STRIDES[:4], straddle_thresh=0).cuda()
    anchors = ag(ImageList(torch.zeros(3, 3, 56, 80, device="cuda"), list(sizes)), fused)
    for l, a in enumerate(anchors_np):
        assert np.array_equal(anchors[0][l].bbox.cpu().numpy(), a)
    return ys, anchors_np, levels, fused, anchors, A, sizes, pre, post


def check_pending(pending, want):
    n_out = pending["n_out"].tolist()
    assert n_out == [len(w[2]) for w in want], (n_out, [len(w[2]) for w in want])
    for i, (wb, ws, wsrc) in enumerate(want):
        assert np.array_equal(pending["src"][i, :n_out[i]].cpu().numpy(), wsrc), i
        np.testing.assert_allclose(pending["objectness"][i, :n_out[i]].cpu().numpy(), ws, rtol=3e-7, atol=0)
        np.testing.assert_allclose(pending["rois"][i, :n_out[i]].cpu().numpy(), wb, rtol=1e-5, atol=2e-4)


@pytest.mark.parametrize("ms", [0, 12])
def test_selector_is_index_exact_on_tie_heavy_inputs(ms):
    ys, anchors_np, levels, fused, anchors, A, sizes, pre, post = tie_case(40 + ms, ms)
    for train, per_batch, fpn in ((True, True, 70), (True, False, 45), (False, True, 45), (False, True, 500)):
        want = F.pyramid_ref(ys, [A] * len(ys), anchors_np, sizes, pre, post, fpn, F.NMS_THRESH, ms, train and per_batch, levels=levels)
        pp = selector(train, per_batch, ms, pre, post, fpn)
        check_pending(pp.launch(anchors, fused, A), want)
        res = pp.forward_fused(anchors, fused, A)
        assert [len(b) for b in res] == [len(w[2]) for w in want]


def test_selector_side_stream_equals_direct_call():
    ys, anchors_np, levels, fused, anchors, A, sizes, pre, post = tie_case(41, 0)
    pp = selector(False, True, 0, pre, post, 45)
    direct = pp.forward_fused(anchors, fused, A)
    pending = pp.launch_on_side_stream(anchors, fused, A, tag="test-pyramid")
    assert "stream" in pending
    side = pp.collect(pending)
    assert "stream" not in pending
    for a, b in zip(direct, side):
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("objectness"), b.get_field("objectness"))


def test_selector_single_level_paths():
    """one level and MIN_SIZE = 0 keeps the single-level pending state (LazyProposals and ops.roi_head_targets read it); one level with
    MIN_SIZE > 0 goes through the pyramid kernels and equals the restatement, without a cross-level cut"""
    ys, anchors_np, levels, fused, anchors, A, sizes, pre, post = tie_case(42, 12)
    one = [[a[0]] for a in anchors]
    pending = selector(False, True, 0, pre, post, 5).launch(one, fused[0], A)
    assert {"props", "scores", "keep", "n_keep", "sizes", "fused"} <= set(pending) and "n_out" not in pending
    listed = selector(False, True, 0, pre, post, 5)(one, [fused[0][:, :A]], [fused[0][:, A:5 * A]])
    assert [len(b) for b in listed] == pending["n_keep"].tolist()
    want = F.pyramid_ref(ys[:1], [A], anchors_np[:1], sizes, pre, post, 5, F.NMS_THRESH, 12, False, levels=levels[:1])
    check_pending(selector(False, True, 12, pre, post, 5).launch(one, fused[0], A), want)


def test_selector_beyond_the_ranking_cap_uses_the_single_level_ranking():
    """pre_nms_top_n above abr_rpn_pyramid_max_k(): the levels are ranked by topk_sigmoid one by one, the rest of the path is the same"""
    maps, A, sizes, pre, post = ((27, 30), (4, 5)), 3, ((108, 120), (100, 110)), 2200, 50
    ys, anchors_np, levels = F.tie_heavy_inputs(43, maps, A, sizes, pre, post, F.NMS_THRESH, 0)
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator
    from abr_iod_amd.structures.image_list import ImageList
    fused = [cuda(y.reshape(2, H, W, -1)).permute(0, 3, 1, 2) for y, (H, W) in zip(ys, maps)]
    ag = AnchorGenerator(sizes=F.SIZES[:2], aspect_ratios=F.RATIOS, anchor_strides=F.STRIDES[:2], straddle_thresh=0).cuda()
    anchors = ag(ImageList(torch.zeros(2, 3, 108, 120, device="cuda"), list(sizes)), fused)
    want = F.pyramid_ref(ys, [A, A], anchors_np, sizes, pre, post, 60, F.NMS_THRESH, 0, False, levels=levels)
    check_pending(selector(False, True, 0, pre, post, 60).launch(anchors, fused, A), want)


# ---------------------------------------------------------------------------------------------------------------------------- module
def fpn_cfg():
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.MODEL.RPN.USE_FPN = True
    c.MODEL.RPN.ANCHOR_STRIDE, c.MODEL.RPN.ANCHOR_SIZES = F.STRIDES, F.SIZES
    c.MODEL.RPN.PRE_NMS_TOP_N_TEST, c.MODEL.RPN.POST_NMS_TOP_N_TEST, c.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = F.PRE, F.POST, F.FPN_POST
    return c


def test_rpn_module_eval_over_five_maps():
    """the shared head on five 64-channel maps, anchors and the multi-level selector: the proposals are the restatement's on the module's
    OWN head outputs (the conv is not judged here); training mode names the missing multi-level loss"""
    from abr_iod_amd.layers._layout import as_nhwc
    from abr_iod_amd.modeling.rpn.rpn import RPNModule
    from abr_iod_amd.structures.image_list import ImageList
    torch.manual_seed(0)
    m = RPNModule(fpn_cfg(), 64).cuda().eval()
    with torch.no_grad():
        for conv in (m.head.cls_logits, m.head.bbox_pred):
            conv.weight.mul_(20)                                               # (std 0.01 weights give near-constant objectness)
    N = len(F.IMAGE_SIZES)
    feats = [torch.randn(N, 64, H, W, device="cuda") for H, W in F.MAPS]
    images = ImageList(torch.zeros(N, 3, 128, 192, device="cuda"), list(F.IMAGE_SIZES))
    with torch.no_grad():
        (boxes, losses), anchors, (obj, reg) = m(images, feats)
    assert losses == {} and len(obj) == len(reg) == len(F.MAPS) and len(boxes) == N
    A = m.head.num_anchors
    ys = [torch.cat((as_nhwc(o), as_nhwc(r)), 3).reshape(N, -1, 5 * A).cpu().numpy() for o, r in zip(obj, reg)]
    anchors_np = [anchors[0][l].bbox.cpu().numpy() for l in range(len(F.MAPS))]
    levels = [F.level_ref(ys[l], A, anchors_np[l], F.IMAGE_SIZES, F.PRE, F.POST, F.NMS_THRESH, 0) for l in range(len(F.MAPS))]
    if F.near_threshold(levels, F.NMS_THRESH, 0):
        pytest.fail("the seeded head outputs put an NMS pair within 1e-5 of the threshold: choose another seed")
    want = F.pyramid_ref(ys, [A] * len(ys), anchors_np, F.IMAGE_SIZES, F.PRE, F.POST, F.FPN_POST, F.NMS_THRESH, 0, False, levels=levels)
    for b, (wb, ws, _) in zip(boxes, want):
        assert len(b) == len(ws)
        np.testing.assert_allclose(b.get_field("objectness").cpu().numpy(), ws, rtol=3e-7, atol=0)
        np.testing.assert_allclose(b.bbox.cpu().numpy(), wb, rtol=1e-5, atol=2e-4)
    m.train()
    with pytest.raises(NotImplementedError, match="multi-level RPN loss"):
        m(images, feats, targets=None)

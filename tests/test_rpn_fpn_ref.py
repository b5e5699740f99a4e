"""CPU: the numpy restatement of the multi-level RPN selection (tests/rpn_fpn_ref.py) against the golden written by the reference's own
AnchorGenerator + RPNPostProcessor (tests/golden/make_golden_rpn_fpn.py -> rpn_fpn.npz), the spacing of the golden's logit grid, and the
configuration plumbing of the feature-pyramid RPN (config keys, make_anchor_generator, make_rpn_postprocessor)."""
import numpy as np
import pytest

import rpn_fpn_ref as F

MODES = [("train_batch", True, True), ("train_image", True, False), ("test", False, False)]


@pytest.fixture(scope="module")
def case(gold):
    g = gold("rpn_fpn")
    L, N = len(F.MAPS), len(F.IMAGE_SIZES)
    ys = F.golden_fused([g["obj_%d" % l] for l in range(L)], [g["reg_%d" % l] for l in range(L)])
    anchors = [g["anchors_%d" % l] for l in range(L)]
    # (scores as the reference's float32 sigmoid gives them: the golden is compared exactly)
    levels = {ms: [F.level_ref(ys[l], len(F.RATIOS), anchors[l], F.IMAGE_SIZES, F.PRE, F.POST, F.NMS_THRESH, ms, F.torch_sigmoid)
                   for l in range(L)] for ms in (0, F.MIN_SIZE)}
    return dict(g=g, ys=ys, anchors=anchors, levels=levels, gt=[g["gt_%d" % i] for i in range(N)])


def test_logit_grid_neighbours_are_32_ulps_apart():
    """the reference ranks with torch.topk, whose tie order is undefined: the golden's logits are all different members of one grid whose
    float32 sigmoids no evaluation can confuse"""
    import ranking_ref as R
    s = R.sigmoid32(F.LOGIT_GRID)
    assert np.all(np.diff(F.LOGIT_GRID) > 0) and np.all(np.diff(s) > 0)
    ulps = np.diff(s.view(np.uint32).astype(np.int64))          # positive floats: the bit patterns count ulps
    assert ulps.min() >= 32, ulps.min()
    total = sum(len(F.IMAGE_SIZES) * H * W * len(F.RATIOS) for H, W in F.MAPS)
    assert len(F.LOGIT_GRID) >= total


def test_golden_logits_are_distinct_across_the_batch(case):
    codes = np.concatenate([case["g"]["obj_%d" % l].reshape(-1) for l in range(len(F.MAPS))])
    assert len(np.unique(codes)) == len(codes)
    assert not any(F.near_threshold(case["levels"][ms], F.NMS_THRESH, ms) for ms in (0, F.MIN_SIZE))


def test_oracle_anchors_equal_the_reference_generator(case):
    for i, hw in enumerate(F.IMAGE_SIZES):
        for l, (a, vis) in enumerate(F.pyramid_anchors(image_hw=hw)):
            assert np.array_equal(a, case["anchors"][l]), l
            assert np.array_equal(vis, case["g"]["vis_%d_%d" % (i, l)].astype(bool)), (i, l)


@pytest.mark.parametrize("ms", [0, F.MIN_SIZE])
@pytest.mark.parametrize("mode,train,per_batch", MODES)
def test_restatement_reproduces_the_reference(case, mode, train, per_batch, ms):
    g = case["g"]
    got = F.pyramid_ref(case["ys"], [len(F.RATIOS)] * len(F.MAPS), case["anchors"], F.IMAGE_SIZES, F.PRE, F.POST, F.FPN_POST, F.NMS_THRESH, ms,
                        per_batch, case["gt"] if train else None, levels=case["levels"][ms])
    for i, (boxes, scores, _) in enumerate(got):
        want_b, want_s = g["boxes_%s_%d_%d" % (mode, ms, i)], g["scores_%s_%d_%d" % (mode, ms, i)]
        assert boxes.shape == want_b.shape, (mode, ms, i)
        assert np.array_equal(scores, want_s), (mode, ms, i)        # same proposals in the same order: every score is unique
        np.testing.assert_allclose(boxes, want_b, rtol=1e-5, atol=2e-4)


def test_min_size_and_the_batch_cut_change_the_golden(case):
    """the stored modes are not copies of each other"""
    g = case["g"]
    assert len(g["scores_train_batch_0_0"]) + len(g["scores_train_batch_0_1"]) == F.FPN_POST + sum(len(x) for x in case["gt"])
    assert len(g["scores_test_0_0"]) == F.FPN_POST
    assert not np.array_equal(g["scores_test_0_0"], g["scores_test_%d_0" % F.MIN_SIZE])
    assert any(len(d["alive"]) < len(d["idx"]) for lev in case["levels"][F.MIN_SIZE] for d in lev)


def test_restatement_agrees_with_the_oracle_per_level(case):
    """a second opinion on the per-level half: oracle.torch_ref.rpn_post_process (float32 NMS of the C oracle, torch.topk)"""
    for l, (H, W) in enumerate(F.MAPS):
        want = F.cross_check_level(case["ys"][l], len(F.RATIOS), H, W, case["anchors"][l], F.IMAGE_SIZES, F.PRE, F.POST, F.NMS_THRESH, F.MIN_SIZE)
        for i, (wb, ws) in enumerate(want):
            d = case["levels"][F.MIN_SIZE][l][i]
            assert np.array_equal(d["scores"][d["keep"]], ws), (l, i)
            assert np.array_equal(d["boxes"][d["keep"]], wb), (l, i)


def test_select_ref_tie_rule():
    s = [np.array([0.5, 0.9, 0.5, 0.5], np.float32), np.array([0.5, 0.5], np.float32)]
    p = [np.array([0, 1, 60, 61]), np.array([0, 120])]
    assert [x.tolist() for x in F.select_ref(s, p, 300, 3, False)] == [[1, 0, 60], [0, 120]]
    assert [x.tolist() for x in F.select_ref(s, p, 300, 5, True)] == [[0, 1, 60, 61], [0]]
    assert [x.tolist() for x in F.select_ref(s, p, 300, 4, True)] == [[0, 1, 60, 61], []]


def test_fpn_rpn_configuration():
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator, make_anchor_generator, make_rpn_postprocessor
    assert cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN == 2000 and cfg.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST == 2000
    assert cfg.MODEL.RPN.FPN_POST_NMS_PER_BATCH is True
    c = cfg.clone()
    c.MODEL.RPN.USE_FPN = True
    c.MODEL.RPN.ANCHOR_STRIDE = F.STRIDES
    c.MODEL.RPN.ANCHOR_SIZES = F.SIZES
    ag = make_anchor_generator(c)
    assert ag.num_anchors_per_location() == [3] * 5
    for l, (st, s) in enumerate(zip(F.STRIDES, F.SIZES)):
        from oracle import ops as O
        assert np.array_equal(ag.level_cell_anchors(l).numpy(), O.cell_anchors(stride=st, sizes=(s,), ratios=F.RATIOS)), l
    assert AnchorGenerator(((32, 64), (128, 256)), (1.0,), (8, 16)).num_anchors_per_location() == [2, 2]     # a size may be a tuple
    with pytest.raises(RuntimeError, match="FPN should have #anchor_strides == #sizes"):
        AnchorGenerator((32, 64, 128), (0.5, 1.0, 2.0), (4, 8))
    one = cfg.clone()
    one.MODEL.RPN.USE_FPN = True                                   # one stride, five sizes
    with pytest.raises(AssertionError, match="FPN should have"):
        make_anchor_generator(one)
    many = cfg.clone()
    many.MODEL.RPN.ANCHOR_STRIDE = F.STRIDES                       # five strides without USE_FPN
    with pytest.raises(AssertionError, match="Non-FPN"):
        make_anchor_generator(many)
    assert make_anchor_generator(cfg).num_anchors_per_location() == [15]
    c.MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN, c.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST, c.MODEL.RPN.FPN_POST_NMS_PER_BATCH = 700, 300, False
    tr, te = (make_rpn_postprocessor(c, BoxCoder((1.0, 1.0, 1.0, 1.0)), t) for t in (True, False))
    assert (tr.fpn_post_nms_top_n, te.fpn_post_nms_top_n) == (700, 300)
    assert tr.fpn_post_nms_per_batch is False and te.fpn_post_nms_per_batch is False
    d = make_rpn_postprocessor(cfg, BoxCoder((1.0, 1.0, 1.0, 1.0)), True)
    assert d.fpn_post_nms_top_n == 2000 and d.fpn_post_nms_per_batch is True
    from abr_iod_amd.modeling.rpn.rpn import RPNPostProcessor
    assert RPNPostProcessor(100, 50, 0.7, 0).fpn_post_nms_top_n == 50      # defaults to post_nms_top_n (inference.py:48-50)


def test_pyramid_entry_points_check_their_arguments():
    """the argument checks sit in front of every allocation and launch, so they run without a GPU: level count, the ranking cap, k_max, the
    delta columns, the selection's mode and in-LDS sort, and N == 0 (nothing to do, no error)"""
    import ctypes as C
    from abr_iod_amd import _lib
    L = _lib.lib()
    err = lambda: L.abr_last_error().decode()                                                    # noqa: E731
    tab = lambda t, v: (t * len(v))(*v)                                                          # noqa: E731
    ptrs, nloc, A, ld = tab(C.c_void_p, [None, None]), tab(C.c_int, [1000, 10]), tab(C.c_int, [3, 3]), tab(C.c_int, [16, 16])
    assert L.abr_rpn_pyramid_max_k() == 2048
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, ld, 2, 0, 2000, 2000, None, None, None) == 0    # N == 0
    assert L.abr_rpn_pyramid_decode(ptrs, nloc, A, ld, ptrs, 2, 0, 2000, 2000, None, None, None, 1.0, 1.0, 1.0, 1.0, 0.0, None, None, None, None) == 0
    assert L.abr_rpn_pyramid_select(None, None, None, None, 0, 2, 2000, 1000, 2000, 1, None, None, None, None, None) == 0
    for bad_L in (0, 9):
        assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, ld, bad_L, 0, 2000, 2000, None, None, None) == -1 and "levels" in err()
        assert L.abr_rpn_pyramid_select(None, None, None, None, 0, bad_L, 2000, 1000, 2000, 0, None, None, None, None, None) == -1 and "levels" in err()
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, ld, 2, 0, 2049, 2049, None, None, None) == -1 and "in-LDS sort" in err()
    assert L.abr_rpn_pyramid_decode(ptrs, nloc, A, ld, ptrs, 2, 0, 2049, 2049, None, None, None, 1.0, 1.0, 1.0, 1.0, 0.0, None, None, None, None) == 0
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, ld, 2, 0, 2000, 1999, None, None, None) == -1 and "k_max" in err()
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, tab(C.c_int, [16, 2]), 2, 0, 2000, 2000, None, None, None) == -1 and "level 1" in err()
    narrow = tab(C.c_int, [16, 14])                                                               # 3 logits + 12 deltas need 15 columns
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, narrow, 2, 0, 2000, 2000, None, None, None) == 0
    assert L.abr_rpn_pyramid_decode(ptrs, nloc, A, narrow, ptrs, 2, 0, 2000, 2000, None, None, None, 1.0, 1.0, 1.0, 1.0, 0.0, None, None, None,
                                    None) == -1 and "delta columns" in err()
    assert L.abr_rpn_pyramid_topk(ptrs, nloc, A, ld, 2, 1, 2000, 2000, None, None, None) == -1 and "null pointer" in err()
    assert L.abr_rpn_pyramid_select(None, None, None, None, 1, 2, 2000, 1000, 2000, 2, None, None, None, None, None) == -1 and "bad args" in err()
    assert L.abr_rpn_pyramid_select(None, None, None, None, 1, 5, 2000, 1000, 5000, 0, None, None, None, None, None) == -1 and "in-LDS sort" in err()
    assert L.abr_rpn_pyramid_select(None, None, None, None, 1, 5, 2000, 1000, 5000, 1, None, None, None, None, None) == -1 and "null pointer" in err()
    assert L.abr_rpn_pyramid_select(None, None, None, None, 70000, 8, 2000, 4096, 5000, 1, None, None, None, None, None) == -1 and "int32" in err()

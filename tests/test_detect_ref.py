"""The float64 softmax / decode reference (tests/detect_ref.py), checked on the CPU before the GPU suite leans on it.

  * on EVERY case the GPU suite runs, the oracle's float32 restatement (oracle.torch_ref.det_softmax_decode: torch's softmax, the C
    box_decode, numpy's clip) lies inside the bounds the kernel is held to -- so the bounds can be met by an honest float32 evaluation and
    the reference computes the same function;
  * the case list contains what it claims: every family in the shape grid, subnormal and exactly-0 / exactly-1 probabilities, dw on both
    sides of the clamp, boxes clipped flat against each of the four sides, one-pixel and inverted proposals, the three odd image sizes;
  * the helpers of the selection tests do what they say (grid boxes never overlap, the oracle accepts C = 1 and an empty image)."""
import numpy as np
import pytest
import torch

import detect_ref as R
from oracle import ops as O
from oracle import torch_ref as T

CASES = R.softmax_cases()


def oracle_f32(case):
    reg = case.deltas
    return T.det_softmax_decode(torch.from_numpy(case.logits), torch.from_numpy(reg), R.proposals_per_image(case), case.sizes_wh,
                                R.WEIGHTS, cls_agnostic=case.cls_agnostic)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_fp32_lies_within_the_gpu_bounds(case):
    ref = R.softmax_decode_f64(case.logits, case.deltas, case.rois, case.img_hw, R.WEIGHTS, case.cls_agnostic)
    prob, boxes = oracle_f32(case)
    K = sum(case.counts)
    assert prob.shape == (K, case.C) and boxes.shape == (K, case.C, 4) and prob.dtype == np.float32 and boxes.dtype == np.float32
    assert np.isfinite(ref.prob).all() and np.isfinite(ref.boxes).all()
    fp, up, fb, ub = R.measure(prob, boxes, ref)
    print("{}: prob {:.2f} ulp ({:.2f} of its bound), boxes {:.2f} EPS*mag ({:.2f} of the bound 8)".format(case.name, up / 2, fp, ub, fb))
    assert (np.abs(prob.astype(np.float64) - ref.prob) <= R.prob_bound(ref)).all()
    assert (np.abs(boxes.astype(np.float64) - ref.boxes) <= R.box_bound(ref)).all()


def test_clamp_constant_is_the_float32_one():
    assert R.CLIP32 == np.float32(4.135166556742356) and R.CLIP == float(np.float32(np.log(1000.0 / 16)))
    assert R.CLIP != np.log(1000.0 / 16)                 # the float64 logarithm is a different number: the reference must not use it


def test_clamp_probe_sits_one_float_either_side():
    c = R.clamp_probe()
    q = c.deltas[:, 2] / np.float32(5)
    assert q[0] == np.nextafter(R.CLIP32, np.float32(0)) and q[1] == R.CLIP32 and q[2] == np.nextafter(R.CLIP32, np.float32(9))
    _, b = oracle_f32(c)
    assert np.array_equal(b[1], b[2]) and (b[0, 0, 2:] < b[1, 0, 2:]).all() and (b[:, 0, :2] == 0).all()
    ref = R.softmax_decode_f64(c.logits, c.deltas, c.rois, c.img_hw)
    assert (ref.boxes[0, 0, 2:] < ref.boxes[1, 0, 2:]).all()     # (rows 1 and 2 may differ in float64: delta / 5 is not rounded there)
    # one float of dw is 4 ulps of e^dw, 8 ulps of x2 = 2031.0 in float32 (6 here, where delta / 5 is not rounded): far more than expf()'s
    # one ulp can hide
    assert ref.boxes[1, 0, 2] - ref.boxes[0, 0, 2] > 6 * 2.0 ** -13 and 2030.99 < ref.boxes[1, 0, 2] < 2031.01


def _case(name):
    return next(c for c in CASES if c.name == name)


def test_logit_families_reach_their_edges():
    tiny = 2.0 ** -126
    p = R.softmax_decode_f64(*_case("logits-plus88")[4:8]).prob
    assert ((p > 0) & (p < tiny)).sum() >= 18 * 257        # the losers sit around e^-88 = 6e-39: nearly all subnormal in float32
    assert (p.astype(np.float32)[(p > 0) & (p < tiny)] > 0).all()
    p = R.softmax_decode_f64(*_case("logits-plus1e4")[4:8]).prob
    assert ((p == 0).sum(1) == 20).all() and ((p == 1).sum(1) == 1).all()
    p = R.softmax_decode_f64(*_case("logits-minus100")[4:8]).prob
    assert (((p > 0) & (p < tiny)).sum(1) == 1).all()
    x = _case("logits-equal").logits
    assert (x == x[:, :1]).all()
    for c in CASES:
        assert np.isfinite(c.logits).all() and np.isfinite(c.deltas).all()


def test_delta_families_reach_their_edges():
    c = _case("deltas-clamp")
    q = c.deltas.reshape(-1, 21, 4)[..., 2].astype(np.float64) / 5.0
    assert (q > R.CLIP).any() and (q < R.CLIP).any() and (np.abs(q - R.CLIP) < 1e-6).all()
    at = R.CLIP32 * np.float32(5)
    assert set(np.unique(c.deltas.reshape(-1, 21, 4)[..., 2:]).tolist()) == {float(at), float(np.nextafter(at, np.float32(99))),
                                                                             float(np.nextafter(at, np.float32(0)))}
    c = _case("deltas-pm60")
    assert set(np.unique(c.deltas.reshape(-1, 21, 4)[..., 2]).tolist()) == {60.0, -60.0, 300.0, -300.0}
    for name, col, hi in (("out_left", 0, False), ("out_right", 0, True), ("out_top", 1, False), ("out_bottom", 1, True)):
        c = _case("deltas-" + name)
        b = R.softmax_decode_f64(c.logits, c.deltas, c.rois, c.img_hw).boxes
        W1 = (c.img_hw[c.rois[:, 0].astype(int), 1 - col] - 1).astype(np.float64)[:, None]
        ext = c.rois[:, 3 + col].astype(np.float64) - c.rois[:, 1 + col] + 1
        live = ext != 0                                    # a proposal of width 0 cannot be moved by dx: it decodes to a point
        want = W1 if hi else np.zeros_like(W1)
        assert live.sum() > 200
        assert (b[live][..., col] == want[live]).all() and (b[live][..., col + 2] == want[live]).all(), name


def test_proposal_families_and_images():
    r = _case("props-one_pixel").rois
    assert (r[:, 3] == r[:, 1]).all() and (r[:, 4] == r[:, 2]).all()
    r = _case("props-inverted").rois
    assert (r[:, 3] <= r[:, 1]).all() and (r[:, 3] < r[:, 1]).any() and (r[:, 3] - r[:, 1] + 1 < 0).any()
    c = _case("props-border")
    hw = c.img_hw[c.rois[:, 0].astype(int)]
    r = c.rois
    assert ((r[:, 1] == 0) | (r[:, 2] == 0) | (r[:, 3] == hw[:, 1] - 1) | (r[:, 4] == hw[:, 0] - 1)).all()
    for c in CASES:
        assert (c.rois[:, 1:] >= 0).all()
        assert c.counts[0] == 0 and c.counts[3] == 0 and c.counts[-1] == 0          # empty images first, in the middle and last
        assert [tuple(s) for s in c.sizes_wh][2] == (1, 1) and (7, 1000) in c.sizes_wh and (600, 9) in c.sizes_wh
    big = _case("shape-C21-K1000")
    assert set(f[0] for f in big.families) == set(R.LOGIT_FAMILIES) and set(f[1] for f in big.families) == set(R.DELTA_FAMILIES)
    assert set(f[2] for f in big.families) == set(R.PROP_FAMILIES) and len(set(big.families)) > 100
    assert all(n > 0 for i, n in enumerate(big.counts) if i in (1, 2, 4, 5))
    assert sorted(set((c.C, sum(c.counts)) for c in CASES if c.name.startswith("shape"))) == \
        [(C, K) for C in (1, 2, 21, 81) for K in (0, 1, 255, 256, 257, 1000)]


def test_grid_boxes_never_overlap():
    b = R.grid_boxes(16384, 1)[:, 0]
    assert (b == np.round(b)).all() and b.max() < 2 ** 10 and len(np.unique(b, axis=0)) == 16384
    sub = np.concatenate([b[:300], b[16000:]])
    iou = O.box_iou(sub, sub)
    assert (iou[~np.eye(len(sub), dtype=bool)] == 0).all() and (np.diag(iou) == 1).all()
    assert len(O.nms(b[:3000], np.full(3000, 0.5, np.float32), 0.5)) == 3000


def test_oracle_filter_takes_one_class_and_empty_images():
    b = R.grid_boxes(5, 1)
    p = np.float32([[0.5], [0.01], [0.7], [0.5], [0.06]])
    (rb, rs, rl), (gb, gs) = T.det_filter_results(p, b, 0.05, 0.5, 100)
    assert rb.shape == (0, 4) and rs.shape == (0,) and rl.shape == (0,) and rl.dtype == np.int64
    assert gs.tolist() == p[[0, 2, 3, 4], 0].tolist() and np.array_equal(gb, b[[0, 2, 3, 4], 0])
    (rb, rs, rl), (gb, gs) = T.det_filter_results(np.zeros((0, 3), np.float32), np.zeros((0, 3, 4), np.float32), 0.05, 0.5, 100)
    assert len(rs) == 0 and len(gs) == 0 and rb.shape == (0, 4) and gb.shape == (0, 4)

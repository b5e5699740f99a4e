"""GPU: the detection post-processing kernels (abr_iod_amd/csrc/detect.hip) at their edges.

SOFTMAX + DECODE against the float64 reference of tests/detect_ref.py, EPS = 2^-24 (half a float32 ulp):

  prob   |got - want| <= EPS (|x_j - max_c x_c| + C + 4) want + 2^-126
         -- the rounding of x - max enters the exponent absolutely, so it is a RELATIVE error of EPS |x - max| on exp();
         -- a positive sum of C terms adds at most (C - 1) EPS;
         -- two expf() (numerator, and the terms of the sum) at one ulp = 2 EPS each and one division at EPS make up the 4 (+1 in C);
         -- 2^-126 is the floor for results that underflow into the subnormal range, where an ulp is absolute (2^-149).
  boxes  |err| <= 8 EPS (|dx| w + |cx| + 0.5 e^dw w (1 + |dw|) + 1)   for x1 / x2, likewise with dy, h, cy, dh for y1 / y2
         -- w = x2 - x1 + 1 is two roundings (2 EPS w), dx = d / weight one, the product one and cx = x1 + 0.5 w carries w's: the
            centre pcx = dx w + cx has at most 5 EPS |dx| w + 4 EPS |cx| + EPS;
         -- e^dw w: expf() 2 EPS, the rounding of dw = d / weight enters the exponent absolutely (EPS |dw|), w 2 EPS, the product 1:
            (5 + |dw|) EPS on 0.5 e^dw w;
         -- the corner's subtraction and the `- 1` add one EPS each on what they produce (the `+ 1`);
         -- 8 covers the sum with room for nothing else; clipping is a clamp to exact bounds, which never increases an error.
  The worst measured values are printed per case; on the MI355X (both layouts, all cases): prob at most 0.63 of its bound (C = 2,
  K = 1000; the worst in ulps is 32.4 = 65 EPS at C = 81, K = 1000, on a loser of a `plus88` row that is still normal: |x - max| = 88
  is the bound's leading term there and the rounding of that subtraction is the error), boxes at most 2.88 EPS mag of the 8 allowed.
  Per family (C = 21, K = 257): logits normal 8.2 ulp / equal 0.2 / plus88 32.3 / plus1e4 0 / minus100 2.1; boxes, deltas normal 2.46
  EPS mag / clamp 1.13 / pm60 2.46 / out_* 2.58 - 2.63; proposals normal 2.49 / one_pixel 2.67 / inverted 2.78 / border 2.60.

DET_SELECT against oracle.torch_ref.det_filter_results on bit-identical prob / boxes: labels, scores, boxes, their order, the counts
and the background list are equal bit for bit.  Cases that are not about NMS use integer boxes on a non-overlapping grid (every IoU is
exactly 0); the NMS cases use integer corners (intersection and union are exact integers, one correctly rounded division each side)
and exact duplicates.

Found and fixed while writing this suite:
  * PostProcessor.forward raised on a batch without a single proposal (`reshape(0, -1)` cannot infer the width);
  * oracle.torch_ref.det_filter_results raised for C = 1 (concatenating the empty list of foreground classes);
  * the launcher ignored hipFuncSetAttribute's result for both LDS requests; it now asks for both before the first launch and refuses
    with a message if the device says no.
"""
import numpy as np
import pytest
import torch

import detect_ref as R

pytestmark = pytest.mark.gpu

CASES = R.softmax_cases()
THRESH = float(np.float32(0.05))


# ------------------------------------------------------------------------------------------------------------------ softmax + decode
def _ref(case):
    return R.softmax_decode_f64(case.logits, case.deltas, case.rois, case.img_hw, R.WEIGHTS, case.cls_agnostic)


def _fused(case, pad=3):
    """one [K, C + ncols + pad] device matrix with NaN in the padding: what a kernel reads beyond its columns would poison the result"""
    K = sum(case.counts)
    f = np.concatenate([case.logits, case.deltas, np.full((K, pad), np.nan, np.float32)], 1)
    return torch.from_numpy(f).cuda()


def _check(got_prob, got_boxes, ref, tag):
    p, b = got_prob.cpu().numpy(), got_boxes.cpu().numpy()
    assert p.shape == ref.prob.shape and b.shape == ref.boxes.shape and p.dtype == np.float32 and b.dtype == np.float32
    fp, up, fb, ub = R.measure(p, b, ref)
    print("{}: prob {:.2f} ulp ({:.2f} of its bound), boxes {:.2f} EPS*mag (of 8)".format(tag, up / 2, fp, ub))
    assert (np.abs(p.astype(np.float64) - ref.prob) <= R.prob_bound(ref)).all(), tag
    assert (np.abs(b.astype(np.float64) - ref.boxes) <= R.box_bound(ref)).all(), tag
    return p, b


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_softmax_decode_vs_float64(case):
    """contiguous inputs and column slices of one fused matrix (incl. the K == 1 slice, whose row stride torch reports arbitrarily)"""
    from abr_iod_amd import ops
    ref = _ref(case)
    C, ncol = case.C, case.deltas.shape[1]
    rois, hw = torch.from_numpy(case.rois).cuda(), torch.from_numpy(case.img_hw).cuda()
    p1, b1 = ops.det_softmax_decode(torch.from_numpy(case.logits).cuda(), torch.from_numpy(case.deltas).cuda(), rois, C, hw, R.WEIGHTS,
                                    cls_agnostic=case.cls_agnostic)
    p1, b1 = _check(p1, b1, ref, case.name + " contiguous")
    f = _fused(case)
    p2, b2 = ops.det_softmax_decode(f[:, :C], f[:, C:C + ncol], rois, C, hw, R.WEIGHTS, cls_agnostic=case.cls_agnostic)
    p2, b2 = _check(p2, b2, ref, case.name + " fused")
    assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)) and np.array_equal(b1.view(np.uint32), b2.view(np.uint32))
    if case.name == "logits-plus1e4":
        assert ((p1 == 0).sum(1) == C - 1).all() and ((p1 == 1).sum(1) == 1).all()


@pytest.mark.parametrize("name", ["shape-C21-K257", "agnostic-4C", "agnostic-4col", "shape-C2-K1"])
def test_softmax_decode_delta_col0_through_the_c_abi(name):
    """logits AND deltas given as the base of the fused matrix, the deltas' first column as `delta_col0` (agnostic: the last four)"""
    from abr_iod_amd import _lib as L
    case = next(c for c in CASES if c.name == name)
    ref = _ref(case)
    C, ncol, K = case.C, case.deltas.shape[1], sum(case.counts)
    f = _fused(case)
    rois, hw = torch.from_numpy(case.rois).cuda(), torch.from_numpy(case.img_hw).cuda()
    prob = torch.empty((K, C), dtype=torch.float32, device="cuda")
    boxes = torch.empty((K, C, 4), dtype=torch.float32, device="cuda")
    ld = f.shape[1]
    L.check(L.lib().abr_det_softmax_decode(L.ptr(f), ld, L.ptr(f), ld, C, ncol - 4 if case.cls_agnostic else -1, L.ptr(rois), K, C, L.ptr(hw),
                                           *R.WEIGHTS, L.ptr(prob), L.ptr(boxes), L.stream()), "det_softmax_decode")
    _check(prob, boxes, ref, name + " delta_col0={}".format(C))


def test_decode_clamp_to_the_float():
    """dw = dh one float below the clamp, at it and one float above it, on a proposal where everything but expf() is exact (w = 64,
    cx = 32, no shift): at and above decode to the same bits, below is narrower -- a clamp constant that is off by one float32 in either
    direction breaks one of the two.  (The error bound cannot see that: one float of dw moves x2 by 8 of the 40 EPS mag it allows.)"""
    from abr_iod_amd import ops
    c = R.clamp_probe()
    prob, box = ops.det_softmax_decode(torch.from_numpy(c.logits).cuda(), torch.from_numpy(c.deltas).cuda(), torch.from_numpy(c.rois).cuda(), 1,
                                       torch.from_numpy(c.img_hw).cuda(), R.WEIGHTS)
    _, b = _check(prob, box, _ref(c), c.name)
    assert np.array_equal(_bits(b[1]), _bits(b[2]))
    assert (b[0, 0, 2:] < b[1, 0, 2:]).all() and (b[:, 0, :2] == 0).all() and (prob.cpu().numpy() == 1).all()


# ------------------------------------------------------------------------------------------------------------------ det_select
def _oracle(prob, boxes, counts, thresh, nms_t, D):
    from oracle import torch_ref as T
    off = R.offsets(counts)
    return [T.det_filter_results(prob[off[i]:off[i + 1]], boxes[off[i]:off[i + 1]], thresh, nms_t, D) for i in range(len(counts))]


def _select(prob, boxes, counts, thresh, nms_t, D, background=True):
    from abr_iod_amd import ops
    out = ops.det_select(torch.from_numpy(prob).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(R.offsets(counts)).cuda(),
                         len(counts), prob.shape[1], max(counts), thresh, nms_t, D, background=background)
    return [None if t is None else t.cpu().numpy() for t in out]


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_equal(out, want, tag, background=True):
    ob, os_, ol, oc, bb, bs, bc = out
    for i, ((rb, rs, rl), (gb, gs)) in enumerate(want):
        n = int(oc[i])
        assert n == len(rs), (tag, i, n, len(rs))
        assert np.array_equal(ol[i, :n], rl), (tag, i)
        assert np.array_equal(_bits(os_[i, :n]), _bits(rs)), (tag, i)
        assert np.array_equal(_bits(ob[i, :n]), _bits(rb).reshape(-1, 4)), (tag, i)
        if background:
            m = int(bc[i])
            assert m == len(gs), (tag, i, m, len(gs))
            assert np.array_equal(_bits(bs[i, :m]), _bits(gs)) and np.array_equal(_bits(bb[i, :m]), _bits(gb).reshape(-1, 4)), (tag, i)
    return [int(v) for v in oc]


def _check_select(prob, boxes, counts, thresh, nms_t, D, tag):
    want = _oracle(prob, boxes, counts, thresh, nms_t, D)
    return _assert_equal(_select(prob, boxes, counts, thresh, nms_t, D), want, tag), want


def _int_boxes(rng, n, C, dup=0.25):
    """[n, C, 4] integer-cornered boxes that overlap a lot; a quarter of the rows repeat an earlier row exactly (per class)"""
    x1, y1 = rng.integers(0, 200, (n, C)), rng.integers(0, 120, (n, C))
    b = np.stack([x1, y1, x1 + rng.integers(0, 80, (n, C)), y1 + rng.integers(0, 80, (n, C))], -1).astype(np.float32)
    for j in range(C):
        for t in np.nonzero(rng.random(n) < dup)[0]:
            if t:
                b[t, j] = b[rng.integers(0, t), j]
    return b


@pytest.mark.parametrize("r_max", [1, 2, 1023, 1024, 1025, 2500, 4096, 4097, 8193, 16384])
def test_select_every_admitted_row_count(r_max):
    """C = 3, images of r_max, 0 and (r_max + 1) / 2 rows.  Up to 2500 every row passes the threshold and survives NMS (at 2500: 5000
    detections in image 0, so the multi-chunk compaction, `pos0 += tot`, and the cut see more than 1024 entries per class); above, about
    2000 rows per class pass, spread over the whole index range with the last row among them.  Scores are multiples of 1/64: long tie
    groups in the sort (equal scores by ascending proposal) and at the cut.  With D = 100 and without a cut.
    m > 1024 runs the multi-element bitonic sort, r_max > 4096 asks for more than 48 KB of LDS for it (128 KB at 16384), r_max > 8192
    for more than 32 KB for the compaction."""
    rng = np.random.default_rng(r_max)
    C, counts = 3, [r_max, 0, (r_max + 1) // 2]
    K = sum(counts)
    passing = np.ones((K, C), bool) if r_max <= 2500 else rng.random((K, C)) < 2000.0 / r_max
    passing[r_max - 1] = True
    prob = np.where(passing, rng.integers(4, 64, (K, C)), rng.integers(0, 4, (K, C))).astype(np.float32) / np.float32(64)
    boxes = np.concatenate([R.grid_boxes(n, C) for n in counts], 0)
    for D in (100, 0):
        got, want = _check_select(prob, boxes, counts, THRESH, 0.5, D, "r_max={} D={}".format(r_max, D))
        if D == 0:
            assert got[0] == int(passing[:r_max, 1:].sum()) and got[1] == 0
            if r_max == 2500:
                assert got[0] == 5000
        elif r_max >= 1023:
            assert got[0] >= 100 and got[0] < 400


def test_select_refuses_more_rows_than_the_sort_holds():
    from abr_iod_amd import ops
    prob = torch.full((16385, 2), 0.5, device="cuda")
    boxes = torch.from_numpy(R.grid_boxes(16385, 2)).cuda()
    off = torch.tensor([0, 16385], dtype=torch.int32).cuda()
    with pytest.raises(RuntimeError, match="16384"):
        ops.det_select(prob, boxes, off, 1, 2, 16385, THRESH, 0.5, 100)
    torch.cuda.synchronize()


def test_select_threshold_is_strict():
    """`p > thresh`: a score equal to the threshold is out, the next float is in; a class where nothing passes (scores at and just below
    the threshold, and 0) and one where everything does.  At threshold 0 a probability of exactly 0 is out and every subnormal is in."""
    n, C = 600, 3
    boxes = R.grid_boxes(n, C)
    for thresh in (np.float32(0.05), np.float32(0.5)):
        above, below = np.nextafter(thresh, np.float32(1)), np.nextafter(thresh, np.float32(0))
        prob = np.empty((n, C), np.float32)
        prob[:, 0] = np.where(np.arange(n) % 2 == 0, thresh, above)
        prob[:, 1] = np.float32([thresh, below, 0.0])[np.arange(n) % 3]
        prob[:, 2] = np.float32([above, 0.75, 1.0])[np.arange(n) % 3]
        for D in (0, 100):
            out = _select(prob, boxes, [n], float(thresh), 0.5, D)
            _assert_equal(out, _oracle(prob, boxes, [n], float(thresh), 0.5, D), "thresh={} D={}".format(thresh, D))
            ob, os_, ol, oc, bb, bs, bc = out
            assert bc[0] == n // 2 and (bs[0, :bc[0]] == above).all()
            assert (ol[0, :oc[0]] == 2).all() and (oc[0] == n if D == 0 else oc[0] == n // 3)      # D = 100: the 200 scores of 1.0 tie at the cut
    sub = R.from_bits([0, 1, 0x00000100, 0x00010000, 0x007FFFFF, 0x00800000, 0x3F000000])         # 0, three subnormals, the largest one, 2^-126, 0.5
    prob = np.stack([sub[np.arange(n) % 7], sub[(np.arange(n) + 3) % 7], sub[(np.arange(n) // 5) % 7]], 1)
    for D in (0, 100, 300):
        out = _select(prob, boxes, [n], 0.0, 0.5, D)
        _assert_equal(out, _oracle(prob, boxes, [n], 0.0, 0.5, D), "thresh=0 D={}".format(D))
        if D == 0:
            assert out[3][0] == int((prob[:, 1:] > 0).sum()) and out[6][0] == int((prob[:, 0] > 0).sum())
            assert (_bits(out[1][0, :out[3][0]]) == 1).sum() == int((_bits(prob[:, 1:]) == 1).sum()) > 0      # 2^-149 is kept


@pytest.mark.parametrize("nms_t", [0.0, 0.5, 1.0])
def test_select_nms_thresholds(nms_t):
    """overlapping integer boxes with exact duplicates: at 0 the best box of a class suppresses every other one (IoU >= 0), at 1 only exact
    duplicates go"""
    rng = np.random.default_rng(7)
    C, counts = 3, [300, 0, 77]
    K = sum(counts)
    prob = (rng.integers(1, 33, (K, C)) / 32.0).astype(np.float32)
    boxes = _int_boxes(rng, K, C)
    for D in (0, 100):
        got, want = _check_select(prob, boxes, counts, THRESH, nms_t, D, "nms={} D={}".format(nms_t, D))
        if D == 0 and nms_t == 0.0:
            assert got == [2, 0, 2]
        if D == 0 and nms_t == 1.0:
            assert 300 < got[0] < 600


def _score_set(name, rng, K, C):
    if name == "distinct":
        return rng.permutation(np.linspace(0.06, 0.99, K * C).astype(np.float32)).reshape(K, C)
    if name == "all_equal":
        return np.full((K, C), 0.5, np.float32)
    if name == "low_byte":
        return R.from_bits(0x3F000000 + rng.integers(0, 256, (K, C)))
    if name == "mid_bytes":
        return R.from_bits(0x3F000000 + (rng.integers(0, 128, (K, C)) << 16) + (rng.integers(0, 4, (K, C)) << 8))
    if name == "exponent":
        return R.from_bits((rng.integers(123, 128, (K, C)) << 23))                   # 2^-4 .. 1.0: only exponent bits differ
    if name == "tie_span":
        return (rng.integers(1, 8, (K, C)) / 8.0).astype(np.float32)
    raise KeyError(name)


@pytest.mark.parametrize("name", ["distinct", "all_equal", "low_byte", "mid_bytes", "exponent", "tie_span"])
def test_select_cut(name):
    """the radix select behind the top-D cut: C = 4 on grid boxes, 600 detections in image 0 and 111 in image 2, D at 0, 1, 100 and one
    below / at / one above each image's total.  `>= kth`: the whole tie group at the cut is kept, in class-major proposal order."""
    rng = np.random.default_rng(len(name))
    C, counts = 4, [200, 0, 37]
    K = sum(counts)
    prob = _score_set(name, rng, K, C)
    assert (prob > THRESH).all()
    boxes = np.concatenate([R.grid_boxes(n, C) for n in counts], 0)
    for D in (0, 1, 100, 110, 111, 112, 599, 600, 601):
        got, want = _check_select(prob, boxes, counts, THRESH, 0.5, D, "{} D={}".format(name, D))
        if name == "all_equal" or D == 0:
            assert got == [600, 0, 111]                   # one bin in all four passes: everything ties with the D-th score
        if name == "distinct" and D > 0:
            assert got == [min(D, 600), 0, min(D, 111)]
        if name == "tie_span" and D == 100:
            (rb, rs, rl), _ = want[0]
            assert len(set(rl[rs == rs.min()].tolist())) == 3 and got[0] > 100          # the tie group at the cut spans all classes


@pytest.mark.parametrize("C,counts", [(1, [30, 0]), (2, [50, 0, 21]), (81, [50, 0, 21])])
def test_select_class_counts(C, counts):
    rng = np.random.default_rng(C)
    K = sum(counts)
    prob = (rng.integers(0, 33, (K, C)) / 32.0).astype(np.float32)
    boxes = _int_boxes(rng, K, C)
    for D in (0, 100):
        got, want = _check_select(prob, boxes, counts, THRESH, 0.5, D, "C={} D={}".format(C, D))
        if C == 1:
            assert got == [0, 0] and len(want[0][1][1]) > 5          # no detections, a filled background list


@pytest.mark.parametrize("counts", [[64], [1], [0], [0, 40, 0, 300, 0], [7, 0, 0, 0, 1100], [0, 0, 0, 0, 0]])
def test_select_batches_and_background_flag(counts):
    """N = 1 and 5, empty images first, in the middle and last, a batch of empty images; background=False: the same detections"""
    rng = np.random.default_rng(sum(counts) + len(counts))
    C, K = 5, sum(counts)
    prob = (rng.integers(0, 33, (K, C)) / 32.0).astype(np.float32)
    boxes = _int_boxes(rng, K, C) if K else np.zeros((0, C, 4), np.float32)
    want = _oracle(prob, boxes, counts, THRESH, 0.5, 100)
    out = _select(prob, boxes, counts, THRESH, 0.5, 100)
    _assert_equal(out, want, "counts={}".format(counts))
    nob = _select(prob, boxes, counts, THRESH, 0.5, 100, background=False)
    assert nob[4] is None and nob[5] is None and nob[6] is None
    _assert_equal(nob, want, "counts={} no background".format(counts), background=False)


def _select_raw(prob, boxes, off, N, C, r_max, thresh, nms_t, D, fill):
    """ops.det_select through the C ABI with the workspace and every output buffer pre-filled with the byte `fill`"""
    from abr_iod_amd import _lib as L
    cap = (C - 1) * r_max

    def buf(shape, dtype):
        t = torch.empty(shape, dtype=dtype, device="cuda")
        if t.numel():
            t.view(torch.uint8).fill_(fill)
        return t

    ob, os_, ol, oc = buf((N, cap, 4), torch.float32), buf((N, cap), torch.float32), buf((N, cap), torch.int64), buf((N,), torch.int32)
    bb, bs, bc = buf((N, r_max, 4), torch.float32), buf((N, r_max), torch.float32), buf((N,), torch.int32)
    nbytes = L.lib().abr_det_select_workspace_bytes(N, C, r_max)
    ws = buf((max(nbytes, 8),), torch.uint8)
    L.check(L.lib().abr_det_select(L.ptr(prob), L.ptr(boxes), L.ptr(off), N, C, r_max, float(thresh), float(nms_t), int(D), cap, L.ptr(ob),
                                   L.ptr(os_), L.ptr(ol), L.ptr(oc), L.ptr(bb), L.ptr(bs), L.ptr(bc), L.ptr(ws), nbytes, L.stream()), "det_select")
    return [t.cpu().numpy() for t in (ob, os_, ol, oc, bb, bs, bc)]


@pytest.mark.parametrize("nms_t,D", [(0.5, 100), (1.0, 0)])
def test_select_reads_nothing_it_has_not_written(nms_t, D):
    """the workspace comes from torch.empty: the same call on a workspace and outputs full of 0xFF bytes (counts of -1, NaN scores, slot
    tables of garbage) and full of zeros gives the oracle's answer both times.  Nothing beyond the counts is required to be written."""
    rng = np.random.default_rng(11)
    C, counts = 3, [0, 1500, 0, 40, 0]
    K = sum(counts)
    prob = (rng.integers(0, 33, (K, C)) / 32.0).astype(np.float32)
    boxes = _int_boxes(rng, K, C, dup=0.1)
    want = _oracle(prob, boxes, counts, THRESH, nms_t, D)
    dp, db, do = torch.from_numpy(prob).cuda(), torch.from_numpy(boxes).cuda(), torch.from_numpy(R.offsets(counts)).cuda()
    for fill in (0xFF, 0x00):
        out = _select_raw(dp, db, do, len(counts), C, max(counts), THRESH, nms_t, D, fill)
        _assert_equal(out, want, "fill={:#x}".format(fill))


def test_select_is_deterministic():
    rng = np.random.default_rng(3)
    C, counts = 4, [1300, 0, 500]
    K = sum(counts)
    prob = (rng.integers(0, 17, (K, C)) / 16.0).astype(np.float32)
    boxes = _int_boxes(rng, K, C)
    a, b = _select(prob, boxes, counts, THRESH, 0.5, 100), _select(prob, boxes, counts, THRESH, 0.5, 100)
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[6], b[6]) and a[3][0] >= 100
    for i in range(len(counts)):
        n, m = a[3][i], a[6][i]
        assert np.array_equal(a[2][i, :n], b[2][i, :n]) and np.array_equal(_bits(a[1][i, :n]), _bits(b[1][i, :n]))
        assert np.array_equal(_bits(a[0][i, :n]), _bits(b[0][i, :n]))
        assert np.array_equal(_bits(a[5][i, :m]), _bits(b[5][i, :m])) and np.array_equal(_bits(a[4][i, :m]), _bits(b[4][i, :m]))


# ------------------------------------------------------------------------------------------------------------------ PostProcessor.forward
@pytest.mark.parametrize("counts,three_d", [([0, 0, 0], False), ([57], False), ([40, 0, 33, 0], False), ([40, 0, 33], True)])
def test_post_processor_forward(counts, three_d):
    """the module against the oracle's filter_results on the module's own prob / boxes (ops.det_softmax_decode of the same inputs): a batch
    where every image is empty, N = 1, a batch whose last image is empty (the background BoxList is that image's: length 0), [K, C, 4]
    regression input."""
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.roi_heads.box_head.inference import PostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    rng = np.random.default_rng(len(counts) + sum(counts))
    C, N, K = 6, len(counts), sum(counts)
    sizes = [(320, 240), (64, 48), (200, 300), (100, 100)][:N]
    props = []
    for (w, h), n in zip(sizes, counts):
        x1, y1 = rng.uniform(0, w - 20, n), rng.uniform(0, h - 20, n)
        props.append(np.stack([x1, y1, x1 + rng.uniform(4, 60, n), y1 + rng.uniform(4, 60, n)], 1).astype(np.float32))
    logits = torch.from_numpy((rng.standard_normal((K, C)) * 2).astype(np.float32)).cuda()
    reg = torch.from_numpy((rng.standard_normal((K, 4 * C)) * 0.5).astype(np.float32)).cuda()
    lists = [BoxList(torch.from_numpy(p).cuda(), s, mode="xyxy") for p, s in zip(props, sizes)]
    pp = PostProcessor(0.05, 0.5, 20)
    res, bg = pp((logits, reg.view(K, C, 4) if three_d else reg), lists)
    rois = torch.from_numpy(np.concatenate([np.concatenate([np.full((len(p), 1), i, np.float32), p], 1) for i, p in enumerate(props)], 0)).cuda()
    hw = torch.tensor([[h, w] for w, h in sizes], dtype=torch.int32).cuda()
    prob, dec = ops.det_softmax_decode(logits, reg, rois, C, hw, R.WEIGHTS)
    want = _oracle(prob.cpu().numpy(), dec.cpu().numpy(), counts, 0.05, 0.5, 20)
    assert len(res) == N
    for i, (r, ((rb, rs, rl), _)) in enumerate(zip(res, want)):
        assert r.size == sizes[i] and r.mode == "xyxy" and len(r) == len(rs)
        assert np.array_equal(r.get_field("labels").cpu().numpy(), rl)
        assert np.array_equal(_bits(r.get_field("scores").cpu().numpy()), _bits(rs))
        assert np.array_equal(_bits(r.bbox.cpu().numpy()).reshape(-1, 4), _bits(rb).reshape(-1, 4))
        assert counts[i] > 0 or len(r) == 0
    gb, gs = want[-1][1]
    assert bg.size == sizes[-1] and len(bg) == len(gs) and (counts[-1] > 0 or len(bg) == 0)
    assert np.array_equal(_bits(bg.get_field("scores").cpu().numpy()), _bits(gs))
    assert np.array_equal(_bits(bg.bbox.cpu().numpy()).reshape(-1, 4), _bits(gb).reshape(-1, 4))
    assert bg.get_field("labels").dtype == torch.int64 and int(bg.get_field("labels").sum()) == 0

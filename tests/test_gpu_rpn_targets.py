"""The RPN / box-head target kernels of rpn.hip against the oracle's plain-C restatement of the same operations, at the edges the model's
own shapes rarely reach: IoUs exactly on a threshold and one step either side, argmax and low-quality ties, a ground-truth box that overlaps
nothing, grids past the 64-workgroup cap of the row-maximum pass, ragged ground-truth counts in one batch, clipped and unclipped decodes with
padded head rows, empty inputs, and the sampler's draw merged back into ascending RoI rows.

Tolerances follow one rule.  oracle/oracle.c restates IoU, Matcher, BoxCoder and the anchor grid in fp32 C without contraction, and the
kernels evaluate the same formulas in the same order under `fp contract(off)` with correctly rounded fp32 division, so IoUs, matches,
labels, anchors, every index and every clamped coordinate must be IDENTICAL to the oracle's.  Only logf / expf differ (device vs glibc): a
log term of an encoding may differ from the oracle by 4 ulps of its value, a decoded coordinate by 4 ulps of |pcx| + 0.5 pw + 1.  A float64
restatement of encode / decode on the same fp32 inputs bounds the whole fp32 error by 4 ulps of the magnitude of the addends each output
sums, which shows the allowance is small.  Every output a wrapper allocates comes back from the allocator pre-filled with NaN (integers:
a sentinel), so an element the kernel should write and does not is seen.
"""
import contextlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
SENT_I = -7777                                       # sentinel of the integer outputs a kernel must overwrite
CLIP = np.float32(np.log(1000.0 / 16))               # box_coder.py:20
W1 = (1.0, 1.0, 1.0, 1.0)
W10 = (10.0, 10.0, 5.0, 5.0)


@pytest.fixture(scope="module")
def O():
    from oracle import ops
    return ops


@pytest.fixture(scope="module")
def R():
    from oracle import torch_ref
    return torch_ref


@pytest.fixture(scope="module")
def ops():
    from abr_iod_amd import ops as o
    return o


@contextlib.contextmanager
def stale_outputs():
    """torch.empty / torch.empty_like return buffers filled with NaN (floats), SENT_I (integers) or 0xA5 (bytes) while the block runs: the
    wrappers allocate their outputs that way, so every element a kernel leaves unwritten shows up in the comparisons"""
    empty, empty_like = torch.empty, torch.empty_like

    def fill(t):
        if t.dtype.is_floating_point:
            t.fill_(float("nan"))
        elif t.dtype == torch.uint8:
            t.fill_(0xA5)
        elif t.dtype != torch.bool:
            t.fill_(SENT_I)
        return t

    torch.empty = lambda *a, **k: fill(empty(*a, **k))
    torch.empty_like = lambda *a, **k: fill(empty_like(*a, **k))
    try:
        yield
    finally:
        torch.empty, torch.empty_like = empty, empty_like


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def _first_bad(bad, what, got, want):
    if bad.any():
        i = np.argwhere(bad)[0]
        r = int(i[0])
        raise AssertionError(f"{what}: row {r}: {got[r]!r} vs {want[r]!r}; {int(bad.reshape(bad.shape[0], -1).any(1).sum())} rows differ")


def assert_same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    _first_bad(got != want, what, got, want)


# ================================================================================================== BoxCoder.encode references
def encode64(gt, ex, w):
    """float64 BoxCoder.encode of the same fp32 inputs and 4 fp32 ulps of the magnitude of each output's addends (the rounding of the
    widths, centres, difference and quotient -- and, for the log terms, of the ratio)"""
    g, e, w = gt.astype(np.float64), ex.astype(np.float64), np.asarray(w, np.float64)
    ew, eh = e[:, 2] - e[:, 0] + 1, e[:, 3] - e[:, 1] + 1
    gw, gh = g[:, 2] - g[:, 0] + 1, g[:, 3] - g[:, 1] + 1
    ecx, ecy = e[:, 0] + 0.5 * ew, e[:, 1] + 0.5 * eh
    gcx, gcy = g[:, 0] + 0.5 * gw, g[:, 1] + 0.5 * gh
    qx, qy = (gcx - ecx) / ew, (gcy - ecy) / eh
    lw, lh = np.log(gw / ew), np.log(gh / eh)
    ref = np.stack([w[0] * qx, w[1] * qy, w[2] * lw, w[3] * lh], 1)
    sx = (np.abs(e[:, 0]) + np.abs(e[:, 2]) + 1) / ew      # relative rounding error of the widths / heights, in units of eps
    sy = (np.abs(e[:, 1]) + np.abs(e[:, 3]) + 1) / eh
    gx = (np.abs(g[:, 0]) + np.abs(g[:, 2]) + 1) / gw
    gy = (np.abs(g[:, 1]) + np.abs(g[:, 3]) + 1) / gh
    mag = np.stack([w[0] * ((np.abs(g[:, 0]) + np.abs(g[:, 2]) + np.abs(e[:, 0]) + np.abs(e[:, 2]) + 2) / ew + np.abs(qx) * (1 + sx)),
                    w[1] * ((np.abs(g[:, 1]) + np.abs(g[:, 3]) + np.abs(e[:, 1]) + np.abs(e[:, 3]) + 2) / eh + np.abs(qy) * (1 + sy)),
                    w[2] * (np.abs(lw) + 1 + sx + gx), w[3] * (np.abs(lh) + 1 + sy + gy)], 1)
    return ref, 4 * EPS * mag


def check_encode(O, got, gt, ex, w, what):
    """got [n,4] fp32 = BoxCoder.encode(gt, ex, w): dx / dy identical to the oracle, the log terms within 4 ulps of it, everything within
    the float64 bound"""
    got = np.asarray(got)
    want = O.box_encode(gt, ex, w)
    assert np.isfinite(got).all(), f"{what}: non-finite targets"
    assert_same(got[:, :2], want[:, :2], f"{what}: dx/dy vs oracle")
    _first_bad(np.abs(got[:, 2:] - want[:, 2:]) > 4 * np.spacing(np.abs(want[:, 2:])), f"{what}: dw/dh vs oracle (4 ulps)", got, want)
    ref, tol = encode64(gt, ex, w)
    _first_bad(np.abs(got - ref) > tol, f"{what}: vs float64", got, ref)


# ================================================================================================== 1. match_encode
def random_scene(rng, n, G, extent=(800.0, 600.0)):
    """G ground-truth boxes and n boxes, half of them jittered copies of a GT box (IoUs across [0, 1]), half anywhere; fp32 non-integers"""
    X, Y = extent
    x1, y1 = rng.uniform(0, X - 20, G), rng.uniform(0, Y - 20, G)
    gw, gh = rng.uniform(8, 300, G), rng.uniform(8, 300, G)
    gt = np.stack([x1, y1, x1 + gw, y1 + gh], 1).astype(np.float32)
    src = rng.integers(0, G, n)
    near = rng.random(n) < 0.5
    cw, ch = gw[src] * np.exp(rng.normal(0, 0.3, n)), gh[src] * np.exp(rng.normal(0, 0.3, n))
    cx = np.where(near, x1[src] + 0.5 * gw[src] + rng.normal(0, 0.15, n) * gw[src], rng.uniform(0, X, n))
    cy = np.where(near, y1[src] + 0.5 * gh[src] + rng.normal(0, 0.15, n) * gh[src], rng.uniform(0, Y, n))
    cw, ch = np.where(near, cw, rng.uniform(4, 400, n)), np.where(near, ch, rng.uniform(4, 400, n))
    boxes = np.stack([cx - 0.5 * cw, cy - 0.5 * ch, cx + 0.5 * cw, cy + 0.5 * ch], 1).astype(np.float32)
    return boxes, gt


def match_ref(O, boxes, gt, hi, lo, lq):
    return O.matcher(O.box_iou(gt, boxes), hi, lo, lq)


def rpn_labels_ref(m, vis):
    lab = (m >= 0).astype(np.float32)
    if vis is not None:
        lab[~vis] = -1
    lab[m == -2] = -1
    return lab


def head_labels_ref(m, gt_labels):
    lab = gt_labels[np.clip(m, 0, None)] if gt_labels is not None else np.ones(len(m), np.int64)
    lab = lab.astype(np.int64).copy()
    lab[m == -1] = 0
    lab[m == -2] = -1
    return lab


def run_match(ops, boxes, gt, gt_labels, vis, hi, lo, lq, w, rpn):
    with stale_outputs():
        m, lab, t = ops.match_encode(cuda(boxes), cuda(gt), None if gt_labels is None else cuda(gt_labels),
                                     None if vis is None else cuda(vis.astype(np.uint8)), hi, lo, lq, w, rpn)
    return host(m), host(lab), host(t)


def check_match(O, ops, boxes, gt, hi, lo, lq, w, vis=None, gt_labels=None, what=""):
    """all three forms of match_encode (fp32 RPN labels with visibility; int64 head labels from gt_labels and with None) against the oracle"""
    m_ref = match_ref(O, boxes, gt, hi, lo, lq)
    gi = np.clip(m_ref, 0, None)
    m, lab, t = run_match(ops, boxes, gt, None, vis, hi, lo, lq, w, True)
    assert_same(m, m_ref, f"{what}: matched")
    assert_same(lab, rpn_labels_ref(m_ref, vis), f"{what}: RPN labels")
    if len(boxes):
        check_encode(O, t, gt[gi], boxes, w, f"{what}: reg_targets")
    for gl in (gt_labels, None):
        m2, lab2, t2 = run_match(ops, boxes, gt, gl, None, hi, lo, lq, w, False)
        assert_same(m2, m_ref, f"{what}: matched (head form)")
        assert_same(lab2, head_labels_ref(m_ref, gl), f"{what}: head labels ({'gt_labels' if gl is not None else 'None'})")
        assert_same(t2, t, f"{what}: head-form targets vs RPN form")
    return m_ref


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1023, 65537, 143640])
@pytest.mark.parametrize("G", [1, 2, 7, 64, 100])
def test_match_encode_sweep(O, R, ops, n, G):
    rng = np.random.default_rng(1000 * n + G)
    boxes, gt = random_scene(rng, n, G)
    vis = rng.random(n) < 0.8
    gt_labels = rng.integers(1, 21, G).astype(np.int64)
    for lq in (True, False):
        for w in (W1, W10):
            m = check_match(O, ops, boxes, gt, 0.7, 0.3, lq, w, vis, gt_labels, f"n={n} G={G} lq={lq} w={w}")
        if n >= 1023:   # the scene reaches every outcome
            assert (m >= 0).any() and (m == -1).any() and (m == -2).any()
    lab, tgt, m = R.rpn_prepare_targets(boxes, vis, gt)
    got_m, got_lab, got_t = run_match(ops, boxes, gt, None, vis, 0.7, 0.3, True, W1, True)
    assert_same(got_m, m, "vs rpn_prepare_targets: matched")
    assert_same(got_lab, lab, "vs rpn_prepare_targets: labels")
    check_encode(O, got_t, gt[np.clip(m, 0, None)], boxes, W1, "vs rpn_prepare_targets: targets")


def column(y0, k, x=0.0):
    """a 1-pixel-wide box of k rows from y0: against the column (x, 0 .. 99) its IoU is exactly the fp32 nearest k / 100"""
    return [x, y0, x, y0 + k - 1]


@pytest.mark.parametrize("hi,lo,expect", [
    (0.7, 0.3, {71: 0, 70: 0, 69: -2, 51: -2, 31: -2, 30: -2, 29: -1}),
    (0.5, 0.5, {71: 0, 51: 0, 50: 0, 49: -1, 31: -1, 30: -1, 29: -1}),
])
def test_match_encode_thresholds_exact(O, ops, hi, lo, expect):
    gt = np.array([column(0, 100)], np.float32)
    ks = list(expect)
    boxes = np.array([column(0, k) for k in ks] + [column(0, 100)], np.float32)   # the last box (IoU 1) owns the low-quality rule
    iou = O.box_iou(gt, boxes)[0]
    assert np.array_equal(iou[:-1], np.array([np.float32(k / 100) for k in ks], np.float32))
    for lq in (False, True):
        m = check_match(O, ops, boxes, gt, hi, lo, lq, W10, what=f"thresholds {hi}/{lo} lq={lq}")
        assert list(m[:-1]) == [expect[k] for k in ks] and m[-1] == 0


def test_match_encode_ties_and_low_quality(O, ops):
    """duplicate GT boxes (argmax ties go to the first); a GT whose maximum two boxes tie, one of which belongs to another GT (each low-quality
    match gets its own argmax); a GT that overlaps nothing (every box takes its argmax); an invisible low-quality box (label -1)"""
    gt = np.array([column(0, 100),            # GT0
                   column(0, 100),            # GT1 = GT0: never an argmax
                   column(100, 100),          # GT2: its maximum (20/130) is tied by boxes 0 and 1
                   [5000, 5000, 5100, 5100],  # GT3: overlaps nothing -> row maximum 0
                   column(0, 100, x=50.0)],   # GT4: best box (index 3) has IoU 0.25, invisible
                  np.float32)
    boxes = np.array([column(70, 50),         # 0: GT0/1 30/120 = 0.25 (argmax GT0), GT2 20/130
                      column(180, 50),        # 1: GT2 20/130 only
                      column(0, 95),          # 2: GT0/1 0.95 -> matched to GT0
                      column(0, 25, x=50.0),  # 3: GT4 0.25 only, invisible
                      [300, 300, 310, 310]],  # 4: overlaps nothing
                     np.float32)
    vis = np.array([True, True, True, False, True])
    iou = O.box_iou(gt, boxes)
    assert iou[2, 0] == iou[2, 1] == iou[2].max() and iou[0, 0] > iou[2, 0] and iou[3].max() == 0
    for lq in (False, True):
        m = check_match(O, ops, boxes, gt, 0.7, 0.3, lq, W1, vis, np.arange(1, 6, dtype=np.int64), what=f"ties lq={lq}")
        assert m[2] == 0
        if lq:   # GT3 overlaps nothing: every box with IoU 0 to it -- all of them -- takes its own argmax
            assert list(m) == [0, 2, 0, 4, 0]
            assert list(rpn_labels_ref(m, vis)) == [1, 1, 1, -1, 1]
        else:
            assert list(m) == [-1, -1, 0, -1, -1]
    # without the box-less GT3, box 4 stays a negative and the ties decide alone
    keep = [0, 1, 2, 4]
    m = check_match(O, ops, boxes, gt[keep], 0.7, 0.3, True, W1, vis, np.arange(1, 5, dtype=np.int64), what="ties, no empty GT")
    assert list(m) == [0, 2, 0, 3, -1]


def test_match_encode_empty(ops):
    from abr_iod_amd._lib import lib, stream
    dev = "cuda"
    m, lab, t = ops.match_encode(torch.empty((0, 4), device=dev), torch.ones((3, 4), device=dev), None, None, 0.7, 0.3, True, W1, True)
    assert m.shape == (0,) and lab.shape == (0,) and t.shape == (0, 4)
    # n = 0 returns before any pointer is touched: null buffers are accepted
    assert lib().abr_match_encode(None, 0, None, None, 3, None, 0.7, 0.3, 1, 1.0, 1.0, 1.0, 1.0, None, None, None, None, None, 0, stream()) == 0
    with pytest.raises(RuntimeError):
        ops.match_encode(torch.ones((5, 4), device=dev), torch.empty((0, 4), device=dev), None, None, 0.7, 0.3, True, W1, True)


def test_match_encode_fresh_stream(O, ops):
    """a first call on a fresh non-blocking stream: the row-maximum workspace is zeroed on the launch stream"""
    rng = np.random.default_rng(7)
    boxes, gt = random_scene(rng, 143640, 64)
    b, g = cuda(boxes), cuda(gt)
    torch.cuda.synchronize()
    ref = [host(x) for x in ops.match_encode(b, g, None, None, 0.7, 0.3, True, W10, True)]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), stale_outputs():
        got = ops.match_encode(b, g, None, None, 0.7, 0.3, True, W10, True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    for r, x, name in zip(ref, got, ("matched", "labels", "targets")):
        assert_same(host(x), r, f"fresh stream: {name}")
    assert_same(ref[0], match_ref(O, boxes, gt, 0.7, 0.3, True), "default stream: matched")


# ================================================================================================== 2. rpn_targets_batched
@pytest.mark.parametrize("N", [1, 2, 5, 9])
def test_rpn_targets_batched(O, R, ops, N):
    """38 x 63 x 15 anchors shared by N images of different sizes (different visibility) and ragged GT counts; the per-image GT tensors are
    rows of one padded [N, g_max, 4] buffer whose padding overlaps the anchors, so a kernel reading past n_gt[i] changes the result"""
    rng = np.random.default_rng(N)
    cell = cuda(O.cell_anchors())
    sizes = [(600 - 37 * i, 1000 - 53 * i) if i % 2 == 0 else (1000 - 53 * i, 600 - 37 * i) for i in range(N)]
    anchors, vis_list = None, []
    for h, w in sizes:
        anchors, v = ops.grid_anchors(cell, 38, 63, 16, h, w, 0)
        vis_list.append(v)
    n_gt = [1, 40, 3, 17, 1, 40, 2, 9, 33][:N]
    g_max = max(n_gt)
    buf = np.empty((N, g_max, 4), np.float32)
    for i, (h, w) in enumerate(sizes):
        x1, y1 = rng.uniform(0, w - 60, g_max), rng.uniform(0, h - 60, g_max)
        bw, bh = rng.uniform(16, 400, g_max), rng.uniform(16, 400, g_max)
        buf[i] = np.stack([x1, y1, np.minimum(x1 + bw, w - 1), np.minimum(y1 + bh, h - 1)], 1)
    gt_dev = cuda(buf)
    gts = [gt_dev[i, :n_gt[i]] for i in range(N)]
    with stale_outputs():
        lab, tgt, _ = ops.rpn_targets_batched(anchors, vis_list, gts, 0.7, 0.3, W1)
    lab, tgt, a = host(lab), host(tgt), host(anchors)
    assert lab.shape == (N, a.shape[0]) and tgt.shape == (N, a.shape[0], 4)
    for i in range(N):
        vis = host(vis_list[i]).astype(bool)
        gt = buf[i, :n_gt[i]]
        l_ref, _, m = R.rpn_prepare_targets(a, vis, gt)
        assert_same(lab[i], l_ref, f"image {i}: labels")
        check_encode(O, tgt[i], gt[np.clip(m, 0, None)], a, W1, f"image {i}: targets")
        _, l1, t1 = ops.match_encode(anchors, gts[i], None, vis_list[i], 0.7, 0.3, True, W1, True)
        assert_same(lab[i], host(l1), f"image {i}: labels vs match_encode")
        assert_same(tgt[i], host(t1), f"image {i}: targets vs match_encode")
    assert len({host(v).tobytes() for v in vis_list}) == N


# ================================================================================================== 3. rpn_decode_clip
def delta_at(value, wt):
    """a delta d with fp32 d / wt == value exactly (the kernel divides by the weight before clipping)"""
    d = np.float32(value) * np.float32(wt)
    for _ in range(8):
        q = np.float32(d) / np.float32(wt)
        if q == np.float32(value):
            return d
        d = np.nextafter(d, np.float32(np.inf) if q < value else np.float32(-np.inf))
    raise AssertionError(f"no fp32 delta with d / {wt} == {value}")


def decode64(d, b, w):
    d, b, w = d.astype(np.float64), b.astype(np.float64), np.asarray(w, np.float64)
    bw, bh = b[:, 2] - b[:, 0] + 1, b[:, 3] - b[:, 1] + 1
    cx, cy = b[:, 0] + 0.5 * bw, b[:, 1] + 0.5 * bh
    dx, dy = d[:, 0] / w[0], d[:, 1] / w[1]
    dw, dh = np.minimum(d[:, 2] / w[2], float(CLIP)), np.minimum(d[:, 3] / w[3], float(CLIP))
    pcx, pcy, pw, ph = dx * bw + cx, dy * bh + cy, np.exp(dw) * bw, np.exp(dh) * bh
    out = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], 1)
    ulp = np.stack([np.abs(pcx) + 0.5 * pw + 1, np.abs(pcy) + 0.5 * ph + 1], 1)[:, [0, 1, 0, 1]]      # 4 ulps of this: vs the oracle
    mag = np.stack([np.abs(dx) * bw + np.abs(b[:, 0]) + np.abs(b[:, 2]) + 1 + 0.5 * pw * (1 + np.abs(dw)) + np.abs(pcx),
                    np.abs(dy) * bh + np.abs(b[:, 1]) + np.abs(b[:, 3]) + 1 + 0.5 * ph * (1 + np.abs(dh)) + np.abs(pcy)], 1)[:, [0, 1, 0, 1]]
    return out, 4 * np.spacing(ulp.astype(np.float32)).astype(np.float64), 4 * EPS * mag


def special_deltas(w):
    """zero; dw / dh at, just below and far above log(1000/16); dw = -30 (the width underflows); centres thrown far outside both ways"""
    below = np.nextafter(CLIP, np.float32(0))
    rows = [(0, 0, 0, 0), (0, 0, CLIP, CLIP), (0, 0, below, below), (0, 0, 50.0, 60.0), (0, 0, -30.0, -30.0), (0, 0, CLIP, -30.0),
            (1e3, 0, 0, 0), (-1e3, 0, 0, 0), (0, 1e3, 0.5, 0.5), (0, -1e3, 0, 0), (1e3, 1e3, CLIP, CLIP), (0.3, -0.2, -0.4, 0.7)]
    return np.array([[delta_at(v, wt) for v, wt in zip(r, w)] for r in rows], np.float32)


def decode_case(O, rng, A, pad, N, w, k_max=40, H=5, W=7):
    cell = O.cell_anchors(sizes=(32, 64, 128, 256, 512)[:max(1, A // 3)], ratios=(0.5, 1.0, 2.0)[:min(3, A)])
    assert cell.shape[0] == A
    anchors, _ = O.grid_anchors(cell, H, W, 16, (H * 16, W * 16))
    n_anchor = anchors.shape[0]
    ld = 5 * A + pad
    reg = np.full((N, H * W, ld), np.nan, np.float32)   # objectness and pad columns: NaN, so a wrong column shows
    reg[:, :, A:5 * A] = (rng.normal(0, 0.6, (N, H * W, 4 * A)) * np.tile(np.asarray(w, np.float32), A)).astype(np.float32)
    k = min(k_max, n_anchor)
    idx = np.empty((N, k), np.int64)
    sp = special_deltas(w)
    for i in range(N):
        idx[i] = np.concatenate([[0, n_anchor - 1], 1 + rng.permutation(n_anchor - 2)[:k - 2]]) if k > 2 else [0, n_anchor - 1][:k]
        for p in range(min(k, len(sp))):
            a = idx[i, p]
            reg[i, a // A, A + 4 * (a % A):A + 4 * (a % A) + 4] = sp[(p + i) % len(sp)]
    return anchors, reg, idx


def decode_ref(O, reg, A, anchors, idx, w):
    N, k = idx.shape
    out, tol, out64, tol64 = (np.empty((N, k, 4)) for _ in range(4))
    for i in range(N):
        a = idx[i]
        cols = A + 4 * (a % A)[:, None] + np.arange(4)[None]
        d = reg[i, a // A][np.arange(k)[:, None], cols]
        out[i] = O.box_decode(d, anchors[a], w)
        out64[i], tol[i], tol64[i] = decode64(d, anchors[a], w)
    return out.astype(np.float32), tol, out64, tol64


@pytest.mark.parametrize("A", [1, 3, 15])
@pytest.mark.parametrize("pad", [0, 1])
@pytest.mark.parametrize("w", [W1, W10])
def test_rpn_decode_clip(O, ops, A, pad, w):
    rng = np.random.default_rng(100 * A + pad)
    img = [(70, 110), (110, 70), (45, 97)]          # a transposed pair: an H / W swap moves the clip
    N = len(img)
    anchors, reg, idx = decode_case(O, rng, A, pad, N, w)
    want, tol, want64, tol64 = decode_ref(O, reg, A, anchors, idx, w)
    hw = np.array(img, np.int32)
    for clip in (True, False):
        with stale_outputs():
            got = host(ops.rpn_decode_clip(cuda(reg), A, cuda(anchors), cuda(idx), cuda(hw), w, A=A, clip=clip))
        what = f"A={A} ld={5 * A + pad} w={w} clip={clip}"
        assert got.shape == want.shape and np.isfinite(got).all(), f"{what}: shape / non-finite"
        ref, ref64 = want.copy(), want64.copy()
        if clip:
            for arr in (ref, ref64):
                arr[..., 0::2] = np.clip(arr[..., 0::2], 0, (hw[:, 1] - 1)[:, None, None])
                arr[..., 1::2] = np.clip(arr[..., 1::2], 0, (hw[:, 0] - 1)[:, None, None])
        _first_bad((np.abs(got - ref) > tol).reshape(-1, 4), f"{what}: vs oracle", got.reshape(-1, 4), ref.reshape(-1, 4))
        _first_bad((np.abs(got - ref64) > tol64).reshape(-1, 4), f"{what}: vs float64", got.reshape(-1, 4), ref64.reshape(-1, 4))
        if clip:   # coordinates the oracle puts beyond the image by more than the allowance are clamped exactly to 0 / W-1 / H-1
            hi = np.stack([hw[:, 1], hw[:, 0]] * 2, 1)[:, None, :].astype(np.float32) - 1
            out_lo, out_hi = want < -tol, want > hi + tol
            assert out_lo.any() and out_hi.any()
            assert_same(got[out_lo], np.zeros(int(out_lo.sum()), np.float32), f"{what}: clamped to 0")
            assert_same(got[out_hi], np.broadcast_to(hi, got.shape)[out_hi], f"{what}: clamped to the far edge")


def test_rpn_decode_clip_empty(O, ops):
    rng = np.random.default_rng(3)
    anchors, reg, idx = decode_case(O, rng, 15, 1, 2, W1)
    hw = cuda(np.array([[600, 1000], [1000, 600]], np.int32))
    out = ops.rpn_decode_clip(cuda(reg), 15, cuda(anchors), cuda(idx[:, :0]), hw, A=15)
    assert out.shape == (2, 0, 4)
    out = ops.rpn_decode_clip(cuda(reg[:0]), 15, cuda(anchors), cuda(idx[:0]), hw[:0], A=15)
    assert out.shape == (0, idx.shape[1], 4)


# ================================================================================================== 4. box_encode_rows, grid_anchors
@pytest.mark.parametrize("n", [0, 1, 257, 70000])
def test_box_encode_rows(O, ops, n):
    rng = np.random.default_rng(n)
    ex, gt = random_scene(rng, n, max(n, 1))
    gt = gt[:n]
    if n:
        ex[::5, 2] = ex[::5, 0]                          # width-1 boxes (x2 == x1), both sides
        gt[1::7, 3] = gt[1::7, 1]
        wide = slice(2, None, 11)                        # boxes thousands of pixels wide and tall
        ex[wide, 2] = ex[wide, 0] + rng.uniform(1000, 6000, ex[wide].shape[0]).astype(np.float32)
        gt[3::13, 3] = gt[3::13, 1] + rng.uniform(1000, 6000, gt[3::13].shape[0]).astype(np.float32)
    for w in (W1, W10):
        with stale_outputs():
            got = host(ops.box_encode_rows(cuda(gt), cuda(ex), w))
        assert got.shape == (n, 4)
        check_encode(O, got, gt, ex, w, f"n={n} w={w}")


@pytest.mark.parametrize("H,W,img", [(1, 1, (16, 16)), (1, 63, (10, 1000)), (38, 1, (600, 9)), (37, 61, (593, 977)),
                                     (38, 63, (600, 1000)), (25, 33, (401, 529))])
@pytest.mark.parametrize("straddle", [0, -1, 5])
def test_grid_anchors(O, ops, H, W, img, straddle):
    for cell in (O.cell_anchors(), O.cell_anchors(stride=8, sizes=(16,), ratios=(1.0,)), O.cell_anchors(sizes=(48, 96), ratios=(0.5, 2.0))):
        stride = 8 if cell.shape[0] == 1 else 16
        want, wvis = O.grid_anchors(cell, H, W, stride, img, straddle)
        with stale_outputs():
            got, vis = ops.grid_anchors(cuda(cell), H, W, stride, img[0], img[1], straddle)
        assert_same(host(got), want, f"anchors A={cell.shape[0]} {H}x{W}")
        assert_same(host(vis), wvis.astype(np.uint8), f"visibility A={cell.shape[0]} {H}x{W} straddle={straddle}")


# ================================================================================================== 5. rpn_loss_indices
def padded_draw(rng, N, n, max_pos, batch, no_pos=False, no_neg=False):
    """the sampler's padded lists: ascending global indices (image offset i * n), -1 padding, counts [N, 2]"""
    pos = np.full((N, max(max_pos, 1)), -1, np.int64)
    neg = np.full((N, batch), -1, np.int64)
    counts = np.zeros((N, 2), np.int32)
    for i in range(N):
        cp = 0 if no_pos else int(rng.integers(1, max_pos + 1))
        cn = 0 if no_neg else int(rng.integers(1, batch - cp + 1))
        pick = rng.permutation(n)[:cp + cn]
        pos[i, :cp] = np.sort(pick[:cp]) + i * n
        neg[i, :cn] = np.sort(pick[cp:]) + i * n
        counts[i] = cp, cn
    return pos, neg, counts


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("A", [3, 15])
@pytest.mark.parametrize("extra", [0, 1])
@pytest.mark.parametrize("kind", ["both", "no_pos", "no_neg"])
def test_rpn_loss_indices(ops, N, A, extra, kind):
    rng = np.random.default_rng(N * 100 + A + extra)
    Cf, n = 5 * A + extra, 7 * 5 * A
    pos, neg, counts = padded_draw(rng, N, n, 12, 40, kind == "no_pos", kind == "no_neg")
    with stale_outputs():
        samp, obj_flat, prow, pcol, denom = (host(t) for t in ops.rpn_loss_indices(cuda(pos), cuda(neg), cuda(counts), A, Cf))
    v = np.concatenate([pos.ravel(), neg.ravel()])
    row = np.where(v >= 0, v // A, -1)
    assert_same(samp, v, "samp")
    assert_same(obj_flat, np.where(v >= 0, row * Cf + v % A, -1), "obj_flat")
    p = pos.ravel()
    assert_same(prow, np.where(p >= 0, p // A, -1), "pos_row")
    assert_same(pcol, np.where(p >= 0, A + 4 * (p % A), 0), "pos_col")
    assert denom.shape == (1,) and denom[0] == np.float32(counts.sum()), f"denom {denom} vs {counts.sum()}"


# ================================================================================================== 6. roi_head_targets, gather_proposals
def proposals(rng, N, k_pre, post, n_keep, n_gt, extent=(1000.0, 600.0)):
    """decoded, score-sorted boxes [N, k_pre, 4], scores, keep [N, post] (a view of an [N + 1, post] buffer of valid indices, so a reader
    past row N - 1 stays in bounds), n_keep [N] and per-image GT boxes / labels that are rows of padded buffers"""
    X, Y = extent
    g_max = max(n_gt)
    gbuf = np.empty((N, g_max, 4), np.float32)
    props = np.empty((N, k_pre, 4), np.float32)
    for i in range(N):
        b, g = random_scene(rng, k_pre, g_max, extent)
        gbuf[i], props[i] = g, np.clip(b, 0, [X - 1, Y - 1, X - 1, Y - 1])
    scores = np.sort(rng.random((N, k_pre)).astype(np.float32), 1)[:, ::-1].copy()
    keep = np.stack([rng.permutation(k_pre)[:post] for _ in range(N + 1)]).astype(np.int32)
    lbuf = rng.integers(1, 21, (N, g_max)).astype(np.int64)
    return props, scores, keep, np.asarray(n_keep, np.int32), gbuf, lbuf


def candidates_ref(O, props, scores, keep, n_keep, gts, gls, post, w):
    out = []
    for i in range(len(gts)):
        nk = min(int(n_keep[i]), post)
        src = keep[i, :nk]
        boxes = np.concatenate([props[i, src], gts[i]])
        obj = np.concatenate([scores[i, src], np.ones(len(gts[i]), np.float32)])
        m = match_ref(O, boxes, gts[i], 0.5, 0.5, False)
        out.append((boxes, obj, head_labels_ref(m, gls[i]), gts[i][np.clip(m, 0, None)]))
    return out


ROI_CASES = {
    # name: N, k_pre, post, n_keep, n_gt, batch_size, max_pos, num_classes
    "n_keep_below_post": (2, 600, 100, [57, 100], [3, 12], 64, 16, 21),
    "gt_only": (2, 200, 50, [0, 0], [2, 9], 64, 16, 11),
    "post_2000": (3, 3000, 2000, [2000, 1300, 2600], [1, 40, 7], 512, 128, 16),
    "max_pos_0": (2, 600, 100, [80, 100], [4, 6], 64, 0, 21),
    "batch_above_candidates": (2, 300, 100, [5, 3], [2, 1], 128, 32, 11),
}


@pytest.mark.parametrize("case", list(ROI_CASES))
def test_roi_head_targets(O, ops, case):
    N, k_pre, post, n_keep, n_gt, B, max_pos, K = ROI_CASES[case]
    rng = np.random.default_rng(list(ROI_CASES).index(case))
    props, scores, keep_buf, n_keep, gbuf, lbuf = proposals(rng, N, k_pre, post, n_keep, n_gt)
    gts, gls = [gbuf[i, :n_gt[i]] for i in range(N)], [lbuf[i, :n_gt[i]] for i in range(N)]
    g_dev, l_dev, keep_dev = cuda(gbuf), cuda(lbuf), cuda(keep_buf)
    args = (cuda(props), cuda(scores), keep_dev[:N], cuda(n_keep), [g_dev[i, :n_gt[i]] for i in range(N)],
            [l_dev[i, :n_gt[i]] for i in range(N)], 0.5, 0.5, W10, B, max_pos, K)
    runs = []
    for agn in (False, True):                          # same seed: the same draw, only col0 may differ
        with stale_outputs():
            t = ops.roi_head_targets(*args, cls_agnostic=agn, seed=12345)
        runs.append({k: host(v) for k, v in t.items() if torch.is_tensor(v)})
    for k in runs[0]:
        if k != "col0":
            assert_same(runs[1][k], runs[0][k], f"{k}: cls_agnostic changed it")
    t = runs[0]
    Pmax = post + max(n_gt)
    ref = candidates_ref(O, props, scores, keep_buf, n_keep, gts, gls, post, W10)
    assert_same(t["n_cand"], np.array([len(r[0]) for r in ref], np.int32), "n_cand")
    total = 0
    for i, (boxes, obj, lab, gt_m) in enumerate(ref):
        nc = len(boxes)
        what = f"{case} image {i}"
        assert_same(t["cand"][i, :nc], boxes, f"{what}: cand")
        assert_same(t["obj_all"][i, :nc], obj, f"{what}: obj_all")
        assert_same(t["labels_all"][i, :nc], lab, f"{what}: labels_all")
        check_encode(O, t["regt_all"][i, :nc], gt_m, boxes, W10, f"{what}: regt_all")
        assert_same(t["cand"][i, nc:], np.zeros((Pmax - nc, 4), np.float32), f"{what}: cand padding")
        assert_same(t["regt_all"][i, nc:], np.zeros((Pmax - nc, 4), np.float32), f"{what}: regt_all padding")
        assert_same(t["obj_all"][i, nc:], np.zeros(Pmax - nc, np.float32), f"{what}: obj_all padding")
        assert_same(t["labels_all"][i, nc:], np.full(Pmax - nc, -1), f"{what}: labels_all padding")

        # the draw: a valid one, by the sampler's rules (its distribution belongs to the sampler tests)
        cp, cn = (int(c) for c in t["counts"][i])
        n_pos, n_neg = int((lab >= 1).sum()), int((lab == 0).sum())
        assert cp == min(n_pos, max_pos) and cn == min(n_neg, B - cp), f"{what}: counts {cp}, {cn} of {n_pos}, {n_neg}"
        pos, neg = t["pos_idx"][i, :cp], t["neg_idx"][i, :cn]
        assert (np.diff(pos) > 0).all() and (np.diff(neg) > 0).all(), f"{what}: draw not ascending"
        assert ((pos >= 0) & (pos < nc)).all() and (lab[pos] >= 1).all(), f"{what}: positives"
        assert ((neg >= 0) & (neg < nc)).all() and (lab[neg] == 0).all(), f"{what}: negatives"
        assert (t["pos_idx"][i, cp:max_pos] == -1).all() and (t["neg_idx"][i, cn:] == -1).all(), f"{what}: draw padding"

        # the merged rows: the ascending union, then padding
        v = np.sort(np.concatenate([pos, neg]))
        d = len(v)
        rows = slice(i * B, (i + 1) * B)
        l_rows = np.concatenate([lab[v], np.full(B - d, -1, np.int64)])
        assert_same(t["sampled_idx"][i], np.concatenate([v, np.full(B - d, -1, np.int64)]), f"{what}: sampled_idx")
        assert_same(t["rois"][rows], np.concatenate([np.full((B, 1), i, np.float32),
                                                     np.concatenate([boxes[v], np.zeros((B - d, 4), np.float32)])], 1), f"{what}: rois")
        assert_same(t["labels"][rows], l_rows, f"{what}: labels")
        assert_same(t["reg_targets"][rows], np.concatenate([t["regt_all"][i, v], np.zeros((B - d, 4), np.float32)]), f"{what}: reg_targets")
        assert_same(t["obj"][rows], np.concatenate([obj[v], np.zeros(B - d, np.float32)]), f"{what}: obj")
        r = np.arange(i * B, (i + 1) * B)
        assert_same(t["pos_rows"][rows], np.where(l_rows > 0, r, -1), f"{what}: pos_rows")
        for run, agn in zip(runs, (False, True)):
            assert_same(run["col0"][rows], K + (np.full(B, 4) if agn else 4 * np.maximum(l_rows, 0)), f"{what}: col0 (cls_agnostic={agn})")
        total += d
    assert t["n_valid"].shape == (1,) and t["n_valid"][0] == np.float32(total), f"n_valid {t['n_valid']} vs {total}"
    if case == "batch_above_candidates":
        assert total < N * B


@pytest.mark.parametrize("N,P", [(2, 64), (3, 1), (2, 0), (0, 5)])
def test_gather_proposals(ops, N, P):
    rng = np.random.default_rng(N * 10 + P)
    k_pre, post = 300, 100
    props, scores, keep_buf, _, _, _ = proposals(rng, max(N, 1), k_pre, post, [post] * max(N, 1), [1] * max(N, 1))
    props, scores, keep = props[:N], scores[:N], keep_buf[:N]
    picks = rng.integers(0, post, (N, P)).astype(np.int64)
    picks[:, :1] = 0
    picks[:, -1:] = post - 1
    with stale_outputs():
        rois, obj = (host(x) for x in ops.gather_proposals(cuda(props), cuda(scores), cuda(keep), cuda(picks.ravel()), P))
    assert rois.shape == (N * P, 5) and obj.shape == (N * P,)
    src = np.take_along_axis(keep, picks, 1) if N * P else np.zeros((N, P), np.int64)
    ii = np.repeat(np.arange(N), P)
    assert_same(rois, np.concatenate([ii[:, None].astype(np.float32), props[ii, src.ravel()]], 1), "rois")
    assert_same(obj, scores[ii, src.ravel()], "obj")

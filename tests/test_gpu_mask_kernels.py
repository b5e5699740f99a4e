"""GPU: the mask head's kernels (abr_iod_amd/csrc/mask.hip) at their edges, each against the plain restatement of tests/mask_ref.py (pinned
to the recorded reference on the CPU by tests/test_mask_ref.py).  Integer, byte and pure-copy results are held to equality; every kernel is
run twice and the two results must be equal.

  compaction      several 1024-row chunks (the running base), the cross-wave prefix, the P_max cut in the first chunk, on the chunk boundary
                  and in a later chunk; nothing written past P_max / K (C ABI, canaries)
  gather          rows longer than one grid pass (64 x 256 float4), out-of-range / duplicate / hugely negative indices
  depth-to-space  h != w in both directions, the 4096-block cap, sums that are exactly 0, -0 and the smallest denormal
  targets         three images of different sizes in one batch, two identical ground-truth boxes (first maximum), padding rules, M from 1
                  to the admitted 256
  loss            gscale, want_grad=False, labels in [Kc, ldk), Kc == ldk, Kc == 1, M == 1, the 1024-block cap, a device n_pos
  select-sigmoid  unpadded and padded ldk, labels outside [0, Kc), logits up to +-inf, the grid cap
  paste           M in {1, 7, 14, 28}, one-pixel-wide canvases, boxes outside / reversed / empty, truncation toward zero, tails of every length

Found and fixed while writing this suite: mask_targets_kernel always interpolated in the four-weight order, which is torch's only while
out_h + out_w <= 128; for 64 < M <= 256 (admitted by the launcher) uint8 targets differed from the reference at the pixels where four set taps'
rounded weights sum to 1 - 2^-24 in one order and to 1 in the other.  The kernel now picks the form by bilinear_four_weight_path(M, M), as the
evaluation's resize already did; M <= 64 is unchanged bit for bit.

Also found: tests/mask_ref.py's paste_f64 formed the source coordinate with two roundings where torch (and the kernel) use one fused
multiply-add; for a box nine pixels wide at M = 1 the coordinate of canvas column 1 is 1.5e-8 fused and exactly 0 unfused, so at threshold 0
the reference lost pixels that torch pastes.  The reference now rounds once (the fixture's paste at threshold 0.5 never saw the difference).

Measured on the MI355X: see MEASUREMENTS.md, "Mask head kernels at their edges".
"""
import functools
import os

import numpy as np
import pytest
import torch

import mask_ref as R
from mask_loss_check import MEASURED, check_loss

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24
DENORM = float(np.float32(2.0 ** -149))
CANARY = -0x5A5A5A5A5A5A5A5B


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ a. compaction
def _label_patterns(K, rng):
    pos = lambda: rng.integers(1, 81, K)                                                      # noqa: E731
    neg = lambda: np.where(rng.random(K) < 0.5, 0, -rng.integers(1, 5, K))                    # noqa: E731  (zeros and negatives mixed)
    idx = np.arange(K)
    out = {"none positive": neg(), "all positive": pos(), "alternating": np.where(idx % 2 == 1, pos(), neg()),
           "random p = 0.25": np.where(rng.random(K) < 0.25, pos(), neg())}
    if K > 0:
        out["only row 0"] = np.where(idx == 0, pos(), neg())
        out["only row K - 1"] = np.where(idx == K - 1, pos(), neg())
        out["rows 63, 64, 1023, 1024"] = np.where(np.isin(idx, (63, 64, 1023, 1024)), pos(), neg())
    if K > 1024:
        out["second chunk only"] = np.where(idx >= 1024, pos(), neg())
    return {k: v.astype(np.int64) for k, v in out.items()}


@pytest.mark.parametrize("K", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 3001])
def test_compaction_vs_nonzero(K):
    """every label pattern x P_max in {0, 1, n - 1, n, n + 1, K} and, beyond one chunk, cuts at 500 (inside the first chunk), 1024 (on the
    boundary) and 1500 (inside the second): rows, labels, inverse map and count equal to nonzero()[:P_max]"""
    from abr_iod_amd import ops
    rng = np.random.default_rng(100 + K)
    for name, labels in _label_patterns(K, rng).items():
        n = int((labels > 0).sum())
        cuts = {0, 1, n - 1, n, n + 1, K} | ({500, 1024, 1500} if K > 1024 else set())
        dev = _cuda(labels)
        for p_max in sorted(c for c in cuts if c >= 0):
            got = [t.cpu().numpy() for t in ops.mask_compact_pos(dev, p_max)]
            again = [t.cpu().numpy() for t in ops.mask_compact_pos(dev, p_max)]
            want = R.compact_ref(labels, p_max)
            tag = "K = {}, {}, P_max = {}".format(K, name, p_max)
            assert int(got[3][0]) == want[3], tag
            for g, a, w, what in zip(got[:3], again[:3], want[:3], ("pos_rows", "pos_labels", "inv")):
                assert g.dtype == np.int64 and np.array_equal(g, w), (tag, what)
                assert np.array_equal(g, a), (tag, what, "two runs differ")


def test_compaction_writes_nothing_past_its_lengths_through_the_c_abi():
    """buffers 64 longer than P_max / K, pre-filled with a canary: a cut in the first, on the boundary of and in a later chunk, and no cut"""
    from abr_iod_amd import _lib as L
    K = 3001
    rng = np.random.default_rng(5)
    labels = np.where(rng.random(K) < 0.6, rng.integers(1, 81, K), -rng.integers(0, 3, K)).astype(np.int64)
    dev = _cuda(labels)
    for p_max in (700, 1024, 1500, K):
        rows, plab = (torch.full((p_max + 64,), CANARY, dtype=torch.int64, device="cuda") for _ in range(2))
        inv = torch.full((K + 64,), CANARY, dtype=torch.int64, device="cuda")
        n_pos = torch.full((3,), -77, dtype=torch.int32, device="cuda")
        L.check(L.lib().abr_mask_compact_pos(L.ptr(dev), K, p_max, L.ptr(rows), L.ptr(plab), L.ptr(inv), L.ptr(n_pos), L.stream()), "mask_compact_pos")
        want = R.compact_ref(labels, p_max)
        for got, w, n in ((rows, want[0], p_max), (plab, want[1], p_max), (inv, want[2], K)):
            got = got.cpu().numpy()
            assert np.array_equal(got[:n], w) and (got[n:] == CANARY).all(), p_max
        assert n_pos.cpu().tolist() == [want[3], -77, -77]


# ------------------------------------------------------------------------------------------------ b. gather rows
ROWS = [2, -1, 0, 3, 2, -(2 ** 40)]       # n_src = 3: an index at n_src, a duplicate, a large negative


@pytest.mark.parametrize("row_floats", [4, 32, 65536, 65540, 200704])
def test_gather_rows_vs_indexing(row_floats):
    """65536 floats are exactly one grid pass (64 blocks x 256 float4); 65540 and the production row 14 * 14 * 1024 take the grid-stride
    loop.  The values are the element's own flat index, so a wrong stride lands on a different number."""
    from abr_iod_amd import ops
    x = np.arange(3 * row_floats, dtype=np.float32).reshape(3, row_floats) + 1        # (exact below 2^24)
    rows = torch.tensor(ROWS, dtype=torch.int64, device="cuda")
    got = ops.mask_gather_rows(_cuda(x), rows)
    again = ops.mask_gather_rows(_cuda(x), rows)
    assert got.shape == (6, row_floats) and torch.equal(got, again)
    assert np.array_equal(got.cpu().numpy(), R.gather_ref(x, ROWS))


def test_gather_rows_edges():
    from abr_iod_amd import ops
    x = torch.randn(3, 2, 2, 8, device="cuda")
    out = ops.mask_gather_rows(x, torch.zeros(0, dtype=torch.int64, device="cuda"))                      # n_out = 0
    assert out.shape == (0, 2, 2, 8)
    out = ops.mask_gather_rows(torch.zeros(0, 8, device="cuda"), torch.full((5,), -1, dtype=torch.int64, device="cuda"))   # n_src = 0
    assert out.shape == (5, 8) and not bool(out.any())
    # round trip through the inverse map of a compaction over three chunks
    K = 2049
    rng = np.random.default_rng(8)
    labels = np.where(rng.random(K) < 0.4, rng.integers(1, 21, K), 0).astype(np.int64)
    labels[[0, 1023, 1024, 2048]] = 7
    rows, _, inv, n_pos = ops.mask_compact_pos(_cuda(labels), K)
    xs = torch.randn(K, 8, device="cuda")
    xg = ops.mask_gather_rows(xs, rows)
    back = ops.mask_gather_rows(xg, inv).cpu()
    posm = torch.from_numpy(labels > 0)
    assert int(n_pos) == int(posm.sum()) and torch.equal(xg[:int(n_pos)].cpu(), xs.cpu()[posm]) and not bool(xg[int(n_pos):].any())
    assert torch.equal(back[posm], xs.cpu()[posm]) and not bool(back[~posm].any())
    # 65535 output rows are the grid's limit
    x4 = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    r = (np.arange(65535) % 5 - 1).astype(np.int64)             # -1 .. 3
    got = ops.mask_gather_rows(_cuda(x4), _cuda(r)).cpu().numpy()
    ok = (r >= 0) & (r < 3)
    assert np.array_equal(got[ok], x4[r[ok]]) and not got[~ok].any()
    with pytest.raises(RuntimeError, match="65535"):
        ops.mask_gather_rows(_cuda(x4), torch.zeros(65536, dtype=torch.int64, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.mask_gather_rows(torch.zeros(3, 6, device="cuda"), torch.zeros(2, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------------------------ c. depth-to-space + bias + ReLU
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (3, 2, 5, 4), (2, 7, 4, 20), (5, 4, 7, 256), (24, 7, 7, 1024)], ids=lambda s: "P%d-h%d-w%d-Cm%d" % s)
def test_depth_to_space_bias_relu_forward_and_backward(shape):
    """random data (every quadrant and channel distinguishable), h != w, the last shape above the 4096-block cap; planted in every quadrant
    of some pixels: y + bias exactly 0, -0, the smallest positive denormal (positive: it passes, and so does its gradient) and its negative"""
    from abr_iod_amd import ops
    P, h, w, Cm = shape
    gen = torch.Generator().manual_seed(P * 1000 + h * 100 + w * 10 + Cm)
    y = torch.randn(P, h, w, 4 * Cm, generator=gen)
    bias = torch.randn(Cm, generator=gen)
    bias[0], bias[1], bias[3] = 0.0, -0.0, 0.0
    flat = y.view(-1, 4, Cm)                                   # [(n, y, x), q, c]
    for px in sorted({0, flat.shape[0] // 2, flat.shape[0] - 1}):
        flat[px, :, 0] = DENORM
        flat[px, :, 1] = -0.0
        flat[px, :, 2] = -bias[2]
        flat[px, :, 3] = -DENORM
    want = R.d2s_ref(y, bias)
    planted = want.view(P, h, 2, w, 2, Cm)[0, 0, :, 0, :, :4]
    assert bool((planted[..., 0] == DENORM).all()) and not bool(planted[..., 1:].any())
    got = ops.mask_d2s_bias_relu(y.cuda(), bias.cuda())
    again = ops.mask_d2s_bias_relu(y.cuda(), bias.cuda())
    assert got.shape == (P, 2 * h, 2 * w, Cm) and torch.equal(got, again)
    assert torch.equal(got.cpu(), want)
    # backward on an activation with more zeros and denormals planted
    out = want.clone()
    out.view(-1)[::7] = 0.0
    out.view(-1)[3::11] = DENORM
    g = torch.randn(out.shape, generator=gen)
    want_gy = R.d2s_backward_ref(g, out)
    gy = ops.mask_d2s_bias_relu_backward(g.cuda(), out.cuda())
    gy2 = ops.mask_d2s_bias_relu_backward(g.cuda(), out.cuda())
    assert gy.shape == (P, h, w, 4 * Cm) and torch.equal(gy, gy2)
    assert torch.equal(gy.cpu(), want_gy)


def test_depth_to_space_edges():
    from abr_iod_amd import ops
    out = ops.mask_d2s_bias_relu(torch.zeros(0, 2, 5, 16, device="cuda"), torch.zeros(4, device="cuda"))
    assert out.shape == (0, 4, 10, 4)
    assert ops.mask_d2s_bias_relu_backward(out, out).shape == (0, 2, 5, 16)
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.mask_d2s_bias_relu(torch.zeros(1, 1, 1, 8, device="cuda"), torch.zeros(2, device="cuda"))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        ops.mask_d2s_bias_relu_backward(torch.zeros(1, 2, 2, 2, device="cuda"), torch.zeros(1, 2, 2, 2, device="cuda"))


# ------------------------------------------------------------------------------------------------ d. targets
TARGET_MS = [1, 2, 7, 16, 17, 28, 64, 65, 96, 256]
SIZES = ((61, 97), (40, 33), (1, 1))                      # (H, W) of the three images
GTS = (np.array([[10, 8, 80, 50], [10, 8, 80, 50], [0, 0, 20, 20], [60, 30, 96, 60]], np.float32),      # 0 and 1 are IDENTICAL boxes
       np.array([[2, 3, 20, 30], [15, 10, 32, 39]], np.float32),
       np.array([[0, 0, 0, 0]], np.float32))
NAMED_ROIS = {  # name -> (image, box, instance that must be chosen)
    "inside the twin boxes": (0, (12, 9, 78, 49), 0),
    "the twin boxes themselves": (0, (10, 8, 80, 50), 0),
    "on instance 2": (0, (1, 1, 19, 22), 2),
    "on instance 3": (0, (58.5, 28.5, 95, 59), 3),
    "disjoint from every box": (0, (85, 0, 96, 6), 0),
    "right of and below the image": (0, (200, 100, 230, 140), 0),
    "corners +-3e9": (0, (-3e9, -3e9, 3e9, 3e9), 0),
    "image 1, whole": (1, (0, 0, 32, 39), None),
    "image 1, .5 corners": (1, (14.5, 9.5, 31.5, 38.5), 1),
    "image 1, on instance 0": (1, (3, 2, 18, 28), 0),
    "image 1, over the corner": (1, (-4, -4, 5, 5), None),
    "image 2, the pixel": (2, (0, 0, 0, 0), 0),
    "image 2, around it": (2, (-5, -5, 5, 5), 0),
    "image 2, inside it": (2, (0.4, 0.4, 0.6, 0.6), 0),
}


@functools.lru_cache(maxsize=None)
def _scene(tag):
    """-> (masks per image (CPU), rois [K,5], pos_rows [K]): uint8 masks of ones with 3 % holes and one zero rectangle per instance (where the
    two forms of the resize differ, and the twins' masks differ), or random float32 masks; the RoIs are the fixture's 20 target boxes on
    image 0 plus the named ones; pos_rows is a fixed permutation of all rows"""
    rng = np.random.default_rng(17)
    masks = []
    for (H, W), gt in zip(SIZES, GTS):
        if tag == "f32":
            masks.append(torch.from_numpy(rng.random((len(gt), H, W)).astype(np.float32)))
            continue
        m = (rng.random((len(gt), H, W)) >= 0.03).astype(np.uint8)
        for i in range(len(gt)):
            y, x = int(rng.integers(0, max(H - 8, 1))), int(rng.integers(0, max(W - 8, 1)))
            m[i, y:y + H // 3, x:x + W // 4] = 0
        masks.append(torch.from_numpy(m))
    if tag == "u8":
        masks[2][:] = 1
        assert bool((masks[0][0] != masks[0][1]).any())
    fixture = np.load(os.path.join(GOLD, "mask_head.npz"))["t_boxes"]
    rois = [(0,) + tuple(b) for b in fixture.tolist()] + [(img,) + tuple(b) for img, b, _ in NAMED_ROIS.values()]
    rois = np.array(rois, np.float32)
    pos_rows = np.random.default_rng(3).permutation(len(rois)).astype(np.int64)
    return masks, rois, pos_rows


@functools.lru_cache(maxsize=None)
def _targets_want(tag, M):
    masks, rois, pos_rows = _scene(tag)
    return R.targets_ref(masks, GTS, rois, pos_rows, M)


@pytest.mark.parametrize("tag", ["u8", "f32"])
@pytest.mark.parametrize("M", TARGET_MS)
def test_mask_targets_batch_of_three_images(tag, M):
    """uint8 exact, float32 <= 1e-6 absolute.  M * M below one block (1, 2, 7), not a multiple of it (17), the fixture's 28, 64 and 65 either
    side of torch's change of operation order, 96 beyond it and the admitted limit 256"""
    from abr_iod_amd import ops
    masks, rois, pos_rows = _scene(tag)
    want, matched = _targets_want(tag, M)
    names = list(NAMED_ROIS)
    for p, row in enumerate(pos_rows.tolist()):            # the reference itself picks the first of the twins and instance 0 when disjoint
        if row >= 20 and NAMED_ROIS[names[row - 20]][2] is not None:
            assert matched[p] == NAMED_ROIS[names[row - 20]][2], names[row - 20]
    args = ([m.cuda() for m in masks], [_cuda(g) for g in GTS], _cuda(rois), _cuda(pos_rows), M)
    got = ops.mask_targets(*args)
    again = ops.mask_targets(*args)
    assert got.shape == want.shape and torch.equal(got, again)
    err = (got.cpu().double() - want.double()).abs()
    print("mask targets (three images)", tag, "M", M, "max abs err", float(err.max()), "mismatching pixels", int((err > 0).sum()), "of", err.numel())
    if tag == "u8":
        bad = (err > 0).flatten(1).any(1).nonzero().flatten().tolist()
        assert not bad, [(int(pos_rows[p]), int((err[p] > 0).sum())) for p in bad]
        assert bool(want.any()) and bool((want == 0).any())
    else:
        assert float(err.max()) <= 1e-6


@pytest.mark.parametrize("tag", ["u8", "f32"])
def test_mask_targets_padding_rules(tag):
    """an image index of -1 or N in the RoI table, an image without instances and pos_rows of -1 or K give zeros; the other rows are unchanged"""
    from abr_iod_amd import ops
    M = 14
    masks, rois, pos_rows = _scene(tag)
    masks = list(masks) + [torch.zeros((0, 20, 20), dtype=masks[0].dtype)]
    gts = list(GTS) + [np.zeros((0, 4), np.float32)]
    N, K0 = len(masks), len(rois)
    rois = np.concatenate((rois, np.array([[-1, 1, 1, 9, 9], [N, 1, 1, 9, 9], [3, 1, 1, 9, 9], [-7, 1, 1, 9, 9], [1e9, 1, 1, 9, 9]], np.float32)))
    K = len(rois)
    rows = np.concatenate((pos_rows[:6], [-1, K, K0, K0 + 1, K0 + 2, K0 + 3, K0 + 4, -(2 ** 40), 2 ** 40], pos_rows[6:12])).astype(np.int64)
    want, matched = R.targets_ref(masks, gts, rois, rows, M)
    assert matched[6:15] == [-1] * 9 and not bool(want[6:15].any()) and all(m >= 0 for m in matched[:6] + matched[15:])
    got = ops.mask_targets([m.cuda() for m in masks], [_cuda(g) for g in gts], _cuda(rois), _cuda(rows), M).cpu()
    assert not bool(got[6:15].any())
    if tag == "u8":
        assert torch.equal(got, want)
    else:
        assert float((got.double() - want.double()).abs().max()) <= 1e-6
    assert torch.equal(got[:6], ops.mask_targets([m.cuda() for m in masks[:3]], [_cuda(g) for g in GTS], _cuda(rois[:K0]), _cuda(pos_rows[:6]), M).cpu())


def test_mask_targets_refuses_more_than_256():
    from abr_iod_amd import ops
    masks, rois, pos_rows = _scene("u8")
    with pytest.raises(RuntimeError, match="mask_targets"):
        ops.mask_targets([m.cuda() for m in masks], [_cuda(g) for g in GTS], _cuda(rois), _cuda(pos_rows), 257)


# ------------------------------------------------------------------------------------------------ e. loss
LOSS_CASES = ["gscale 0.37", "labels in [Kc, ldk)", "Kc == ldk", "Kc == 1", "M == 1", "P = 64 at M = 28", "device n_pos below the labelled rows"]


@pytest.mark.parametrize("case", LOSS_CASES)
def test_mask_loss_more_edges(case):
    """through check_loss (1e-6 of the sum of |addends| for the loss, 8 * 2^-24 / (n M M) per gradient element; two runs equal;
    want_grad=False gives the same loss bits)"""
    gen = torch.Generator().manual_seed(23)
    P, K, M, kw = 7, 21, 14, {}
    if case == "Kc == ldk":
        K = 24
    elif case == "Kc == 1":
        K = 1
    elif case == "M == 1":
        M = 1
    elif case == "P = 64 at M = 28":       # 64 * 784 * 6 float4 = 301056 > 1024 blocks x 256
        P, M = 64, 28
    x = torch.randn(P, K, M, M, generator=gen) * 3
    labels = torch.randint(1, max(K, 2), (P,), generator=gen)
    t = (torch.rand(P, M, M, generator=gen) > 0.5).float()
    if case == "gscale 0.37":
        one = check_loss(x, labels, t, tag=case + " (gscale 1)")
        assert check_loss(x, labels, t, tag=case, gscale=0.37) == one            # the gradient scales, the loss does not
        return
    if case == "labels in [Kc, ldk)":      # rows 1 to 4 contribute nothing and have zero gradient (without a device count the mean's denominator stays P)
        labels = torch.tensor([3, 21, 22, 23, 0, 20, 1, 22][:P])
    elif case == "Kc == ldk":
        labels[:] = 23
        kw["ldk"] = 24
    elif case == "Kc == 1":                # no admissible label: 0, the only channel, is the background
        labels = torch.tensor([0, 1, 2, 3, -1, 1, 0])
        assert check_loss(x, labels, t, tag=case) == 0.0
        return
    elif case == "device n_pos below the labelled rows":
        kw["n_pos"] = 5
    got = check_loss(x, labels, t, tag=case, **kw)
    assert got > 0
    print("mask loss, worst so far: rel to addends", MEASURED["loss rel to addends"], "gradient / its bound", MEASURED["grad of its bound"])


# ------------------------------------------------------------------------------------------------ f. select + sigmoid
SPECIAL = [0.0, -0.0, 88.0, -88.0, 104.0, -104.0, float("inf"), float("-inf")]


@pytest.mark.parametrize("ldk,Kc", [(5, 5), (8, 5), (24, 21)])
def test_select_sigmoid_vs_float64(ldk, Kc):
    """absolute 4 * 2^-24 against float64; labels of -1 and Kc give zeros, label 0 is selected; the other channels hold NaN"""
    from abr_iod_amd import ops
    gen = torch.Generator().manual_seed(ldk)
    D, M = 9, 14
    labels = torch.tensor([0, Kc - 1, -1, Kc, 1, 2, 0, Kc - 1, 3])
    x = torch.full((D, M, M, ldk), float("nan"))
    for d, l in enumerate(labels.tolist()):
        if 0 <= l < Kc:
            x[d, :, :, l] = torch.randn(M, M, generator=gen) * 4
            x[d, 0, :len(SPECIAL), l] = torch.tensor(SPECIAL)
    want = R.select_sigmoid_ref(x, Kc, labels)
    got = ops.mask_select_sigmoid(x.cuda(), Kc, labels.cuda())
    again = ops.mask_select_sigmoid(x.cuda(), Kc, labels.cuda())
    assert got.shape == (D, 1, M, M) and torch.equal(got, again)
    err = float((got.cpu().double() - want).abs().max())
    print("select + sigmoid ldk", ldk, "Kc", Kc, "max abs err", err, "=", err / EPS, "EPS")
    assert err <= 4 * EPS
    assert not bool(got[2].any()) and not bool(got[3].any()) and bool(got[0].any())
    assert got.cpu()[0, 0, 0, :len(SPECIAL)].tolist() == [0.5, 0.5, 1.0, got.cpu()[0, 0, 0, 3].item(), 1.0, 0.0, 1.0, 0.0]


def test_select_sigmoid_empty_and_above_the_grid_cap():
    """D = 1338 at M = 28: 1338 * 784 = 1048992 outputs, above 4096 blocks x 256"""
    from abr_iod_amd import ops
    out = ops.mask_select_sigmoid(torch.zeros(0, 14, 14, 8, device="cuda"), 5, torch.zeros(0, dtype=torch.int64, device="cuda"))
    assert out.shape == (0, 1, 14, 14)
    gen = torch.Generator().manual_seed(9)
    D, M, ldk, Kc = 1338, 28, 8, 5
    x = torch.randn(D, M, M, ldk, generator=gen) * 4
    labels = torch.randint(-1, Kc + 1, (D,), generator=gen)
    labels[-1] = Kc - 1
    want = torch.sigmoid(torch.gather(x.double(), 3, labels.clamp(0, Kc - 1).view(D, 1, 1, 1).expand(D, M, M, 1)))[..., 0]
    want[(labels < 0) | (labels >= Kc)] = 0
    got = ops.mask_select_sigmoid(x.cuda(), Kc, labels.cuda())
    assert torch.equal(got, ops.mask_select_sigmoid(x.cuda(), Kc, labels.cuda()))
    err = float((got.cpu()[:, 0].double() - want).abs().max())
    print("select + sigmoid D 1338 M 28 max abs err", err, "=", err / EPS, "EPS")
    assert err <= 4 * EPS and bool(got[-1].any())


# ------------------------------------------------------------------------------------------------ g. paste
@pytest.mark.parametrize("name", [c.name for c in R.paste_cases()])
def test_paste_vs_float64(name):
    """thresholds 0, 0.25, 0.5 and 0.9: every pixel equal to (float64 value > threshold, 0 where nothing is written) except where that value
    lies within 1e-6 of the threshold (threshold 0: 0 < v <= 1e-6); those are at most 1e-3 of the case's pixels"""
    from abr_iod_amd import ops
    c = next(c for c in R.paste_cases() if c.name == name)
    vals, written = R.paste_reference(name)
    prob, boxes = c.prob.cuda(), c.boxes.cuda()
    excused, differing = [], []
    for t in R.PASTE_THRESHOLDS:
        got = ops.mask_paste(prob, boxes, c.H, c.W, t)
        again = ops.mask_paste(prob, boxes, c.H, c.W, t)
        assert got.dtype == torch.uint8 and got.shape == (c.D, 1, c.H, c.W) and torch.equal(got, again)
        want, near = R.paste_expected(vals, written, t)
        bad = (got.cpu()[:, 0] != want) & ~near
        assert not bool(bad.any()), (name, t, [(c.kinds[d], y, x) for d, y, x in bad.nonzero()[:5].tolist()])
        assert int(near.sum()) <= 1e-3 * want.numel()
        excused.append(int(near.sum()))
        differing.append(int((got.cpu()[:, 0] != want).sum()))
    print("paste", name, "pixels", written.numel(), "excused per threshold", excused, "of which differing", differing)


def test_paste_edges():
    from abr_iod_amd import ops
    out = ops.mask_paste(torch.zeros(0, 1, 14, 14, device="cuda"), torch.zeros(0, 4, device="cuda"), 5, 3, 0.5)
    assert out.shape == (0, 1, 5, 3) and out.dtype == torch.uint8
    with pytest.raises(RuntimeError, match="negative threshold"):
        ops.mask_paste(torch.zeros(1, 1, 14, 14, device="cuda"), torch.zeros(1, 4, device="cuda"), 5, 3, -1.0)

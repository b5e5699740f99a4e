"""GPU: the keypoint head's kernels (abr_iod_amd/csrc/keypoint.hip) at their edges, each against the host restatement of tests/keypoint_ref.py.

Targets are index-exact.  The fold is compared with torch.nn.functional.conv_transpose2d in float64 and the unfold is checked as its exact
adjoint.  The loss and its low-resolution gradient use the bounds tests/test_gpu_loss_kernels.py uses for softmax_ce, a mean-reduced loss
against float64: the loss within 1e-6 of the mean of the rows' (max |z| + |lse|); a gradient element within
|gscale| / n_valid * eps * (8 + 2 * (max |z| + max |z| + |lse|)) per softmax term, times 4 here, because a low-resolution element is the sum of
up to 16 such terms whose bilinear weights add up to exactly 4 (2 per axis).

The decode test accepts a (RoI, keypoint) pair when the kernel's index is the float64 argmax, or when the float64 resized value at the
kernel's index lies within 32 * eps * max |map| of the float64 maximum (16 fp32 multiply-adds whose weight magnitudes sum below 2); at most
2 % of the pairs may pass by the second rule alone.  Measured on the CPU when this test was written, with the restatement itself run in
float32 numpy against float64 on the same inputs: 0 of 216 pairs needed the second rule."""
import numpy as np
import pytest
import torch

import keypoint_ref as R

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
TOL = 1e-6


@pytest.fixture(scope="module")
def ops():
    from abr_iod_amd import ops as o
    return o


def dev(a, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).cuda()


def f64(t):
    return t.detach().cpu().double()


# ================================================================================================== kp_select_targets
def _batch(M):
    """three images with 3, 1 and 2 instances, K = 5: keypoints on x1, on x2 (the M - 1 rule), outside, invisible; an instance with no visible
    keypoint inside its box; an image whose positives are all dropped; a zero-width RoI"""
    gt = [np.array([[10, 10, 50, 60], [100, 20, 180, 90], [200, 200, 260, 280]], np.float32),
          np.array([[30, 30, 90, 120]], np.float32),
          np.array([[5, 5, 45, 45], [60, 60, 61, 100]], np.float32)]
    kp0 = np.array([[[10, 10, 2], [50, 60, 2], [30.5, 35.25, 1], [55, 30, 2], [20, 20, 0]],        # corners, inside, outside the box, invisible
                    [[100, 50, 2], [180, 90, 1], [140.3, 55.7, 2], [99, 50, 2], [150, 95, 2]],
                    [[230, 240, 0], [270, 240, 2], [230, 300, 2], [0, 0, 0], [199, 199, 2]]], np.float32)    # nothing visible inside: dropped
    kp1 = np.array([[[40, 40, 0], [95, 60, 2], [60, 125, 1], [0, 0, 0], [29, 29, 2]]], np.float32)      # image 1: every positive dropped
    kp2 = np.array([[[5, 5, 1], [45, 45, 1], [25, 25, 2], [44.999, 5.001, 2], [46, 25, 2]],
                    [[60, 60, 2], [61, 100, 2], [60.5, 80, 2], [60, 80, 2], [61, 80, 2]]], np.float32)
    rois = np.array([[0, 10, 10, 50, 60], [0, 12, 8, 48, 63], [0, 300, 300, 340, 340], [0, 98, 22, 182, 88], [0, 200, 200, 260, 280],
                     [1, 30, 30, 90, 120], [1, 28, 33, 88, 118],
                     [2, 5, 5, 45, 45], [2, 60, 60, 60, 100], [2, 60, 60, 61, 100], [2, 7, 3, 44, 47], [0, 101, 19, 179, 91]], np.float32)
    labels = np.array([1, 1, 0, 1, 1, 1, 1, 1, 1, 1, -1, 2], np.int64)
    return gt, [kp0, kp1, kp2], rois, labels


@pytest.mark.parametrize("M", [8, 24, 56])
def test_select_targets_index_exact(ops, M):
    gt, kps, rois, labels = _batch(M)
    full = R.select_targets(rois, labels, gt, kps, M, 64)["n_pos"]
    assert full == 7      # rows 0, 1, 3, 7, 8 (zero width: its instance has visible keypoints inside its box), 9 and 11
    for p_max in (full + 3, full, full - 1, 0):
        want = R.select_targets(rois, labels, gt, kps, M, p_max)
        got = ops.kp_select_targets(dev(rois), dev(labels, torch.int64), [dev(g) for g in gt], [dev(k) for k in kps], M, p_max)
        for key in ("pos_rows", "inv", "targets", "valid"):
            assert np.array_equal(got[key].cpu().numpy(), want[key]), (M, p_max, key, got[key].cpu().tolist(), want[key].tolist())
        assert got["n_pos"].item() == want["n_pos"] and got["n_valid"].item() == want["n_valid"], (M, p_max)
    want = R.select_targets(rois, labels, gt, kps, M, full)
    rows = want["pos_rows"].tolist()
    assert 4 not in rows and 5 not in rows and 6 not in rows and 2 not in rows and 10 not in rows
    p0, p8 = rows.index(0), rows.index(8)
    assert want["targets"][p0, 0] == 0 and want["valid"][p0, 0] == 1                      # on (x1, y1)
    assert want["targets"][p0, 1] == (M - 1) * M + (M - 1) and want["valid"][p0, 1] == 1   # on (x2, y2): the M - 1 rule
    assert want["valid"][p0].tolist() == [1, 1, 1, 0, 0]
    # the zero-width RoI: 0 * inf and x / 0 are invalid, a keypoint exactly on x2 == x1 takes the boundary rule
    assert want["valid"][p8].tolist() == [1, 0, 0, 1, 0], want["valid"][p8].tolist()


def test_select_targets_canaries(ops):
    """through the C ABI: nothing is written past any output's length"""
    from abr_iod_amd import _lib as L
    M, p_max, pad = 24, 5, 16
    gt, kps, rois, labels = _batch(M)
    K, Rn = 5, len(labels)
    want = R.select_targets(rois, labels, gt, kps, M, p_max)
    gts, kpd = [dev(g) for g in gt], [dev(k) for k in kps]
    tab = torch.tensor([t.data_ptr() for t in gts + kpd], dtype=torch.int64).cuda()
    n_gt = torch.tensor([g.shape[0] for g in gt], dtype=torch.int32).cuda()
    bufs = dict(pos_rows=(p_max, torch.int64), inv=(Rn, torch.int64), n_pos=(1, torch.int32), targets=(p_max * K, torch.int64),
                valid=(p_max * K, torch.uint8), n_valid=(1, torch.int32))
    out = {k: torch.full((n + pad,), 77, dtype=dt, device="cuda") for k, (n, dt) in bufs.items()}
    r, l = dev(rois), dev(labels, torch.int64)
    L.check(L.lib().abr_kp_select_targets(r.data_ptr(), l.data_ptr(), Rn, tab.data_ptr(), tab.data_ptr() + 8 * 3, n_gt.data_ptr(), 3, K, M, p_max,
                                          out["pos_rows"].data_ptr(), out["inv"].data_ptr(), out["n_pos"].data_ptr(), out["targets"].data_ptr(),
                                          out["valid"].data_ptr(), out["n_valid"].data_ptr(), L.stream()), "kp_select_targets")
    torch.cuda.synchronize()
    for k, (n, _) in bufs.items():
        assert torch.all(out[k][n:] == 77), k
        w = np.asarray(want[k]).reshape(-1)
        assert np.array_equal(out[k][:n].cpu().numpy().astype(np.int64), w.astype(np.int64)), k


# ================================================================================================== fold / unfold
@pytest.mark.parametrize("K", [1, 3, 4, 5, 17])
def test_deconv_fold_and_adjoint(ops, K):
    g = torch.Generator().manual_seed(K)
    Kp, C = R.kp_pad(K), 8
    for P, h, w in [(1, 1, 1), (1, 2, 3), (2, 3, 2), (1, 7, 7), (3, 2, 7), (0, 3, 3)]:
        x = torch.randn(P, h, w, C, generator=g, dtype=torch.float64)
        wt = torch.randn(16 * Kp, C, generator=g, dtype=torch.float64).float().double()
        wt.reshape(4, 4, Kp, C)[:, :, K:] = 0          # the padding rows of the GEMM weight are zero
        bias = torch.randn(K, generator=g).double()
        y = (x @ wt.t()).float()                        # the GEMM's output, as the planner would hand it over
        out = ops.kp_deconv_fold(y.cuda(), bias.float().cuda())
        assert tuple(out.shape) == (P, Kp, 2 * h, 2 * w)
        assert torch.all(out[:, K:] == 0), "padding planes"
        if P == 0:
            assert tuple(ops.kp_deconv_unfold(out, K).shape) == (0, h, w, 16 * Kp)
            continue
        # against the host restatement on the same y: at most four addends and the bias
        ref = R.fold(y.double(), bias)
        mag = R.fold(y.double().abs(), bias.abs())
        assert torch.all((f64(out) - ref).abs() <= 4 * EPS * mag + 1e-30), (K, P, h, w)
        # and against ConvTranspose2d itself in float64 (y carries one fp32 rounding of each of its C-term sums)
        want = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), R.gemm_columns_to_weight(wt, K), bias, stride=2, padding=1)
        ymag = (x.abs() @ wt.abs().t())
        bound = R.fold(ymag, bias.abs())[:, :K] * 8 * EPS + 1e-30
        assert torch.all((f64(out)[:, :K] - want).abs() <= bound), (K, P, h, w)
        # the unfold is the exact adjoint: <fold(y) - bias, g> == <y, unfold(g)>, and it is a pure gather (every element a copy or a zero)
        gr = torch.randn(P, Kp, 2 * h, 2 * w, generator=g)
        gy = ops.kp_deconv_unfold(gr.cuda(), K)
        assert tuple(gy.shape) == (P, h, w, 16 * Kp)
        assert torch.all(gy.reshape(P, h, w, 16, Kp)[..., K:] == 0), "padding columns"
        lhs = (R.fold(y.double(), torch.zeros(K, dtype=torch.float64)) * gr.double()).sum().item()
        rhs = (y.double() * f64(gy)).sum().item()
        scale = (R.fold(y.double().abs(), torch.zeros(K, dtype=torch.float64)) * gr.double().abs()).sum().item()
        assert abs(lhs - rhs) <= 1e-12 * scale + 1e-300, (K, P, h, w, lhs, rhs)
        y1 = torch.zeros_like(y)
        ref_gy = torch.autograd.functional.vjp(lambda t: R.fold(t, torch.zeros(K, dtype=torch.float64)), y1.double(), gr.double())[1]
        assert torch.equal(f64(gy), ref_gy), "the unfold copies"


# ================================================================================================== upsample
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 5), (28, 28)])
def test_upsample2x(ops, H, W):
    g = torch.Generator().manual_seed(H * 100 + W)
    for K in (1, 5):
        x = torch.randn(3, R.kp_pad(K), H, W, generator=g)
        got = ops.kp_upsample2x(x.cuda(), K)
        want = R.upsample2x(x.double()[:, :K])
        mag = R.upsample2x(x.double().abs()[:, :K])
        assert tuple(got.shape) == (3, K, 2 * H, 2 * W)
        assert torch.all((f64(got) - want).abs() <= 8 * EPS * mag + 1e-30), (H, W, K)
    assert tuple(ops.kp_upsample2x(torch.zeros(0, 4, H, W).cuda(), 3).shape) == (0, 3, 2 * H, 2 * W)


# ================================================================================================== loss
def run_loss(ops, x, K, tgt, valid, gscale=1.0, what=""):
    P, Kp, H, W = x.shape
    nv = int(valid.sum())
    n_valid = torch.tensor([nv], dtype=torch.int32).cuda()
    xd, td, vd = x.cuda(), tgt.cuda(), valid.cuda()
    loss, grad, rows = ops.kp_loss(xd, K, td, vd, n_valid, gscale=gscale, want_grad=True)
    ref, gref, addends = R.loss_and_grad(x, K, tgt, valid)
    sel = valid.bool()
    bound = TOL * (float(addends[sel].sum()) / nv if nv else 0.0)
    got = loss.item()
    assert np.isfinite(got) and abs(got - ref) <= bound, f"{what}: loss {got!r} vs float64 {ref!r} (bound {bound:.3e})"
    zmax = f64(x)[:, :K].abs().amax((2, 3)) + addends              # the upsampled logits are convex combinations: max |z| <= max |x|
    scale = 4 * abs(gscale) / max(nv, 1) * EPS * (8 + 2 * zmax) * sel.double()
    full = torch.zeros(P, Kp, dtype=torch.float64)
    full[:, :K] = scale
    err = (f64(grad) - gscale * gref).abs()
    assert torch.isfinite(grad).all(), what
    assert torch.all(err <= full[:, :, None, None]), f"{what}: gradient off by {err.max().item():.3e}"
    dead = torch.ones(P, Kp, dtype=torch.bool)
    dead[:, :K] = ~sel
    assert torch.all(f64(grad)[dead] == 0), f"{what}: invalid rows and padding channels must be exact zeros"
    # the row-sum table against the gradient's own sums (H W addends)
    own = f64(grad).sum((2, 3))
    assert torch.all((f64(rows) - own).abs() <= 2 * EPS * np.log2(max(H * W, 2)) * f64(grad).abs().sum((2, 3)) + 1e-30), f"{what}: row sums"
    # bit-identical on a second run
    loss2, grad2, rows2 = ops.kp_loss(xd, K, td, vd, n_valid, gscale=gscale, want_grad=True)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(rows, rows2), f"{what}: two runs differ"
    # without the gradient the loss is the same
    assert torch.equal(ops.kp_loss(xd, K, td, vd, n_valid)[0], loss), what
    return got


@pytest.mark.parametrize("H", [2, 4, 28])
def test_loss_corners_edges_and_spread(ops, H):
    g = torch.Generator().manual_seed(H)
    W, K, M = H, 5, 2 * H
    spots = [(0, 0), (0, M - 1), (M - 1, 0), (M - 1, M - 1), (0, M // 2), (M // 2, 0), (M - 1, M // 2), (M // 2, M - 1), (M // 2, M // 2 - 1)]
    P = 4
    x = 3 * torch.randn(P, R.kp_pad(K), H, W, generator=g)
    x[1] *= 80.0 / x[1].abs().max()                 # a +-80 spread: the exponentials need the maximum subtracted
    x[:, K:] = 123.0                                # padding channels hold anything
    tgt = torch.zeros(P, K, dtype=torch.int64)
    for i in range(P * K):
        y, xx = spots[i % len(spots)]
        tgt[i // K, i % K] = y * M + xx
    valid = torch.ones(P, K, dtype=torch.uint8)
    valid[2, 1] = 0
    valid[3, 4] = 0
    tgt[2, 1] = tgt[3, 4] = 0
    for gscale in (1.0, 0.37):
        run_loss(ops, x, K, tgt, valid, gscale, f"H={H} gscale={gscale}")


def test_loss_invalid_single_and_padded_rows(ops):
    g = torch.Generator().manual_seed(5)
    H, W, K = 4, 6, 3
    x = torch.randn(5, 4, H, W, generator=g)
    tgt = torch.randint(0, 4 * H * W, (5, K), generator=g)
    none = torch.zeros(5, K, dtype=torch.uint8)
    assert run_loss(ops, x, K, tgt * 0, none, what="all invalid") == 0.0
    one = none.clone()
    one[3, 2] = 1
    run_loss(ops, x, K, tgt * one.long(), one, what="a single valid row")
    # -1 padded rows: the selection's tail rows carry valid = 0, targets = 0 and whatever the predictor made of zero features
    some = torch.ones(5, K, dtype=torch.uint8)
    some[3:] = 0
    run_loss(ops, x, K, tgt * some.long(), some, gscale=2.5, what="padded rows")
    # n_valid == 0 on the device with valid flags set: loss 0 and zero gradients (the reference's sum() * 0)
    loss, grad, rows = ops.kp_loss(x.cuda(), K, tgt.cuda(), some.cuda(), torch.zeros(1, dtype=torch.int32).cuda(), want_grad=True)
    assert loss.item() == 0.0 and torch.all(grad == 0) and torch.all(rows == 0)
    # P == 0
    loss, grad, rows = ops.kp_loss(torch.zeros(0, 4, H, W).cuda(), K, torch.zeros(0, K, dtype=torch.int64).cuda(),
                                   torch.zeros(0, K, dtype=torch.uint8).cuda(), torch.zeros(1, dtype=torch.int32).cuda(), want_grad=True)
    assert loss.item() == 0.0 and grad.numel() == 0


def test_loss_refuses_planes_over_capacity(ops):
    from abr_iod_amd import _lib as L
    cap = L.lib().abr_kp_loss_max_plane()
    assert cap == 4096
    H, W = 64, 65
    args = (torch.zeros(1, 4, H, W).cuda(), 1, torch.zeros(1, 1, dtype=torch.int64).cuda(), torch.ones(1, 1, dtype=torch.uint8).cuda(),
            torch.ones(1, dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError, match="does not fit"):
        ops.kp_loss(*args)
    ok = ops.kp_loss(torch.zeros(1, 4, 64, 64).cuda(), 1, *args[2:])[0].item()      # exactly at capacity: a constant map gives log(4 H W)
    assert abs(ok - np.log(4 * 64 * 64)) <= 1e-5


# ================================================================================================== decode
def _maps(D, K, side, seed):
    """a smooth field plus one clear peak per keypoint"""
    rng = np.random.default_rng(seed)
    yy, xx = np.meshgrid(np.arange(side), np.arange(side), indexing="ij")
    maps = np.zeros((D, K, side, side), np.float32)
    for d in range(D):
        for k in range(K):
            a, b, ph = rng.uniform(0.2, 1.2, 2), rng.uniform(0.05, 0.5, 2), rng.uniform(0, 6, 2)
            cy, cx = rng.uniform(0.5, side - 1.5, 2)
            field = a[0] * np.sin(b[0] * yy + ph[0]) + a[1] * np.cos(b[1] * xx + ph[1])
            maps[d, k] = field + 6.0 * np.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * 1.7 ** 2))
    return maps


BOXES = np.array([[10.2, 20.1, 10.7, 20.4],          # narrower than a pixel both ways: max(w, 1)
                  [5, 6, 37, 30],                    # integer sides
                  [3.3, 4.4, 40.9, 29.1],            # fractional sides: the w / ceil(w) correction
                  [50, 50, 56.5, 55.2],              # smaller than the map: downscale
                  [0, 0, 311.5, 190.25],             # many times larger than the map
                  [-20.5, -10.25, 30, 700.75]], np.float32)      # reaching outside the image


def check_decode(ops, maps, boxes, what):
    D, K = maps.shape[:2]
    xy, logit = ops.kp_decode(dev(maps), dev(boxes))
    xy, logit = xy.cpu().numpy(), logit.cpu().numpy()
    index, resized = R.heatmaps_to_keypoints(maps, boxes)
    second = 0
    for d in range(D):
        _, _, gw, gh = R.grid_sides(boxes[d])
        xs, ys = R.xy_grid(boxes[d], gw, gh)
        for k in range(K):
            tol = 32 * EPS * float(np.abs(maps[d, k]).max())
            # x, y -> the kernel's index: both are exact functions of it (and distinct per grid column / row: the spacing is about a pixel)
            xi, yi = np.nonzero(xs == xy[d, k, 0])[0], np.nonzero(ys == xy[d, k, 1])[0]
            assert len(xi) == 1 and len(yi) == 1, f"{what}: ({d},{k}): ({xy[d, k, 0]}, {xy[d, k, 1]}) is no grid point's coordinate"
            i = int(yi[0]) * gw + int(xi[0])
            flat = resized[d][k].reshape(-1)
            assert xy[d, k, 2] == 1.0
            if i != index[d, k]:
                assert flat[index[d, k]] - flat[i] <= tol, f"{what}: ({d},{k}): index {i} vs float64 argmax {index[d, k]}"
                second += 1
            assert abs(float(logit[d, k]) - flat[i]) <= tol, f"{what}: ({d},{k}): logit {logit[d, k]} vs {flat[i]}"
    return second, D * K


@pytest.mark.parametrize("side,K", [(8, 1), (8, 17), (56, 1), (56, 17)])
def test_decode_against_float64(ops, side, K):
    maps = _maps(len(BOXES), K, side, seed=side * 100 + K)
    second, total = check_decode(ops, maps, BOXES, f"side={side} K={K}")
    assert second <= 0.02 * total, f"{second} of {total} pairs agree with float64 only within the rounding bound"


def test_decode_ties_take_the_lowest_index(ops):
    boxes = np.array([[4, 4, 60, 60], [0, 0, 8, 8], [2, 3, 300.5, 200.5]], np.float32)
    const = np.full((3, 2, 8, 8), 1.5, np.float32)          # constant: cubic weights sum to 1 up to rounding, so only the 1:1 box is exact
    xy, logit = ops.kp_decode(dev(const), dev(boxes))
    assert xy[1].cpu().tolist() == [[0.5, 0.5, 1.0]] * 2 and logit[1].cpu().tolist() == [1.5, 1.5]
    two = np.zeros((1, 1, 8, 8), np.float32)                # two equal peaks, resized 1:1 (an 8 x 8 box): exact copies
    two[0, 0, 5, 2] = two[0, 0, 2, 6] = 4.0
    xy, logit = ops.kp_decode(dev(two), dev(np.array([[10, 20, 18, 28]], np.float32)))
    assert xy[0, 0].cpu().tolist() == [16.5, 22.5, 1.0] and logit.item() == 4.0
    # a constant 56 x 56 map resized 1:1: every lane of every wave holds equal values, index 0 must come through both reduction steps
    xy, logit = ops.kp_decode(dev(np.full((2, 3, 56, 56), -2.25, np.float32)), dev(np.array([[7, 9, 63, 65], [0, 0, 56, 56]], np.float32)))
    assert xy.cpu().tolist() == [[[7.5, 9.5, 1.0]] * 3, [[0.5, 0.5, 1.0]] * 3] and torch.all(logit == -2.25)
    # no detections
    xy, logit = ops.kp_decode(torch.zeros(0, 17, 56, 56).cuda(), torch.zeros(0, 4).cuda())
    assert tuple(xy.shape) == (0, 17, 3) and tuple(logit.shape) == (0, 17)

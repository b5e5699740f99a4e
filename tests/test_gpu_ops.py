"""GPU parity tests: the HIP path (through the C ABI) vs the oracle and the reference-generated goldens.

Integer / index outputs are compared bit-exact; floating point within the tolerance written at each assert.
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def T(a, dev="cuda"):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def nhwc(x):  # numpy NCHW -> torch NHWC on device
    return T(np.ascontiguousarray(np.transpose(x, (0, 2, 3, 1))))


@pytest.fixture(scope="module")
def O():
    from oracle import ops
    return ops


@pytest.fixture(scope="module")
def R():
    from oracle import torch_ref
    return torch_ref


# ------------------------------------------------------------------------------------------ ROIAlign
def test_roi_align_taps_bit_exact(gold, O):
    """integer tap indices of the kernel's own indexing code == oracle's, on goldens and on 600x1000-shaped proposals"""
    from abr_iod_amd import ops
    g = gold("roi_align")
    for sr in (0, 2):
        idx, grid = ops.roi_align_taps(T(g["rois"]), 10, 14, 1 / 16, 7, 7, sr, 16)
        ridx, rgrid = O.roi_align_taps(g["rois"], 10, 14, 1 / 16, 7, 7, sr, 16)
        assert np.array_equal(grid.cpu().numpy(), rgrid)
        assert np.array_equal(idx.cpu().numpy(), ridx)
    rng = np.random.default_rng(0)
    K = 4096
    x1 = rng.uniform(-20, 980, K); y1 = rng.uniform(-20, 580, K)
    w = np.exp(rng.uniform(np.log(2), np.log(900), K)); h = np.exp(rng.uniform(np.log(2), np.log(560), K))
    rois = np.stack([rng.integers(0, 4, K), x1, y1, np.minimum(x1 + w, 1010), np.minimum(y1 + h, 610)], 1).astype(np.float32)
    idx, grid = ops.roi_align_taps(T(rois), 38, 63, 0.0625, 7, 7, 0, 64)
    ridx, rgrid = O.roi_align_taps(rois, 38, 63, 0.0625, 7, 7, 0, 64)
    assert np.array_equal(grid.cpu().numpy(), rgrid)
    assert np.array_equal(idx.cpu().numpy(), ridx)


@pytest.mark.parametrize("name,hw", [("roi_align", (10, 14)), ("roi_align_c4", (38, 63))])
def test_roi_align_forward_golden_bit_exact(gold, name, hw):
    from abr_iod_amd import _C, ops
    g = gold(name)
    for sr in (0, 2):
        want = g[f"out_sr{sr}"]
        # drop-in NCHW entry point (maskrcnn_benchmark._C.roi_align_forward signature)
        got = _C.roi_align_forward(T(g["feat"]), T(g["rois"]), 1 / 16, 7, 7, sr).cpu().numpy()
        assert np.array_equal(got, want), f"NCHW sr={sr}: max abs diff {np.abs(got - want).max()}"
        # native NHWC kernel
        got = ops.roi_align_forward(nhwc(g["feat"]), T(g["rois"]), 1 / 16, 7, 7, sr).permute(0, 3, 1, 2).cpu().numpy()
        assert np.array_equal(got, want), f"NHWC sr={sr}: max abs diff {np.abs(got - want).max()}"
    if name == "roi_align":
        got = _C.roi_align_forward(T(g["feat"]), T(g["rois"]), 0.0625, 3, 5, 0).cpu().numpy()
        assert np.array_equal(got, g["out_sr0_3x5"])


def test_roi_align_forward_bin_step_and_empty(gold):
    from abr_iod_amd import _C, ops
    g = gold("roi_align_c4")
    full = ops.roi_align_forward(nhwc(g["feat"]), T(g["rois"]), 0.0625, 7, 7, 0)
    even = ops.roi_align_forward(nhwc(g["feat"]), T(g["rois"]), 0.0625, 7, 7, 0, bin_step=2)
    assert even.shape == (40, 4, 4, 24)
    assert torch.equal(even, full[:, ::2, ::2, :].contiguous())
    out = _C.roi_align_forward(T(g["feat"]), torch.zeros((0, 5), device="cuda"), 0.0625, 7, 7, 0)
    assert out.shape == (0, 24, 7, 7)


def test_roi_align_backward_vs_oracle(gold, O):
    from abr_iod_amd import _C, ops
    g = gold("roi_align_c4")
    rng = np.random.default_rng(1)
    for sr in (0, 2):
        gy = rng.standard_normal((40, 24, 7, 7)).astype(np.float32)
        want = O.roi_align_backward(gy, g["rois"], 0.0625, 7, 7, 2, 24, 38, 63, sr)
        got = _C.roi_align_backward(T(gy), T(g["rois"]), 0.0625, 7, 7, 2, 24, 38, 63, sr).cpu().numpy()
        # same per-tap products; only the fp32 summation order of the atomics differs
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
        for method in ("gather", "scatter"):  # atomic-free gather (training default) and per-RoI atomic scatter
            got = ops.roi_align_backward(nhwc(gy), T(g["rois"]), 0.0625, 7, 7, sr, 2, 38, 63, 24, method=method).permute(0, 3, 1, 2).cpu().numpy()
            np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)
        a1 = ops.roi_align_backward(nhwc(gy), T(g["rois"]), 0.0625, 7, 7, sr, 2, 38, 63, 24)
        a2 = ops.roi_align_backward(nhwc(gy), T(g["rois"]), 0.0625, 7, 7, sr, 2, 38, 63, 24)
        assert torch.equal(a1, a2)  # the gather form is deterministic (fixed summation order)
        acc = ops.roi_align_backward(nhwc(gy), T(g["rois"]), 0.0625, 7, 7, sr, 2, 38, 63, 24, out=a1.clone())
        assert torch.allclose(acc, 2 * a1, rtol=1e-6, atol=1e-6)
    # bin_step=2 backward == full backward of a gradient that is zero on the odd bins
    gy = rng.standard_normal((40, 24, 7, 7)).astype(np.float32)
    gz = np.zeros_like(gy); gz[:, :, ::2, ::2] = gy[:, :, ::2, ::2]
    want = O.roi_align_backward(gz, g["rois"], 0.0625, 7, 7, 2, 24, 38, 63, 0)
    ge = nhwc(gy)[:, ::2, ::2, :].contiguous()
    got = ops.roi_align_backward(ge, T(g["rois"]), 0.0625, 7, 7, 0, 2, 38, 63, 24, bin_step=2).permute(0, 3, 1, 2).cpu().numpy()
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-5)


def test_roi_align_full_size_properties():
    """BASELINE size (B=2, C=1024, 38x63, 1024 RoIs): constant map -> constant output; linearity; adjointness."""
    from abr_iod_amd import ops
    torch.manual_seed(0)
    B, H, W, Ch, K = 2, 38, 63, 1024, 1024
    x1 = torch.rand(K) * 900; y1 = torch.rand(K) * 500
    rois = torch.stack([torch.randint(0, B, (K,)).float(), x1, y1, x1 + 16 + torch.rand(K) * 600, y1 + 16 + torch.rand(K) * 400], 1).cuda()
    rois[:, 3].clamp_(max=999); rois[:, 4].clamp_(max=599)
    ones = torch.full((B, H, W, Ch), 3.0, device="cuda")
    out = ops.roi_align_forward(ones, rois, 0.0625, 7, 7, 0)
    assert torch.allclose(out, torch.full_like(out, 3.0), rtol=0, atol=1e-5)  # weights of every sample sum to 1
    a = torch.randn(B, H, W, Ch, device="cuda"); b = torch.randn(B, H, W, Ch, device="cuda")
    ya, yb, yab = (ops.roi_align_forward(t, rois, 0.0625, 7, 7, 0) for t in (a, b, a + 2 * b))
    assert torch.allclose(yab, ya + 2 * yb, rtol=1e-4, atol=1e-4)
    gy = torch.randn_like(ya)
    gx = ops.roi_align_backward(gy, rois, 0.0625, 7, 7, 0, B, H, W, Ch)
    lhs = (ya.double() * gy.double()).sum().item(); rhs = (a.double() * gx.double()).sum().item()
    assert abs(lhs - rhs) < 1e-4 * max(1.0, abs(lhs))


@pytest.mark.parametrize("B,H,W,Ch", [(3, 13, 21, 256), (1, 38, 63, 512), (4, 9, 17, 1024), (2, 7, 30, 2048), (2, 11, 9, 1536), (5, 5, 5, 64)])
def test_roi_align_backward_gather_reaches_every_tile_under_the_xcd_mapping(B, H, W, Ch):
    """The gather's workgroups take their (channel chunk, image, row, x-tile) from the XCD they run on (round 6; 1, 2, 4 or 8 chunks of 256
    channels; any other count -- 1536 channels -- keeps the 3-D grid): odd extents, every chunk count, spatial tile counts that do not divide by
    the XCDs per chunk.  A missed or doubled tile shows against the per-RoI atomic scatter form; bin_step = 2 too."""
    from abr_iod_amd import ops
    torch.manual_seed(B * 1000 + Ch)
    K = 64 * B
    x1 = torch.rand(K) * (W * 16 - 40); y1 = torch.rand(K) * (H * 16 - 40)
    rois = torch.stack([torch.randint(0, B, (K,)).float(), x1, y1, x1 + 8 + torch.rand(K) * W * 10, y1 + 8 + torch.rand(K) * H * 10], 1).cuda()
    rois[:, 3].clamp_(max=W * 16 - 1); rois[:, 4].clamp_(max=H * 16 - 1)
    for step in (1, 2):
        P = (7 + step - 1) // step
        gy = torch.randn(K, P, P, Ch, device="cuda")
        got = ops.roi_align_backward(gy, rois, 0.0625, 7, 7, 2, B, H, W, Ch, bin_step=step)
        want = ops.roi_align_backward(gy, rois, 0.0625, 7, 7, 2, B, H, W, Ch, bin_step=step, method="scatter")
        assert torch.allclose(got, want, rtol=1e-4, atol=1e-4 * float(want.abs().max())), (step, float((got - want).abs().max()))
        assert torch.equal(got, ops.roi_align_backward(gy, rois, 0.0625, 7, 7, 2, B, H, W, Ch, bin_step=step))


# ------------------------------------------------------------------------------------------ NMS
def test_nms_golden_index_exact(gold, O):
    from abr_iod_amd import _C
    g = gold("nms")
    for thr, key in ((0.5, "keep_5"), (0.7, "keep_7")):
        got = _C.nms(T(g["boxes"]), T(g["scores"]), thr).cpu().numpy()
        assert got.dtype == np.int64 and np.array_equal(got, g[key])
    # '>=' (CPU, canonical) vs '>' (CUDA) on the IoU == thr pair
    assert 1 not in _C.nms(T(g["boxes"]), T(g["scores"]), 0.5).cpu().numpy()
    assert 1 in _C.nms(T(g["boxes"]), T(g["scores"]), 0.5, strict_gt=True).cpu().numpy()
    assert _C.nms(torch.zeros((0, 4), device="cuda"), torch.zeros((0,), device="cuda"), 0.5).numel() == 0


def test_nms_large_vs_oracle(O):
    """RPN-sized: 2 images x up to 6000 sorted proposals, batched, early stop at max_keep."""
    from abr_iod_amd import ops
    rng = np.random.default_rng(3)
    N, n = 2, 6000
    cx = rng.uniform(0, 1000, (N, n)); cy = rng.uniform(0, 600, (N, n))
    w = np.exp(rng.uniform(np.log(16), np.log(500), (N, n))); h = np.exp(rng.uniform(np.log(16), np.log(400), (N, n)))
    boxes = np.stack([np.clip(cx - w / 2, 0, 999), np.clip(cy - h / 2, 0, 599), np.clip(cx + w / 2, 0, 999), np.clip(cy + h / 2, 0, 599)], -1).astype(np.float32)
    counts = np.array([6000, 4321], np.int32)
    scores = -np.arange(n, dtype=np.float32)  # already sorted descending
    for max_keep in (1000, 6000):
        keep, nk = ops.nms_sorted_batched(T(boxes), T(counts), 0.7, max_keep)
        keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
        for i in range(N):
            want = O.nms(boxes[i, :counts[i]], scores[:counts[i]], 0.7)[:max_keep]
            assert nk[i] == len(want)
            assert np.array_equal(keep[i, :nk[i]], want)


@pytest.mark.parametrize("case", ["chunk_edges", "all_duplicates", "no_overlap", "limit_inside_block", "ragged_counts"])
def test_nms_chunked_sweep_edge_cases(O, case):
    """The NMS runs in chunks of 2048 boxes (lazy mask, csrc/nms.hip) and sweeps 256-box blocks: box counts on / around the chunk and
    block boundaries, keep limits that fall inside a block, lists where every box or no box is suppressed -- keep lists equal the oracle's."""
    from abr_iod_amd import ops
    rng = np.random.default_rng(11)

    def boxes_for(n, spread=1000.0, size=(16, 300)):
        cx = rng.uniform(0, spread, n); cy = rng.uniform(0, spread * 0.6, n)
        w = np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), n)); h = np.exp(rng.uniform(np.log(size[0]), np.log(size[1]), n))
        return np.stack([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], -1).astype(np.float32)

    if case == "chunk_edges":
        sets = [(boxes_for(n), mk) for n, mk in ((1, 5), (63, 100), (64, 100), (255, 300), (256, 300), (257, 300), (2047, 3000), (2048, 3000),
                                                  (2049, 3000), (4096 + 17, 5000), (6143, 700))]
    elif case == "all_duplicates":
        b = np.tile(np.array([[10, 10, 200, 150]], np.float32), (3000, 1))
        sets = [(b, 100)]
    elif case == "no_overlap":     # a grid of disjoint boxes: everything is kept until the limit
        g = np.arange(2500)
        b = np.stack([(g % 50) * 20, (g // 50) * 20, (g % 50) * 20 + 10, (g // 50) * 20 + 10], -1).astype(np.float32)
        sets = [(b, 2500), (b, 2048), (b, 300), (b, 257)]
    elif case == "limit_inside_block":
        b = boxes_for(5000, spread=4000.0, size=(8, 60))
        sets = [(b, mk) for mk in (1, 2, 63, 64, 65, 255, 256, 257, 1000, 2049)]
    else:
        sets = None
    if sets is not None:
        for b, mk in sets:
            n = len(b)
            scores = -np.arange(n, dtype=np.float32)
            keep, nk = ops.nms_sorted_batched(T(b[None]), T(np.array([n], np.int32)), 0.7, mk)
            want = O.nms(b, scores, 0.7)[:mk]
            got = keep.cpu().numpy()[0, :int(nk.cpu()[0])]
            assert np.array_equal(got, want), (case, n, mk, len(got), len(want))
        return
    # ragged: four images with different counts in one batched call (one of them empty)
    n = 5000
    b = np.stack([boxes_for(n) for _ in range(4)])
    counts = np.array([5000, 2048, 0, 333], np.int32)
    keep, nk = ops.nms_sorted_batched(T(b), T(counts), 0.7, 600)
    keep, nk = keep.cpu().numpy(), nk.cpu().numpy()
    for i in range(4):
        want = O.nms(b[i, :counts[i]], -np.arange(counts[i], dtype=np.float32), 0.7)[:600] if counts[i] else np.zeros((0,), np.int64)
        assert nk[i] == len(want) and np.array_equal(keep[i, :nk[i]], want), i


# ------------------------------------------------------------------------------------------ focal / smooth-L1
def test_sigmoid_focal(gold, O):
    from abr_iod_amd import _C
    g = gold("sigmoid_focal")
    lo = _C.sigmoid_focalloss_forward(T(g["logits"]), T(g["targets"]), 6, 2.0, 0.25).cpu().numpy()
    np.testing.assert_allclose(lo, O.sigmoid_focal_forward(g["logits"], g["targets"], 2.0, 0.25), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(lo, g["loss"], rtol=2e-5, atol=1e-7)
    d = _C.sigmoid_focalloss_backward(T(g["logits"]), T(g["targets"]), T(g["d_loss"]), 6, 2.0, 0.25).cpu().numpy()
    np.testing.assert_allclose(d, O.sigmoid_focal_backward(g["logits"], g["targets"], g["d_loss"], 2.0, 0.25), rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(d, g["d_logits"], rtol=2e-4, atol=2e-6)


def test_smooth_l1(gold):
    from abr_iod_amd import ops
    g = gold("smooth_l1")
    n = g["x"].size
    for tag, beta, scale in (("b19_sum", 1 / 9, 1.0), ("b1_sum", 1.0, 1.0), ("b19_mean", 1 / 9, 1.0 / n)):
        loss, grad = ops.smooth_l1(T(g["x"]), T(g["t"]), beta, scale=scale, want_grad=True)
        np.testing.assert_allclose(loss[0].item(), g[f"{tag}_loss"], rtol=1e-6)
        np.testing.assert_allclose(grad.cpu().numpy(), g[f"{tag}_grad"], rtol=1e-5, atol=1e-8)


# ------------------------------------------------------------------------------------------ box-head / distillation losses
def test_box_head_losses(gold):
    from abr_iod_amd import ops
    g = gold("box_head_loss")
    for (ko, ka) in ((16, 21), (11, 21), (11, 16)):
        p = f"k{ko}_{ka}"
        logits, reg, labels, rt = T(g[f"{p}_logits"]), T(g[f"{p}_reg"]), T(g[f"{p}_labels"]), T(g[f"{p}_rt"])
        for dist in ("id", "l2"):
            loss, dz = ops.softmax_ce(logits, labels, inclusive=(dist == "id"), n_old=ko - 1, want_grad=True)
            np.testing.assert_allclose(loss[0].item(), g[f"{p}_{dist}_cls"], rtol=1e-5)          # 1e-4 budget
            np.testing.assert_allclose(dz.cpu().numpy(), g[f"{p}_{dist}_dlogits"], rtol=1e-4, atol=1e-8)
            pos = torch.nonzero(labels > 0).squeeze(1)
            lb, dr = ops.smooth_l1_rows(reg, rt, pos, 4 * labels[pos], 1.0, scale=1.0 / labels.numel(), want_grad=True)
            np.testing.assert_allclose(lb[0].item(), g[f"{p}_{dist}_box"], rtol=1e-5)
            np.testing.assert_allclose(dr.cpu().numpy(), g[f"{p}_{dist}_dreg"], rtol=1e-5, atol=1e-9)


def test_roi_distillation(gold):
    from abr_iod_amd import ops
    g = gold("roi_distill")
    for (ko, ka) in ((16, 21), (11, 21), (11, 16), (21, 21)):
        p = f"k{ko}_{ka}"
        for dist in ("id", "l2"):
            if f"{p}_{dist}_loss" not in g.files:
                with pytest.raises(RuntimeError):  # K_all == K_old with dist='id': shape error in the reference too
                    ops.roi_distill(T(g[f"{p}_zs"]), T(g[f"{p}_bs"]), T(g[f"{p}_zt"]), T(g[f"{p}_bt"]), dist_id=True)
                continue
            loss, dzt, dbt = ops.roi_distill(T(g[f"{p}_zs"]), T(g[f"{p}_bs"]), T(g[f"{p}_zt"]), T(g[f"{p}_bt"]),
                                             dist_id=(dist == "id"), want_grad=True)
            np.testing.assert_allclose(loss[0].item(), g[f"{p}_{dist}_loss"], rtol=1e-5)
            np.testing.assert_allclose(dzt.cpu().numpy(), g[f"{p}_{dist}_dzt"], rtol=1e-4, atol=1e-8)
            np.testing.assert_allclose(dbt.cpu().numpy().reshape(g[f"{p}_{dist}_dbt"].shape), g[f"{p}_{dist}_dbt"], rtol=1e-5, atol=1e-9)


def test_ard(gold):
    from abr_iod_amd import _lib, ops
    g = gold("ard")
    for tag in ("s", "m"):
        fs, ft = g[f"{tag}_fs"], g[f"{tag}_ft"]
        for gamma in (0, 1, 5):
            loss, coef = ops.ard_forward(nhwc(fs), nhwc(ft), float(gamma))
            np.testing.assert_allclose(loss[0].item(), g[f"{tag}_loss_g{gamma}"], rtol=1e-5)      # 1e-4 relative budget
            np.testing.assert_allclose(coef[:, 0].cpu().numpy().reshape(g[f"{tag}_att_s"].shape), g[f"{tag}_att_s"], rtol=1e-5)
            if f"{tag}_dft_g{gamma}" in g.files:
                gr = ops.ard_backward(nhwc(fs), nhwc(ft), coef, float(gamma)).permute(0, 3, 1, 2).cpu().numpy()
                want = g[f"{tag}_dft_g{gamma}"]
                np.testing.assert_allclose(gr, want, rtol=1e-4, atol=1e-5 * np.abs(want).max())
        # reference tensor layout (NCHW) entry
        loss, coef = ops.ard_forward(T(fs), T(ft), 1.0, layout=_lib.NCHW)
        np.testing.assert_allclose(loss[0].item(), g[f"{tag}_loss_g1"], rtol=1e-5)
        gr = ops.ard_backward(T(fs), T(ft), coef, 1.0, layout=_lib.NCHW).cpu().numpy()
        np.testing.assert_allclose(gr, g[f"{tag}_dft_g1"], rtol=1e-4, atol=1e-5 * np.abs(g[f"{tag}_dft_g1"]).max())


def test_ard_full_size_properties(R):
    """[256,1024,7,7] (B=4): identical maps -> 0; loss vs torch-CPU oracle on a subsample-free run."""
    from abr_iod_amd import ops
    torch.manual_seed(0)
    fs = torch.randn(256, 7, 7, 1024, device="cuda")
    loss, _ = ops.ard_forward(fs, fs, 1.0)
    assert loss[0].item() == 0.0  # identical maps: both attention maps are bitwise equal -> afd == pad == 0 exactly
    ft = fs + 0.3 * torch.randn_like(fs)
    loss, coef = ops.ard_forward(fs, ft, 1.0)
    want = R.ard_loss(fs[:32].permute(0, 3, 1, 2).cpu(), ft[:32].permute(0, 3, 1, 2).cpu(), 1.0).item()
    l32, _ = ops.ard_forward(fs[:32].contiguous(), ft[:32].contiguous(), 1.0)
    assert abs(l32[0].item() - want) < 1e-5 * abs(want)


# ------------------------------------------------------------------------------------------ RPN glue
def test_anchors_match_encode_decode(gold, O):
    from abr_iod_amd import ops
    g = gold("anchors")
    cell = T(g["cell"].astype(np.float32))
    for i in (0, 1):
        a, v = ops.grid_anchors(cell, 38, 63, 16, int(g["image_sizes"][i][0]), int(g["image_sizes"][i][1]))
        assert np.array_equal(a.cpu().numpy(), g[f"bbox{i}"]) and np.array_equal(v.cpu().numpy().astype(bool), g[f"vis{i}"].astype(bool))
    g = gold("matcher")
    for tag, hi, lo, lq in (("rpn", 0.7, 0.3, True), ("head", 0.5, 0.5, False)):
        m, lab, tgt = ops.match_encode(T(g["prop"]), T(g["gt"]), None, None, hi, lo, lq, (1, 1, 1, 1), rpn_labels=True)
        assert np.array_equal(m.cpu().numpy(), g[f"{tag}_matched"])
    g = gold("rpn")
    for i in (0, 1):
        m, lab, tgt = ops.match_encode(T(g[f"anchors{i}"]), T(g[f"gt{i}"]), None, T(g[f"vis{i}"].astype(np.uint8)), 0.7, 0.3, True,
                                       (1, 1, 1, 1), rpn_labels=True)
        assert np.array_equal(m.cpu().numpy(), g["rpn_matched"][i])
        assert np.array_equal(lab.cpu().numpy(), g["rpn_labels"][i])
        np.testing.assert_allclose(tgt.cpu().numpy(), g["rpn_reg_targets"][i], rtol=1e-5, atol=1e-6)
    g = gold("box_coder")
    ex = T(g["ex"])
    idx = torch.arange(64, device="cuda").view(1, 64)
    hw = torch.tensor([[100000, 100000]], dtype=torch.int32, device="cuda")
    for tag, w in (("rpn", (1, 1, 1, 1)), ("head", (10, 10, 5, 5))):
        for c in range(3):
            d = T(g[f"{tag}_deltas"]).view(1, 64, 12)
            out = ops.rpn_decode_clip(d, 4 * c, ex, idx, hw, w)[0].cpu().numpy()
            want = np.clip(g[f"{tag}_dec"][:, 4 * c:4 * c + 4], 0, 99999)
            np.testing.assert_allclose(out, want, rtol=1e-5, atol=1e-3)


# ------------------------------------------------------------------------------------------ conv engine
def _conv_ref(x, w, stride, pad, scale, bias, residual, relu):
    y = torch.nn.functional.conv2d(x, w, stride=stride, padding=pad)
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
    if residual is not None:
        y = y + residual
    return torch.relu(y) if relu else y


CONV_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad   (shapes that exercise every tile config + edges)
    (2, 64, 19, 23, 64, 1, 1, 0),      # BN=64 path
    (2, 64, 19, 23, 256, 3, 1, 1),     # 3x3 halo
    (1, 256, 38, 63, 512, 1, 2, 0),    # stride-2 1x1 (layer3.0 / downsample)
    (2, 128, 16, 16, 76, 1, 1, 0),     # Cout not a multiple of 32 (fused RPN cls+bbox head)
    (1, 4, 37, 45, 64, 7, 2, 3),       # padded stem, SMALL_C path
    (1, 1024, 38, 63, 1024, 3, 1, 1),  # RPN 3x3 at full C4 size
    (512, 512, 4, 4, 512, 3, 1, 1),    # layer4 conv2 on 512 RoIs
    (8, 2048, 1, 1, 108, 1, 1, 0),     # predictor FC
]


@pytest.mark.parametrize("case", CONV_CASES)
def test_conv_forward_vs_torch_cpu(case):
    from abr_iod_amd import ops
    B, Cin, H, W, Cout, k, s, p = case
    torch.manual_seed(hash(case) % 1000)
    x = torch.randn(B, Cin, H, W); w = torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    scale = torch.rand(Cout) + 0.5; bias = torch.randn(Cout) * 0.1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    res = torch.randn(B, Cout, Ho, Wo)
    want = _conv_ref(x, w, s, p, scale, bias, res, True)
    got = ops.conv_forward(x.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(0, 2, 3, 1).contiguous().cuda(), s, p,
                           scale=scale.cuda(), bias=bias.cuda(), residual=res.permute(0, 2, 3, 1).contiguous().cuda(), relu=True)
    got = got.permute(0, 3, 1, 2).cpu()
    # fp32 MFMA == fmaf chain; torch CPU (oneDNN) sums in another order: 1e-4 of the output scale (north_star tolerance)
    assert (got - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())
    plain = ops.conv_forward(x.permute(0, 2, 3, 1).contiguous().cuda(), w.permute(0, 2, 3, 1).contiguous().cuda(), s, p)
    want = _conv_ref(x, w, s, p, None, None, None, False)
    assert (plain.permute(0, 3, 1, 2).cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[1] % 4 == 0 and c[4] % 4 == 0])
def test_conv_backward_vs_torch_autograd(case):
    from abr_iod_amd import ops
    B, Cin, H, W, Cout, k, s, p = case
    if k == 7:
        pytest.skip("stem is frozen (FREEZE_CONV_BODY_AT=2): no backward on the path")
    torch.manual_seed(1 + hash(case) % 1000)
    x = torch.randn(B, Cin, H, W, requires_grad=True); w = (torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5).requires_grad_(True)
    scale = torch.rand(Cout) + 0.5
    y = torch.nn.functional.conv2d(x, w, stride=s, padding=p) * scale.view(1, -1, 1, 1)
    gy = torch.randn_like(y)
    y.backward(gy)
    xg = x.detach().permute(0, 2, 3, 1).contiguous().cuda(); wg = w.detach().permute(0, 2, 3, 1).contiguous().cuda()
    gyg = gy.permute(0, 2, 3, 1).contiguous().cuda(); sc = scale.cuda()
    dw = torch.zeros_like(wg)
    ops.conv_wgrad(xg, gyg, dw, s, p, scale=sc)
    want = w.grad.permute(0, 2, 3, 1)
    assert (dw.cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())
    wt = ops.conv_dgrad_weights(wg, sc)
    if s == 1:
        dx = ops.conv_forward(gyg, wt, 1, k - 1 - p)
    else:  # stride-2 1x1: rows land on the even pixels of a zeroed tensor
        dx = ops.conv_forward(gyg, wt, 1, 0, out_hw=(H, W), out_stride=(s, s))
    want = x.grad.permute(0, 2, 3, 1)
    assert (dx.cpu() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


def test_pointwise_and_sgd():
    from abr_iod_amd import ops
    torch.manual_seed(0)
    x = torch.randn(2, 3, 33, 47)
    got = ops.nchw_to_nhwc(x.cuda(), cpad=4).cpu()
    assert torch.equal(got[..., :3], x.permute(0, 2, 3, 1)) and torch.all(got[..., 3] == 0)
    y = torch.randn(2, 64, 37, 45)
    mp = ops.maxpool3x3s2(y.permute(0, 2, 3, 1).contiguous().cuda()).permute(0, 3, 1, 2).cpu()
    assert torch.equal(mp, torch.nn.functional.max_pool2d(y, 3, 2, 1))
    z = torch.randn(16, 4, 4, 2048)
    ap = ops.avgpool_forward(z.cuda()).cpu()
    assert torch.allclose(ap, z.mean(dim=(1, 2)), rtol=1e-6, atol=1e-6)
    back = ops.nhwc_to_nchw(ops.nchw_to_nhwc(y.cuda())).cpu()
    assert torch.equal(back, y)
    # fused multi-tensor SGD vs torch.optim.SGD with per-tensor groups (solver/build.py:7-21)
    sizes = [1000, 64, 4096, 7]
    ps = [torch.randn(s) for s in sizes]; gs = [torch.randn(s) for s in sizes]
    lrs = [0.01, 0.02, 0.01, 0.02]; wds = [1e-4, 0.0, 1e-4, 0.0]
    ref = [p.clone().requires_grad_(True) for p in ps]
    opt = torch.optim.SGD([{"params": [r], "lr": lr, "weight_decay": wd} for r, lr, wd in zip(ref, lrs, wds)], lr=0.01, momentum=0.9)
    flat_p = torch.cat(ps).cuda(); flat_m = torch.zeros_like(flat_p)
    seg = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device="cuda")
    lr_d = torch.tensor(lrs, device="cuda"); wd_d = torch.tensor(wds, device="cuda")
    for step in range(3):
        for r, g_ in zip(ref, gs):
            r.grad = g_.clone() * (step + 1)
        opt.step()
        flat_g = torch.cat([g_ * (step + 1) for g_ in gs]).cuda()
        ops.sgd_momentum_(flat_p, flat_g, flat_m, seg, lr_d, wd_d, 0.9, first_step=(step == 0))
    assert torch.allclose(flat_p.cpu(), torch.cat([r.detach() for r in ref]), rtol=1e-6, atol=1e-7)


def test_fused_sampler():
    """abr_sample_pos_neg == BalancedPositiveNegativeSampler semantics: counts, membership, ascending unique indices, -1 padding,
    and a uniform draw (every candidate is chosen with the same frequency)."""
    from abr_iod_amd import ops
    torch.manual_seed(0)
    N, n = 3, 5000
    labels = torch.zeros(N, n)
    labels[0, torch.randperm(n)[:40]] = 1           # fewer positives than the cap
    labels[1, torch.randperm(n)[:700]] = 1          # more positives than the cap
    labels[2, :] = -1; labels[2, 100:130] = 1; labels[2, 200:260] = 0   # not enough negatives either
    labels[0, torch.randperm(n)[:500]] = -1
    lab = labels.cuda()
    pos, neg, counts = ops.sample_pos_neg(lab, 256, 128, index_offset_per_image=n, seed=1234)
    c = counts.cpu().numpy()
    want = [(min(int((labels[i] >= 1).sum()), 128),) for i in range(N)]
    for i in range(N):
        npos = want[i][0]; nneg = min(int((labels[i] == 0).sum()), 256 - npos)
        assert tuple(c[i]) == (npos, nneg)
        p = pos[i].cpu(); q = neg[i].cpu()
        assert (p[npos:] == -1).all() and (q[nneg:] == -1).all()
        p, q = p[:npos] - i * n, q[:nneg] - i * n
        assert (p[1:] > p[:-1]).all() and (q[1:] > q[:-1]).all()            # ascending, unique
        assert (labels[i][p] >= 1).all() and (labels[i][q] == 0).all()
    # int64 labels (box head), single image
    li = torch.randint(-1, 4, (3000,)).cuda()
    p, q, c = ops.sample_pos_neg(li, 512, 128, seed=7)
    assert int(c[0, 0]) == 128 and int(c[0, 1]) == 384 and (li[p[0]] >= 1).all() and (li[q[0, :384]] == 0).all() and (q[0, 384:] == -1).all()
    # uniformity: 700 positives, 128 drawn, 600 independent draws -> each chosen ~ 600*128/700 = 109.7 times (sigma ~ 9.5)
    hits = torch.zeros(n)
    for s in range(600):
        p, _, _ = ops.sample_pos_neg(lab[1:2], 256, 128, seed=1000 + s)
        hits[p[0].cpu() - 0] += 1
    h = hits[labels[1] >= 1]
    assert abs(h.mean().item() - 600 * 128 / 700) < 1e-3 and h.std().item() < 13 and h.min() > 60 and h.max() < 160
    assert hits[labels[1] < 1].sum() == 0


@pytest.mark.parametrize("n", [3000, 8192, 8193, 36000, 63000, 70000, 151000])
def test_fused_sampler_draw_is_the_k_smallest_keys(n):
    """The draw is defined (csrc/sampler.hip): every candidate of a class gets the 32-bit key hash(seed, image, index); the k smallest keys
    (ties by index) are taken and written in ascending index order.  Restated in numpy and compared exactly, for both workgroup sizes
    (n <= 8192: 256 threads, above: 1024), per-wave ranges that do not divide n, more than 64 visits per lane (70000: the labels are re-read) and
    more candidates than the LDS byte cache holds (151000: every pass hashes)."""
    from abr_iod_amd import ops
    rng = np.random.default_rng(n)
    N, batch, max_pos, seed = 3, 256, 128, 987654321
    labels = rng.integers(-1, 2, (N, n)).astype(np.float32)      # ~1/3 each: ignored / negative / positive
    labels[1, rng.permutation(n)[: n - 50]] = -1                  # an image with fewer candidates than the quota
    pos, neg, counts = ops.sample_pos_neg(T(labels), batch, max_pos, seed=seed)
    pos, neg, counts = pos.cpu().numpy(), neg.cpu().numpy(), counts.cpu().numpy()

    def keys(img, idx):
        with np.errstate(over="ignore"):
            z = np.uint64(seed) + np.uint64(0x9E3779B97F4A7C15) * ((np.uint64(img) << np.uint64(32)) | idx.astype(np.uint64)) + np.uint64(0x632BE59BD9B4E019)
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return ((z >> np.uint64(16)) & np.uint64(0xFFFFFFFF)).astype(np.int64)

    for i in range(N):
        p_all, n_all = np.nonzero(labels[i] >= 1)[0], np.nonzero(labels[i] == 0)[0]
        k_pos = min(len(p_all), max_pos)
        k_neg = min(len(n_all), batch - k_pos)
        assert tuple(counts[i]) == (k_pos, k_neg)
        for cand, k, got in ((p_all, k_pos, pos[i]), (n_all, k_neg, neg[i])):
            order = np.lexsort((cand, keys(i, cand)))             # by key, ties by index
            want = np.sort(cand[order[:k]])
            assert np.array_equal(got[:k], want), (n, i, k)
            assert (got[k:] == -1).all()


def test_topk_sigmoid_matches_torch():
    """fused sigmoid + sorted top-k == torch.sigmoid(...).topk(sorted=True) (values exact up to 1 ulp of expf, order identical
    wherever scores differ; ties resolved by ascending index)."""
    from abr_iod_amd import ops
    torch.manual_seed(0)
    N, H, W, A, ld = 3, 38, 63, 15, 76
    y = torch.randn(N, H * W, ld, device="cuda") * 3
    y[0, :50, :A] = 25.0   # a saturated tie group (sigmoid == 1.0f)
    for k in (12000, 6000, 100):
        sc, idx = ops.topk_sigmoid(y, A, k)
        ref_s, ref_i = torch.sigmoid(y[:, :, :A].reshape(N, -1)).topk(k, dim=1, sorted=True)
        assert torch.allclose(sc, ref_s, rtol=2e-7, atol=0)
        assert (sc[:, 1:] <= sc[:, :-1]).all()
        g = torch.sigmoid(y[:, :, :A].reshape(N, -1)).gather(1, idx)          # idx really points at those scores
        assert torch.allclose(g, sc, rtol=2e-7, atol=0)
        assert all(len(set(idx[i].tolist())) == k for i in range(N))           # no duplicates
        strict = ref_s[:, 1:] < ref_s[:, :-1]                                  # where the order is unambiguous it is identical
        same = (idx == ref_i)
        assert same[:, 1:-1][strict[:, :-1] & strict[:, 1:]].float().mean() > 0.999
    assert idx[0, :50].tolist() == sorted(idx[0, :50].tolist())               # tie group: ascending index


@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (1, 8, 8), (4, 150, 250)])
def test_bottleneck_tail_fused(B, H, W):
    """abr_conv_tail64_forward (conv3x3 64->64 + bn + relu + conv1x1 64->256 + bn + residual + relu in one launch, o2 kept on the compute unit)
    equals the two abr_conv_forward launches it replaces BIT FOR BIT (same products, same order), ragged last tile included; and both agree with
    float64 (resnet.py:327-346)."""
    from abr_iod_amd import ops
    torch.manual_seed(B * 1000 + H)
    ops.conv_cache_clear()      # the library caches packed planes per (weight ADDRESS, w_version): fresh tensors may reuse an address
    ver = 100000 + B * 1000 + H   # ... and every tensor of this test gets a version of its own
    o1 = torch.relu(torch.randn(B, H, W, 64, device="cuda"))
    w2 = torch.randn(64, 3, 3, 64, device="cuda") * 0.06
    w3 = torch.randn(256, 1, 1, 64, device="cuda") * 0.15
    s2, b2 = torch.rand(64, device="cuda") + 0.5, torch.randn(64, device="cuda") * 0.2
    s3, b3 = torch.rand(256, device="cuda") + 0.5, torch.randn(256, device="cuda") * 0.2
    idt = torch.randn(B, H, W, 256, device="cuda")
    o2 = ops.conv_forward(o1, w2, 1, 1, scale=s2, bias=b2, relu=True, math=ops.MATH_BF16X6, w_version=ver)
    want = ops.conv_forward(o2, w3, 1, 0, scale=s3, bias=b3, residual=idt, relu=True, math=ops.MATH_BF16X6, w_version=ver)
    assert ops.bottleneck_tail64_applies(o1, w2, w3, ops.MATH_BF16X6)
    got = ops.bottleneck_tail64(o1, w2, w3, s2, b2, s3, b3, idt, ver, ver)
    assert torch.equal(got, want)
    assert ops.x6_range_flags(reset=False) == 0
    if H <= 40:
        x64 = o1.double().permute(0, 3, 1, 2)
        r2 = torch.relu(torch.nn.functional.conv2d(x64, w2.double().permute(0, 3, 1, 2), padding=1) * s2.double().view(1, -1, 1, 1) + b2.double().view(1, -1, 1, 1))
        r3 = torch.relu(torch.nn.functional.conv2d(r2, w3.double().permute(0, 3, 1, 2)) * s3.double().view(1, -1, 1, 1) + b3.double().view(1, -1, 1, 1)
                        + idt.double().permute(0, 3, 1, 2))
        err = (got.double().permute(0, 3, 1, 2) - r3).abs().max().item()
        assert err < 2e-5 * r3.abs().max().item(), err


def test_topk_sigmoid_scratch_survives_changing_shapes():
    """The ranking's per-stream scratch (key array + level-1 histogram) is reused across calls: a SMALLER feature map after a larger one, and
    another batch size, on the same stream must not find stale bytes where the histogram expects zeros (ragged VOC batches, the 600x600 mosaic
    batches next to 600x1000 ones, variable-size inference).  Every call of the sequence is checked against torch."""
    from abr_iod_amd import ops
    torch.manual_seed(1)
    A, ld = 15, 76
    seq = [(4, 38 * 63, 12000), (4, 38 * 38, 6000), (2, 25 * 40, 2000), (4, 38 * 63, 12000), (1, 13 * 17, 300), (5, 38 * 38, 12000), (3, 50 * 84, 12000)]
    for N, hw, k in seq:
        y = torch.randn(N, hw, ld, device="cuda") * 4
        k = min(k, hw * A)
        sc, idx = ops.topk_sigmoid(y, A, k)
        s_all = torch.sigmoid(y[:, :, :A].reshape(N, -1))
        ref_s, _ = s_all.topk(k, dim=1, sorted=True)
        assert torch.allclose(sc, ref_s, rtol=2e-7, atol=0), (N, hw, k)
        assert int(idx.min()) >= 0 and int(idx.max()) < hw * A, (N, hw, k)
        assert torch.allclose(s_all.gather(1, idx), sc, rtol=2e-7, atol=0)
        assert all(len(set(idx[i].tolist())) == k for i in range(N))


def test_rpn_postprocessor_matches_reference_order(gold):
    """RPNPostProcessor (inference.py:76-147) on the fixed logits of tests/golden/rpn.npz, training and test mode: the proposals come out in the
    reference's ORDER (descending objectness, NMS survivors, first post_nms, GT appended in training) with the reference's boxes and scores."""
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator, RPNPostProcessor
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    g = gold("rpn")
    obj, reg = T(g["objectness"]), T(g["box_regression"])
    sizes = [tuple(int(v) for v in s) for s in g["image_sizes"]]
    ag = AnchorGenerator(sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(16,), straddle_thresh=0).cuda()
    anchors = ag(ImageList(torch.zeros(2, 3, 160, 224, device="cuda"), sizes), [torch.zeros(2, 8, 10, 14, device="cuda")])
    for i in (0, 1):
        assert np.array_equal(anchors[i][0].bbox.cpu().numpy(), g[f"anchors{i}"])
    targets = [BoxList(T(g["gt0"]), (224, 160)), BoxList(T(g["gt1"]), (200, 150))]
    for tag, (pre, post, train) in {"train": (600, 100, True), "test": (300, 50, False)}.items():
        pp = RPNPostProcessor(pre_nms_top_n=pre, post_nms_top_n=post, nms_thresh=0.7, min_size=0, box_coder=BoxCoder((1., 1., 1., 1.)))
        pp.train(train)
        res = pp(anchors, [obj], [reg], targets if train else None)
        for i, b in enumerate(res):
            wb, ws = g[f"{tag}_boxes{i}"], g[f"{tag}_scores{i}"]
            assert tuple(b.bbox.shape) == wb.shape, (tag, i, b.bbox.shape, wb.shape)
            np.testing.assert_allclose(b.get_field("objectness").cpu().numpy(), ws, rtol=3e-7, atol=0)    # same order: scores line up one by one
            np.testing.assert_allclose(b.bbox.cpu().numpy(), wb, rtol=1e-5, atol=2e-4)


def test_conv_split_k_equals_unsplit(tmp_path):
    """abr_conv_forward splits the K range of badly quantised tiles over several workgroups (partial sums + last-arrival reduce).
    Same inputs with the plan disabled (ABR_IGEMM_SPLIT=0, read once per process -> two child processes): equal up to fp32
    re-association, and bitwise reproducible run to run (checked inside the child)."""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    outs = []
    for mode in ("0", "1"):
        f = str(tmp_path / ("split%s.npz" % mode))
        env = dict(os.environ, ABR_IGEMM_SPLIT=mode)
        subprocess.run([sys.executable, os.path.join(root, "tools", "conv_split_check.py"), f], check=True, env=env, timeout=600)
        outs.append(np.load(f))
    for k in outs[0].files:
        a, b = outs[0][k], outs[1][k]
        assert a.shape == b.shape
        np.testing.assert_allclose(b, a, rtol=2e-5, atol=2e-5 * float(np.abs(a).max()))


@pytest.mark.parametrize("M,N,K,k", [(2304, 108, 2048, 1), (256, 80, 2048, 1), (300, 64, 576, 3), (1000, 84, 4096, 1)])
def test_conv_small_grid_split_k_hand_off_under_uneven_load(M, N, K, k):
    """Small grid + long K (the predictor FCs): every 64 x 64 tile is split along K over up to 16 workgroups whose partial sums meet in the
    last arrival (conv_igemm.hip, dispatch_igemm).  The hand-off is checked the way it fails: back-to-back launches with fresh data while
    another stream keeps part of the chip busy, EVERY output word against float64 and against a repeat of the same call (the round-5 bug --
    the ticket taken before the partial stores had drained -- showed as wrong sums in a few per cent of the words, run to run)."""
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(M + N)
    side = torch.cuda.Stream()
    big_a = torch.randn(4096, 4096, device="cuda", generator=g)
    Cin = K // (k * k)
    hw = int(round(M ** 0.5)) if k == 3 else 1
    rows = hw * hw if k == 3 else M
    for it in range(12):
        x = torch.randn((1, hw, hw, Cin) if k == 3 else (M, 1, 1, Cin), device="cuda", generator=g)
        w = torch.randn(N, k, k, Cin, device="cuda", generator=g) * 0.05
        b = torch.randn(N, device="cuda", generator=g)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(1 + it % 3):
                big_a @ big_a          # uneven load: some compute units are busy, some are not
        y1 = ops.conv_forward(x, w, 1, k // 2, bias=b)
        y2 = ops.conv_forward(x, w, 1, k // 2, bias=b)
        torch.cuda.synchronize()
        assert torch.equal(y1, y2)
        xn = x.permute(0, 3, 1, 2).double().cpu()
        wn = w.permute(0, 3, 1, 2).double().cpu()
        ref = torch.nn.functional.conv2d(xn, wn, b.double().cpu(), padding=k // 2).permute(0, 2, 3, 1).reshape(rows, N)
        bound = torch.nn.functional.conv2d(xn.abs(), wn.abs(), padding=k // 2).permute(0, 2, 3, 1).reshape(rows, N)
        err = ((y1.reshape(rows, N).double().cpu() - ref).abs() / bound).max().item()
        assert err <= 8 * 2.0 ** -24, (it, err * 2 ** 24)   # units of 2^-24 sum|x||w| (measured: <= 1.2)


@pytest.mark.parametrize("shape", [(2, 13, 18, 256, 128), (3, 4, 4, 512, 512), (1, 38, 63, 256, 256), (2, 8, 8, 1024, 160)])
def test_conv3x3_winograd_matches_torch(shape):
    """Wide stride-1 pad-1 3x3 convs take the Winograd F(4x4,3x3) path (conv_winograd.hip + 36 batched MFMA GEMMs).  Against
    torch's CPU conv in float64: error stays at fp32 re-association level (the bound is relative to the largest output)."""
    from abr_iod_amd import ops
    B, H, W, Cin, Cout = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, H, W, Cin, generator=g)
    w = torch.randn(Cout, 3, 3, Cin, generator=g) * 0.05
    sc = torch.rand(Cout, generator=g) + 0.5
    bi = torch.randn(Cout, generator=g)
    mk = torch.randn(B, H, W, Cout, generator=g)
    ref = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), padding=1)
    ref = ref * sc.double().view(1, -1, 1, 1) + bi.double().view(1, -1, 1, 1)
    ref = ref.permute(0, 2, 3, 1)
    y_plain = ops.conv_forward(x.cuda(), w.cuda(), 1, 1, scale=sc.cuda(), bias=bi.cuda()).cpu().double()
    y_relu = ops.conv_forward(x.cuda(), w.cuda(), 1, 1, scale=sc.cuda(), bias=bi.cuda(), relu=True).cpu().double()
    y_mask = ops.conv_forward(x.cuda(), w.cuda(), 1, 1, scale=sc.cuda(), bias=bi.cuda(), mask=mk.cuda()).cpu().double()
    tol = 5e-5 * float(ref.abs().max())   # F(4x4,3x3) in fp32: ~2e-5 at Cin = 1024 (direct implicit GEMM: ~2e-6); the path's bar is 1e-4
    assert float((y_plain - ref).abs().max()) <= tol, float((y_plain - ref).abs().max()) / float(ref.abs().max())
    assert float((y_relu - ref.clamp(min=0)).abs().max()) <= tol
    assert float((y_mask - torch.where(mk.double() > 0, ref, torch.zeros_like(ref))).abs().max()) <= tol
    # weight gradient through the Winograd domain (36 batched GEMMs over the tile axis + G^T dU G), accumulating into dw
    gy = torch.randn(B, H, W, Cout, generator=g)
    wd = w.double().permute(0, 3, 1, 2).clone().requires_grad_(True)
    yy = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wd, padding=1) * sc.double().view(1, -1, 1, 1)
    yy.backward(gy.permute(0, 3, 1, 2).double())
    ref_dw = wd.grad.permute(0, 2, 3, 1)
    dw0 = torch.randn(Cout, 3, 3, Cin, generator=g)
    dw = ops.conv_wgrad(x.cuda(), gy.cuda(), dw0.clone().cuda(), 1, 1, scale=sc.cuda()).cpu().double()
    err = float((dw - dw0.double() - ref_dw).abs().max()) / float(ref_dw.abs().max())
    assert err <= 5e-5, err


# ---------------------------------------------------------------------------------------------- bf16 math mode (BASELINE configs[4])
BF16_CASES = [
    # B, Cin, H, W, Cout, k, stride, pad
    (2, 64, 19, 23, 64, 1, 1, 0),       # one k-tile, BN=64 tiles
    (2, 64, 19, 23, 256, 3, 1, 1),      # 3x3 halo (direct: no Winograd in bf16 mode)
    (1, 256, 38, 63, 512, 1, 2, 0),     # stride-2 1x1
    (2, 128, 16, 16, 76, 1, 1, 0),      # Cout not a multiple of 32
    (4, 256, 38, 63, 256, 3, 1, 1),     # layer3 conv2 at full size, 128x128 tiles, ragged M
    (64, 512, 4, 4, 2048, 1, 1, 0),     # layer4 expand
]


def _bf16r(t):
    return t.bfloat16().float()   # round-to-nearest-even, what v_cvt_pk_bf16_f32 does


@pytest.mark.parametrize("case", BF16_CASES)
def test_conv_bf16_mode_equals_float64_conv_of_rounded_operands(case):
    """bf16 x bf16 products are exact in fp32, so the bf16 MFMA path must agree with a float64 convolution of the ROUNDED operands
    up to fp32 summation order -- and must differ from the unrounded result by a bf16-sized amount (the mode is really on)."""
    from abr_iod_amd import ops
    B, Cin, H, W, Cout, k, s, p = case
    torch.manual_seed(7 + Cin + Cout)
    x = torch.randn(B, Cin, H, W); w = torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    scale = torch.rand(Cout) + 0.5; bias = torch.randn(Cout) * 0.1
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    res = torch.randn(B, Cout, Ho, Wo)
    xg = x.permute(0, 2, 3, 1).contiguous().cuda(); wg = w.permute(0, 2, 3, 1).contiguous().cuda()
    got = ops.conv_forward(xg, wg, s, p, scale=scale.cuda(), bias=bias.cuda(), residual=res.permute(0, 2, 3, 1).contiguous().cuda(),
                           relu=True, math=ops.MATH_BF16).permute(0, 3, 1, 2).cpu().double()
    y64 = torch.nn.functional.conv2d(_bf16r(x).double(), _bf16r(w).double(), stride=s, padding=p)
    want = torch.relu(y64 * scale.double().view(1, -1, 1, 1) + bias.double().view(1, -1, 1, 1) + res.double())
    tol = 2e-5 * max(1.0, want.abs().max().item())
    assert (got - want).abs().max().item() < tol
    exact = torch.relu(torch.nn.functional.conv2d(x.double(), w.double(), stride=s, padding=p) * scale.double().view(1, -1, 1, 1)
                       + bias.double().view(1, -1, 1, 1) + res.double())
    rel = ((got - exact).norm() / exact.norm()).item()
    assert 1e-4 < rel < 2e-2, rel
    # default mode is untouched: exact fp32
    f32 = ops.conv_forward(xg, wg, s, p).permute(0, 3, 1, 2).cpu().double()
    plain = torch.nn.functional.conv2d(x.double(), w.double(), stride=s, padding=p)
    assert (f32 - plain).abs().max().item() < 1e-4 * max(1.0, plain.abs().max().item())


@pytest.mark.parametrize("case", BF16_CASES)
def test_conv_bf16_mode_backward(case):
    from abr_iod_amd import ops
    B, Cin, H, W, Cout, k, s, p = case
    torch.manual_seed(11 + Cin + Cout)
    x = torch.randn(B, Cin, H, W); w = torch.randn(Cout, Cin, k, k) / (Cin * k * k) ** 0.5
    scale = torch.rand(Cout) + 0.5
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    gy = torch.randn(B, Cout, Ho, Wo)
    xg = x.permute(0, 2, 3, 1).contiguous().cuda(); wg = w.permute(0, 2, 3, 1).contiguous().cuda()
    gyg = gy.permute(0, 2, 3, 1).contiguous().cuda(); sc = scale.cuda()
    # weight gradient: dW = scale * sum_m r(gy)^T r(im2col(x))
    dw = torch.zeros_like(wg)
    ops.conv_wgrad(xg, gyg, dw, s, p, scale=sc, math=ops.MATH_BF16)
    xr = _bf16r(x).double().requires_grad_(True); wr = _bf16r(w).double().requires_grad_(True)
    y = torch.nn.functional.conv2d(xr, wr, stride=s, padding=p)
    y.backward(_bf16r(gy).double())
    want = (wr.grad * scale.double().view(-1, 1, 1, 1)).permute(0, 2, 3, 1)
    assert (dw.cpu().double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())
    # input gradient = forward kernel on gy with the flipped, scale-folded weight copy (that copy is what gets rounded)
    wt = ops.conv_dgrad_weights(wg, sc)
    if s == 1:
        dx = ops.conv_forward(gyg, wt, 1, k - 1 - p, math=ops.MATH_BF16)
    else:
        dx = ops.conv_forward(gyg, wt, 1, 0, out_hw=(H, W), out_stride=(s, s), math=ops.MATH_BF16)
    # (a dgrad whose reduction width Cout is not a multiple of 64 has no bf16 k-tile and computes in exact fp32, like the stem)
    rnd = _bf16r if Cout % 64 == 0 else (lambda t: t)
    wsr = rnd(w * scale.view(-1, 1, 1, 1)).double()
    xr2 = x.double().requires_grad_(True)
    torch.nn.functional.conv2d(xr2, wsr, stride=s, padding=p).backward(rnd(gy).double())
    want = xr2.grad.permute(0, 2, 3, 1)
    assert (dx.cpu().double() - want).abs().max().item() < 2e-5 * max(1.0, want.abs().max().item())


# ---------------------------------------------------------------------------------------------- bf16x6: fp32-accurate on bf16 MFMA
@pytest.mark.parametrize("case", [c for c in CONV_CASES if c[1] % 32 == 0] + BF16_CASES[4:])
def test_conv_bf16x6_mode_is_fp32_accurate(case):
    """Exact three-way bf16 split of both operands, six cross products, fp32 accumulate: the result must meet the SAME criterion
    against float64 as the fp32 MFMA kernels (and does so with a smaller error), forward, input gradient and weight gradient."""
    from abr_iod_amd import ops
    B, Cin, H, W, Cout, k, s, p = case
    torch.manual_seed(23 + Cin + Cout + k)
    x = torch.randn(B, Cin, H, W, dtype=torch.float64, requires_grad=True)
    w = (torch.randn(Cout, Cin, k, k, dtype=torch.float64) / (Cin * k * k) ** 0.5).requires_grad_(True)
    scale = torch.rand(Cout) + 0.5
    y = torch.nn.functional.conv2d(x, w, stride=s, padding=p)
    gy = torch.randn_like(y)
    (y * scale.double().view(1, -1, 1, 1)).backward(gy)
    xg = x.detach().float().permute(0, 2, 3, 1).contiguous().cuda(); wg = w.detach().float().permute(0, 2, 3, 1).contiguous().cuda()
    gyg = gy.float().permute(0, 2, 3, 1).contiguous().cuda(); sc = scale.cuda()
    # the fp32 inputs ARE the operands: compare with float64 arithmetic on exactly those values
    x64 = xg.cpu().double().permute(0, 3, 1, 2); w64 = wg.cpu().double().permute(0, 3, 1, 2); gy64 = gyg.cpu().double().permute(0, 3, 1, 2)
    xr = x64.clone().requires_grad_(True); wr = w64.clone().requires_grad_(True)
    yr = torch.nn.functional.conv2d(xr, wr, stride=s, padding=p)
    (yr * scale.double().view(1, -1, 1, 1)).backward(gy64)

    def close(got, want, tol):
        return (got.cpu().double() - want).abs().max().item() < tol * max(1.0, want.abs().max().item())
    tol = 5e-5 if (k == 3 and Cin >= 128) else 1e-5   # Winograd-domain GEMMs carry the transforms' fp32 rounding, as in fp32 mode
    got = ops.conv_forward(xg, wg, s, p, math=ops.MATH_BF16X6).permute(0, 3, 1, 2)
    assert close(got, yr.detach(), tol)
    import os
    os.environ["ABR_IGEMM_FC_SPLIT"] = "0"   # the yardstick is the fp32 MFMA kernel's SEQUENTIAL chain over K (the split-K form it takes on
    try:                                      # small grids since round 5 has shorter chains and a smaller error than any sequential kernel)
        f32 = ops.conv_forward(xg, wg, s, p).permute(0, 3, 1, 2)
    finally:
        del os.environ["ABR_IGEMM_FC_SPLIT"]
    err6 = (got.cpu().double() - yr.detach()).norm().item(); err32 = (f32.cpu().double() - yr.detach()).norm().item()
    assert err6 < 1.5 * err32 + 1e-12, (err6, err32)     # never meaningfully worse than the fp32 MFMA chain
    dw = torch.zeros_like(wg)
    ops.conv_wgrad(xg, gyg, dw, s, p, scale=sc, math=ops.MATH_BF16X6)
    assert close(dw, wr.grad.permute(0, 2, 3, 1), tol * 2)
    wt = ops.conv_dgrad_weights(wg, sc)
    if s == 1:
        dx = ops.conv_forward(gyg, wt, 1, k - 1 - p, math=ops.MATH_BF16X6)
    else:
        dx = ops.conv_forward(gyg, wt, 1, 0, out_hw=(H, W), out_stride=(s, s), math=ops.MATH_BF16X6)
    assert close(dx, xr.grad.permute(0, 2, 3, 1), tol * 2)


@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3"])
def test_winograd_input_transform_is_shared_between_forward_and_wgrad(math):
    """abr_conv_desc::wino_v: the forward pass keeps its Winograd-domain input V and the weight gradient reads it instead of
    transforming x again -- same outputs as the self-contained calls (the gradient call must not even look at x)."""
    from abr_iod_amd import ops
    m = {"bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f32": ops.MATH_F32}[math]
    g = torch.Generator(device="cuda").manual_seed(3)
    for (B, H, W, Cin, Cout) in [(2, 38, 63, 256, 256), (96, 7, 7, 512, 512), (1, 21, 10, 128, 192)]:
        x = torch.randn(B, H, W, Cin, device="cuda", generator=g)
        w = torch.randn(Cout, 3, 3, Cin, device="cuda", generator=g) / (9 * Cin) ** 0.5
        gy = torch.randn(B, H, W, Cout, device="cuda", generator=g)
        sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
        v = ops.wino_v_alloc(x, w, 1, 1, m)
        assert v is not None and v.numel() == 36 * B * ((H + 3) // 4) * ((W + 3) // 4) * Cin
        y_keep = ops.conv_forward(x, w, 1, 1, scale=sc, relu=True, math=m, wino_v=v)
        assert torch.equal(y_keep, ops.conv_forward(x, w, 1, 1, scale=sc, relu=True, math=m))
        dw_ref = torch.zeros_like(w); dw = torch.zeros_like(w)
        ops.conv_wgrad(x, gy, dw_ref, 1, 1, scale=sc, math=m)
        ops.conv_wgrad(torch.full_like(x, float("nan")), gy, dw, 1, 1, scale=sc, math=m, wino_v=v)   # x is NOT read
        assert torch.isfinite(dw).all()
        assert (dw - dw_ref).abs().max().item() <= 1e-5 * max(1.0, dw_ref.abs().max().item())
    # not a Winograd conv (stride 2 / 1x1 / narrow): nothing to keep
    x = torch.randn(1, 16, 16, 64, device="cuda")
    assert ops.wino_v_alloc(x, torch.zeros(64, 3, 3, 64, device="cuda"), 1, 1, m) is None
    assert ops.wino_v_alloc(torch.randn(1, 16, 16, 256, device="cuda"), torch.zeros(256, 1, 1, 256, device="cuda"), 1, 0, m) is None
    assert ops.wino_v_alloc(torch.randn(1, 16, 16, 256, device="cuda"), torch.zeros(256, 3, 3, 256, device="cuda"), 1, 1, ops.MATH_BF16) is None
    if math == "bf16x6":
        # Cout % 32 != 0: the forward runs direct, so nothing is kept, and the weight gradient (still Winograd) transforms x itself -- a wino_v
        # handed to it anyway is not read.  Both meet the bf16x6 criterion against float64 (test_conv_bf16x6_mode_is_fp32_accurate).
        x = torch.randn(2, 21, 10, 128, device="cuda", generator=g)
        w = torch.randn(136, 3, 3, 128, device="cuda", generator=g) / (9 * 128) ** 0.5
        gy = torch.randn(2, 21, 10, 136, device="cuda", generator=g)
        sc = torch.rand(136, device="cuda", generator=g) + 0.5
        assert ops.wino_v_alloc(x, w, 1, 1, m) is None
        xr = x.cpu().double().permute(0, 3, 1, 2).requires_grad_(True); wr = w.cpu().double().permute(0, 3, 1, 2).requires_grad_(True)
        yr = torch.nn.functional.conv2d(xr, wr, padding=1)
        (yr * sc.cpu().double().view(1, -1, 1, 1)).backward(gy.cpu().double().permute(0, 3, 1, 2))
        y = ops.conv_forward(x, w, 1, 1, math=m).permute(0, 3, 1, 2).cpu().double()
        assert (y - yr.detach()).abs().max().item() < 5e-5 * max(1.0, yr.abs().max().item())
        dw = torch.zeros_like(w)
        ops.conv_wgrad(x, gy, dw, 1, 1, scale=sc, math=m, wino_v=torch.full((36 * 2 * 6 * 3 * 128,), float("nan"), device="cuda"))
        want = wr.grad.permute(0, 2, 3, 1)
        assert (dw.cpu().double() - want).abs().max().item() < 1e-4 * max(1.0, want.abs().max().item())


def _unpack_planes(planes, rows, K):
    """inverse of abr_conv_pack_weights (include/abr_iod_hip.h): uint8 buffer -> float64 [3, rows_padded, K] of the three bf16 planes"""
    nb, ks = (rows + 31) // 32, K // 16
    t = planes.view(torch.bfloat16).view(nb, ks, 3, 64, 8).double()      # chunk (nb, ks, plane): 64 lanes x 8 bf16
    lane = torch.arange(64, device=planes.device)
    out = torch.zeros(3, nb * 32, K, dtype=torch.float64, device=planes.device)
    for half in range(2):   # lane l: row nb*32 + (l & 31), k = ks*16 + (l >> 5)*8 ..
        sel = t[:, :, :, lane[half * 32:(half + 1) * 32], :]               # [nb, ks, 3, 32 rows, 8]
        out.view(3, nb, 32, ks, 16)[:, :, :, :, half * 8:half * 8 + 8] = sel.permute(2, 0, 3, 1, 4)
    return out


def test_bf16x6_packed_weight_planes_are_exact_and_give_identical_results():
    """abr_conv_pack_weights + the weights-direct bf16x6 kernel (conv_igemm_x6w_kernel): the fragment-packed planes add back to the fp32
    weights EXACTLY (rows zero-padded to 32), and feeding them straight into the matrix cores -- the caller's planes or the library's
    per-(w, w_version) cache -- gives results bit-identical to splitting the weight tile inside every workgroup, on all three tile
    instances, for ragged Cout, a narrow direct 3x3, a stride-2 1x1 and the dgrad form."""
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    for rows, K in [(76, 1024), (512, 256), (64, 576), (33, 48)]:
        w = torch.randn(rows, K, device="cuda", generator=g) * torch.logspace(-6, 3, K, device="cuda")
        pl = _unpack_planes(ops.pack_weights(w), rows, K)
        back = pl.sum(0)
        assert torch.equal(back[:rows], w.double()) and not bool(back[rows:].any())     # exact, not merely close; pad rows are zero
        assert torch.equal(pl[0][:rows].float(), w.bfloat16().float())                  # plane 0 = bf16(w), round to nearest even
    cases = [(64, 32, 32, 512, 256, 1, 1, 0),    # 128x128 tiles
             (2, 19, 23, 64, 64, 3, 1, 1),       # 128x64 tiles, narrow direct 3x3
             (2, 38, 63, 256, 76, 1, 1, 0),      # 64x64 tiles (K <= 256), Cout = 76: the last 32-row block is zero-padded
             (1, 38, 63, 128, 256, 1, 2, 0),     # stride-2 1x1
             (2, 38, 63, 1024, 76, 1, 1, 0),     # the fused RPN heads
             (4, 150, 250, 64, 256, 1, 1, 0)]    # layer1 expand at the benchmark's size (residual + ReLU epilogue)
    for ver, (B, H, W, Cin, Cout, k, s, p) in enumerate(cases):
        w = torch.randn(Cout, k, k, Cin, device="cuda", generator=g) / (Cin * k * k) ** 0.5
        x = torch.randn(B, H, W, Cin, device="cuda", generator=g)
        sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
        res = torch.randn(B, (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1, Cout, device="cuda", generator=g) if k == 1 and s == 1 else None
        kw = dict(scale=sc, relu=True, residual=res, math=ops.MATH_BF16X6)
        want = ops.conv_forward(x, w, s, p, **kw)                                                  # no planes, no version: packed into stream scratch per call
        got = ops.conv_forward(x, w, s, p, w_planes=ops.pack_weights(w), **kw)

        def same(a, b, M, N, K):
            return torch.equal(a, b)
        M_ = B * ((H + 2 * p - k) // s + 1) * ((W + 2 * p - k) // s + 1)
        assert same(got, want, M_, Cout, Cin * k * k)
        assert torch.equal(ops.conv_forward(x, w, s, p, w_version=100 + ver, **kw), got)          # library cache
        assert torch.equal(ops.conv_forward(x, w, s, p, w_version=100 + ver, **kw), got)          # ... hit
        if s == 1 and Cout % 32 == 0:
            wt = ops.conv_dgrad_weights(w, sc)
            gy = torch.randn(B, H, W, Cout, device="cuda", generator=g)
            a = ops.conv_forward(gy, wt, 1, k - 1 - p, math=ops.MATH_BF16X6)
            b = ops.conv_forward(gy, wt, 1, k - 1 - p, math=ops.MATH_BF16X6, w_planes=ops.pack_weights(wt))
            assert same(b, a, M_, Cin, Cout * k * k)
            assert torch.equal(b, ops.conv_forward(gy, wt, 1, k - 1 - p, math=ops.MATH_BF16X6, w_version=200 + ver))
    # an out-of-domain weight is caught when it is packed (the weights-direct kernel does not inspect weights again)
    assert ops.x6_range_flags() == 0
    w = torch.randn(64, 1, 1, 64, device="cuda", generator=g)
    w[3, 0, 0, 5] = 2.0 ** -120
    ops.pack_weights(w)
    assert ops.x6_range_flags() & ops.X6_FLAG_TINY


def test_winograd_weight_cache_follows_w_version():
    """abr_conv_desc::w_version: the Winograd-domain weights are derived once per (weight address, version) -- the second call with
    the same pair must not depend on the weight transform running again, a new version must pick up new weight values, and
    w_version = 0 never caches."""
    from abr_iod_amd import ops
    g = torch.Generator(device="cuda").manual_seed(11)
    x = torch.randn(2, 20, 24, 128, device="cuda", generator=g)
    w = torch.randn(128, 3, 3, 128, device="cuda", generator=g) / (9 * 128) ** 0.5
    ref = lambda ww: torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), ww.permute(0, 3, 1, 2).double(), padding=1).permute(0, 2, 3, 1)
    close = lambda y, r: (y.double() - r).abs().max().item() <= 5e-5 * r.abs().max().item()
    for math in (ops.MATH_F32, ops.MATH_BF16X6):
        w1 = w.clone()
        r1 = ref(w1)
        y_a = ops.conv_forward(x, w1, 1, 1, math=math, w_version=7)
        y_b = ops.conv_forward(x, w1, 1, 1, math=math, w_version=7)          # cache hit
        assert close(y_a, r1) and torch.equal(y_a, y_b)
        assert torch.equal(y_a, ops.conv_forward(x, w1, 1, 1, math=math))     # same arithmetic as the uncached path
        w1.mul_(-2.0)                                                         # in-place change of the weights ...
        y_c = ops.conv_forward(x, w1, 1, 1, math=math, w_version=9)          # ... announced by a new version
        assert close(y_c, ref(w1))
        y_d = ops.conv_forward(x, w1, 1, 1, math=math, w_version=0)          # and never cached with version 0
        assert torch.equal(y_c, y_d)


@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3"])
def test_wgrad_split_reduction_is_deterministic_and_accumulates(math):
    """Split-M weight gradients park their partial tiles and a second launch adds them in split order (conv_wgrad.hip::wgrad_reduce_kernel):
    the same call gives bit-identical results every time (the round-1 fp32 atomics did not), `dw +=` still accumulates over calls
    (a weight used twice per step), and the values agree with float64.  Shapes: few output tiles x many rows (the split path),
    direct and Winograd-domain, plus one with a single split (plain stores)."""
    from abr_iod_amd import ops
    m = {"bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f32": ops.MATH_F32}[math]
    g = torch.Generator(device="cuda").manual_seed(5)
    for (B, H, W, Cin, Cout, k, pad) in [(2, 38, 63, 256, 1024, 1, 0), (1, 75, 125, 512, 128, 1, 0), (2, 38, 63, 256, 256, 3, 1), (8, 4, 4, 2048, 512, 1, 0)]:
        x = torch.randn(B, H, W, Cin, device="cuda", generator=g)
        gy = torch.randn(B, H, W, Cout, device="cuda", generator=g)
        sc = torch.rand(Cout, device="cuda", generator=g) + 0.5
        runs = []
        for _ in range(3):
            dw = torch.zeros(Cout, k, k, Cin, device="cuda")
            ops.conv_wgrad(x, gy, dw, 1, pad, scale=sc, math=m)
            runs.append(dw)
        assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2]), "split-M reduction must not depend on arrival order"
        twice = runs[0].clone()
        ops.conv_wgrad(x, gy, twice, 1, pad, scale=sc, math=m)        # dw += : a second contribution lands on top of the first
        assert (twice - 2 * runs[0]).abs().max().item() <= 1e-6 * runs[0].abs().max().item()
        if k == 1:
            ref = torch.einsum("bhwo,bhwi->oi", gy.double(), x.double()) * sc.double()[:, None]
            got = runs[0].view(Cout, Cin).double()
        else:
            xp = torch.nn.functional.pad(x.double(), (0, 0, 1, 1, 1, 1))
            ref = torch.stack([torch.stack([torch.einsum("bhwo,bhwi->oi", gy.double(), xp[:, r:r + H, s:s + W]) for s in range(3)], 1) for r in range(3)], 1)
            ref = ref * sc.double()[:, None, None, None]
            got = runs[0].double()
            ref = ref.view_as(got)
        scale = float(ref.abs().max())
        assert float((got - ref).abs().max()) <= (5e-5 if k == 3 else 1e-5) * scale


def test_avgpool_backward_fused_with_the_relu_of_its_input():
    """ops.avgpool_backward(g, shape, relu_of=y): the pooling's backward and the backward of the ReLU that produced the pooled tensor in one pass"""
    from abr_iod_amd import ops
    torch.manual_seed(0)
    y = torch.relu(torch.randn(37, 4, 4, 64, device="cuda"))
    g = torch.randn(37, 64, device="cuda")
    want = ops.relu_backward(ops.avgpool_backward(g, tuple(y.shape)), y)
    got = ops.avgpool_backward(g, tuple(y.shape), relu_of=y)
    assert torch.equal(got, want)
    ref = (g.view(37, 1, 1, 64) / 16.0).expand(37, 4, 4, 64) * (y > 0)
    assert torch.equal(got, ref)


@pytest.mark.parametrize("math", ["f16x3", "bf16x6", "f32"])
def test_bottleneck_forward_table_equals_the_per_conv_calls(math, monkeypatch):
    """One abr_conv_run per bottleneck forward (resnet.py::_FwdPlan: the block's four abr_conv_op with everything constant filled in once) against
    the four conv_forward calls it replaces: same kernels, same arguments -> bit-identical outputs and an equally valid amax tag; with and without
    a downsample branch, stride 1 / 2, a second input shape, and after the weights moved (new version: the table is still valid, its planes are not)"""
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone import resnet as R
    m = {"f16x3": ops.MATH_F16X3, "bf16x6": ops.MATH_BF16X6, "f32": ops.MATH_F32}[math]
    torch.manual_seed(11)
    for cin, cb, cout, stride in ((256, 128, 512, 2), (512, 128, 512, 1), (64, 64, 256, 1)):
        blk = R.Bottleneck(cin, cb, cout, stride).cuda()
        blk.math = m
        for bn in (blk.bn1, blk.bn2, blk.bn3) + ((blk.downsample[1],) if blk.downsample is not None else ()):
            bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1); bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5); bn.invalidate()
        R.bump_param_version()
        with torch.no_grad():
            for shape in ((2, 20, 24, cin), (1, 9, 13, cin)):
                x = torch.randn(shape, device="cuda")
                monkeypatch.setattr(R, "BLOCK_PLANS", False)
                ref, _ = blk.fwd(x, False)
                monkeypatch.setattr(R, "BLOCK_PLANS", True)
                for rep in range(2):
                    got, saved = blk.fwd(x, False)
                    assert saved is None and torch.equal(got, ref), (math, cin, shape, rep)
                    assert (ops.amax_of(got)[0] is not None) == (m == ops.MATH_F16X3)
            if not (m == ops.MATH_BF16X6 and cb == 64):
                assert len(blk.__dict__.get("_fwd_plans", {})) == 2
            blk.conv2.weight.mul_(1.5)          # the weights move (as after an optimiser step): new version, same table
            R.bump_param_version()
            x = torch.randn(2, 20, 24, cin, device="cuda")
            monkeypatch.setattr(R, "BLOCK_PLANS", False)
            ref, _ = blk.fwd(x, False)
            monkeypatch.setattr(R, "BLOCK_PLANS", True)
            got, _ = blk.fwd(x, False)
            assert torch.equal(got, ref)
    assert ops.x6_range_flags(reset=True) == 0

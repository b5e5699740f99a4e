"""The trainable stem's kernels (FREEZE_CONV_BODY_AT = 0): the max-pool backward fused with the stem's ReLU mask, against torch-CPU autograd of
relu -> max_pool2d(3, 2, 1), and the 7x7 stride-2 weight gradient on the 4-channel padded image, against float64."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _data(kind, B, C, H, W, gen):
    if kind == "randn":
        return torch.randn(B, C, H, W, generator=gen)
    if kind == "tied":     # post-ReLU / quantised data: many equal maxima in one window
        return torch.randint(-1, 3, (B, C, H, W), generator=gen).float()
    if kind == "zero":     # windows that are all zero
        x = torch.randn(B, C, H, W, generator=gen)
        x[:, :, : H // 2] = 0.0
        return x
    if kind == "nan":      # a NaN wins its windows (torch: `val > max || isnan(val)`)
        x = torch.randn(B, C, H, W, generator=gen)
        x[0, 1, H // 2, W // 2] = float("nan")
        x[1, C - 1, 0, W - 1] = float("nan")
        return x
    raise ValueError(kind)


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=1234.5), torch.nan_to_num(b, nan=1234.5)) and torch.equal(a.isnan(), b.isnan())


CASES = [(C, H, W, kind) for C in (4, 64) for (H, W) in ((13, 17), (12, 16), (13, 16), (12, 17)) for kind in ("randn", "tied", "zero", "nan")]
# maps of one or two pixels a side: every window hangs over the border, and the quads of the last row / column are cut
CASES += [(C, H, W, kind) for C in (4, 64) for (H, W) in ((1, 1), (1, 2), (2, 1), (2, 2), (3, 3), (1, 7), (7, 1))
          for kind in ("randn", "tied", "zero", "nan")]


@pytest.mark.parametrize("case", CASES, ids=["C{}-{}x{}-{}".format(*c) for c in CASES])
def test_maxpool_relu_backward_vs_torch(case):
    from abr_iod_amd import ops
    C, H, W, kind = case
    gen = torch.Generator().manual_seed(hash(case) % 10007)
    x = _data(kind, 2, C, H, W, gen).requires_grad_(True)
    y = torch.relu(x)
    p = torch.nn.functional.max_pool2d(y, 3, 2, 1)
    g = torch.randn(p.shape, generator=gen)
    gx, = torch.autograd.grad(p, x, g)
    # per input element: how many windows route to it, and the sum of their |g| (both through torch's own routing)
    cnt, = torch.autograd.grad(torch.nn.functional.max_pool2d(torch.relu(x), 3, 2, 1), x, torch.ones_like(g))
    sabs, = torch.autograd.grad(torch.nn.functional.max_pool2d(torch.relu(x), 3, 2, 1), x, g.abs())

    yd = y.detach().permute(0, 2, 3, 1).contiguous().cuda()
    gd = g.permute(0, 2, 3, 1).contiguous().cuda()
    got = ops.maxpool3x3s2_backward(yd, gd)
    again = ops.maxpool3x3s2_backward(yd, gd)
    assert torch.equal(got, again), "two runs differ"
    got = got.permute(0, 3, 1, 2).cpu()
    assert not got.isnan().any() and not gx.isnan().any()
    one = cnt <= 1
    assert torch.equal(got[one], gx[one]), "an element with at most one routed window differs from torch"
    # several windows: the order of at most four fp32 additions may differ from torch's
    err = (got - gx).abs()
    assert bool((err <= 2.0 ** -22 * sabs).all()), float((err - 2.0 ** -22 * sabs).max())
    assert int(cnt.max()) <= 4


def test_maxpool_relu_backward_writes_every_element():
    from abr_iod_amd import ops
    torch.manual_seed(0)
    y = torch.relu(torch.randn(2, 9, 11, 8)).cuda()
    g = torch.randn(2, 5, 6, 8).cuda()
    ref = ops.maxpool3x3s2_backward(y, g)
    from abr_iod_amd._lib import lib, ptr, stream
    out = torch.full_like(y, float("nan"))   # a stale buffer: every element must be overwritten, zeros included
    assert lib().abr_maxpool3x3s2_backward(ptr(y), ptr(g), 2, 9, 11, 8, ptr(out), stream()) == 0
    assert torch.equal(out, ref)
    with pytest.raises(RuntimeError):
        ops.maxpool3x3s2_backward(y, g[:, :4])


def _stem_wgrad_case(B, H, W, seed):
    from abr_iod_amd import ops
    gen = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, H, W), generator=gen).float() - torch.tensor([102.9801, 115.9465, 122.7717]).view(1, 3, 1, 1)
    Ho, Wo = (H + 6 - 7) // 2 + 1, (W + 6 - 7) // 2 + 1
    gy = torch.randn(B, 64, Ho, Wo, generator=gen)
    gy[gy < 0] = 0.0                      # a ReLU-masked gradient, as the max-pool backward leaves it
    scale = (torch.rand(64, generator=gen) + 0.5) / 64
    xh = ops.nchw_to_nhwc(img.cuda(), cpad=4)
    dw = torch.zeros(64, 7, 7, 4, device="cuda")
    ops.conv_wgrad(xh, gy.permute(0, 2, 3, 1).contiguous().cuda(), dw, 2, 3, scale=scale.cuda(), math=ops.MATH_F32)
    want = torch.nn.grad.conv2d_weight(img.double(), (64, 3, 7, 7), gy.double() * scale.double().view(1, -1, 1, 1), stride=2, padding=3)
    got = dw.cpu()
    assert torch.all(got[..., 3] == 0), "the padded input channel's weight gradient must be exactly 0"
    err = float((got[..., :3].permute(0, 3, 1, 2).double() - want).abs().max())
    print("stem wgrad", (B, H, W), "max err", err, "output scale", float(want.abs().max()))
    assert err < 1e-4 * max(1.0, float(want.abs().max()))


def test_stem_weight_gradient_small():
    _stem_wgrad_case(2, 61, 83, 1)


def test_stem_weight_gradient_fullsize():
    _stem_wgrad_case(4, 600, 1000, 2)

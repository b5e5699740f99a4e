"""GPU: the pooling and layout kernels of csrc/elementwise.hip at their edges -- max_pool2d(3, 2, 1) on maps of 1 ... 5 pixels a side with
ties, -inf and NaN; the two NCHW -> NHWC routes and NHWC -> NCHW at channel counts, map sizes and paddings that are no multiple of the
32 x 32 tile; the average pool forward against float64 and its two backward forms bit for bit; ops.scale_; and one case just past every
launcher's grid cap, where some workgroup takes a second trip through its grid-stride loop."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
NAN = float("nan")


def _same(a, b):
    """bit-equal apart from NaN payloads, NaNs at the same places"""
    return torch.equal(torch.nan_to_num(a, nan=1234.5), torch.nan_to_num(b, nan=1234.5)) and torch.equal(a.isnan(), b.isnan())


def _abi():
    from abr_iod_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


# ------------------------------------------------------------------------------------------------------------------ max pool forward
def _pool_data(kind, B, C, H, W, gen):
    """NCHW"""
    if kind == "randn":
        return torch.randn(B, C, H, W, generator=gen)
    if kind == "tied":        # many equal maxima in one window
        return torch.randint(-1, 3, (B, C, H, W), generator=gen).float()
    if kind == "neginf":      # every window keeps its starting value
        return torch.full((B, C, H, W), float("-inf"))
    if kind == "halfinf":
        x = torch.randn(B, C, H, W, generator=gen)
        x[torch.rand(B, C, H, W, generator=gen) < 0.5] = float("-inf")
        return x
    if kind == "nan":         # a NaN wins every window it lies in: at two corners and in the middle
        x = torch.randn(B, C, H, W, generator=gen)
        x[0, 0, 0, 0] = NAN
        x[0, 1, H - 1, W - 1] = NAN
        x[1, C - 1, H // 2, W // 2] = NAN
        return x
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["randn", "tied", "neginf", "halfinf", "nan"])
@pytest.mark.parametrize("C", [4, 8, 64])
def test_maxpool_forward_tiny_maps_vs_torch(C, kind):
    from abr_iod_amd import ops
    L, ptr, stream = _abi()
    gen = torch.Generator().manual_seed(C * 7 + len(kind))
    B = 2
    for H in range(1, 6):
        for W in range(1, 6):
            x = _pool_data(kind, B, C, H, W, gen)
            want = F.max_pool2d(x, 3, 2, 1).permute(0, 2, 3, 1).contiguous()
            xd = x.permute(0, 2, 3, 1).contiguous().cuda()
            got = ops.maxpool3x3s2(xd)
            assert tuple(got.shape) == tuple(want.shape)
            assert _same(got.cpu(), want), (H, W)
            out = torch.full_like(got, NAN)      # a stale buffer: every element is overwritten
            if kind == "nan":
                out.fill_(7.0)
            assert L.abr_maxpool3x3s2(ptr(xd), B, H, W, C, ptr(out), stream()) == 0
            assert _same(out.cpu(), want), (H, W)


# ------------------------------------------------------------------------------------------------------------------ layout
MAPS = [(1, 1), (1, 31), (4, 8), (3, 11), (37, 45)]


def _to_nhwc_case(x, cpad):
    """both the ops entry and the C ABI into a NaN-prefilled buffer: exact against permute, the pad channels exactly 0"""
    from abr_iod_amd import ops
    L, ptr, stream = _abi()
    B, C, H, W = x.shape
    xd = x.cuda()
    want = x.permute(0, 2, 3, 1).contiguous()
    out = torch.full((B, H, W, cpad), NAN, device="cuda")
    assert L.abr_nchw_to_nhwc_pad(ptr(xd), B, C, H, W, cpad, ptr(out), stream()) == 0
    got = out.cpu()
    assert torch.equal(got[..., :C], want), (B, C, H, W, cpad)
    assert not got[..., C:].isnan().any() and torch.count_nonzero(got[..., C:]) == 0, (B, C, H, W, cpad)
    assert torch.equal(ops.nchw_to_nhwc(xd, cpad=cpad), out)
    return out


@pytest.mark.parametrize("C", [1, 5, 31, 32, 33, 65])
def test_nchw_to_nhwc_general_route(C):
    gen = torch.Generator().manual_seed(C)
    for H, W in MAPS:
        for B in (1, 3):
            x = torch.randn(B, C, H, W, generator=gen)
            for cpad in sorted({C, C + 1, (C + 31) // 32 * 32}):
                assert cpad != 4
                _to_nhwc_case(x, cpad)


@pytest.mark.parametrize("C", [1, 2, 3, 4])
def test_nchw_to_nhwc_four_wide_route(C):
    gen = torch.Generator().manual_seed(40 + C)
    for H, W in MAPS:
        for B in (1, 3):
            _to_nhwc_case(torch.randn(B, C, H, W, generator=gen), 4)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 31, 32, 33, 65])
def test_nhwc_to_nchw_and_round_trip(C):
    from abr_iod_amd import ops
    L, ptr, stream = _abi()
    gen = torch.Generator().manual_seed(80 + C)
    for H, W in MAPS:
        for B in (1, 3):
            y = torch.randn(B, H, W, C, generator=gen)
            yd = y.cuda()
            out = torch.full((B, C, H, W), NAN, device="cuda")
            assert L.abr_nhwc_to_nchw(ptr(yd), B, C, H, W, ptr(out), stream()) == 0
            assert torch.equal(out.cpu(), y.permute(0, 3, 1, 2).contiguous()), (B, C, H, W)
            assert torch.equal(ops.nhwc_to_nchw(yd), out)
            assert torch.equal(ops.nchw_to_nhwc(out), yd), "the round trip is exact"
            assert torch.equal(ops.nhwc_to_nchw(ops.nchw_to_nhwc(out)), out)


# ------------------------------------------------------------------------------------------------------------------ average pool
def _hw(HW):
    return {1: (1, 1), 49: (7, 7), 50: (5, 10)}[HW]


def _avgpool_forward_case(N, HW, C, seed):
    """|err| <= (HW + 2) 2^-24 mean|x|: HW - 1 sequential fp32 adds, one product and the rounded 1 / HW"""
    from abr_iod_amd import ops
    torch.manual_seed(seed)
    x = torch.randn(N, *_hw(HW), C, device="cuda") * (1 + 3 * torch.rand(1, 1, 1, C, device="cuda"))
    got = ops.avgpool_forward(x)
    assert tuple(got.shape) == (N, C)
    if N == 0:
        return 0.0
    L, ptr, stream = _abi()
    out = torch.full((N, C), NAN, device="cuda")     # a stale buffer: every element is overwritten
    assert L.abr_avgpool_forward(ptr(x), N, HW, C, ptr(out), stream()) == 0
    assert torch.equal(out, got)
    x64 = x.double().view(N, HW, C)
    err = (got.double() - x64.mean(1)).abs()
    bound = (HW + 2) * U * x64.abs().mean(1)
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print("avgpool_forward error/bound N={} HW={} C={}: {:.3f}".format(N, HW, C, ratio))
    assert torch.all(err <= bound)
    return ratio


@pytest.mark.parametrize("C", [4, 2048])
@pytest.mark.parametrize("HW", [1, 49, 50])
@pytest.mark.parametrize("N", [0, 1, 513])
def test_avgpool_forward_vs_float64(N, HW, C):
    _avgpool_forward_case(N, HW, C, seed=N + HW + C)


def _special_y(shape, gen):
    """a ReLU output with +0, -0, a denormal, NaN and -1 planted over its first quarter: the gate y > 0 gives 0, 0, pass, 0, 0"""
    y = torch.relu(torch.randn(shape, generator=gen))
    flat = y.view(-1)
    q = max(flat.numel() // 4, min(flat.numel(), 5))
    special = torch.tensor([0.0, -0.0, 1e-41, NAN, -1.0])
    flat[:q] = special[torch.arange(q) % 5]
    return y


def _avgpool_backward_case(N, HW, C, seed):
    """plain: g * fp32(1 / HW) broadcast over HW, bit for bit; masked (emit_amax=False): the same where y > 0, else 0.  Both through ops and
    through the C ABI into NaN-prefilled buffers."""
    from abr_iod_amd import ops
    L, ptr, stream = _abi()
    gen = torch.Generator().manual_seed(seed)
    shape = (N,) + _hw(HW) + (C,)
    g = torch.randn(N, C, generator=gen)
    inv = torch.tensor(np.float32(1.0) / np.float32(HW))
    want = (g * inv).view(N, 1, 1, C).expand(shape).contiguous()
    gd = g.cuda()
    got = ops.avgpool_backward(gd, shape)
    assert tuple(got.shape) == shape and torch.equal(got.cpu(), want)
    out = torch.full(shape, NAN, device="cuda")
    assert L.abr_avgpool_backward(ptr(gd), N, HW, C, ptr(out), stream()) == 0
    assert torch.equal(out.cpu(), want)
    # masked
    y = _special_y(shape, gen)
    want_m = torch.where(y > 0, want, torch.zeros_like(want))
    if N:
        assert float(want_m.view(-1)[2]) == float(want.view(-1)[2]) and not want_m.isnan().any()
    yd = y.cuda()
    got = ops.avgpool_backward(gd, shape, relu_of=yd, emit_amax=False)
    assert torch.equal(got.cpu(), want_m)
    out = torch.full(shape, NAN, device="cuda")
    assert L.abr_avgpool_relu_backward(ptr(gd), ptr(yd), N, HW, C, ptr(out), stream()) == 0
    assert torch.equal(out.cpu(), want_m)


@pytest.mark.parametrize("C", [4, 2048])
@pytest.mark.parametrize("HW", [1, 49, 50])
@pytest.mark.parametrize("N", [0, 1, 5])
def test_avgpool_backward_plain_and_masked_exact(N, HW, C):
    _avgpool_backward_case(N, HW, C, seed=N * 3 + HW + C)


# ------------------------------------------------------------------------------------------------------------------ ops.scale_
def _scale_case(n, s, s_dev, seed):
    from abr_iod_amd import ops
    torch.manual_seed(seed)
    x = torch.randn(n, device="cuda")
    k = np.float32(1.0 if s is None else s) * (np.float32(1.0) if s_dev is None else np.float32(s_dev))
    want = x.cpu() * torch.tensor(k)
    sd = None if s_dev is None else torch.tensor([s_dev], device="cuda")
    kw = {}
    if s is not None:
        kw["s"] = s
    if sd is not None:
        kw["s_dev"] = sd
    back = ops.scale_(x, **kw)
    assert back is x and torch.equal(x.cpu(), want), (n, s, s_dev)


@pytest.mark.parametrize("s,s_dev", [(0.3, None), (None, 1.7), (0.3, 1.7), (-3.0, 1e-3)])
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_scale_inplace_exact(n, s, s_dev):
    _scale_case(n, s, s_dev, seed=n)


def test_scale_of_none_is_none():
    from abr_iod_amd import ops
    assert ops.scale_(None) is None and ops.scale_(None, 2.0, None) is None


# ------------------------------------------------------------------------------------------------------------------ past the grid caps
def test_scale_past_its_grid_cap():
    """4096 workgroups of 256: one element more, and workgroup 0 takes a second trip"""
    _scale_case(4096 * 256 + 1, 0.3, 1.7, seed=1)


def test_nchw_to_nhwc4_past_its_grid_cap():
    """4096 workgroups of 256 pixels per image"""
    H, W = 1025, 1024
    assert H * W > 4096 * 256
    _to_nhwc_case(torch.randn(1, 3, H, W, generator=torch.Generator().manual_seed(2)), 4)


def test_avgpool_forward_past_its_grid_cap():
    N, HW, C = 4097, 1, 2048
    assert N * C // 4 > 8192 * 256
    _avgpool_forward_case(N, HW, C, seed=3)


def test_avgpool_backward_past_its_grid_cap():
    N, HW, C = 128, 49, 2048
    assert N * HW * C // 4 > 8192 * 256
    _avgpool_backward_case(N, HW, C, seed=4)


def test_maxpool_forward_and_backward_past_their_grid_cap():
    """1 x 1025 x 1025 x 64 against ATen's own max-pool on the device (the NHWC tensor is its channels-last input), with the assertions of
    the small cases: the forward bit-equal; the backward equal between two runs, exact where at most one window routes to an element, and
    within the reordering of at most four fp32 additions elsewhere"""
    from abr_iod_amd import ops
    B, H, W, C = 1, 1025, 1025, 64
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    assert B * Ho * Wo * C // 4 > 16384 * 256
    torch.manual_seed(5)
    x = torch.randn(B, H, W, C, device="cuda")
    x[0, 0, 0, 0] = NAN
    x[0, H - 1, W - 1, C - 1] = NAN
    got = ops.maxpool3x3s2(x)
    want = F.max_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1)
    assert tuple(got.shape) == (B, Ho, Wo, C) and _same(got, want.contiguous())
    L, ptr, stream = _abi()
    got.fill_(7.0)                                   # a stale buffer: every element is overwritten
    assert L.abr_maxpool3x3s2(ptr(x), B, H, W, C, ptr(got), stream()) == 0
    assert _same(got, want.contiguous())
    del got, want
    # backward through the ReLU that produced y
    xin = torch.randn(B, H, W, C, device="cuda").permute(0, 3, 1, 2).requires_grad_(True)
    pool = lambda: F.max_pool2d(torch.relu(xin), 3, 2, 1)
    g = torch.randn(B, C, Ho, Wo, device="cuda").contiguous(memory_format=torch.channels_last)
    gx, = torch.autograd.grad(pool(), xin, g)
    cnt, = torch.autograd.grad(pool(), xin, torch.ones_like(g))
    sabs, = torch.autograd.grad(pool(), xin, g.abs())
    y = torch.relu(xin.detach()).permute(0, 2, 3, 1).contiguous()
    gd = g.permute(0, 2, 3, 1).contiguous()
    got = torch.full_like(y, NAN)
    assert L.abr_maxpool3x3s2_backward(ptr(y), ptr(gd), B, H, W, C, ptr(got), stream()) == 0
    assert torch.equal(got, ops.maxpool3x3s2_backward(y, gd)), "two runs differ"
    got = got.permute(0, 3, 1, 2)
    assert not got.isnan().any() and not gx.isnan().any()
    one = cnt <= 1
    assert torch.equal(got[one], gx[one]), "an element with at most one routed window differs from torch"
    err = (got - gx).abs()
    assert bool((err <= 2.0 ** -22 * sabs).all()), float((err - 2.0 ** -22 * sabs).max())
    assert int(cnt.max()) <= 4

"""GPU: every amax word a kernel emits equals max |tensor|, bit for bit.

The f16x3 / f16 arithmetics scale each contraction operand by a power of two taken from the operand's amax word (csrc/common.h: 64 bits of
device memory, (epoch << 32) | bits of max |x|, written by the kernel that produced the tensor).  The other tests assert that a tag exists,
or that a consumer given the tag returns the same bits as one that lets the library reduce the tensor -- which only proves that the two amaxes
share a binade.  Here the VALUE of each word is read back (tests/amax_words.py) and compared with the integer maximum over the magnitudes of
the tensor the kernel stored: a producer that misses the lane, row or column holding the maximum, over-reports, skips the ragged last row
block or skips the scalar-store columns of a Cout % 4 != 0 conv fails.  Emitters: the fallback reduction (h3_amax_kernel), both conv
epilogues (conv_igemm.hip: the fp32 kernel and the split-operand kernel, vector and scalar store paths, split-K, scatter), the Winograd
output transform, avgpool_bwd_masked_kernel, deform_col2im_coord_kernel; and the words handed on as upper bounds (ops.amax_carry_bound)."""
import math

import pytest
import torch

from amax_words import abs_bits, as_float, expect, own_word, read_word

pytestmark = pytest.mark.gpu

U = 2.0 ** -24       # fp32 unit roundoff


def _ops():
    from abr_iod_amd import ops
    return ops, ops.L


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, device="cuda", generator=g)


# ------------------------------------------------------------------------------------------ the reduction and the emit protocol (abr_h3_amax)
CAP = 2048 * 256 * 4                   # floats one sweep of the capped grid covers: 2048 workgroups x 256 lanes x one float4
SIZES = [0, 1, 2, 3, 4, 5, 1023, 1024, 1025, CAP + 1024 + 3]     # the last: the smallest n past the cap with a scalar tail


def _reduce(x, addr, epoch, n=None):
    ops, L = _ops()
    L.check(L.lib().abr_h3_amax(L.ptr(x), x.numel() if n is None else n, addr, epoch, L.stream()), "h3_amax")


def _plant_positions(n):
    pos = {0, n - 1}                   # the first element; the last (in the scalar tail when n % 4 != 0)
    if n >= 4:
        pos.add(n // 4 * 4 - 1)        # the last element of the last full float4
    if n > CAP:
        pos.update((CAP - 1, CAP, CAP + 1))    # the end of the first sweep and the first float4 of the second
    return sorted(pos)


@pytest.mark.parametrize("n", SIZES)
def test_reduction_finds_a_planted_maximum_wherever_it_sits(n):
    keep, addr = own_word()
    g = _gen(n % 1000 + 1)
    if n == 0:
        _reduce(torch.empty(0, device="cuda"), addr, 9)
        assert read_word(addr) == (9, 0)                 # n = 0 leaves (epoch << 32) | 0
        return
    base = _randn(g, n)
    epoch = 1
    expect_plain = base.clone()
    _reduce(expect_plain, addr, epoch)
    expect(addr, epoch, expect_plain, "n=%d, N(0,1)" % n)
    for i, p in enumerate(_plant_positions(n)):
        x = base.clone()
        x[p] = -1e3 if i % 2 else 1e3
        epoch += 1
        _reduce(x, addr, epoch)
        assert read_word(addr) == (epoch, abs_bits(torch.tensor([1e3]))), (n, p, read_word(addr))
        expect(addr, epoch, x, "n=%d, planted at %d" % (n, p))


def _from_bits(bits):
    return torch.tensor(bits, dtype=torch.int64).to(torch.int32).view(torch.float32).cuda()


def test_reduction_orders_magnitudes_as_integers():
    """-0.0 -> 0; a denormal maximum keeps its bits; inf -> 0x7F800000; a NaN's payload sorts above inf"""
    keep, addr = own_word()
    g = _gen(3)
    x = torch.full((1031,), -0.0, device="cuda")
    assert abs_bits(x) == 0 and int(x.view(torch.int32)[0]) != 0
    _reduce(x, addr, 1)
    assert read_word(addr) == (1, 0)
    bits = [0] * 1031
    bits[5], bits[700], bits[1030] = 0x00000123, 0x80000456, 0x00000400      # denormals; the largest one is negative
    x = _from_bits(bits)
    _reduce(x, addr, 2)
    assert read_word(addr) == (2, 0x456)
    expect(addr, 2, x, "denormals")
    x = _randn(g, 1031)
    x[517] = float("-inf")
    _reduce(x, addr, 3)
    assert read_word(addr) == (3, 0x7F800000)
    x.view(torch.int32)[1029] = 0xFFC12345 - (1 << 32)  # a negative quiet NaN with a payload, written as bits
    assert int(x.view(torch.int32)[1029]) & 0x7FFFFFFF == 0x7FC12345
    _reduce(x, addr, 4)
    assert read_word(addr) == (4, 0x7FC12345)
    expect(addr, 4, x, "nan")


def test_emit_protocol_on_one_word():
    """one 64-bit unsigned max per workgroup: inside an epoch the value only grows, a later epoch replaces it, an earlier one never does"""
    keep, addr = own_word()
    g = _gen(4)
    x = _randn(g, 5000).clamp_(-2.5, 2.5)

    def run(epoch, peak, scale=1.0):
        t = x * scale
        t[1234] = peak
        _reduce(t, addr, epoch)
        return read_word(addr)

    b = lambda v: abs_bits(torch.tensor([v], dtype=torch.float32))
    assert run(5, 3.0) == (5, b(3.0))
    assert run(5, 2.75) == (5, b(3.0))                            # smaller data, same epoch: unchanged
    assert run(5, -7.5) == (5, b(7.5))                            # larger data: grows
    assert run(6, 2.0 ** -20, 2.0 ** -30) == (6, b(2.0 ** -20))   # a later epoch replaces whatever the word held
    assert run(4, 1e30) == (6, b(2.0 ** -20))                     # an earlier epoch never does
    assert run(0x80000001, 1.0, 0.25) == (0x80000001, b(1.0))     # the comparison is unsigned


# ----------------------------------------------------------------------------------------------------------------------- conv epilogues
def _maths():
    ops, _ = _ops()
    return {"f32": ops.MATH_F32, "bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f16": ops.MATH_F16}


ALL = ("f32", "bf16x6", "f16x3", "f16")


class Case(object):
    """one conv geometry: x [B,H,W,Cin], w [Cout,k,k,Cin]; scatter = the stride-2 1x1 dgrad form (rows land on every second pixel of a zeroed
    [B, 2 Ho, 2 Wo, Cout] tensor), second = its second pass, which adds into the first pass's tensor (residual = out = gx)"""

    def __init__(self, name, B, H, W, Cin, Cout, k=1, stride=1, pad=0, wino=False, scatter=False, second=False, maths=ALL, residual=True):
        self.name, self.B, self.H, self.W, self.Cin, self.Cout, self.k, self.stride, self.pad = name, B, H, W, Cin, Cout, k, stride, pad
        self.wino, self.scatter, self.second, self.maths = wino, scatter, second, maths
        self.residual = residual and not wino          # the Winograd route takes no residual
        self.Ho, self.Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
        self.M = B * self.Ho * self.Wo
        self.out_shape = (B, 2 * self.Ho, 2 * self.Wo, Cout) if scatter else (B, self.Ho, self.Wo, Cout)
        self.geom = dict(out_hw=(2 * self.Ho, 2 * self.Wo), out_stride=(2, 2)) if scatter else {}

    def index(self, row, col):
        """(row, column) of the GEMM -> index into the output tensor"""
        b, rem = divmod(row, self.Ho * self.Wo)
        ho, wo = divmod(rem, self.Wo)
        s = 2 if self.scatter else 1
        return (b, ho * s, wo * s, col)

    def takes_wino(self, mname):
        return self.wino and mname != "f16"            # the one-product fp16 mode stays direct (conv_route)


def _cases():
    cs = []
    # 1x1, Cin 64: ragged 32-row epilogue blocks x {full, ragged 32-column block on the vector path, Cout % 4 != 0: the scalar store path}
    for M in (1, 31, 32, 33, 129):
        for Cout in (64, 36, 66, 5):
            cs.append(Case("1x1 M%d Cout%d" % (M, Cout), M, 1, 1, 64, Cout))
    # small grid + long K: the fp32 kernel splits these along K (test_conv_small_grid_split_k_hand_off_under_uneven_load's shapes)
    for (M, N, K, k) in ((2304, 108, 2048, 1), (256, 80, 2048, 1), (300, 64, 576, 3), (1000, 84, 4096, 1)):
        if k == 3:
            hw = int(round(M ** 0.5))
            cs.append(Case("splitK %dx%dx%d k3" % (M, N, K), 1, hw, hw, K // 9, N, k=3, pad=1))
        else:
            cs.append(Case("splitK %dx%dx%d" % (M, N, K), M, 1, 1, K, N))
    # the Winograd forward shapes of test_conv3x3_winograd_matches_torch with H % 4 != 0 / W % 4 != 0 partial tiles
    for (B, H, W, Cin, Cout) in ((2, 13, 18, 256, 128), (3, 4, 4, 512, 512)):
        cs.append(Case("wino %dx%dx%d %d->%d" % (B, H, W, Cin, Cout), B, H, W, Cin, Cout, k=3, pad=1, wino=True))
    # the 7x7 stride-2 stem on 4 channels: the fp32 kernel (the split arithmetics have no 4-channel k-tile)
    cs.append(Case("stem 7x7 s2", 2, 30, 37, 4, 64, k=7, stride=2, pad=3, maths=("f32",)))
    # the strided scatter of a stride-2 1x1 conv's input gradient, fresh and as the second pass into the same tensor
    cs.append(Case("scatter fresh", 2, 6, 5, 256, 64, scatter=True, residual=False))
    cs.append(Case("scatter second pass", 2, 6, 5, 128, 64, scatter=True, second=True))
    return cs


CASES = _cases()
CONV_PARAMS = [(c, m) for c in CASES for m in c.maths]


def _positions(M, Cout):
    pos = [(0, 0), (M - 1, Cout - 1)]
    if M >= 32:
        pos.append((31, min(Cout - 1, 17)))              # the last row of the first full 32-row block
    if M % 32:
        pos.append((M // 32 * 32, Cout // 2))            # the first row of the ragged block
    pos.append((M // 2, (Cout - 1) // 4 * 4))            # a column in the last group of 4 (partial when Cout % 4 != 0)
    return sorted(set(pos))


class _Data(object):
    def __init__(self, c, seed):
        g = _gen(seed)
        self.x = _randn(g, c.B, c.H, c.W, c.Cin)
        self.w = _randn(g, c.Cout, c.k, c.k, c.Cin) / (c.k * c.k * c.Cin) ** 0.5
        self.scale = torch.rand(c.Cout, device="cuda", generator=g) + 0.5
        self.bias = _randn(g, c.Cout) * 0.1
        self.res = _randn(g, *c.out_shape)
        if c.second:    # the first pass's operands (another Cin, as conv1's and the downsample branch's gradients have)
            self.x1 = _randn(g, c.B, c.H, c.W, 256)
            self.w1 = _randn(g, c.Cout, 1, 1, 256) / 16


def _run_conv(c, d, mname, relu, use_res, mask=None, bias=None):
    """-> (out, word, epoch) of the conv with the epilogue asked for; the route is asked of the library first and must be the case's"""
    ops, _ = _ops()
    m = _maths()[mname]
    bias = d.bias if bias is None else bias
    use_res = use_res or c.second
    ptr = torch.zeros(4)         # stands for "a residual / mask is given" in the route query (the route looks at the pointer only)
    rm, fw, _, _ = ops.conv_route_info(d.x.shape, d.w.shape, c.stride, c.pad, d.scale, bias, ptr if use_res else None,
                                       ptr if mask is not None else None, relu, math=m, **c.geom)
    assert rm == m, "%s under %s runs in arithmetic %d" % (c.name, mname, rm)
    assert fw == c.takes_wino(mname), "%s under %s: drawn for %s, the library takes %s" % (
        c.name, mname, "Winograd" if c.takes_wino(mname) else "direct", "Winograd" if fw else "direct")
    kw = dict(scale=d.scale, bias=bias, mask=mask, relu=relu, math=m, emit_amax=True, **c.geom)
    if c.second:
        gx = ops.conv_forward(d.x1, d.w1, 1, 0, math=m, **c.geom)
        out = ops.conv_forward(d.x, d.w, c.stride, c.pad, residual=gx, out=gx, **kw)
        assert out is gx
    else:
        out = ops.conv_forward(d.x, d.w, c.stride, c.pad, residual=d.res if use_res else None, **kw)
    word, epoch = ops.amax_of(out)
    assert word is not None, "%s under %s: the output carries no amax tag" % (c.name, mname)
    assert tuple(out.shape) == c.out_shape
    return out, word, epoch


@pytest.mark.parametrize("c,mname", CONV_PARAMS, ids=["%s-%s" % (c.name.replace(" ", "_"), m) for c, m in CONV_PARAMS])
def test_conv_epilogue_word_equals_max_of_the_stored_tensor(c, mname):
    ops, _ = _ops()
    d = _Data(c, 100 + CASES.index(c))
    # dense: scale, bias, ReLU and a residual where the route takes one
    out, word, epoch = _run_conv(c, d, mname, relu=True, use_res=c.residual)
    assert abs_bits(out) != 0
    expect(word, epoch, out, "%s %s dense" % (c.name, mname))
    # single survivor: the epilogue mask is > 0 at exactly one (row, column): the word is that element's magnitude (no ReLU: the survivor
    # must not be clamped to zero) -- fails if any lane's contribution is dropped
    for (row, col) in _positions(c.M, c.Cout):
        idx = c.index(row, col)
        mask = torch.full(c.out_shape, -1.0, device="cuda")
        mask[idx] = 1.0
        out, word, epoch = _run_conv(c, d, mname, relu=False, use_res=c.residual, mask=mask)
        v = out[idx].item()
        assert v != 0.0, (c.name, mname, row, col)
        assert int((out != 0).sum()) == 1, (c.name, mname, row, col)
        got = read_word(word)
        assert got == (epoch, abs_bits(out[idx].reshape(1))), "%s %s survivor (%d, %d) = %r: word holds epoch %d, %r" % (
            c.name, mname, row, col, v, got[0], as_float(got[1]))
    # all zero: ReLU behind a large negative bias
    out, word, epoch = _run_conv(c, d, mname, relu=True, use_res=False, bias=torch.full((c.Cout,), -1e6, device="cuda"))
    # (the second pass of the scatter adds the first pass's values, far below 1e6, before the ReLU: zero as well)
    assert abs_bits(out) == 0 and read_word(word) == (epoch, 0), (c.name, mname, read_word(word))
    assert ops.x6_range_flags(reset=True) == 0


def test_conv_descriptor_takes_any_word():
    """abr_conv_desc.out_amax is any uint64_t*: a word the caller owns, at an epoch of the caller's choosing, through the C ABI"""
    import ctypes as C
    ops, L = _ops()
    g = _gen(7)
    x, w = _randn(g, 33, 1, 1, 64), _randn(g, 66, 1, 1, 64) / 8
    for m in (ops.MATH_F32, ops.MATH_F16X3):
        keep, addr = own_word()
        d = ops.conv_desc(x.shape, w.shape, 1, 0, math=m)
        if ops.uses_amax(m):
            d.x_amax, d.x_amax_epoch = ops.amax_of(ops.amax_compute(x))
        d.out_amax, d.out_amax_epoch = addr, 0x12345
        out = torch.empty(33, 1, 1, 66, device="cuda")
        L.check(L.lib().abr_conv_forward(C.byref(d), L.ptr(x), L.ptr(w), L.ptr(out), L.stream()), "conv_forward")
        expect(addr, 0x12345, out, "owned word, math %d" % m)
    assert ops.x6_range_flags(reset=True) == 0


# ------------------------------------------------------------------------------------------------------------ bottleneck forward table
@pytest.mark.parametrize("cin,cb,cout,stride", [(256, 128, 512, 2), (64, 64, 256, 1)])
def test_bottleneck_forward_table_tags_hold_the_maxima(cin, cb, cout, stride, monkeypatch):
    """resnet.py::_FwdPlan (one abr_conv_run per bottleneck forward) with save=True tags o1, o2 and the output with words the table's convs
    wrote: each holds its tensor's maximum"""
    ops, _ = _ops()
    from abr_iod_amd.modeling.backbone import resnet as R
    torch.manual_seed(13)
    blk = R.Bottleneck(cin, cb, cout, stride).cuda()
    blk.math = ops.MATH_F16X3
    for bn in (blk.bn1, blk.bn2, blk.bn3) + ((blk.downsample[1],) if blk.downsample is not None else ()):
        bn.weight.uniform_(0.5, 1.5); bn.bias.normal_(0, 0.1); bn.running_mean.normal_(0, 0.1); bn.running_var.uniform_(0.5, 1.5); bn.invalidate()
    R.bump_param_version()
    monkeypatch.setattr(R, "BLOCK_PLANS", True)
    with torch.no_grad():
        x = torch.randn(1, 9, 13, cin, device="cuda")
        out, saved = blk.fwd(x, True)
    plans = blk.__dict__.get("_fwd_plans", {})
    assert len(plans) == 1 and all(p.save for p in plans.values()), "the block did not run its forward table"
    _, t1, t2, out2, _, _ = saved
    assert out2 is out
    for name, t in (("o1", t1), ("o2", t2), ("out", out)):
        word, epoch = ops.amax_of(t)
        assert word is not None, name
        assert abs_bits(t) != 0
        expect(word, epoch, t, "bottleneck %d-%d-%d %s" % (cin, cb, cout, name))
    assert ops.x6_range_flags(reset=True) == 0


# ------------------------------------------------------------------------------------------------------ abr_avgpool_relu_backward_amax
def _avgpool(g, y, addr, epoch):
    ops, L = _ops()
    N, HW, C = y.shape
    gx = torch.empty_like(y)
    L.check(L.lib().abr_avgpool_relu_backward_amax(L.ptr(g), L.ptr(y), N, HW, C, L.ptr(gx), addr, epoch, L.stream()), "avgpool_relu_backward_amax")
    return gx


AVG_SHAPES = [(N, HW, C) for N in (1, 37) for HW in (1, 16, 49) for C in (4, 64, 2048)] + [(128, 49, 2048)]   # the last: 3.2 M float4 lanes,
#                                                                                                              past the 8192-workgroup cap


@pytest.mark.parametrize("N,HW,C", AVG_SHAPES)
def test_avgpool_relu_backward_word(N, HW, C):
    keep, addr = own_word()
    g = _gen(N * 1000 + HW * 10 + C % 7)
    gr, y = _randn(g, N, C), _randn(g, N, HW, C)
    gx = _avgpool(gr, y, addr, 3)
    assert abs_bits(gx) != 0
    expect(addr, 3, gx, "random")
    # the maximum in the last image's last pixel and channel, negative
    gr2, y2 = gr.clone(), y.clone()
    gr2[N - 1, C - 1], y2[N - 1, HW - 1, C - 1] = -1e3, 0.5
    gx = _avgpool(gr2, y2, addr, 4)
    want = torch.tensor(1e3, dtype=torch.float32) * (torch.tensor(1.0, dtype=torch.float32) / HW)       # g * (1.f / HW), as the kernel forms it
    assert gx[N - 1, HW - 1, C - 1].item() == -want.item()
    assert read_word(addr) == (4, abs_bits(want.reshape(1)))
    expect(addr, 4, gx, "planted in the last image")
    # a maximum the mask removes must not be reported: |g| = 1e6 in a channel whose y is 0 at every pixel of that image
    gr3, y3 = gr.clone(), y.clone()
    gr3[N // 2, C // 2], y3[N // 2, :, C // 2] = 1e6, 0.0
    gx = _avgpool(gr3, y3, addr, 5)
    assert float(gx.abs().max()) < 1e3
    expect(addr, 5, gx, "masked maximum")
    # y <= 0 everywhere: (epoch << 32)
    gx = _avgpool(gr, -y.abs(), addr, 6)
    assert abs_bits(gx) == 0 and read_word(addr) == (6, 0)


# ------------------------------------------------------------------------------------------------- abr_deform_col2im_coord's d_om word
DCN_FORMS = [(C, dg, False) for C in (64, 128, 256) for dg in (1, 2)] + [(C, 1, True) for C in (64, 128, 256)]
B_, H_, W_ = 1, 3, 5          # rows = 135: no multiple of the rows per workgroup (256 / C for C <= 256)


def _dcn_inputs(C, dg, modulated, seed):
    g = _gen(seed)
    com = 27 if modulated else 18 * dg
    Com = com + 5             # padded: the kernel writes the padding channels of d_om as 0 and never reads om's
    x = 5.0 + 0.01 * _randn(g, B_, H_, W_, C)       # nearly constant: the mask gradient (~ the sample's value) outweighs the offsets' (~ differences)
    om = torch.full((B_, H_, W_, Com), 1e3, device="cuda")
    om[..., :com] = (torch.rand(B_, H_, W_, com, device="cuda", generator=g) * 2 - 1) * 0.3
    dcol = _randn(g, B_, H_, W_, 9 * C)
    return x, om, dcol, com, Com


def _dcn(x, om, dcol, dg, modulated, addr, epoch):
    ops, L = _ops()
    B, H, W, C = x.shape
    dx, d_om = torch.zeros_like(x), torch.full_like(om, float("nan"))
    L.check(L.lib().abr_deform_col2im_coord(L.ptr(dcol), L.ptr(x), L.ptr(om), B, H, W, C, om.shape[3], dg, int(modulated), L.ptr(dx), L.ptr(d_om),
                                            addr, epoch, L.stream()), "deform_col2im_coord")
    return d_om


def _argmax(d_om):
    flat = int(d_om.abs().flatten().argmax())
    return flat // d_om.shape[3], flat % d_om.shape[3]       # (pixel, channel)


@pytest.mark.parametrize("C,dg,modulated", DCN_FORMS)
def test_deform_coord_gradient_word(C, dg, modulated):
    keep, addr = own_word()
    x, om, dcol, com, Com = _dcn_inputs(C, dg, modulated, C + dg + 7 * modulated)
    d_om = _dcn(x, om, dcol, dg, modulated, addr, 11)
    assert bool(torch.isfinite(d_om).all()) and abs_bits(d_om) != 0 and bool((d_om[..., com:] == 0).all())
    expect(addr, 11, d_om, "random")                         # over the whole padded tensor
    last = B_ * H_ * W_ - 1
    # the maximum in the last row (last pixel, tap 8): the tap's sample is pulled back inside the image
    om2, dc2 = om.clone(), dcol.clone()
    for gi in range(dg):
        om2[0, H_ - 1, W_ - 1, 16 + 18 * gi], om2[0, H_ - 1, W_ - 1, 17 + 18 * gi] = -0.5, -0.5
    x2 = x.clone()
    x2[0, H_ - 1, W_ - 1] = 50.0                             # a step at the corner: the offsets' gradient of this tap is large
    dc2.view(-1, 9 * C)[last, 8 * C + 1] = 1e4
    d_om = _dcn(x2, om2, dc2, dg, modulated, addr, 12)
    pix, ch = _argmax(d_om)
    assert pix == last and ch in ((16, 17, 26) if modulated else (16, 17)), (pix, ch)
    expect(addr, 12, d_om, "planted in the last row")
    if dg == 2:     # the maximum in the second deformable group's channels
        dc3 = dcol.clone()
        dc3.view(-1, 9 * C)[7, 4 * C + C // 2 + 3] = 1e6         # pixel 7, tap 4, a channel of the second group
        x3 = x + _randn(_gen(5), *x.shape)                   # (differences between neighbours of order 1: the offsets' gradient is not tiny)
        d_om = _dcn(x3, om, dc3, dg, modulated, addr, 13)
        pix, ch = _argmax(d_om)
        assert pix == 7 and ch in (18 + 8, 18 + 9), (pix, ch)
        expect(addr, 13, d_om, "planted in the second group")
    if modulated:   # the maximum in a mask-gradient channel (18 + k)
        dc4 = dcol.clone()
        dc4.view(-1, 9 * C)[6, 4 * C + 9] = 1e6                  # pixel 6, tap 4
        d_om = _dcn(x, om, dc4, dg, modulated, addr, 14)
        pix, ch = _argmax(d_om)
        assert pix == 6 and ch == 18 + 4, (pix, ch)
        expect(addr, 14, d_om, "planted in a mask-gradient channel")
    # every sample outside the image: (epoch << 32)
    om5 = om.clone()
    om5[..., :18 * dg] = 100.0
    d_om = _dcn(x, om5, dcol, dg, modulated, addr, 15)
    assert abs_bits(d_om) == 0 and read_word(addr) == (15, 0)


# ------------------------------------------------------------------------------------------------------ carried bounds (amax_carry_bound)
def _carried(dst, src, what):
    """dst carries src's (word, epoch); -> (bits of the word, max |dst| bits)"""
    ops, _ = _ops()
    tag = ops.amax_of(src)
    assert tag[0] is not None and ops.amax_of(dst) == tag, what
    epoch, bits = read_word(tag[0])
    assert epoch == tag[1] and bits == abs_bits(src), what
    return bits, abs_bits(dst)


def _safe_for_h3_scales(bits, dst):
    """the hard condition of abr::h3_scales, restated: with E = floor(log2(amax)) the operands are divided by s = 2^(E - 14), and
    max |dst| / s must stay inside fp16: max |dst| <= 65504 * 2^(E - 14)"""
    E = math.floor(math.log2(as_float(bits)))
    assert float(dst.abs().max()) <= 65504.0 * 2.0 ** (E - 14)


def test_exact_copies_and_subsets_carry_their_sources_word():
    ops, _ = _ops()
    g = _gen(21)
    # max-pool: every pooled value is one of x's
    x = _randn(g, 2, 33, 41, 64)
    x[1, 32, 40, 63] = -1e3               # the maximum is negative and in the last window: never selected, the bound still holds
    ops.amax_compute(x)
    p = ops.maxpool3x3s2(x)
    bits, got = _carried(p, x, "maxpool")
    assert got <= bits and got != 0
    xr = torch.relu(_randn(g, 2, 33, 41, 64))
    ops.amax_compute(xr)
    bits, got = _carried(ops.maxpool3x3s2(xr), xr, "maxpool of a ReLU's output")
    assert got == bits                    # (every pixel lies in some window: equal for a non-negative tensor)
    # relu_backward, not in place: a masked copy
    gr, y = _randn(g, 3, 17, 19, 36), _randn(g, 3, 17, 19, 36)
    ops.amax_compute(gr)
    out = ops.relu_backward(gr, y)
    bits, got = _carried(out, gr, "relu_backward")
    assert got <= bits and got != 0 and out.data_ptr() != gr.data_ptr()
    # the mask head's row gather (mask_head.py, _GatherRowsFn): rows of the head output, zeros for the -1 padding
    from abr_iod_amd.layers._layout import as_nhwc, from_nhwc
    from abr_iod_amd.modeling.roi_heads.mask_head.mask_head import _GatherRowsFn
    feat = _randn(g, 12, 4, 4, 32)
    feat[11, 3, 3, 31] = 77.0             # the maximum sits in a row the gather does not take
    ops.amax_compute(feat)
    rows = torch.tensor([3, -1, 0, 7, 7, -1, 10], dtype=torch.int64, device="cuda")
    picked = _GatherRowsFn.apply(from_nhwc(feat), rows, rows)
    ph = as_nhwc(picked)
    bits, got = _carried(ph, feat, "mask head row gather")
    assert got <= bits and got != 0 and got == abs_bits(feat[[3, 0, 7, 10]])
    # the box head's detection-row subset of the joint output (box_head.py, forward_joint: x_det = x[:kd] under the joint output's word)
    xj = ops.conv_forward(_randn(g, 9, 4, 4, 64), _randn(g, 96, 1, 1, 64) / 8, 1, 0, relu=True, math=ops.MATH_F16X3)
    assert ops.amax_of(xj)[0] is not None
    x_det = xj[:5]
    ops.amax_carry_bound(x_det, xj)
    bits, got = _carried(x_det, xj, "detection rows of the joint head output")
    assert got <= bits and got != 0
    assert ops.x6_range_flags(reset=True) == 0


def _plateau(g, H, W, C, lo, hi, peak):
    """a feature map that is constant at its maximum over [lo, hi) x [lo, hi) (every second channel negative), small noise elsewhere"""
    f = 0.1 * _randn(g, 1, H, W, C)
    sign = torch.ones(C, device="cuda")
    sign[1::2] = -1.0
    f[0, lo:hi, lo:hi, :] = peak * sign
    return f


def test_deform_im2col_stays_below_its_sources_word_up_to_rounding():
    """cols = m * (bilinear sample of x) under x's word.  Rounding, from the kernel's own order (deform.hip): lh = h - floor(h) is exact,
    hh = fl(1 - lh) errs by at most u/2 absolutely (u = 2^-24), so hh + lh <= 1 + u/2 and likewise hw + lw; the four product weights are
    rounded once each: their sum is at most (1 + u/2)^2 (1 + u); the first tap is fl(w x) and the three others are fused multiply-adds, one
    rounding each, on partial sums that never exceed the final one in magnitude for a constant x: (1 + u)^4; the modulation m = 1 / (1 + e)
    <= 1 adds one rounding.  In all (1 + u/2)^2 (1 + u)^6 < 1 + 8 u: max |cols| <= amax (1 + 8 * 2^-24)."""
    ops, _ = _ops()
    g = _gen(31)
    C, H, W = 64, 12, 12
    peak = 1.9999999                       # (just below a power of two: the mantissa is nearly all ones, roundings go up)
    x = _plateau(g, H, W, C, 2, 10, peak)
    ops.amax_compute(x)
    for modulated in (False, True):
        com = 27 if modulated else 18
        om = (torch.rand(1, H, W, com, device="cuda", generator=g) * 2 - 1) * 0.9
        om[0, :, ::2, :18] = 0.5           # half-integer offsets: every weight is 1/4, the sample of the plateau is the plateau
        if modulated:
            om[..., 18:] = 30.0            # sigmoid = 1 in fp32
        cols = ops.deform_im2col(x, om, 1, modulated)
        bits, got = _carried(cols, x, "deform_im2col")
        amax, top = float(as_float(bits)), float(cols.abs().max())
        assert amax == float(torch.tensor(peak, dtype=torch.float32))
        assert top >= amax * (1 - 8 * U)   # the inputs hit the edge
        assert top <= amax * (1 + 8 * U), (top, amax, (top / amax - 1) / U)
        _safe_for_h3_scales(bits, cols)


def test_roi_align_pooled_tensors_stay_below_the_feature_maps_word_up_to_rounding():
    """RoIAlign at sampling ratio 2, as the box (and with it the C4 mask) head and the keypoint head configure it, under the feature map's word.
    Rounding, from the kernel's own order (roi_align.hip, no contraction): per sample the weights sum to at most (1 + u/2)^2 (1 + u) as for
    deform_im2col; the four products and the three additions are rounded once each: (1 + u)^4; the four samples of a bin are accumulated
    with three more roundings and divided by the count with one: (1 + u)^4 again.  In all (1 + u/2)^2 (1 + u)^9 < 1 + 11 u, inside the
    1 + 16 * 2^-24 this test holds the kernel to: max |pooled| <= amax (1 + 16 * 2^-24)."""
    ops, _ = _ops()
    from abr_iod_amd.layers._layout import as_nhwc, from_nhwc
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import _JointPoolFn
    g = _gen(41)
    C, H, W, scale = 16, 40, 40, 1.0 / 16
    peak = 1.9999999
    fh = _plateau(g, H, W, C, 4, 36, peak)
    ops.amax_compute(fh)

    def rois(rows):
        return torch.tensor([[0.0] + [v * 16.0 for v in r] for r in rows], dtype=torch.float32, device="cuda")

    # inside the plateau: bins of 2 pixels whose samples fall on half-integer coordinates (weights of exactly 1/4), of 2.3 pixels at
    # fractional coordinates (rounded weights), bins smaller than a pixel; and boxes across the plateau's edge and the map's
    inside = [[6.0, 6.0, 20.0, 20.0], [6.3, 7.7, 22.4, 23.8], [10.1, 9.9, 13.6, 13.4], [5.5, 5.5, 33.5, 33.5]]
    across = [[0.0, 0.0, 39.0, 39.0], [30.2, 1.1, 44.0, 12.7], [-3.0, 20.0, 9.0, 31.0]]
    det, soft = rois(inside + across), rois(inside[:2] + across[:1])
    joint, pooled_soft = _JointPoolFn.apply(from_nhwc(fh), det, soft, 7, scale, 2)
    kp = ops.roi_align_forward(fh, det, scale, 14, 14, 2)          # the keypoint head's form (keypoint_head.py, _run)
    ops.amax_carry_bound(kp, fh)
    for name, t in (("joint (even bins)", as_nhwc(joint)), ("soft (all bins)", as_nhwc(pooled_soft)), ("keypoint pooler", kp)):
        bits, got = _carried(t, fh, name)
        amax, top = float(as_float(bits)), float(t.abs().max())
        assert top >= amax * (1 - 16 * U), name       # the inputs hit the edge
        assert top <= amax * (1 + 16 * U), (name, top, amax, (top / amax - 1) / U)
        _safe_for_h3_scales(bits, t)

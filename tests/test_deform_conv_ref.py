"""CPU: the float64 restatement of the general deformable convolution (tests/deform_conv_ref.py) is what it claims to be, before the GPU
suite (tests/test_gpu_deform_conv.py) measures the kernels against it:
  * zero offsets give torch's conv2d (half of it under a mask of 0.5), integer offsets the correspondingly shifted taps;
  * its autograd gradients are the central differences of the function; the written-out coordinate terms equal them;
  * the dyadic family evaluates to the same coordinates in fp32 and float64 and sits on the accept boundary;
  * an honest float32 restatement (sequential and pairwise sums) meets the GPU suite's bounds on the same inputs with a margin of at least 4;
  * at most 1 % of a random case's samples lie within 1e-4 of an integer coordinate.
And what needs no GPU of the feature itself: the C ABI's argument checks, output-size inference, the assertion and error texts, state_dict
keys and shapes and __repr__ of the three layer classes."""
import pytest
import torch
import torch.nn.functional as F

import deform_conv_ref as R
from abr_iod_amd.layers import dcn  # noqa: F401  (the feature this restatement is for: without it the module does not collect)

IDS = [c.id for c in R.CASES]


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _conv64(d, c, x=None):
    x = d["x"].double() if x is None else x
    y = F.conv2d(_nchw(x), _nchw(d["w"].double()), stride=c.stride, padding=c.padding, dilation=c.dilation, groups=c.groups)
    return y.permute(0, 2, 3, 1)


# ----------------------------------------------------------------------------------------------------------------- what the restatement is
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_zero_offsets_give_conv2d(c):
    d = R.make_inputs(c, "small", True)
    off = torch.zeros_like(d["offset"]).double()
    want = _conv64(d, c)
    got = R.deform_conv_ref(d["x"].double(), off, None, d["w"].double(), None, **R.geom(c))
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    half = R.deform_conv_ref(d["x"].double(), off, torch.full_like(d["mask"], 0.5).double(), d["w"].double(), d["bias"].double(), **R.geom(c))
    assert float((half - (0.5 * want + d["bias"].double())).abs().max()) <= 1e-12 * float(want.abs().max() + 1)


@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_integer_offsets_give_the_shifted_taps(c):
    d = R.make_inputs(c, "small", False)
    gen = torch.Generator().manual_seed(5)
    off = torch.randint(-3, 4, d["offset"].shape, generator=gen).double()
    Ho, Wo = R.out_size(c)
    K, gs, M = c.kernel[0] * c.kernel[1], c.C // c.dg, 16
    xp = F.pad(d["x"].double(), (0, 0, M, M, M, M))
    h, w = R.sample_points(off, c, torch.float64)                       # [B,Ho,Wo,dg,K], integers
    h, w = h.long().repeat_interleave(gs, 3), w.long().repeat_interleave(gs, 3)      # [B,Ho,Wo,C,K]
    bi = torch.arange(c.B).view(c.B, 1, 1, 1, 1)
    ci = torch.arange(c.C).view(1, 1, 1, c.C, 1)
    taps = xp[bi, h + M, w + M, ci].permute(0, 1, 2, 4, 3)              # [B,Ho,Wo,K,C]
    got = R.deform_cols_general_ref(d["x"].double(), off, None, **R.geom(c))
    assert torch.equal(got, R.to_cols(taps, c.groups))


def _smooth_case():
    """case g with every fractional part in [0.2, 0.8], the last tap row and column moved one pixel back: no sample within 1e-3 of a
    bilinear kink, none outside the box (the border taps still have corners outside the image)"""
    c = R.CASE["g_dg2"]
    d = R.make_inputs(c, "small", True)
    gen = torch.Generator().manual_seed(11)
    Ho, Wo = R.out_size(c)
    off = (torch.rand(c.B, Ho, Wo, c.dg, 9, 2, generator=gen) * 0.6 + 0.2).double()
    off[..., 6:, 0] -= 1        # taps with i = 2
    off[..., 2::3, 1] -= 1      # taps with j = 2
    d["offset"] = off.view(c.B, Ho, Wo, c.dg * 18)
    h, w = R.sample_points(d["offset"], c, torch.float64)
    assert bool(((h > -1) & (h < c.H) & (w > -1) & (w < c.W)).all())
    for t in (h, w):
        fr = t - torch.floor(t)
        assert bool(((fr > 1e-3) & (fr < 1 - 1e-3)).all())
    return c, d


def test_autograd_is_the_central_difference():
    c, d = _smooth_case()
    ops = [d["x"].double(), d["offset"].double(), d["mask"].double()]
    gy = d["gy"].double()

    def loss(x, off, m):
        cols = R.deform_cols_general_ref(x, off, m, exact_point=True, **R.geom(c))
        return (R.contract(cols, d["w"].double(), d["bias"].double()).view(gy.shape) * gy).sum()

    leaves = [t.clone().requires_grad_(True) for t in ops]
    grads = torch.autograd.grad(loss(*leaves), leaves)
    # the fp32-point form (what the GPU suite uses) has the same gradients: its offsets here are exact in neither, so compare at fp32 inputs
    gen = torch.Generator().manual_seed(3)
    for name, i in (("x", 0), ("offset", 1), ("mask", 2)):
        worst, h = 0.0, 1e-6
        for _ in range(40):
            at = tuple(int(torch.randint(0, s, (1,), generator=gen)) for s in ops[i].shape)
            p, m = [t.clone() for t in ops], [t.clone() for t in ops]
            p[i][at] += h
            m[i][at] -= h
            fd = float(loss(*p) - loss(*m)) / (2 * h)
            worst = max(worst, abs(fd - float(grads[i][at])) / max(1.0, abs(fd)))
        print(f"FD {name}: worst relative difference {worst:.3e}")
        assert worst < 1e-6, (name, worst)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_written_out_coordinate_terms_are_the_autograd_gradients(c, family, masked):
    d = R.make_inputs(c, family, masked)
    r = R.kernel_bounds(d, c)
    d_off, d_m = R.coord_terms(d["dcol"].double(), d["x"].double(), d["offset"].double(), None if not masked else d["mask"].double(), **R.geom(c))
    assert R.worst_ratio(d_off, r["d_offset"], r["d_offset_tol"]) <= 1e-6
    if masked:
        assert R.worst_ratio(d_m, r["d_mask"], r["d_mask_tol"]) <= 1e-6
    else:
        assert d_m is None and r["d_mask"] is None


def test_dyadic_family_is_the_same_in_float32_and_float64():
    samples = low = high = last = 0
    for c in R.CASES:
        d = R.make_inputs(c, "dyadic", False)
        a = R.sample_points(d["offset"], c, torch.float64)
        b = R.sample_points(d["offset"], c, torch.float32)
        assert torch.equal(a[0], b[0].double()) and torch.equal(a[1], b[1].double()), c.id
        samples += a[0].numel()
        low += int((a[0] == -1).sum())
        high += int((a[0] == c.H).sum())
        last += int((a[0] == c.H - 1).sum())
        cols = R.deform_cols_general_ref(d["x"].double(), d["offset"].double(), None, **R.geom(c))
        Ho, Wo = R.out_size(c)
        t = R.from_cols(cols, c.B, Ho, Wo, c.kernel[0] * c.kernel[1])                       # [B,Ho,Wo,K,C]
        rejected = ((a[0] == -1) | (a[0] == c.H)).permute(0, 1, 2, 4, 3).repeat_interleave(c.C // c.dg, -1)
        assert torch.count_nonzero(t[rejected]) == 0, c.id
    print(f"DYADIC {samples} samples, 0 differences, {low} at h = -1, {high} at h = H (rejected), {last} at h = H - 1 (accepted)")
    assert low > 0 and high > 0 and last > 0


@pytest.mark.parametrize("family", ["small", "wide"])
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_near_share_of_random_cases(c, family):
    near, outside = R.near_share(R.make_inputs(c, family, False), c, 1e-4)
    print(f"NEAR {c.id} {family}: {100 * near:.3f} % within 1e-4 of an integer, {100 * outside:.1f} % outside the box")
    assert near <= 0.01
    if family == "wide" and c.H >= 7:
        assert 0.2 <= outside <= 0.5


# --------------------------------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("c", R.CASES, ids=IDS)
def test_honest_float32_meets_the_bounds_with_margin(c, family, masked):
    d = R.make_inputs(c, family, masked)
    r = R.kernel_bounds(d, c)
    m = d["mask"]
    for order in ("seq", "pair"):
        cols = R.deform_cols_general_ref(d["x"], d["offset"], m, dtype=torch.float32, order=order, **R.geom(c))
        d_off, d_m = R.coord_terms(d["dcol"], d["x"], d["offset"], m, dtype=torch.float32, order=order, **R.geom(c))
        ratios = {"cols": R.worst_ratio(cols, r["cols"], r["cols_tol"]), "d_offset": R.worst_ratio(d_off, r["d_offset"], r["d_offset_tol"])}
        if masked:
            ratios["d_mask"] = R.worst_ratio(d_m, r["d_mask"], r["d_mask_tol"])
        print(f"RATIO f32 {order} {c.id} {family} mask={int(masked)}: " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) + " of the bound")
        assert max(ratios.values()) <= 0.25, ratios
        assert torch.all(cols[r["cols_tol"] <= 1e-38] == 0)


# ------------------------------------------------------------------------------------------------------------- the feature, without a GPU
def _abi(fn, B=2, H=7, W=9, C=8, Ho=7, Wo=9, kh=3, kw=3, sh=1, sw=1, ph=1, pw=1, dlh=1, dlw=1, groups=1, dg=1):
    from abr_iod_amd import _lib
    L = _lib.lib()
    ints = (B, H, W, C, Ho, Wo, kh, kw, sh, sw, ph, pw, dlh, dlw, groups, dg)
    if fn == "abr_deform_im2col_general":
        rc = L.abr_deform_im2col_general(None, None, None, *ints, None, None)
    else:
        rc = L.abr_deform_col2im_coord_general(None, None, None, None, *ints, None, None, None, None)
    return rc, L.abr_last_error().decode()


@pytest.mark.parametrize("fn", ["abr_deform_im2col_general", "abr_deform_col2im_coord_general"])
def test_abi_argument_checks_name_the_argument(fn):
    """every refusal returns before any launch: the pointers are all null, and the last check -- reached only by a valid geometry -- says so"""
    short = fn[len("abr_"):]
    for kwargs, word in [(dict(kh=7, kw=8, ph=3, pw=3, Wo=8), "kh * kw"), (dict(B=0), "B, H, W, C"), (dict(C=-8), "B, H, W, C"),
                         (dict(kh=0), "kh, kw"), (dict(sh=0), "stride_h"), (dict(dlw=0), "dil_h, dil_w"), (dict(ph=-1), "pad_h"),
                         (dict(groups=0), "groups, dg"), (dict(C=12, groups=8), "multiple of groups"), (dict(C=12, dg=8), "multiple of dg"),
                         (dict(C=12, groups=2), "C / groups = 6"), (dict(C=12, dg=2), "C / dg = 6"), (dict(C=6), "C / groups = 6"),
                         (dict(Ho=8), "Ho = 8"), (dict(Wo=10), "Wo = 10"), (dict(H=1, ph=0, Ho=1), "Ho = 1"), (dict(sh=2), "Ho = 7"),
                         (dict(B=1 << 15, H=1 << 8, W=1 << 8, Ho=1 << 8, Wo=1 << 8, C=4), "2^31"), (dict(), "must not be null")]:
        rc, msg = _abi(fn, **kwargs)
        assert rc < 0 and short in msg and word in msg, (kwargs, rc, msg)
    # just below the limit on the lane count, B*Ho*Wo*K*C/4 = 2^31 - 2^16, the geometry passes (only the null pointers stop it); at 2^31 it does not
    rc, msg = _abi(fn, B=(1 << 15) - 1, H=1 << 8, W=1 << 8, Ho=1 << 8, Wo=1 << 8, C=4, kh=1, kw=1, ph=0, pw=0)
    assert rc < 0 and "must not be null" in msg, msg
    rc, msg = _abi(fn, B=1 << 15, H=1 << 8, W=1 << 8, Ho=1 << 8, Wo=1 << 8, C=4, kh=1, kw=1, ph=0, pw=0)
    assert rc < 0 and "2^31" in msg, msg


def test_output_size_inference_and_error_texts():
    from abr_iod_amd.layers.dcn import DeformConvFunction, ModulatedDeformConvFunction, deform_conv, modulated_deform_conv
    from abr_iod_amd import ops
    for c in R.CASES:
        x, w = torch.zeros(c.B, c.C, c.H, c.W), torch.zeros(c.Cout, c.C // c.groups, *c.kernel)
        assert DeformConvFunction._output_size(x, w, c.padding, c.dilation, c.stride) == (c.B, c.Cout) + R.out_size(c)
        assert ops.deform_out_size(c.H, c.W, c.kernel, c.stride, c.padding, c.dilation) == R.out_size(c)

        class Ctx:
            geom = (c.kernel, c.stride, c.padding, c.dilation)
        assert ModulatedDeformConvFunction._infer_shape(Ctx, x, w) == (c.B, c.Cout) + R.out_size(c)
    w = torch.zeros(8, 8, 3, 3)
    with pytest.raises(ValueError, match=r"convolution input is too small \(output would be 2x8x0x7\)"):
        deform_conv(torch.zeros(2, 8, 2, 9), torch.zeros(2, 18, 1, 7), w)
    with pytest.raises(ValueError, match="Expected 4D tensor as input, got 3D tensor instead."):
        deform_conv(torch.zeros(8, 7, 9), torch.zeros(2, 18, 5, 7), w)
    with pytest.raises(AssertionError, match="im2col step must divide batchsize"):
        deform_conv(torch.zeros(3, 8, 7, 9), torch.zeros(3, 18, 5, 7), w, 1, 0, 1, 1, 1, 2)
    # a CPU tensor raises, as everywhere in this package (after the checks above, which need no device)
    with pytest.raises(RuntimeError, match="device tensors"):
        deform_conv(torch.zeros(3, 8, 7, 9), torch.zeros(3, 18, 5, 7), w, 1, 0, 1, 1, 1, 3)
    with pytest.raises(RuntimeError, match="device tensors"):
        modulated_deform_conv(torch.zeros(3, 8, 7, 9), torch.zeros(3, 18, 5, 7), torch.zeros(3, 9, 5, 7), w)


def test_layer_classes_keep_the_reference_surface():
    import abr_iod_amd.layers as layers
    from abr_iod_amd.layers import DeformConv, ModulatedDeformConv, ModulatedDeformConvPack
    assert layers.deform_conv is layers.dcn.deform_conv and layers.modulated_deform_conv is layers.dcn.modulated_deform_conv
    torch.manual_seed(0)
    m = DeformConv(16, 12, (3, 5), stride=(2, 1), padding=(1, 2), dilation=1, groups=2, deformable_groups=4)
    assert repr(m) == ("DeformConv(in_channels=16, out_channels=12, kernel_size=(3, 5), stride=(2, 1), dilation=(1, 1), padding=(1, 2), groups=2, "
                       "deformable_groups=4, bias=False)")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"weight": (12, 8, 3, 5)}
    bound = 1.0 / (16 * 3 * 5) ** 0.5
    assert 0.8 * bound < float(m.weight.detach().abs().max()) <= bound
    assert m.weight.permute(0, 2, 3, 1).is_contiguous()          # OHWI memory behind the OIHW shape
    with pytest.raises(AssertionError):
        DeformConv(16, 12, 3, bias=True)
    with pytest.raises(AssertionError, match="in_channels 6 cannot be divisible by groups 4"):
        DeformConv(6, 12, 3, groups=4)
    # a checkpoint in plain OIHW memory loads into it and comes back out
    w = torch.randn(12, 8, 3, 5)
    m.load_state_dict({"weight": w})
    assert torch.equal(m.state_dict()["weight"], w) and m.weight.permute(0, 2, 3, 1).is_contiguous()

    m = ModulatedDeformConv(8, 6, 3, stride=2, padding=1, dilation=1, groups=1, deformable_groups=2, bias=True)
    assert repr(m) == ("ModulatedDeformConv(in_channels=8, out_channels=6, kernel_size=(3, 3), stride=2, dilation=1, padding=1, groups=1, "
                       "deformable_groups=2, bias=True)")
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"weight": (6, 8, 3, 3), "bias": (6,)}
    assert torch.count_nonzero(m.bias) == 0 and float(m.weight.detach().abs().max()) <= 1.0 / 72 ** 0.5
    assert list(ModulatedDeformConv(8, 6, 3, bias=False).state_dict()) == ["weight"]

    m = ModulatedDeformConvPack(8, 6, 3, stride=1, padding=1, deformable_groups=2)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {"weight": (6, 8, 3, 3), "bias": (6,), "conv_offset_mask.weight": (54, 8, 3, 3),
                                                                      "conv_offset_mask.bias": (54,)}
    assert torch.count_nonzero(m.conv_offset_mask.weight) == 0 and torch.count_nonzero(m.conv_offset_mask.bias) == 0
    assert repr(m).startswith("ModulatedDeformConvPack(in_channels=8, out_channels=6, kernel_size=(3, 3), stride=1, ")
    with pytest.raises(NotImplementedError, match="groups == 1"):
        ModulatedDeformConvPack(8, 8, 3, groups=2)


def test_c_entry_points_refuse_without_a_device():
    from abr_iod_amd import _C
    x, w, off = torch.zeros(2, 8, 7, 9), torch.zeros(8, 8, 3, 3), torch.zeros(2, 18, 7, 9)
    e = torch.zeros(0)
    with pytest.raises(RuntimeError, match="device tensors"):
        _C.deform_conv_forward(x, w, off, torch.zeros(2, 8, 7, 9), e, e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 2)
    with pytest.raises(RuntimeError, match="device tensors"):
        _C.modulated_deform_conv_forward(x, w, e, e, off, torch.zeros(2, 9, 7, 9), torch.zeros(2, 8, 7, 9), e, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, False)

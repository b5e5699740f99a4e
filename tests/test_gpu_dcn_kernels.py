"""GPU: the deformable-conv kernels (abr_deform_im2col, abr_deform_col2im_coord) against a float64 pure-torch restatement of the
semantics (modulated_deform_conv / deform_conv of the reference, restated in abr_iod_amd/csrc/deform.hip).  The restatement's autograd
supplies dx, d(offsets) and d(mask).  The sample point is rounded to fp32 as the kernel computes it, so both take the same floors."""
import pytest
import torch

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def deform_cols_ref(x, om, dg, modulated, want_abs=False):
    """x [B,H,W,C], om [B,H,W,Com] float64 (autograd-able) -> cols [B,H,W,9C] float64.  want_abs: also sum_corners |v| (inside the box)
    per (tap, channel), for error bounds."""
    B, H, W, C = x.shape
    gs = C // dg
    dev = x.device
    ho = torch.arange(H, device=dev, dtype=torch.float32).view(1, H, 1)
    wo = torch.arange(W, device=dev, dtype=torch.float32).view(1, 1, W)
    bi = torch.arange(B, device=dev).view(B, 1, 1)
    cols, absv = [], []
    for k in range(9):
        i, j = divmod(k, 3)
        parts, aparts = [], []
        m = torch.sigmoid(om[..., 18 + k]).unsqueeze(-1) if modulated else None
        for g in range(dg):
            dh, dw = om[..., 2 * k + 18 * g], om[..., 2 * k + 1 + 18 * g]
            # the sample point in fp32 (the kernel's arithmetic), the offset's gradient flowing through it with slope 1
            h = (ho - 1 + i + dh.detach().float()).double() + (dh - dh.detach())
            w = (wo - 1 + j + dw.detach().float()).double() + (dw - dw.detach())
            # a non-finite or huge coordinate lies outside the box whatever else holds; a detached constant outside the box stands in for it,
            # so that neither .long() nor autograd (0 * NaN) ever sees it -- `inside` makes its value and its gradient zero
            h = torch.where(torch.isfinite(h) & (h.abs() <= 2.0 ** 24), h, torch.full_like(h, -5.0).detach())
            w = torch.where(torch.isfinite(w) & (w.abs() <= 2.0 ** 24), w, torch.full_like(w, -5.0).detach())
            inside = ((h > -1) & (w > -1) & (h < H) & (w < W)).unsqueeze(-1)
            hl, wl = torch.floor(h.detach()), torch.floor(w.detach())
            lh, lw = h - hl, w - wl
            val = 0.0
            av = 0.0
            for dy, dx_, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
                hc, wc = (hl + dy).long(), (wl + dx_).long()
                ok = ((hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)).unsqueeze(-1)
                v = x[bi, hc.clamp(0, H - 1), wc.clamp(0, W - 1)][..., g * gs:(g + 1) * gs]
                v = torch.where(ok, v, torch.zeros_like(v))
                val = val + wt.unsqueeze(-1) * v
                av = av + v.abs()
            val = torch.where(inside, val, torch.zeros_like(val))
            parts.append(val)
            aparts.append(torch.where(inside, av, torch.zeros_like(av)).detach())
        val = torch.cat(parts, -1)
        if modulated:
            val = val * m
        cols.append(val)
        absv.append(torch.cat(aparts, -1))
    out = torch.cat(cols, -1)
    return (out, torch.cat(absv, -1)) if want_abs else out


def _offsets(B, H, W, com, com_pad, scale, seed, dev, pad_value=1e3):
    """fp32 offsets of the given scale whose fractional parts stay >= 1e-4 away from the integers (same floors in fp32 and float64);
    the padding channels hold garbage that must never be read (pad_value = NaN: any read of them shows in the result)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    om = (torch.rand(B, H, W, com, generator=g) * 2 - 1) * scale
    fr = om - torch.floor(om)
    om = torch.where((fr < 1e-4) | (fr > 1 - 1e-4), om + 0.01, om)
    pad = torch.full((B, H, W, com_pad - com), pad_value)
    return torch.cat([om, pad], -1).float().to(dev)


def _check(x, om, dg, modulated, dcol_seed=7):
    from abr_iod_amd import ops
    B, H, W, C = x.shape
    com = 27 if modulated else 18 * dg
    cols = ops.deform_im2col(x, om, dg, modulated)
    x64 = x.double().requires_grad_(True)
    om64 = om.double().requires_grad_(True)
    ref, absv = deform_cols_ref(x64, om64, dg, modulated, want_abs=True)
    # im2col: within a few fp32 ulp of sum |w_c v_c| (the mask's rounding included)
    x_abs = x.double().abs()
    bound = deform_cols_ref(x_abs, om.double(), dg, modulated)
    err = (cols.double() - ref.detach()).abs()
    worst = {"cols": float((err / (12 * U * bound + 1e-38)).max())}
    assert torch.all(err <= 12 * U * bound + 1e-38), float((err / (bound + 1e-30)).max())
    assert torch.all(cols[bound == 0] == 0)
    # backward
    g = torch.Generator(device="cpu").manual_seed(dcol_seed)
    dcol = torch.randn(B, H, W, 9 * C, generator=g).float().to(x.device)
    dx, d_om = ops.deform_col2im_coord(dcol, x, om, dg, modulated)
    rdx, rdom = torch.autograd.grad(ref, (x64, om64), dcol.double())
    # dx: fp32 adds in any order -- bounded by the number of adds times the sum of |terms| (the VJP of |dcol|, all coefficients >= 0)
    xa = x.double().requires_grad_(True)
    dx_abs, = torch.autograd.grad(deform_cols_ref(xa, om.double(), dg, modulated), (xa,), dcol.double().abs())
    e = (dx.double() - rdx).abs()
    worst["dx"] = float((e / (48 * U * dx_abs + 1e-38)).max())
    assert torch.all(e <= 48 * U * dx_abs + 1e-38), float((e / (dx_abs + 1e-30)).max())
    # d_om: per group, a sum over C/dg channels of terms bounded by |dcol| m sum|v|
    gs = C // dg
    m = torch.sigmoid(om.double()[..., 18:27]) if modulated else torch.ones(B, H, W, 9, dtype=torch.float64, device=x.device)
    S = (dcol.double().abs() * absv).view(B, H, W, 9, dg, gs).sum(-1)          # [B,H,W,9,dg]
    tol = (gs + 16) * U * S * m.unsqueeze(-1) + 1e-38
    e_off = (d_om[..., :18 * dg].double() - rdom[..., :18 * dg]).abs().view(B, H, W, dg, 9, 2).amax(-1).permute(0, 1, 2, 4, 3)
    worst["d_off"] = float((e_off / tol).max())
    if modulated:
        e_m = (d_om[..., 18:27].double() - rdom[..., 18:27]).abs()
        worst["d_mask"] = float((e_m / ((gs + 16) * U * S[..., 0] * 0.25 + 4 * U * rdom[..., 18:27].abs() + 1e-38)).max())
    print("deform error/bound C={} dg={} v{} {}x{}x{} Com={}:".format(C, dg, 2 if modulated else 1, B, H, W, om.shape[-1]),
          " ".join("{} {:.3f}".format(k, v) for k, v in worst.items()))
    for gi in range(dg):
        for k in range(9):
            for t in range(2):
                ch = 2 * k + t + 18 * gi
                ee = (d_om[..., ch].double() - rdom[..., ch]).abs()
                assert torch.all(ee <= tol[..., k, gi]), (ch, float(ee.max()), float(tol[..., k, gi].max()))
    if modulated:
        for k in range(9):
            ee = (d_om[..., 18 + k].double() - rdom[..., 18 + k]).abs()
            assert torch.all(ee <= (gs + 16) * U * S[..., k, 0] * 0.25 + 4 * U * rdom[..., 18 + k].abs() + 1e-38), k
    assert torch.all(d_om[..., com:] == 0), "padding channels of d_om must be written as zero"
    return cols, dx, d_om, ref


CASES = [(64, 1, False), (128, 1, False), (256, 1, False), (64, 2, False), (128, 2, False), (256, 2, False),
         (64, 1, True), (128, 1, True), (256, 1, True)]


@pytest.mark.parametrize("C,dg,modulated", CASES)
@pytest.mark.parametrize("scale", [0.0, 0.7, 3.0])
def test_random_offsets(C, dg, modulated, scale):
    torch.manual_seed(C + dg + int(scale * 10))
    B, H, W = 2, 7, 11
    com = 27 if modulated else 18 * dg
    com_pad = (com + 31) // 32 * 32
    x = torch.randn(B, H, W, C, device="cuda")
    om = _offsets(B, H, W, com, com_pad, scale, seed=C * 3 + dg, dev="cuda")
    if modulated:
        om[..., 18:27] = torch.randn(B, H, W, 9, device="cuda") * 2
    _check(x, om, dg, modulated)


@pytest.mark.parametrize("C,dg,modulated", [(64, 1, False), (128, 2, False), (128, 1, True)])
def test_exact_positions_and_borders(C, dg, modulated):
    """integer and half-integer offsets (exact in fp32): sample points on the grid, halfway between, at exactly -1 and H-1 / W-1"""
    from abr_iod_amd import ops
    torch.manual_seed(3)
    B, H, W = 2, 6, 8
    com = 27 if modulated else 18 * dg
    com_pad = (com + 31) // 32 * 32
    vals = torch.tensor([-2.0, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 1.5, 2.0])
    idx = torch.randint(0, len(vals), (B, H, W, com))
    om = torch.cat([vals[idx], torch.full((B, H, W, com_pad - com), -7.0)], -1).cuda()
    if modulated:
        om[..., 18:27] = torch.randn(B, H, W, 9, device="cuda")
    x = torch.randn(B, H, W, C, device="cuda")
    cols, dx, d_om, ref = _check(x, om, dg, modulated)
    # zero offsets on the border taps sample at exactly -1 (outside: 0) and at H-1 (inside, upper corner outside)
    om0 = torch.zeros(B, H, W, com_pad, device="cuda")
    cols0 = ops.deform_im2col(x, om0, dg, modulated)
    c0 = cols0.view(B, H, W, 9, C)
    assert torch.all(c0[:, 0, :, 0] == 0) and torch.all(c0[:, :, 0, 0] == 0)
    mult = 0.5 if modulated else 1.0
    assert torch.equal(c0[:, H - 1, W - 1, 4], x[:, H - 1, W - 1] * mult)


@pytest.mark.parametrize("C,dg,modulated", [(64, 1, False), (128, 2, False), (256, 1, True)])
def test_samples_outside_give_exact_zeros(C, dg, modulated):
    from abr_iod_amd import ops
    B, H, W = 2, 5, 6
    com = 27 if modulated else 18 * dg
    com_pad = (com + 31) // 32 * 32
    om = torch.zeros(B, H, W, com_pad, device="cuda")
    om[..., :18 * dg:2] = H + 3.25      # every dh: below the image
    om[..., 1:18 * dg:2] = -0.5
    x = torch.randn(B, H, W, C, device="cuda")
    cols = ops.deform_im2col(x, om, dg, modulated)
    assert torch.count_nonzero(cols) == 0
    dcol = torch.randn(B, H, W, 9 * C, device="cuda")
    dx, d_om = ops.deform_col2im_coord(dcol, x, om, dg, modulated)
    assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(d_om) == 0


def test_cols_inherit_amax_bound_and_d_om_carries_word():
    from abr_iod_amd import ops
    B, H, W, C = 1, 4, 5, 64
    x = ops.amax_compute(torch.randn(B, H, W, C, device="cuda"))
    om = torch.randn(B, H, W, 32, device="cuda")
    n0 = ops.amax_reductions[0]
    cols = ops.deform_im2col(x, om, 1, False)
    assert ops.amax_of(cols)[0] == ops.amax_of(x)[0]
    dx, d_om = ops.deform_col2im_coord(torch.randn(B, H, W, 9 * C, device="cuda"), x, om, 1, False)
    assert ops.amax_of(d_om)[0] is not None
    assert ops.amax_reductions[0] == n0


# ---------------------------------------------------------------------------------------------- every width the C ABI admits
# (C, dg, modulated).  The backward takes any power of two C in [4, 1024]: gs = C / dg decides the xor butterfly's span (4 ... 64) and the
# number of waves summed through LDS (gs / 64: 2 ... 16); 256 // C is the number of (pixel, tap) rows per workgroup (0: one row of C lanes).
WIDTHS = (4, 8, 16, 32, 512, 1024)
GROUPED = [(16, 4), (32, 4), (64, 4), (64, 16), (512, 2), (512, 8), (1024, 2), (1024, 4)]
WIDTH_CASES = [(C, 1, False) for C in WIDTHS] + [(C, 1, True) for C in WIDTHS] + [(C, dg, False) for C, dg in GROUPED]
# a later edit must not drop a path silently: with several groups (these and CASES' 64 / 2, 128 / 2, 256 / 2) gs takes every power of two in
# [4, 512]; the widths here reach every number of rows per workgroup but CASES' 2 and 1
assert {C // dg for C, dg, _ in WIDTH_CASES if dg > 1} == {4, 8, 16, 64, 256, 512}
assert {C // dg for C, dg, _ in WIDTH_CASES + CASES if dg > 1} == {4, 8, 16, 32, 64, 128, 256, 512}
assert {C // dg for C, dg, _ in WIDTH_CASES} == {4, 8, 16, 32, 64, 256, 512, 1024}
assert {256 // C for C, _, _ in WIDTH_CASES} == {64, 32, 16, 8, 4, 0}
assert {C for C, _, m in WIDTH_CASES if m} == set(WIDTHS)


def _case(B, H, W, C, dg, modulated, scale, seed, com_pad=None, pad_value=float("nan")):
    com = 27 if modulated else 18 * dg
    com_pad = (com + 31) // 32 * 32 if com_pad is None else com_pad
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = torch.randn(B, H, W, C, generator=g).cuda()
    om = _offsets(B, H, W, com, com_pad, scale, seed=seed + 1, dev="cuda", pad_value=pad_value)
    if modulated:
        om[..., 18:27] = (torch.randn(B, H, W, 9, generator=g) * 2).cuda()
    return x, om


def _deterministic(x, om, dg, modulated, cols, d_om):
    """cols and d_om are sums in a fixed order: bit-identical from call to call (dx, from atomics, only meets its bound)"""
    from abr_iod_amd import ops
    g = torch.Generator(device="cpu").manual_seed(7)     # _check's dcol
    dcol = torch.randn(*x.shape[:3], 9 * x.shape[3], generator=g).float().cuda()
    assert torch.equal(ops.deform_im2col(x, om, dg, modulated), cols), "cols differ between two calls"
    _, again = ops.deform_col2im_coord(dcol, x, om, dg, modulated)
    assert not d_om.isnan().any() and torch.equal(again, d_om), "d_om differs between two calls"


@pytest.mark.parametrize("C,dg,modulated", WIDTH_CASES)
@pytest.mark.parametrize("scale", [0.0, 0.7, 3.0])
def test_every_admitted_width(C, dg, modulated, scale):
    """1 x 3 x 5: 135 (pixel, tap) rows, a multiple of no rows-per-workgroup in 2 ... 64 -- the last workgroup is ragged"""
    x, om = _case(1, 3, 5, C, dg, modulated, scale, seed=C * 5 + dg + int(scale * 10))
    cols, _, d_om, _ = _check(x, om, dg, modulated)
    _deterministic(x, om, dg, modulated, cols, d_om)


@pytest.mark.parametrize("dg,modulated", [(1, False), (4, False), (1, True)])
def test_widest_row_on_the_usual_map(dg, modulated):
    """C = 1024 (16 waves per row) at the map of test_random_offsets"""
    x, om = _case(2, 7, 11, 1024, dg, modulated, 0.7, seed=41 + dg)
    cols, _, d_om, _ = _check(x, om, dg, modulated)
    _deterministic(x, om, dg, modulated, cols, d_om)


# ---------------------------------------------------------------------------------------------- padding channels
# (C, dg, modulated, Com): no padding at all (nothing to zero-fill), the product's padding, padding wider than C (the fill loop's second trip)
PADDING = [(64, 16, False, 288), (64, 1, True, 27), (64, 1, False, 32), (64, 1, True, 32), (4, 1, False, 64), (8, 1, True, 64)]


@pytest.mark.parametrize("C,dg,modulated,com_pad", PADDING)
def test_padding_channels_never_read_and_written_as_zero(C, dg, modulated, com_pad):
    from abr_iod_amd._lib import lib, ptr, stream
    B, H, W = 2, 3, 5
    com = 27 if modulated else 18 * dg
    x, om = _case(B, H, W, C, dg, modulated, 1.5, seed=C + com_pad, com_pad=com_pad)      # the padding holds NaN
    assert om.shape[-1] == com_pad and bool(om[..., com:].isnan().all())
    cols, _, d_om, _ = _check(x, om, dg, modulated)
    assert not cols.isnan().any() and not d_om.isnan().any()
    # a stale buffer: every element of d_om must be overwritten, the padding with zeros
    g = torch.Generator(device="cpu").manual_seed(7)
    dcol = torch.randn(B, H, W, 9 * C, generator=g).float().cuda()
    dx = torch.zeros_like(x)
    out = torch.full_like(om, float("nan"))
    assert lib().abr_deform_col2im_coord(ptr(dcol), ptr(x), ptr(om), B, H, W, C, com_pad, dg, int(modulated), ptr(dx), ptr(out), None, 0,
                                         stream()) == 0
    assert torch.equal(out, d_om)
    assert out[..., com:].numel() == (com_pad - com) * B * H * W and torch.count_nonzero(out[..., com:]) == 0


# ---------------------------------------------------------------------------------------------- tiny maps
@pytest.mark.parametrize("dg,modulated", [(1, False), (2, False), (1, True)])
@pytest.mark.parametrize("scale", ["zero", 0.0, 0.7, 3.0])
@pytest.mark.parametrize("H,W", [(1, 1), (1, 9), (9, 1), (2, 2)])
def test_tiny_maps(H, W, scale, dg, modulated):
    """1-pixel and 1-row maps; "zero": offsets of exactly 0 (the border taps sample at exactly -1 and at H - 1; _offsets' 0.0 gives 0.01)"""
    s = 0.0 if scale == "zero" else scale
    x, om = _case(2, H, W, 64, dg, modulated, s, seed=H * 31 + W + dg + int(s * 10))
    if scale == "zero":
        om[..., :18 * dg] = 0.0
    _check(x, om, dg, modulated)


# ---------------------------------------------------------------------------------------------- non-finite and huge offsets
POISON = [float("inf"), float("-inf"), float("nan"), 1e30, -1e30, 3e38, -3e38]


@pytest.mark.parametrize("C,dg,modulated", [(8, 1, False), (64, 2, False), (64, 1, True), (512, 2, False), (1024, 1, True)])
def test_nonfinite_and_huge_offsets_are_outside(C, dg, modulated):
    """a tenth of the (pixel, tap, group) offsets has dh, dw or both replaced by +-inf, NaN, +-1e30 or +-3e38: such a tap lies outside the box
    -- exactly 0 in cols, nothing added to dx, exactly 0 in d_om -- and no NaN appears anywhere; every other tap meets _check's bounds"""
    from abr_iod_amd import ops
    B, H, W = 2, 5, 7
    x, om = _case(B, H, W, C, dg, modulated, 3.0, seed=C + 7 * dg)
    g = torch.Generator(device="cpu").manual_seed(C)
    bad = torch.rand(B, H, W, 9 * dg, generator=g) < 0.1                      # per (pixel, group, tap): channel pair 2k + 18g
    which = torch.randint(0, 3, (B, H, W, 9 * dg), generator=g)              # 0: dh, 1: dw, 2: both
    val = torch.tensor(POISON)[torch.randint(0, len(POISON), (B, H, W, 9 * dg, 2), generator=g)]
    hit = torch.stack([bad & (which != 1), bad & (which != 0)], -1)         # [B,H,W,9dg,2]
    assert int(bad.sum()) >= len(POISON)
    off = om[..., :18 * dg].cpu().view(B, H, W, 9 * dg, 2)
    om[..., :18 * dg] = torch.where(hit, val, off).view(B, H, W, 18 * dg).cuda()
    cols, dx, d_om, _ = _check(x, om, dg, modulated)
    assert bool(cols.isfinite().all()) and bool(dx.isfinite().all()) and bool(d_om.isfinite().all())
    bad = bad.cuda().view(B, H, W, dg, 9)                                       # [.., g, k]
    gs = C // dg
    c = cols.view(B, H, W, 9, dg, gs).permute(0, 1, 2, 4, 3, 5)                 # [.., g, k, gs]
    assert torch.count_nonzero(c[bad]) == 0
    d = d_om[..., :18 * dg].view(B, H, W, dg, 9, 2)
    assert torch.count_nonzero(d[bad]) == 0
    if modulated:
        assert torch.count_nonzero(d_om[..., 18:27][bad[..., 0, :]]) == 0
    # with every tap poisoned nothing at all is sampled: dx stays exactly zero
    om[..., :18 * dg:2] = float("nan")
    dcol = torch.randn(B, H, W, 9 * C, device="cuda")
    dx, d_om = ops.deform_col2im_coord(dcol, x, om, dg, modulated)
    assert torch.count_nonzero(ops.deform_im2col(x, om, dg, modulated)) == 0
    assert torch.count_nonzero(dx) == 0 and torch.count_nonzero(d_om) == 0


# ---------------------------------------------------------------------------------------------- saturated masks
@pytest.mark.parametrize("C", [16, 64, 256])
def test_saturated_mask_logits(C):
    """m is 0 or 1 to fp32 at +-16, +-40, +-80 and exactly at +-inf, where the mask's gradient is exactly 0 (e = inf must not give inf * 0).
    (+-88 ... +-104 are left out: there 1 / (1 + e) is denormal in fp32, and a flush would be a false alarm.)"""
    B, H, W = 2, 4, 5
    x, om = _case(B, H, W, C, 1, True, 0.7, seed=C + 3)
    logits = torch.tensor([16.0, -16.0, 40.0, -40.0, 80.0, -80.0, float("inf"), float("-inf"), 0.0])
    pix = torch.arange(B * H * W).view(B, H, W, 1)
    om[..., 18:27] = logits[(torch.arange(9).view(1, 1, 1, 9) + pix) % 9].cuda()      # one value per tap, rotated from pixel to pixel
    cols, dx, d_om, _ = _check(x, om, 1, True)
    assert bool(cols.isfinite().all()) and bool(dx.isfinite().all()) and bool(d_om.isfinite().all())
    inf = om[..., 18:27].isinf()
    assert torch.count_nonzero(d_om[..., 18:27][inf]) == 0
    c = cols.view(B, H, W, 9, C)
    assert torch.count_nonzero(c[om[..., 18:27] == float("-inf")]) == 0


# ---------------------------------------------------------------------------------------------- forward-only widths and refusals
def _forward_check(x, om, dg, modulated):
    """_check's forward half, with its bound"""
    from abr_iod_amd import ops
    cols = ops.deform_im2col(x, om, dg, modulated)
    ref = deform_cols_ref(x.double(), om.double(), dg, modulated)
    bound = deform_cols_ref(x.double().abs(), om.double(), dg, modulated)
    err = (cols.double() - ref).abs()
    print("deform forward error/bound C={} dg={}: cols {:.3f}".format(x.shape[3], dg, float((err / (12 * U * bound + 1e-38)).max())))
    assert torch.all(err <= 12 * U * bound + 1e-38), float((err / (bound + 1e-30)).max())
    assert torch.all(cols[bound == 0] == 0)


@pytest.mark.parametrize("C,dg", [(96, 1), (96, 2), (96, 3), (12, 1), (12, 3)])
@pytest.mark.parametrize("scale", [0.0, 0.7, 3.0])
def test_forward_only_widths(C, dg, scale):
    """C / dg a multiple of 4 but C no power of two: the forward is right, the backward refuses (an argument check, before any launch)"""
    from abr_iod_amd import ops
    x, om = _case(1, 3, 5, C, dg, False, scale, seed=C + dg + int(scale * 10))
    _forward_check(x, om, dg, False)
    with pytest.raises(RuntimeError, match="power of two"):
        ops.deform_col2im_coord(torch.zeros(1, 3, 5, 9 * C, device="cuda"), x, om, dg, False)


def test_refusals():
    """every one an ABR_REQUIRE that returns before any launch"""
    from abr_iod_amd import ops

    def both(C, dg, modulated, com, fwd_match, bwd_match):
        x = torch.zeros(1, 2, 2, C, device="cuda")
        om = torch.zeros(1, 2, 2, com, device="cuda")
        if fwd_match is not None:
            with pytest.raises(RuntimeError, match=fwd_match):
                ops.deform_im2col(x, om, dg, modulated)
        with pytest.raises(RuntimeError, match=bwd_match):
            ops.deform_col2im_coord(torch.zeros(1, 2, 2, 9 * C, device="cuda"), x, om, dg, modulated)

    both(2048, 1, False, 32, None, "power of two")                        # (the forward admits 2048 channels)
    both(64, 2, True, 32, "one deformable group", "one deformable group")
    both(64, 1, False, 17, "too few channels", "too few channels")
    both(64, 1, True, 26, "too few channels", "too few channels")
    both(64, 2, False, 35, "too few channels", "too few channels")
    both(12, 2, False, 64, "multiple of 4", "power of two")               # C / dg = 6
    both(64, 32, False, 576, "multiple of 4", "multiple of 4")            # C / dg = 2
    both(2, 1, False, 32, "multiple of 4", "power of two")

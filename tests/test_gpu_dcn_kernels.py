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


def _offsets(B, H, W, com, com_pad, scale, seed, dev):
    """fp32 offsets of the given scale whose fractional parts stay >= 1e-4 away from the integers (same floors in fp32 and float64);
    the padding channels hold garbage that must never be read"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    om = (torch.rand(B, H, W, com, generator=g) * 2 - 1) * scale
    fr = om - torch.floor(om)
    om = torch.where((fr < 1e-4) | (fr > 1 - 1e-4), om + 0.01, om)
    pad = torch.full((B, H, W, com_pad - com), 1e3)
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
    assert torch.all(e <= 48 * U * dx_abs + 1e-38), float((e / (dx_abs + 1e-30)).max())
    # d_om: per group, a sum over C/dg channels of terms bounded by |dcol| m sum|v|
    gs = C // dg
    m = torch.sigmoid(om.double()[..., 18:27]) if modulated else torch.ones(B, H, W, 9, dtype=torch.float64, device=x.device)
    S = (dcol.double().abs() * absv).view(B, H, W, 9, dg, gs).sum(-1)          # [B,H,W,9,dg]
    tol = (gs + 16) * U * S * m.unsqueeze(-1) + 1e-38
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

"""Float64 pure-torch restatement of the general deformable convolution (abr_deform_im2col_general / abr_deform_col2im_coord_general and the
op above them: include/abr_iod_hip.h), generalising deform_cols_ref of tests/test_gpu_dcn_kernels.py, with the case table both suites share.

As there: the sample point is rounded to fp32 as the kernel computes it (same floors), autograd supplies every gradient, and `want_abs`
returns the sums of |v| the bounds are built from.  Layouts are the library's: x [B,H,W,C], offset [B,Ho,Wo,dg*2K], mask [B,Ho,Wo,dg*K],
cols [groups, B*Ho*Wo, K*C/groups], weight OHWI [Cout,kh,kw,C/groups].

Beside the autograd form there is an explicit one (`coord_terms`): the per-channel terms of d_offset and d_mask written out, in float64 or
-- the honest float32 restatement -- in float32 with a chosen summation order."""
from collections import namedtuple

import torch

U = 2.0 ** -24
# The bounds of tests/test_gpu_dcn_kernels.py, kept where they hold: dx 48 U times the VJP of |dcol|; coordinates (C/dg + 16) U S.
# Columns: that file's 12 U sum|w v| leaves the honest float32 restatement a margin of 3.9 (no mask, the 7 x 7 kernel's 3,087 samples per
# channel) and 3.4 (a mask: one more rounding), not 4.  From the addend count instead: a column is 4 products of 4 roundings each (1 - lh,
# 1 - lw, their product, times v) under at most 3 additions, 7 roundings on the longest chain, 8 with the mask's product; the constant is
# twice that first-order worst case, 14 U and 16 U (tests/test_deform_conv_ref.py prints the honest ratios: at most 0.23 of either).
COLS_C, COLS_MASK_C, DX_C, COORD_C = 14, 16, 48, 16
# contractions (tests/test_gpu_ops.py, tests/test_gpu_f16x3_admission.py): 8 U sum|a||b| relative, 2^-39 amax absolute (f16x3's floor)
CONV_C, CONV_FLOOR = 8, 2.0 ** -39

Case = namedtuple("Case", "id B H W C Cout kernel stride padding dilation groups dg")


def _case(id, B=2, H=7, W=9, C=8, Cout=8, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, dg=1):
    return Case(id, B, H, W, C, Cout, kernel, stride, padding, dilation, groups, dg)


CASES = [
    _case("a_3x3_s1_p1"),
    _case("b_3x3_s2_p1", stride=(2, 2)),
    _case("c_3x3_p2_d2", padding=(2, 2), dilation=(2, 2)),
    _case("d_1x1", kernel=(1, 1), padding=(0, 0)),
    _case("e_3x5_s21_p12", kernel=(3, 5), stride=(2, 1), padding=(1, 2)),
    _case("f_groups2", C=16, groups=2),
    _case("g_dg2", C=16, dg=2),
    _case("h_groups2_dg4", C=16, groups=2, dg=4),
    _case("i_cout6_per_group", C=16, Cout=12, groups=2),
    _case("j_5x5_to_2x2", H=5, W=5, stride=(2, 2), padding=(0, 0)),
    _case("j_3x3_to_1x1", H=3, W=3, stride=(2, 2), padding=(0, 0)),
    _case("k_batch3", B=3),
    _case("l_7x7_c4", C=4, kernel=(7, 7), padding=(3, 3)),
]
CASE = {c.id: c for c in CASES}
FAMILIES = ("small", "wide", "dyadic")       # 0.5 px; about a third of the samples outside; multiples of 1/4 with samples on the accept boundary


def out_size(c):
    return tuple((n + 2 * p - (d * (k - 1) + 1)) // s + 1 for n, k, s, p, d in zip((c.H, c.W), c.kernel, c.stride, c.padding, c.dilation))


def geom(c):
    return dict(kernel=c.kernel, stride=c.stride, padding=c.padding, dilation=c.dilation, groups=c.groups, dg=c.dg)


def random_offsets(shape, scale, gen):
    """fp32 offsets of the given scale whose fractional parts stay >= 1e-4 away from the integers (same floors in fp32 and float64), built as
    _offsets of tests/test_gpu_dcn_kernels.py builds them"""
    om = (torch.rand(*shape, generator=gen) * 2 - 1) * scale
    fr = om - torch.floor(om)
    return torch.where((fr < 1e-4) | (fr > 1 - 1e-4), om + 0.01, om).float()


def make_inputs(c, family, masked, seed=0):
    """-> dict of float32 CPU tensors x, offset, mask (None unless masked; values in (0, 2)), w (OHWI), bias, dcol, gy"""
    gen = torch.Generator(device="cpu").manual_seed(1000 * seed + sum(map(ord, c.id + family)) + int(masked))
    Ho, Wo = out_size(c)
    K = c.kernel[0] * c.kernel[1]
    shape = (c.B, Ho, Wo, c.dg * 2 * K)
    if family == "small":
        offset = random_offsets(shape, 0.5, gen)
    elif family == "wide":
        offset = random_offsets(shape, 0.4 * max(c.H, c.W), gen)      # (a third outside on the 7 x 9 maps, fewer on the tiny ones of case j)
    else:
        offset = (torch.randint(-8, 9, shape, generator=gen) / 4.0).float()
        # the first and last tap rows of every pixel: samples at exactly h = -1, h = H (rejected) and h = H - 1 (accepted), whatever the pixel
        ho = torch.arange(Ho).view(1, Ho, 1, 1) * c.stride[0] - c.padding[0]
        off = offset.view(c.B, Ho, Wo, c.dg, K, 2)
        last = (c.kernel[0] - 1) * c.dilation[0]
        off[..., 0, 0] = torch.where(torch.arange(Wo).view(1, 1, Wo, 1) % 2 == 0, -1.0 - ho, c.H - 1.0 - ho).expand(c.B, Ho, Wo, c.dg)
        off[..., K - 1, 0] = (c.H - ho - last).expand(c.B, Ho, Wo, c.dg).float()
    d = {"offset": offset, "x": torch.randn(c.B, c.H, c.W, c.C, generator=gen)}
    d["mask"] = (torch.rand(c.B, Ho, Wo, c.dg * K, generator=gen) * 1.98 + 0.01) if masked else None
    Cg = c.C // c.groups
    d["w"] = torch.randn(c.Cout, c.kernel[0], c.kernel[1], Cg, generator=gen) / (K * Cg) ** 0.5
    d["bias"] = torch.randn(c.Cout, generator=gen)
    d["dcol"] = torch.randn(c.groups, c.B * Ho * Wo, K * Cg, generator=gen)
    d["gy"] = torch.randn(c.B, Ho, Wo, c.Cout, generator=gen)
    return d


# ------------------------------------------------------------------------------------------------------------------------ the restatement
def _taps(x, offset, kernel, stride, padding, dilation, dg, dtype=torch.float64, exact_point=False):
    """for every tap k: (k, inside [B,Ho,Wo,C], lh, lw [B,Ho,Wo,C], the four corner values [B,Ho,Wo,C], zero where the corner is outside).
    dtype float64: the sample point is formed in fp32 (the kernel's one add) and everything after it in float64, the offsets' gradient
    flowing through with slope 1.  dtype float32: all of it in float32.  exact_point: the sample point in float64 too (the function whose
    central differences the gradients are checked against: with the fp32 point it is a staircase in the offsets)."""
    B, H, W, C = x.shape
    Ho, Wo = offset.shape[1], offset.shape[2]
    kh, kw = kernel
    K, gs = kh * kw, C // dg
    off = offset.view(B, Ho, Wo, dg, K, 2)
    ho = torch.arange(Ho, device=x.device).view(1, Ho, 1, 1) * stride[0] - padding[0]
    wo = torch.arange(Wo, device=x.device).view(1, 1, Wo, 1) * stride[1] - padding[1]
    bi = torch.arange(B, device=x.device).view(B, 1, 1, 1)
    ci = torch.arange(C, device=x.device).view(1, 1, 1, C)
    for k in range(K):
        i, j = divmod(k, kw)
        dh = off[..., k, 0].repeat_interleave(gs, -1)
        dw = off[..., k, 1].repeat_interleave(gs, -1)
        if exact_point:
            h, w = (ho + i * dilation[0]).double() + dh, (wo + j * dilation[1]).double() + dw
        else:
            h = (ho + i * dilation[0]).float() + dh.detach().float()
            w = (wo + j * dilation[1]).float() + dw.detach().float()
        if dtype == torch.float64 and not exact_point:
            h = h.double() + (dh - dh.detach())
            w = w.double() + (dw - dw.detach())
        # a non-finite or huge coordinate lies outside the box; a detached constant outside the box stands in for it
        h = torch.where(torch.isfinite(h) & (h.abs() <= 2.0 ** 24), h, torch.full_like(h, -5.0).detach())
        w = torch.where(torch.isfinite(w) & (w.abs() <= 2.0 ** 24), w, torch.full_like(w, -5.0).detach())
        inside = (h > -1) & (w > -1) & (h < H) & (w < W)
        hl, wl = torch.floor(h.detach()), torch.floor(w.detach())
        vs = []
        for dy, dx_ in ((0, 0), (0, 1), (1, 0), (1, 1)):
            hc, wc = (hl + dy).long(), (wl + dx_).long()
            ok = (hc >= 0) & (hc < H) & (wc >= 0) & (wc < W)
            v = x[bi, hc.clamp(0, H - 1), wc.clamp(0, W - 1), ci]
            vs.append(torch.where(ok, v, torch.zeros_like(v)))
        yield k, inside, h - hl, w - wl, vs


def _mask_of(mask, k, K, gs):
    B, Ho, Wo = mask.shape[:3]
    return mask.view(B, Ho, Wo, -1, K)[..., k].repeat_interleave(gs, -1)


def to_cols(t, groups):
    """[B,Ho,Wo,K,C] -> [groups, B*Ho*Wo, K*C/groups]"""
    B, Ho, Wo, K, C = t.shape
    return t.reshape(B * Ho * Wo, K, groups, C // groups).permute(2, 0, 1, 3).reshape(groups, B * Ho * Wo, K * (C // groups))


def from_cols(cols, B, Ho, Wo, K):
    """[groups, B*Ho*Wo, K*C/groups] -> [B,Ho,Wo,K,C]"""
    groups = cols.shape[0]
    return cols.reshape(groups, B * Ho * Wo, K, -1).permute(1, 2, 0, 3).reshape(B, Ho, Wo, K, -1)


def deform_cols_general_ref(x, offset, mask, kernel, stride, padding, dilation, groups, dg, want_abs=False, dtype=torch.float64, order="seq",
                            exact_point=False):
    """-> cols [groups, B*Ho*Wo, K*C/groups] (autograd-able in float64).  want_abs: also sum_corners |v| inside the box, in cols' layout.
    dtype float32: the honest restatement, the four products summed in `order`: "seq" ((a + b) + c) + d, "pair" (a + b) + (c + d)."""
    K, gs = kernel[0] * kernel[1], x.shape[3] // dg
    vals, absv = [], []
    for k, inside, lh, lw, (v1, v2, v3, v4) in _taps(x, offset, kernel, stride, padding, dilation, dg, dtype, exact_point):
        t1, t2, t3, t4 = (1 - lh) * (1 - lw) * v1, (1 - lh) * lw * v2, lh * (1 - lw) * v3, lh * lw * v4
        val = ((t1 + t2) + t3) + t4 if order == "seq" else (t1 + t2) + (t3 + t4)
        val = torch.where(inside, val, torch.zeros_like(val))
        if mask is not None:
            val = val * _mask_of(mask, k, K, gs)
        vals.append(val)
        av = v1.abs() + v2.abs() + v3.abs() + v4.abs()
        absv.append(torch.where(inside, av, torch.zeros_like(av)).detach())
    out = to_cols(torch.stack(vals, 3), groups)
    return (out, to_cols(torch.stack(absv, 3), groups)) if want_abs else out


def _sum_last(t, order):
    if order == "seq":
        acc = t[..., 0]
        for i in range(1, t.shape[-1]):
            acc = acc + t[..., i]
        return acc
    while t.shape[-1] > 1:
        if t.shape[-1] % 2:
            t = torch.cat([t, torch.zeros_like(t[..., :1])], -1)
        t = t[..., ::2] + t[..., 1::2]
    return t[..., 0]


def coord_terms(dcol, x, offset, mask, kernel, stride, padding, dilation, groups, dg, dtype=torch.float64, order="seq"):
    """The gradients of the coordinates written out: -> (d_offset [B,Ho,Wo,dg*2K], d_mask [B,Ho,Wo,dg*K] or None), the per-channel terms
    summed over each deformable group's channels in `order` ("seq": ascending, "pair": pairwise), in `dtype`."""
    B, H, W, C = x.shape
    Ho, Wo = offset.shape[1], offset.shape[2]
    K, gs = kernel[0] * kernel[1], C // dg
    g5 = from_cols(dcol, B, Ho, Wo, K)
    d_off = torch.zeros(B, Ho, Wo, dg, K, 2, dtype=dtype, device=x.device)
    d_m = torch.zeros(B, Ho, Wo, dg, K, dtype=dtype, device=x.device)
    for k, inside, lh, lw, (v1, v2, v3, v4) in _taps(x, offset, kernel, stride, padding, dilation, dg, dtype):
        gc = g5[..., k, :]
        gm = gc * _mask_of(mask, k, K, gs) if mask is not None else gc
        zero = torch.zeros_like(gc)
        th = torch.where(inside, gm * ((1 - lw) * (v3 - v1) + lw * (v4 - v2)), zero)
        tw = torch.where(inside, gm * ((1 - lh) * (v2 - v1) + lh * (v4 - v3)), zero)
        tm = torch.where(inside, gc * ((1 - lh) * (1 - lw) * v1 + (1 - lh) * lw * v2 + lh * (1 - lw) * v3 + lh * lw * v4), zero)
        d_off[..., k, 0] = _sum_last(th.view(B, Ho, Wo, dg, gs), order)
        d_off[..., k, 1] = _sum_last(tw.view(B, Ho, Wo, dg, gs), order)
        d_m[..., k] = _sum_last(tm.view(B, Ho, Wo, dg, gs), order)
    return d_off.view(B, Ho, Wo, dg * 2 * K), (d_m.view(B, Ho, Wo, dg * K) if mask is not None else None)


def contract(cols, w, bias=None):
    """cols [groups, rows, K*Cg], OHWI w [Cout,kh,kw,Cg] (float64) -> [rows, Cout]: the grouped contraction, then the bias"""
    groups = cols.shape[0]
    Cog = w.shape[0] // groups
    y = torch.cat([cols[g] @ w[g * Cog:(g + 1) * Cog].reshape(Cog, -1).t() for g in range(groups)], -1)
    return y if bias is None else y + bias


def deform_conv_ref(x, offset, mask, w, bias, kernel, stride, padding, dilation, groups, dg):
    """the whole op in float64 -> y [B,Ho,Wo,Cout]"""
    cols = deform_cols_general_ref(x, offset, mask, kernel, stride, padding, dilation, groups, dg)
    return contract(cols, w, bias).view(offset.shape[0], offset.shape[1], offset.shape[2], w.shape[0])


# ------------------------------------------------------------------------------------------------------------------------------ the bounds
def kernel_bounds(d, c, dcol=None, dcol_tol=None):
    """float64 reference values and bounds of the two kernels on inputs d (make_inputs, any device):
    -> dict cols, cols_tol, dx, dx_tol, d_offset, d_offset_tol, d_mask, d_mask_tol (the last two None without a mask).
    dcol: the columns' gradient (default d["dcol"]); dcol_tol: how far the kernel's own dcol may be from it (the whole op, whose dcol comes
    out of a contraction) -- every backward bound is linear in |dcol| with coefficients >= 0, so the two compose."""
    g = geom(c)
    x64 = d["x"].double().requires_grad_(True)
    off64 = d["offset"].double().requires_grad_(True)
    m64 = None if d["mask"] is None else d["mask"].double().requires_grad_(True)
    dcol = (d["dcol"] if dcol is None else dcol).double()
    slack = torch.zeros_like(dcol) if dcol_tol is None else dcol_tol
    ref, absv = deform_cols_general_ref(x64, off64, m64, want_abs=True, **g)
    mabs = None if m64 is None else m64.detach().abs()
    r = {"cols": ref.detach(), "absv": absv}
    r["cols_tol"] = (COLS_C if m64 is None else COLS_MASK_C) * U * deform_cols_general_ref(d["x"].double().abs(), d["offset"].double(), mabs, **g) + 1e-38
    grads = torch.autograd.grad(ref, (x64, off64) + (() if m64 is None else (m64,)), dcol)
    r["dx"], r["d_offset"], r["d_mask"] = grads[0], grads[1], (grads[2] if m64 is not None else None)
    xa = d["x"].double().requires_grad_(True)
    dx_abs, = torch.autograd.grad(deform_cols_general_ref(xa, d["offset"].double(), mabs, **g), (xa,), DX_C * U * (dcol.abs() + slack) + slack)
    r["dx_tol"] = dx_abs + 1e-38
    B, Ho, Wo = d["offset"].shape[:3]
    K, gs = c.kernel[0] * c.kernel[1], c.C // c.dg

    def S(a):       # sum over each deformable group's channels of a * sum|v| -> [B,Ho,Wo,dg,K]
        return from_cols(a * absv, B, Ho, Wo, K).view(B, Ho, Wo, K, c.dg, gs).sum(-1).permute(0, 1, 2, 4, 3)

    tol_m = (gs + COORD_C) * U * S(dcol.abs() + slack) + S(slack)
    tol_o = tol_m if mabs is None else tol_m * mabs.view(B, Ho, Wo, c.dg, K)
    r["d_offset_tol"] = tol_o.unsqueeze(-1).expand(B, Ho, Wo, c.dg, K, 2).reshape(B, Ho, Wo, c.dg * 2 * K) + 1e-38
    r["d_mask_tol"] = None if m64 is None else tol_m.reshape(B, Ho, Wo, c.dg * K) + 1e-38
    return r


def contraction_tol(A, B):
    """the project's bound on a contraction A [M,K] @ B [N,K]^T run by the conv entry points in any of the fp32-accurate arithmetics
    (tests/test_gpu_ops.py, tests/test_gpu_f16x3_admission.py): 8 U sum|a||b|, plus f16x3's absolute floor of 2^-39 amax per element"""
    A, B = A.abs(), B.abs()
    return CONV_C * U * (A @ B.t()) + CONV_FLOOR * (A.max() * B.sum(1)[None, :] + B.amax(1)[None, :] * A.sum(1)[:, None])


def op_bounds(d, c, with_bias):
    """float64 reference values and bounds of the whole op on inputs d: the output and the five gradients for the upstream gradient d["gy"].
    The column bound composed with the contraction bound: y sees the kernel's columns (cols_tol) through |w|; dcol is a contraction of gy
    with w, and dx / d_offset / d_mask take it through kernel_bounds(dcol_tol=); dw is a contraction of gy with the kernel's columns; db
    is a sum of B*Ho*Wo addends in an order the test does not know (U times the addend count times sum|gy|)."""
    w, gy = d["w"].double(), d["gy"].double()
    bias = d["bias"].double() if with_bias else None
    groups, Cout = c.groups, c.Cout
    Cog = Cout // groups
    rows = gy.shape[0] * gy.shape[1] * gy.shape[2]
    gy2 = gy.reshape(rows, Cout)
    kb = kernel_bounds(d, c)
    cols, cols_tol = kb["cols"], kb["cols_tol"]
    r = {"y": contract(cols, w, bias).view(gy.shape)}
    y_tol, dcol, dcol_tol, dw, dw_tol = [], [], [], [], []
    for g in range(groups):
        Wg, gyg = w[g * Cog:(g + 1) * Cog].reshape(Cog, -1), gy2[:, g * Cog:(g + 1) * Cog]
        seen = cols[g].abs() + cols_tol[g]                      # what the kernel's columns may be, in magnitude
        y_tol.append(contraction_tol(seen, Wg) + cols_tol[g] @ Wg.abs().t())
        dcol.append(gyg @ Wg)
        dcol_tol.append(contraction_tol(gyg, Wg.t()))
        dw.append(gyg.t() @ cols[g])
        dw_tol.append(contraction_tol(gyg.t(), seen.t()) + gyg.abs().t() @ cols_tol[g])
    r["y_tol"] = torch.cat(y_tol, -1).view(gy.shape) + U * r["y"].abs() + 1e-38
    r["dw"] = torch.cat(dw, 0).view(w.shape)
    r["dw_tol"] = torch.cat(dw_tol, 0).view(w.shape) + 1e-38
    r["db"], r["db_tol"] = gy2.sum(0), rows * U * gy2.abs().sum(0) + 1e-38
    back = kernel_bounds(d, c, torch.stack(dcol), torch.stack(dcol_tol))
    for k in ("dx", "dx_tol", "d_offset", "d_offset_tol", "d_mask", "d_mask_tol"):
        r[k] = back[k]
    return r


def worst_ratio(got, want, tol):
    return float(((got.double() - want).abs() / tol).max())


def sample_points(offset, c, dtype):
    """(h, w) [B,Ho,Wo,dg,K] of every sample, the base and the one add in `dtype`"""
    B, Ho, Wo = offset.shape[:3]
    K = c.kernel[0] * c.kernel[1]
    off = offset.to(dtype).view(B, Ho, Wo, c.dg, K, 2)
    k = torch.arange(K)
    i, j = (k // c.kernel[1]).view(1, 1, 1, 1, K), (k % c.kernel[1]).view(1, 1, 1, 1, K)
    ho = torch.arange(Ho).view(1, Ho, 1, 1, 1) * c.stride[0] - c.padding[0]
    wo = torch.arange(Wo).view(1, 1, Wo, 1, 1) * c.stride[1] - c.padding[1]
    return (ho + i * c.dilation[0]).to(dtype) + off[..., 0], (wo + j * c.dilation[1]).to(dtype) + off[..., 1]


def near_share(d, c, eps):
    """share of the samples with a coordinate within eps of an integer, and share outside the open box"""
    near = out = n = 0
    for _, inside, lh, lw, _ in _taps(d["x"].double(), d["offset"].double(), c.kernel, c.stride, c.padding, c.dilation, c.dg):
        near += int((((lh < eps) | (lh > 1 - eps) | (lw < eps) | (lw > 1 - eps)) & inside).sum())
        out += int((~inside).sum())
        n += inside.numel()
    return near / n, out / n

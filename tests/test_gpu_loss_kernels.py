"""The loss / distillation / optimiser kernels against float64 references of the same operation, at the edges the model's own shapes never
reach: empty and tiny inputs, grids past their cap (grid-stride loops, many-workgroup deterministic sums), -1 padded index lists and device
denominators, pitched inputs and gradient slices, K from 1 to 128, n_old at both ends, both ARD layouts, extreme logits, determinism.

Tolerances follow one rule.  A loss is bounded by TOL * (sum of |the addends that formula sums|) rather than by the result, so that a
result made small by cancellation still gets a bound of the size of its rounding error; every bound below is at least 10x smaller than
dropping or double-counting one term at n ~ 2000 (checked where that n is used, see `_check_sanity`).  A gradient element is bounded by a
few fp32 ulps of the largest addend of its row (for a softmax: scaled by the magnitude of the logits, whose rounding sets the exponent's
error).  Columns outside a kernel's range are filled with a sentinel and must come back unchanged.
"""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)
TOL = 1e-6                 # relative to the sum of |addends| (about 8 fp32 ulps)
SENT = -12345.0            # sentinel of the gradient columns a kernel must not write


@pytest.fixture(scope="module")
def R():
    from oracle import torch_ref
    return torch_ref


@pytest.fixture(scope="module")
def ops():
    from abr_iod_amd import ops as o
    return o


def f64(t):
    return t.detach().cpu().double()


def _check_loss(got, ref, addends, what):
    bound = TOL * addends
    assert math.isfinite(got), f"{what}: loss {got} is not finite (want {ref})"
    assert abs(got - ref) <= bound, f"{what}: loss {got!r} vs float64 {ref!r}: |d| = {abs(got - ref):.3e} > {bound:.3e}"
    return bound


def _check_sanity(bound, row_terms, n, what):
    """the loss bound must be 10x below the change that dropping (or double-counting) one median term of n would make"""
    assert 10 * bound < float(np.median(np.abs(row_terms))) / n, f"{what}: bound {bound:.3e} would not see one term of {n} missing"


def _check_grad(got, ref, row_scale, what):
    """got / ref [n, K] (float64 on the CPU); row_scale [n]: a few ulps' worth of the row's largest addend"""
    assert torch.isfinite(got).all(), f"{what}: non-finite gradient"
    err = (got - ref).abs()
    tol = row_scale.reshape(-1, *([1] * (err.dim() - 1)))
    bad = err > tol
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{what}: gradient at {i}: {got[i].item()!r} vs float64 {ref[i].item()!r} (tol {tol.flatten()[i[0]].item():.3e}); "
                             f"{int(bad.sum())} elements out of bound")


def _pitched(n, K, extra, fill=SENT):
    """a [n, K + extra] buffer of `fill` and its [:, :K] column slice (rows contiguous, pitch K + extra)"""
    buf = torch.full((n, K + extra), fill, dtype=torch.float32, device="cuda")
    return buf, buf[:, :K]


# ================================================================================================== softmax_ce (plain and inclusive "id")
def ce_ref(R, z, labels, inclusive, n_old):
    """float64 mean loss, d loss / d z, per-row addend magnitudes (max |z| + |lse|) and the rows' counted flags, through
    oracle.torch_ref.box_head_loss on the counted rows (label < 0 rows are ignored; all ignored -> loss 0, gradient 0)"""
    z64, lab = f64(z), labels.cpu()
    valid = lab >= 0
    grad = torch.zeros_like(z64)
    lse = torch.logsumexp(z64, dim=1)
    addends = z64.abs().amax(dim=1) + lse.abs()
    if not bool(valid.any()):
        return 0.0, grad, addends, valid
    zv = z64[valid].clone().requires_grad_(True)
    nv, K = zv.shape
    cls, _ = R.box_head_loss(zv, torch.zeros(nv, 4 * K, dtype=torch.float64), lab[valid], torch.zeros(nv, 4, dtype=torch.float64),
                             dist_type="id" if inclusive else "l2", n_old=n_old)
    cls.backward()
    grad[valid] = zv.grad
    return cls.item(), grad, addends, valid


def run_ce(ops, R, z, labels, inclusive, n_old, gscale=1.0, extra=0, what=""):
    n, K = z.shape
    buf, gview = _pitched(n, K, extra)
    loss, g = ops.softmax_ce(z, labels, inclusive=inclusive, n_old=n_old, gscale=gscale, want_grad=True, grad_out=gview)
    ref, gref, addends, valid = ce_ref(R, z, labels, inclusive, n_old)
    nv = max(int(valid.sum()), 1)
    bound = _check_loss(loss[0].item(), ref, float(addends[valid].sum()) / nv if valid.any() else 0.0, what)
    # the gradient row's addends are softmax terms <= 1 (times gscale / n_valid); their exponents carry the logits' rounding
    zmax = f64(z).abs().amax(dim=1) + addends
    scale = abs(gscale) / nv * EPS * (8 + 2 * zmax) * valid.double()
    _check_grad(f64(g), gscale * gref, scale, what)
    if extra:
        assert torch.all(buf[:, K:] == SENT), f"{what}: columns past K were written"
    return bound, addends[valid].numpy()


@pytest.mark.parametrize("K", [1, 2, 7, 8, 9, 16, 21, 81, 128])
def test_softmax_ce_plain_every_width(ops, R, K):
    g = torch.Generator().manual_seed(K)
    for n in (1, 3, 37, 2001):
        z = (3 * torch.randn(n, K, generator=g)).cuda()
        labels = torch.randint(0, K, (n,), generator=g).cuda()
        bound, _ = run_ce(ops, R, z, labels, False, 0, extra=5 if n > 1 else 0, what=f"plain K={K} n={n}")
        if n == 2001 and K > 1:   # (K = 1: every term is exactly 0)
            lse = torch.logsumexp(f64(z), 1)
            _check_sanity(bound, (lse - f64(z).gather(1, labels.cpu()[:, None])[:, 0]).numpy(), n, f"plain K={K}")


@pytest.mark.parametrize("K", [2, 7, 9, 21, 81, 128])
def test_softmax_ce_inclusive_n_old_and_label_classes(ops, R, K):
    """n_old at 0, in between and at K-1; labels 0, within 1..n_old and above n_old (where they exist) in every case"""
    g = torch.Generator().manual_seed(100 + K)
    for n_old in sorted({0, K // 2, K - 1}):
        n = 2003
        z = (2.5 * torch.randn(n, K, generator=g)).cuda()
        lab = torch.randint(0, K, (n,), generator=g)
        lab[0] = 0
        lab[1] = min(1, n_old) if n_old >= 1 else 0
        lab[2] = K - 1
        run_ce(ops, R, z, lab.cuda(), True, n_old, gscale=0.37, extra=3, what=f"inclusive K={K} n_old={n_old}")


def test_softmax_ce_ignored_rows(ops, R):
    g = torch.Generator().manual_seed(7)
    n, K = 515, 21
    z = torch.randn(n, K, generator=g).cuda()
    lab = torch.randint(0, K, (n,), generator=g)
    lab[::3] = -1
    for inclusive in (False, True):
        run_ce(ops, R, z, lab.cuda(), inclusive, 15, extra=4, what=f"ignored rows inclusive={inclusive}")
        # all ignored: the header's contract (rows ignored) gives 0 and a zero gradient, not the NaN of an empty mean
        buf, gview = _pitched(n, K, 4)
        loss, _ = ops.softmax_ce(z, torch.full((n,), -1, dtype=torch.int64, device="cuda"), inclusive=inclusive, n_old=15, want_grad=True,
                                 grad_out=gview)
        assert loss[0].item() == 0.0
        assert torch.all(buf[:, :K] == 0) and torch.all(buf[:, K:] == SENT)


def test_softmax_ce_empty(ops):
    buf = torch.full((4, 21), SENT, device="cuda")
    loss, _ = ops.softmax_ce(torch.empty(0, 21, device="cuda"), torch.empty(0, dtype=torch.int64, device="cuda"), inclusive=True, n_old=15,
                             want_grad=True, grad_out=buf[:0])
    assert loss[0].item() == 0.0
    assert torch.all(buf == SENT)


def test_softmax_ce_extreme_logits(ops, R):
    """the inclusive background term lse(z[0..n_old]) with the old-class slice far below a new class: the slice's own maximum must shift
    it (exp(z - row max) of the slice is 0 in fp32 once the gap passes ~88-104); and all-equal rows at +-80"""
    K, n_old = 21, 15
    z = torch.zeros(6, K)
    z[0, :16] = -120.0                     # the issue's case: loss 118.84, not inf; gradient finite
    z[1, :16] = -95.0
    z[1, 3] = -90.0
    z[2, :16] = -300.0 + torch.arange(16.0)
    z[3, :] = 80.0
    z[4, :] = -80.0
    z[5, :16] = -70.0                      # 70 below: the rescaled path's near side
    labels = torch.tensor([0, 0, 0, 0, 0, 17])
    run_ce(ops, R, z.cuda(), labels.cuda(), True, n_old, extra=3, what="extreme inclusive")
    # and each such row alone (no averaging with ordinary rows), label 0 and a new class
    for r in range(5):
        for lab in (0, 18):
            run_ce(ops, R, z[r:r + 1].cuda(), torch.tensor([lab]).cuda(), True, n_old, what=f"extreme inclusive row {r} label {lab}")
    run_ce(ops, R, z.cuda(), torch.tensor([0, 3, 20, 7, 0, 1]).cuda(), False, 0, extra=3, what="extreme plain")


# ================================================================================================== roi_distill (id and l2)
def rd_ref(R, zs, bs, zt, bt, dist_id):
    zt64 = f64(zt).requires_grad_(True)
    bt64 = f64(bt).requires_grad_(True)
    loss = R.roi_distillation_loss(f64(zs), f64(bs), zt64, bt64, dist="id" if dist_id else "l2")
    loss.backward()
    return loss.item(), zt64.grad, bt64.grad


def run_rd(ops, R, zs, bs, zt, bt, dist_id, gscale=1.0, extra=0, what=""):
    """zs [n,K_old], bs [n,K_old,4], zt [n,K_all], bt [n,K_all,4] (contiguous); with extra > 0 every one of them is passed as a column
    slice of a wider buffer and the gradients go into column slices of sentinel-filled buffers"""
    n, K_old = zs.shape
    K_all = zt.shape[1]
    args = [zs, bs.reshape(n, -1), zt, bt.reshape(n, -1)]
    if extra:
        wide = []
        for a in args:
            buf = torch.randn(n, a.shape[1] + extra, device="cuda")
            buf[:, :a.shape[1]] = a
            wide.append(buf[:, :a.shape[1]])
        args = wide
    gz_buf, gz = _pitched(n, K_all, extra)
    gb_buf, gb = _pitched(n, 4 * K_all, extra)
    loss, dzt, dbt = ops.roi_distill(*args, dist_id=dist_id, gscale=gscale, want_grad=True, d_zt=gz, d_bt=gb)
    ref, gz_ref, gb_ref = rd_ref(R, zs, bs, zt, bt, dist_id)
    zs64, zt64, bs64, bt64 = f64(zs), f64(zt), f64(bs), f64(bt)
    box2 = ((bt64[:, 1:K_old] - bs64[:, 1:]) ** 2).sum(2)
    box_add = box2.sum(1) / max(K_old - 1, 1)
    zmax = zs64.abs().amax(1) + zt64.abs().amax(1)
    if dist_id:   # addends: lab_c * (z_t[c] - den) and lab_0 * (lse_bg - den): bounded by max|z_t| + |den| + |lse_bg|
        den = torch.logsumexp(zt64, 1)
        bg = torch.logsumexp(zt64[:, [0] + list(range(K_old, K_all))], 1)
        cls_add = zt64.abs().amax(1) + den.abs() + bg.abs()
        gsc = EPS * (8 + 2 * (zmax + den.abs())) / (n * K_old)
    else:         # addends: d_c^2 and the rounding of d_c = (zt - mean zt) - (zs - mean zs) it carries
        d = (zt64[:, :K_old] - zt64.mean(1, keepdim=True)) - (zs64 - zs64.mean(1, keepdim=True))
        cls_add = (d * d + 2 * d.abs() * (zs64.abs() + zt64[:, :K_old].abs() + zmax[:, None])).sum(1) / K_old
        gsc = EPS * 16 * (2 * zmax + d.abs().amax(1) + 1) / (n * K_old)
    addends = float((cls_add + box_add).sum()) / n + float((2 * box2.sqrt() * (bt64[:, 1:K_old].abs() + bs64[:, 1:].abs()).sum(2)).sum()) / n / max(K_old - 1, 1)
    bound = _check_loss(loss[0].item(), ref, addends, what)
    _check_grad(f64(dzt), gscale * gz_ref, abs(gscale) * gsc, what + " d_zt")
    bsc = 2 * abs(gscale) / (n * max(K_old - 1, 1)) * 8 * EPS * (bt64.abs() + torch.cat([bs64, torch.zeros(n, K_all - K_old, 4, dtype=torch.float64)], 1).abs())
    err = (f64(dbt).reshape(n, K_all, 4) - gscale * gb_ref).abs()
    assert torch.isfinite(f64(dbt)).all() and torch.all(err <= bsc), f"{what} d_bt: max err {err.max().item():.3e}"
    if extra:
        assert torch.all(gz_buf[:, K_all:] == SENT) and torch.all(gb_buf[:, 4 * K_all:] == SENT), f"{what}: columns past the slice were written"
    return bound, (cls_add, box2.sum(1) / max(K_old - 1, 1))


def _rd_data(g, n, K_old, K_all, s=2.0):
    return (s * torch.randn(n, K_old, generator=g)).cuda(), torch.randn(n, K_old, 4, generator=g).cuda(), \
           (s * torch.randn(n, K_all, generator=g)).cuda(), torch.randn(n, K_all, 4, generator=g).cuda()


@pytest.mark.parametrize("K_all", [3, 21, 81, 128])
@pytest.mark.parametrize("dist_id", [True, False])
def test_roi_distill_shapes(ops, R, K_all, dist_id):
    g = torch.Generator().manual_seed(K_all * 2 + dist_id)
    for K_old in sorted({2, K_all // 2 + 1, K_all - 1}):
        for n in (1, 17, 2003):
            zs, bs, zt, bt = _rd_data(g, n, K_old, K_all)
            bound, _ = run_rd(ops, R, zs, bs, zt, bt, dist_id, gscale=0.61, extra=3 if n > 1 else 0, what=f"roi_distill id={dist_id} "
                              f"K_old={K_old} K_all={K_all} n={n}")
            if n == 2003 and not dist_id:
                # the l2 loss's own per-RoI terms (d^2 mean + box); the id loss's terms are checked in the extreme test's rows
                zs64, zt64 = f64(zs), f64(zt)
                d = (zt64[:, :K_old] - zt64.mean(1, keepdim=True)) - (zs64 - zs64.mean(1, keepdim=True))
                _check_sanity(bound, (d * d).mean(1).numpy(), n, f"roi_distill l2 K_old={K_old}")


def test_roi_distill_empty_and_dense(ops, R):
    zs = torch.empty(0, 16, device="cuda")
    gz = torch.full((3, 21), SENT, device="cuda")
    gb = torch.full((3, 84), SENT, device="cuda")
    loss, _, _ = ops.roi_distill(zs, torch.empty(0, 64, device="cuda"), torch.empty(0, 21, device="cuda"), torch.empty(0, 84, device="cuda"),
                                 dist_id=True, want_grad=True, d_zt=gz[:0], d_bt=gb[:0])
    assert loss[0].item() == 0.0 and torch.all(gz == SENT) and torch.all(gb == SENT)


def test_roi_distill_extreme_logits(ops, R):
    """id branch: an old-class target logit 120 above every background logit (0 and K_old..K_all-1): the background set's
    lse must be shifted by its own maximum; and ties at +-80"""
    K_old, K_all = 16, 21
    g = torch.Generator().manual_seed(5)
    zs, bs, zt, bt = _rd_data(g, 5, K_old, K_all)
    zt = zt.cpu()
    zt[0] = 0.0
    zt[0, 5] = 120.0
    zt[1] = -40.0
    zt[1, 1:K_old] = 60.0 + torch.arange(K_old - 1.0)
    zt[2] = 80.0
    zt[3] = -80.0
    zt[4, 0] = -250.0
    zt[4, 7] = 0.0
    zs = zs.cpu()
    zs[2] = 80.0
    zs[3] = -80.0
    run_rd(ops, R, zs.cuda(), bs, zt.cuda(), bt, True, extra=2, what="roi_distill id extreme")
    for r in range(5):
        run_rd(ops, R, zs[r:r + 1].cuda(), bs[r:r + 1], zt[r:r + 1].cuda(), bt[r:r + 1], True, what=f"roi_distill id extreme row {r}")
        run_rd(ops, R, zs[r:r + 1].cuda(), bs[r:r + 1], zt[r:r + 1].cuda(), bt[r:r + 1], False, what=f"roi_distill l2 extreme row {r}")


# ================================================================================================== ARD
@pytest.mark.parametrize("HW", [1, 49, 1024])
@pytest.mark.parametrize("C", [64, 37])
def test_ard_layouts_and_gamma(ops, R, HW, C):
    """NHWC with C % 4 == 0 is the VEC4 path; C % 4 != 0 and NCHW the strided one.  Both layouts, gamma 0 / 1 / 5"""
    from abr_iod_amd import _lib
    g = torch.Generator().manual_seed(HW * 131 + C)
    N = 3
    fs = torch.randn(N, C, HW, generator=g)
    ft = fs + 0.4 * torch.randn(N, C, HW, generator=g)
    _ard_case(ops, R, _lib, fs, ft, f"HW={HW} C={C}")


def test_ard_large_features(ops, R):
    """features whose per-position mean square spans more than 88 across HW: the HW softmax in fp32 must stay finite and match"""
    from abr_iod_amd import _lib
    g = torch.Generator().manual_seed(11)
    N, C, HW = 2, 24, 49
    amp = torch.linspace(0.1, 11.0, HW)                        # mean_c F^2 from ~0.01 to ~121
    fs = torch.randn(N, C, HW, generator=g)
    fs = fs / fs.pow(2).mean(1, keepdim=True).sqrt() * amp
    ft = fs * (1 + 0.05 * torch.randn(N, C, HW, generator=g))
    _ard_case(ops, R, _lib, fs, ft, "large features")


def _ard_case(ops, R, _lib, fs, ft, what):
    N, C, HW = fs.shape
    fs64, ft64 = fs.double(), ft.double()
    m = torch.maximum(fs64.pow(2).mean(1), ft64.pow(2).mean(1))
    cond = 1 + float(m.max())                   # the exponents' magnitude: their rounding sets the attention maps' error
    for gamma in (0.0, 1.0, 5.0):
        ft_req = ft64.clone().requires_grad_(True)
        ref = R.ard_loss(fs64.reshape(N, C, HW, 1), ft_req.reshape(N, C, HW, 1), gamma)
        ref.backward()
        a_s = R.attention_map(fs64.reshape(N, C, HW, 1)).reshape(N, 1, HW)
        afd_add = float((a_s * (fs64 - ft64) ** 2).mean())
        addends = (afd_add + gamma * 2.0) * cond          # pad = mean |A_t - A_s| with A_t, A_s each of mean 1
        gmax = ft_req.grad.abs().amax()
        for layout in ("nhwc", "nchw"):
            if layout == "nhwc":
                a, b = fs.permute(0, 2, 1).contiguous().cuda(), ft.permute(0, 2, 1).contiguous().cuda()
                lay = _lib.NHWC
            else:
                a, b = fs.reshape(N, C, HW, 1).cuda(), ft.reshape(N, C, HW, 1).cuda()
                lay = _lib.NCHW
            loss, coef = ops.ard_forward(a, b, gamma, layout=lay)
            tag = f"ard {what} {layout} gamma={gamma}"
            _check_loss(loss[0].item(), ref.item(), 16 * addends, tag)
            assert abs(loss[1].item() + gamma * loss[2].item() - loss[0].item()) <= 4 * EPS * abs(loss[0].item()) + 1e-30
            gr = ops.ard_backward(a, b, coef, gamma, gscale=0.5, layout=lay)
            gr = f64(gr.permute(0, 2, 1) if layout == "nhwc" else gr.reshape(N, C, HW))
            tol = 64 * EPS * cond * 0.5 * float(gmax) + 1e-30
            _check_grad(gr.reshape(N, -1), 0.5 * ft_req.grad.reshape(N, -1), torch.full((N,), tol, dtype=torch.float64), tag)


def test_ard_empty(ops):
    loss, coef = ops.ard_forward(torch.empty(0, 49, 64, device="cuda"), torch.empty(0, 49, 64, device="cuda"), 1.0)
    assert torch.all(loss[:3] == 0)
    assert ops.ard_backward(torch.empty(0, 49, 64, device="cuda"), torch.empty(0, 49, 64, device="cuda"), coef, 1.0).numel() == 0


# ================================================================================================== smooth_l1 / smooth_l1_rows
def sl1_ref(d, beta):
    a = d.abs()
    return torch.where(a < beta, 0.5 * a * a / beta, a - 0.5 * beta), torch.where(a < beta, d / beta, torch.sign(d))


@pytest.mark.parametrize("n", [0, 1, 5, 1027, 2001, 1024 * 256 * 2 + 37])
def test_smooth_l1(ops, n):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    t = torch.randn(n, generator=g)
    for beta, scale, gscale in ((1.0 / 9, 1.0, 1.0), (1.0, 1.0 / max(n, 1), 0.3)):
        loss, grad = ops.smooth_l1(x.cuda(), t.cuda(), beta, scale=scale, gscale=gscale, want_grad=True)
        d = x.double() - t.double()
        val, gr = sl1_ref(d, beta)
        # addends: each term and the rounding of d = x - t it carries
        add = float((val + (x.double().abs() + t.double().abs()) * torch.where(d.abs() < beta, d.abs() / beta, torch.ones_like(d))).sum()) * scale
        bound = _check_loss(loss[0].item(), float(val.sum()) * scale, add, f"smooth_l1 n={n} beta={beta}")
        if n == 2001:
            _check_sanity(bound, (val * scale).numpy(), 1, f"smooth_l1 beta={beta}")
        if n:
            want = gr * gscale * scale
            tol = 4 * EPS * abs(gscale * scale) * (1 + (x.double().abs() + t.double().abs()) / beta)
            assert torch.all((f64(grad) - want).abs() <= tol), f"smooth_l1 n={n}: gradient"


def test_smooth_l1_rows_padding_and_denominator(ops):
    """rows[i] = -1 entries are skipped; denom_dev replaces the scale's denominator (max(*denom, 1)); 4 columns at col0 of a wide row"""
    g = torch.Generator().manual_seed(3)
    nr, cols = 1003, 84
    x = torch.randn(nr, cols, generator=g)
    t = torch.randn(700, 4, generator=g)
    rows = torch.randperm(nr, generator=g)[:700]          # distinct rows: each gradient element written once
    col0 = 4 * torch.randint(0, cols // 4, (700,), generator=g)
    rows_p = rows.clone()
    rows_p[::7] = -1
    for denom in (None, 0.0, 517.0):
        dd = None if denom is None else torch.tensor([denom], device="cuda")
        scale = 1.0 if denom is None else 2.0
        loss, grad = ops.smooth_l1_rows(x.cuda(), t.cuda(), rows_p.cuda(), col0.cuda(), 1.0 / 9, scale=scale, gscale=0.5, want_grad=True,
                                        trows=torch.arange(700).cuda(), denom_dev=dd)
        eff = scale / (1.0 if denom is None else max(denom, 1.0))
        keep = rows_p >= 0
        xs = x.double()[rows_p[keep][:, None], col0[keep][:, None] + torch.arange(4)]
        d = xs - t.double()[keep]
        val, gr = sl1_ref(d, 1.0 / 9)
        _check_loss(loss[0].item(), float(val.sum()) * eff, float((val + 9 * d.abs().clamp(max=1 / 9) * (xs.abs() + t.double()[keep].abs())).sum()) * eff,
                    f"smooth_l1_rows denom={denom}")
        want = torch.zeros(nr, cols, dtype=torch.float64)
        want[rows_p[keep][:, None], col0[keep][:, None] + torch.arange(4)] = gr * 0.5 * eff
        assert torch.all((f64(grad) - want).abs() <= 4 * EPS * 0.5 * eff * 10), f"smooth_l1_rows denom={denom}: gradient"


# ================================================================================================== bce_logits_gather
@pytest.mark.parametrize("n_idx", [0, 1, 6, 2001, 256 * 256 + 4099])
def test_bce_logits_gather(ops, n_idx):
    g = torch.Generator().manual_seed(n_idx + 1)
    n_x = max(2 * n_idx, 8)
    x = 4 * torch.randn(n_x, generator=g)
    y = (torch.rand(n_x, generator=g) > 0.5).float()
    idx = torch.randperm(n_x, generator=g)[:n_idx]
    for pad, denom in ((False, None), (True, None), (True, 0.0), (True, 123.0)):
        ip = idx.clone()
        if pad and n_idx:
            ip[1::5] = -1
        dd = None if denom is None else torch.tensor([denom], device="cuda")
        loss, grad = ops.bce_logits_gather(x.cuda(), y.cuda(), ip.cuda(), gscale=0.7, want_grad=True, denom_dev=dd)
        tag = f"bce n_idx={n_idx} pad={pad} denom={denom}"
        if n_idx == 0:
            assert loss[0].item() == 0.0 and torch.all(grad == 0), tag
            continue
        # the header's contract: the mean's denominator is n_idx (padding included) unless denom_dev gives it
        inv = 1.0 / (n_idx if denom is None else max(denom, 1.0))
        k = ip[ip >= 0]
        xv, yv = x.double()[k], y.double()[k]
        val = torch.nn.functional.binary_cross_entropy_with_logits(xv, yv, reduction="none")
        bound = _check_loss(loss[0].item(), float(val.sum()) * inv, float((val + xv.abs() + 1).sum()) * inv, tag)
        if n_idx == 2001 and not pad:
            _check_sanity(bound, (val * inv).numpy(), 1, tag)
        want = torch.zeros(n_x, dtype=torch.float64)
        want[k] = (torch.sigmoid(xv) - yv) * inv * 0.7
        assert torch.all((f64(grad) - want).abs() <= 8 * EPS * 0.7 * inv), tag + ": gradient"


# ================================================================================================== feat_distill / rpn_distill
def _away_from_zero(g, shape, margin=0.05):
    """differences d with |d - mean d| >= margin / 2: no element of max(d, 0) sits near its kink (fp32 vs float64 masks agree)"""
    s = torch.where(torch.rand(shape, generator=g) < 0.5, -1.0, 1.0)
    return s * (margin + 0.5 * torch.rand(shape, generator=g))


@pytest.mark.parametrize("shape", [(0,), (1,), (7,), (2001,), (2048 * 256 * 2 + 5,), (4, 1024, 38, 63)])
def test_feat_distill(ops, R, shape):
    g = torch.Generator().manual_seed(sum(shape))
    n = math.prod(shape)
    t = torch.randn(shape, generator=g)
    delta = _away_from_zero(g, shape)
    while n > 1 and (delta.double() - delta.double().mean()).abs().min() < 0.02:    # (small n: redraw until no difference sits at the kink)
        delta = _away_from_zero(g, shape)
    s = t + delta
    loss, d = ops.feat_distill(s.cuda(), t.cuda(), want_grad=True)
    if n == 0:
        assert loss[0].item() == 0.0
        return
    tq = t.double().requires_grad_(True)
    ref = R.feature_distillation_loss([s.double()], [tq])
    ref.backward()
    diff = (s.double() - s.double().mean()) - (tq.detach() - tq.detach().mean())
    assert n == 1 or diff.abs().min() > 0.01          # no subgradient ties (n = 1: d = 0 exactly in both, and so is the gradient)
    pos = diff.clamp(min=0)
    bound = _check_loss(loss[0].item(), ref.item(), float((pos + (diff > 0) * (s.double().abs() + t.double().abs() + 1)).sum()) / n, f"feat n={n}")
    if n == 2001:
        _check_sanity(bound, pos[pos > 0].numpy() / n, 1, "feat")
    assert torch.all((f64(d) - tq.grad).abs() <= 4 * EPS / n), f"feat n={n}: gradient"


def _rpn_views(t, extra):
    """NHWC [N,H,W,c] -> a row-strided view into a [N,H,W,c+extra] buffer (as the fused head output's column slices are)"""
    if not extra:
        return t.cuda()
    buf = torch.randn(*t.shape[:3], t.shape[3] + extra).cuda()
    buf[..., :t.shape[3]] = t.cuda()
    return buf[..., :t.shape[3]]


@pytest.mark.parametrize("N,H,W,A,extra", [(0, 5, 5, 15, 0), (1, 1, 1, 1, 0), (1, 9, 15, 15, 61), (2, 38, 50, 15, 61),
                                           (4, 38, 63, 15, 0), (2, 200, 200, 15, 0)])
def test_rpn_distill(ops, R, N, H, W, A, extra):
    g = torch.Generator().manual_seed(N * 1000 + H + A)
    thr = 0.1
    ot = torch.randn(N, H, W, A, generator=g)
    diff = _away_from_zero(g, (N, H, W, A))
    diff = torch.where((diff - thr).abs() < 0.02, diff + 0.05, diff)        # nor near the bbox threshold
    os_ = ot + diff
    rt = torch.randn(N, H, W, 4 * A, generator=g)
    rs = rt + 0.3 * torch.randn(N, H, W, 4 * A, generator=g)
    for use_bbox in (True, False):
        tag = f"rpn N={N} H={H} W={W} A={A} extra={extra} bbox={use_bbox}"
        loss, go, gr = ops.rpn_distill(_rpn_views(os_, extra), _rpn_views(rs, extra), _rpn_views(ot, 2 * extra), _rpn_views(rt, extra), thr,
                                       use_bbox, want_grad=True)
        if N == 0:
            assert loss[0].item() == 0.0, tag
            continue
        otq = ot.double().requires_grad_(True)
        rtq = rt.double().requires_grad_(True)
        nchw = lambda v: v.permute(0, 3, 1, 2)                                   # noqa: E731
        ref = R.rpn_distillation_loss(([nchw(os_.double())], [nchw(rs.double())]), ([nchw(otq)], [nchw(rtq)]), thr,
                                      "l2" if use_bbox else "None")
        ref.backward()
        n = N * H * W * A
        d64 = os_.double() - ot.double()
        p = d64.clamp(min=0)
        m = (d64 > thr).double()[..., None]
        dd = (rs.double() - rt.double()).reshape(N, H, W, A, 4) * m * use_bbox
        ab = (rs.double().abs() + rt.double().abs()).reshape(N, H, W, A, 4)
        add = float((p * p + 2 * p * (os_.double().abs() + ot.double().abs())).sum() + (dd * dd + 2 * dd.abs() * ab).sum()) / n
        bound = _check_loss(loss[0].item(), ref.item(), add, tag)
        if n == 9 * 15 * 15:
            terms = p * p + (dd * dd).sum(-1)
            _check_sanity(bound, terms[p > 0].numpy(), n, tag)
        assert torch.all((f64(go) - otq.grad).abs() <= 4 * EPS * (p + os_.double().abs() + ot.double().abs()) * 2 / n), tag + ": d_obj"
        want_r = rtq.grad if rtq.grad is not None else torch.zeros_like(rtq)
        assert torch.all((f64(gr) - want_r).abs() <= 4 * EPS * (dd.abs() + ab).reshape(N, H, W, 4 * A) * 2 / n), tag + ": d_reg"


# ================================================================================================== determinism and streams
def _calls(ops):
    g = torch.Generator().manual_seed(21)
    z = (3 * torch.randn(4099, 21, generator=g)).cuda()
    lab = torch.randint(-1, 21, (4099,), generator=g).cuda()
    zs, bs, zt, bt = _rd_data(g, 4099, 16, 21)
    x = torch.randn(1024 * 256 * 2 + 37, generator=g).cuda()
    t = torch.randn(1024 * 256 * 2 + 37, generator=g).cuda()
    idx = torch.randperm(x.numel(), generator=g)[:256 * 256 + 4099].cuda()
    y = (torch.rand(x.numel(), generator=g) > 0.5).float().cuda()
    fs = torch.randn(64, 49, 256, generator=g).cuda()
    ft = fs + 0.3 * torch.randn(64, 49, 256, generator=g).cuda()
    fm = torch.randn(2, 256, 38, 63, generator=g).cuda()

    def run():
        out = []
        for inclusive in (False, True):
            loss, gz = ops.softmax_ce(z, lab, inclusive=inclusive, n_old=15, want_grad=True)
            out += [loss[:1].clone(), gz.clone()]
        for dist_id in (False, True):
            loss, a, b = ops.roi_distill(zs, bs, zt, bt, dist_id=dist_id, want_grad=True)
            out += [loss[:1].clone(), a.clone(), b.clone()]
        loss, gx = ops.smooth_l1(x, t, 1.0 / 9, want_grad=True)
        out += [loss[:1].clone(), gx.clone()]
        loss, gx = ops.bce_logits_gather(x, y, idx, want_grad=True)
        out += [loss[:1].clone(), gx.clone()]
        loss, coef = ops.ard_forward(fs, ft, 1.0)
        out += [loss[:3].clone(), ops.ard_backward(fs, ft, coef, 1.0)]
        loss, d = ops.feat_distill(fm, fm * 0.9 + 0.1, want_grad=True)
        out += [loss.clone(), d.clone()]
        db = torch.zeros(2048, device="cuda")
        out.append(ops.bias_grad(fs.reshape(-1, 2048)[:1549], db).clone())
        return out
    return run


def test_losses_are_deterministic_and_stream_independent(ops):
    """two calls give the same bits, and so does a non-blocking side stream's first use (its deterministic-sum ring and tickets are new)"""
    run = _calls(ops)
    a = run()
    b = run()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    busy = torch.randn(4096, 4096, device="cuda")
    for _ in range(8):                 # keep the default stream busy: the side stream's first launches must not depend on its queue
        busy = (busy @ busy.T) * 1e-4
    with torch.cuda.stream(side):
        c = run()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    for i, (u, v, w) in enumerate(zip(a, b, c)):
        assert torch.isfinite(u).all(), f"output {i}: not finite"
        assert torch.equal(u, v), f"output {i}: two calls differ"
        assert torch.equal(u, w), f"output {i}: a non-default stream gives different bits"


# ================================================================================================== loss_sum, bias_grad, sgd, small ones
@pytest.mark.parametrize("n", [1, 8])
def test_loss_sum_forward_backward(ops, n):
    g = torch.Generator().manual_seed(n)
    vals = (10 * torch.randn(n, generator=g)).tolist()
    w = (torch.rand(n, generator=g) * 2).tolist()              # (both exact in fp32: the kernel takes float weights)
    groups = [i % 2 for i in range(n)] if n > 1 else [1]
    terms = [torch.tensor(v, device="cuda", requires_grad=True) for v in vals]
    total, parts = ops.loss_sum(terms, w, groups)
    ref = sum(wi * vi for wi, vi in zip(w, vals))
    g0 = sum(wi * vi for wi, vi, gi in zip(w, vals, groups) if gi == 0)
    g1 = sum(wi * vi for wi, vi, gi in zip(w, vals, groups) if gi == 1)
    add = (n + 1) * EPS / TOL * sum(abs(wi * vi) for wi, vi in zip(w, vals))    # n fp32 products and n - 1 additions
    _check_loss(total.item(), ref, add, "loss_sum total")
    p = parts.cpu().tolist()
    assert p[0] == total.item()
    _check_loss(p[1], g0, add, "loss_sum group 0")
    _check_loss(p[2], g1, add, "loss_sum group 1")
    (total * 2.5).backward()
    for i, t in enumerate(terms):
        assert abs(t.grad.item() - 2.5 * w[i]) <= 2 * EPS * abs(2.5 * w[i]), f"term {i} gradient"


@pytest.mark.parametrize("C", [1, 4, 76, 2048])
@pytest.mark.parametrize("M", [1, 255, 257, 3000])
def test_bias_grad(ops, C, M):
    """db += column sums, M not a multiple of the 256 rows a workgroup takes, C not a multiple of its 64 columns"""
    g = torch.Generator().manual_seed(C * 7 + M)
    gy = torch.randn(M, C, generator=g)
    db0 = torch.randn(C, generator=g)
    want = db0.double() + gy.double().sum(0)
    db = db0.cuda()
    ops.bias_grad(gy.cuda(), db)
    tol = 4 * EPS * (db0.double().abs() + gy.double().abs().sum(0)) + 1e-30
    assert torch.all((f64(db) - want).abs() <= tol), f"bias_grad M={M} C={C}"


def test_bias_grad_empty(ops):
    db = torch.full((76,), 3.0, device="cuda")
    ops.bias_grad(torch.empty(0, 76, device="cuda"), db)
    assert torch.all(db == 3.0)


@pytest.mark.parametrize("sizes", [
    [0, 3, 0, 5, 1, 2, 7, 0, 4, 9, 1, 1, 2, 6],                 # ends not multiples of 4, 1-3 float segments inside one float4, empty ones
    [1 + (i * 37) % 101 for i in range(300)] + [0, 2],          # 302 segments: the table is not staged in LDS; total not a multiple of 4
    [4 * 300] + [3] * 290,                                       # > 256 segments of 3
])
def test_sgd_momentum_segments(ops, sizes):
    g = torch.Generator().manual_seed(len(sizes))
    k = len(sizes)
    lrs = (0.01 + 0.02 * torch.rand(k, generator=g)).tolist()
    wds = [1e-4 if i % 2 else 0.0 for i in range(k)]
    ps = [torch.randn(s, generator=g) for s in sizes]
    gs = [[torch.randn(s, generator=g) for s in sizes] for _ in range(3)]
    ref = [p.double().clone().requires_grad_(True) for p in ps]
    opt = torch.optim.SGD([{"params": [r], "lr": lr, "weight_decay": wd} for r, lr, wd in zip(ref, lrs, wds)], lr=0.01, momentum=0.9)
    flat_p = torch.cat(ps).cuda()
    flat_m = torch.full_like(flat_p, SENT)       # the first step must not read the momentum buffer
    seg = torch.tensor(np.cumsum(sizes), dtype=torch.int64, device="cuda")
    lr_d, wd_d = torch.tensor(lrs, device="cuda"), torch.tensor(wds, device="cuda")
    for step in range(3):
        for r, g_ in zip(ref, gs[step]):
            r.grad = g_.double() * 0.5
        opt.step()
        ops.sgd_momentum_(flat_p, torch.cat(gs[step]).cuda(), flat_m, seg, lr_d, wd_d, 0.9, gscale=0.5, first_step=(step == 0))
    want = torch.cat([r.detach() for r in ref])
    scale = torch.cat([p.double().abs() + 0.1 for p in ps])
    assert torch.all((f64(flat_p) - want).abs() <= 16 * EPS * scale), f"sgd: max err {(f64(flat_p) - want).abs().max().item():.3e}"


@pytest.mark.parametrize("n", [1, 3, 4, 1025, 1024 * 256 * 8 + 3])
def test_relu_backward_add_inplace(ops, n):
    g = torch.Generator().manual_seed(n)
    gr, y, b = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    masked, summed = torch.where(y > 0, gr, torch.zeros_like(gr)), gr + b
    assert torch.equal(ops.relu_backward(gr.cuda(), y.cuda()).cpu(), masked)
    a = gr.clone().cuda()
    ops.add_(a, b.cuda())
    assert torch.equal(a.cpu(), summed)
    gi = gr.cuda()
    ops.relu_backward_(gi, y.cuda())
    assert torch.equal(gi.cpu(), masked)


@pytest.mark.parametrize("C", [1, 3, 4, 7, 1023, 1024])
def test_channel_mean(ops, C):
    g = torch.Generator().manual_seed(C)
    x = torch.randn(2, 7, 7, C, generator=g)
    got = f64(ops.channel_mean(x.cuda()))
    want = x.double().mean(-1)
    tol = 4 * EPS * x.double().abs().mean(-1) * max(1.0, math.log2(C))
    assert torch.all((got - want).abs() <= tol), f"channel_mean C={C}"

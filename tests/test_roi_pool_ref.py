"""The numpy references of tests/roi_pool_ref.py checked on the CPU, before the GPU suites (tests/test_gpu_roi_pool.py,
tests/test_gpu_deform_roi_pool.py) trust them:

  * ROIPool: the float32 bin borders and the integer-exact ones disagree on exactly the three rows the contract names, and nowhere else;
  * PS-RoI pooling: the float64 backward is the gradient of the float64 forward (central differences in feat, trans and mask_logits); at most
    1 % of a random case's outputs are `near` an accept boundary; the dyadic family evaluates to the same sample coordinates in float32 and
    float64, has samples exactly ON an accept boundary and partially filled bins; the kernel's float32 cell arithmetic gives the exact cells;
  * an honest float32 restatement (sequential and pairwise sums) meets the GPU suites' bounds on the same inputs with a margin of at least 4.
"""
import numpy as np
import pytest

import roi_align_ref as R
import roi_pool_ref as P
from roi_pool_ref import DYADIC_CASES, POOL_CASES, PS_CASES, RANDOM_CASES


# --------------------------------------------------------------------------------------------------------------------------- ROIPool
def test_float32_and_exact_borders_differ_on_the_three_rows_only():
    H, W, scale = 38, 63, 0.0625
    rois = P.length_rows(scale)            # lengths 1 .. 63 along x, all starting at pixel 0
    lengths = np.arange(1, 64)
    found = []
    for Pn in (2, 3, 5, 6, 7, 14):
        f32 = P.pool_bins(rois, scale, Pn, Pn, H, W + 2, np.float32)      # (a map two pixels wider: the clip must not hide end 58 at length 57 ... 63)
        exact = P.pool_bins(rois, scale, Pn, Pn, H, W + 2, exact=True)
        assert np.array_equal(f32.hs, exact.hs) and np.array_equal(f32.he, exact.he)   # heights 1 .. 7: no difference
        for k, b in zip(*np.nonzero(f32.ws != exact.ws)):
            found.append((Pn, int(lengths[k]), int(b), "start", int(f32.ws[k, b]), int(exact.ws[k, b])))
        for k, b in zip(*np.nonzero(f32.we != exact.we)):
            found.append((Pn, int(lengths[k]), int(b), "end", int(f32.we[k, b]), int(exact.we[k, b])))
    assert sorted(f[:4] for f in found) == sorted(P.DISCRIMINATING), found
    vals = {f[:4]: f[4:] for f in found}
    assert vals[(7, 57, 6, "end")] == (58, 57) and vals[(14, 57, 13, "end")] == (58, 57) and vals[(14, 62, 7, "start")] == (30, 31)


def test_rounding_rows_round_half_away_from_zero():
    q = P.pool_bins(np.array([[0, 8, -8, 24, -24]], np.float32), 0.0625, 1, 1, 100, 100)
    assert P.round_half_away(np.float32([0.5, -0.5, 1.5, -1.5, 0.49999997, 2.5])).tolist() == [1, -1, 2, -2, 0, 3]
    assert (q.ws[0, 0], q.hs[0, 0]) == (1, 0)     # x1 = 8 px -> 1; y1 = -8 px -> -1, clipped to 0


def test_pool_forward_semantics():
    f = np.zeros((1, 4, 4, 3), np.float32)
    f[0, :, :, 0] = 2.0                                   # ties: first pixel of the bin
    f[0, :, :, 1] = -np.inf                               # nothing above -FLT_MAX
    f[0, :, :, 2] = np.arange(16, dtype=np.float32).reshape(4, 4)
    f[0, 1, 1, 2] = np.nan
    out, arg = P.pool_forward(f, np.array([[0, 0, 0, 3, 3], [0, 50, 50, 60, 60]], np.float32), 1.0, 2, 2)
    assert arg[0, :, :, 0].tolist() == [[0, 2], [8, 10]] and (out[0, :, :, 0] == 2.0).all()
    assert (arg[0, :, :, 1] == -1).all() and (out[0, :, :, 1] == -P.FLT_MAX).all()
    assert arg[0, :, :, 2].tolist() == [[4, 7], [13, 15]]  # the NaN at pixel 5 never wins
    assert (arg[1] == -1).all() and (out[1] == 0).all()   # outside: empty bins


# --------------------------------------------------------------------------------------------------------------------------- PS-RoI pooling
def test_float32_cells_are_the_exact_cells():
    combos = {(c.P, c.part, c.G) for c in PS_CASES} | {(7, 7, 1), (3, 3, 1), (7, 7, 7), (14, 7, 2)}
    for Pn, part, G in sorted(combos):
        a, b = P.ps_cells_exact(Pn, part, G), P.ps_cells(Pn, part, G)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]), (Pn, part, G)
    # where the reference's float32 expression is NOT the exact integer, for P and part (or G) up to 28: the part cell of three bins, one cell low
    off = []
    for Pn in range(1, 29):
        for part in range(1, 29):
            a, b = P.ps_cells_exact(Pn, part, part), P.ps_cells(Pn, part, part)
            assert np.array_equal(a[1], b[1]), (Pn, part)                 # the group cell (one rounded division of an exact product) always is
            off += [(Pn, part, int(i), int(a[0][i]), int(b[0][i])) for i in np.nonzero(a[0] != b[0])[0]]
    assert off == [(22, 22, 13, 13, 12), (23, 23, 7, 7, 6), (23, 23, 14, 14, 13)], off


def _fd_case():
    """boxes well inside a 10 x 12 map at scale 1/4, small offsets: no sample is rejected, clamped, or close to a pixel centre's kink"""
    rng = np.random.default_rng(5)
    B, H, W, OD, Pn, part, spp, tstd = 2, 10, 12, 4, 3, 3, 2, 0.1
    rois = np.array([[0, 9, 7, 30, 25], [1, 13, 10, 33, 29], [0, 6, 14, 22, 31], [1, 17, 5, 38, 22]], np.float32)
    feat = rng.standard_normal((B, H, W, OD))
    trans = rng.uniform(-0.8, 0.8, (len(rois), 2, part, part))
    logits = rng.standard_normal((len(rois), Pn, Pn))
    grad = rng.standard_normal((len(rois), Pn, Pn, OD))
    return feat, rois, trans, logits, grad, (0.25, OD, 1, Pn, part, spp, tstd)


def test_float64_backward_is_the_gradient_of_the_forward():
    feat, rois, trans, logits, grad, args = _fd_case()
    H, W = feat.shape[1:3]
    g = P.ps_geometry(rois, trans, H, W, args[0], args[3], args[4], args[5], args[6])
    assert g.ok.all() and not g.clamped.any() and not g.near.any()
    frac = np.minimum(np.minimum(g.dx, 1 - g.dx), np.minimum(g.dy, 1 - g.dy))
    assert frac.min() > 1e-3, frac.min()                   # no sample within the differences' reach of a bilinear kink
    assert not P.psroi_forward(feat, rois, trans, logits, *args).near.any()
    got = P.psroi_backward(grad, feat, rois, trans, logits, *args)

    def loss(f, t, m):
        return float((P.psroi_forward(f, rois, t, m, *args).out * grad).sum())

    rng = np.random.default_rng(6)
    operands = [feat, trans, logits]
    for sub, (name, gx, h) in enumerate((("feat", got.gfeat, 1e-4), ("trans", got.gtrans, 1e-6), ("mask_logits", got.glogits, 1e-5))):
        worst = 0.0
        for _ in range(40):
            at = tuple(int(rng.integers(0, s)) for s in operands[sub].shape)
            xp, xm = operands[sub].copy(), operands[sub].copy()
            xp[at] += h
            xm[at] -= h
            fd = (loss(*[xp if i == sub else o for i, o in enumerate(operands)]) - loss(*[xm if i == sub else o for i, o in enumerate(operands)])) / (2 * h)
            worst = max(worst, abs(fd - gx[at]) / max(1.0, abs(fd)))
        print(f"FD {name}: worst relative difference {worst:.3e}")
        assert worst < 1e-6, (name, worst)


@pytest.mark.parametrize("c", RANDOM_CASES, ids=[c.id for c in RANDOM_CASES])
def test_near_share_of_random_cases(c):
    feat, rois, trans, logits, _ = c.inputs()
    r = P.psroi_forward(feat, rois, trans, logits, *c.args)
    full = c.spp * c.spp
    share = r.near.mean()
    print(f"NEAR {c.id}: {100 * share:.3f} % near, {100 * (r.count == 0).mean():.1f} % empty, {100 * ((r.count > 0) & (r.count < full)).mean():.1f} % partial")
    assert share <= 0.01
    assert (r.count == 0).any() and ((r.count > 0) & (r.count < full)).any()    # the family reaches empty and partially filled bins


def test_dyadic_family_is_the_same_in_float32_and_float64():
    samples = on_boundary = partial = bins = 0
    for c in DYADIC_CASES:
        _, rois, trans, _, _ = c.inputs()
        a = P.ps_geometry(rois, trans, c.H, c.W, c.scale, c.P, c.part, c.spp, c.tstd, np.float64)
        b = P.ps_geometry(rois, trans, c.H, c.W, c.scale, c.P, c.part, c.spp, c.tstd, np.float32)
        assert np.array_equal(a.w, b.w.astype(np.float64)) and np.array_equal(a.h, b.h.astype(np.float64)), c.id
        assert np.array_equal(a.ok, b.ok)
        samples += a.w.size
        on_boundary += int(a.on_boundary.sum())
        cnt = a.ok.sum((-1, -2))
        partial += int(((cnt > 0) & (cnt < c.spp * c.spp)).sum())
        bins += cnt.size
    print(f"DYADIC {samples} samples, 0 differences, {on_boundary} exactly on an accept boundary, {partial} of {bins} bins partial")
    assert on_boundary > 0 and partial > 0


# --------------------------------------------------------------------------------------------------------------------------- the bounds
@pytest.mark.parametrize("c", PS_CASES, ids=[c.id for c in PS_CASES])
def test_honest_float32_psroi_meets_the_bounds_with_margin(c):
    feat, rois, trans, logits, grad = c.inputs()
    want = P.psroi_forward(feat, rois, trans, logits, *c.args)
    keep = ~c.excluded(want.near)
    for order in ("seq", "pair"):
        got = P.psroi_forward(feat, rois, trans, logits, *c.args, dtype=np.float32, order=order)
        assert np.array_equal(got.count[keep], want.count[keep])
        ratio = R.worst_ratio(np.where(keep, got.out, want.out), want.out, P.scaled(want.S, want.n)) / R.TOL
        print(f"RATIO f32 {order} psroi fwd {c.id} {ratio:.3f} of the bound")
        assert ratio <= 0.25
    # for the record, not asserted: float32 sample COORDINATES as well -- their rounding error times the bilinear slope, not the sums, then
    # decides the error (this is why the kernels compute the coordinates in double)
    got = P.psroi_forward(feat, rois, trans, logits, *c.args, dtype=np.float32, geom_dtype=np.float32)
    same = keep & (got.count == want.count)
    ratio = R.worst_ratio(np.where(same, got.out, want.out), want.out, P.scaled(want.S, want.n)) / R.TOL
    print(f"RATIO f32 coordinates too, psroi fwd {c.id} {ratio:.3f} of the bound")
    grad = np.where(keep, grad, 0).astype(np.float32)
    w64 = P.psroi_backward(grad, feat, rois, trans, logits, *c.args)
    # (float32 decides the same samples on the outputs that are not near a boundary; the others carry no gradient)
    g32 = P.psroi_backward(grad, feat, rois, trans, logits, *c.args, dtype=np.float32)
    for name, got, ref, S, n in (("gfeat", g32.gfeat, w64.gfeat, w64.Sfeat, w64.nfeat), ("gtrans", g32.gtrans, w64.gtrans, w64.Strans, w64.ntrans),
                                 ("glogits", g32.glogits, w64.glogits, w64.Slogits, w64.nlogits)):
        if ref is None:
            assert got is None
            continue
        ratio = R.worst_ratio(got, ref, P.scaled(S, n)) / R.TOL
        print(f"RATIO f32 psroi {name} {c.id} {ratio:.3f} of the bound")
        assert ratio <= 0.25


@pytest.mark.parametrize("c", [c for c in POOL_CASES if c.feat in ("normal", "ties") and c.rois != "empty"][:8], ids=lambda c: c.id)
def test_honest_float32_roi_pool_backward_meets_the_bound_with_margin(c):
    rois, feat = c.make_rois(), c.make_feat()
    _, arg = P.pool_forward(feat, rois, c.scale, c.PH, c.PW)
    grad = c.make_grad(len(rois))
    want, S, n = P.pool_backward(grad, rois, arg, c.B, c.H, c.W)
    got, _, _ = P.pool_backward(grad, rois, arg, c.B, c.H, c.W, dtype=np.float32)
    ratio = R.worst_ratio(got, want, P.scaled(S, n)) / R.TOL
    print(f"RATIO f32 roi_pool bwd {c.id} {ratio:.3f} of the bound (most addends on one element: {int(n.max())})")
    assert ratio <= 0.25

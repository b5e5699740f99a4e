"""The float64 RoIAlign reference (tests/roi_align_ref.py) and its bound, checked on the CPU before the GPU is trusted with them.

  * its integer taps and grids are the oracle's, bit for bit, on the edge zoo and 4096 random RoIs;
  * the float32 oracle -- an honest float32 implementation in the reference's summation order -- passes `check` on every case the GPU suite
    uses, forward and backward, so TOL * S is a bound an honest kernel can meet;
  * `check` catches a dropped RoI, taps one pixel off, a wrong count, exchanged channel slices, a doubled bin and a stray write.

Runtime of the reference on a CPU-only development machine (numpy with its threaded BLAS), full size B = 4, 38 x 63 x 1024, K = 2048 RoIs (512 per image,
`random_rois`): forward (value and S) 2.4 s, backward (value and S) 4.2 s (1.5 s with bin_step 2) -- far under a minute, so K stays 2048.

No case needed a bound of its own: the oracle's worst |err| / S over all of `CASES` is 7.3e-7 (backward, sampling_ratio 3, C = 8), 5.4e-7 on the
full-size backward and 2.7e-7 on any forward; every test, here and on the GPU, asserts the one TOL = 1e-6.
"""
import numpy as np
import pytest

import roi_align_ref as R
from roi_align_ref import CASES, check


@pytest.fixture(scope="module")
def O():
    from oracle import ops
    return ops


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


def oracle_forward(O, c, feat, rois):
    if len(rois) == 0:
        return np.zeros((0,) + c.pooled + (c.C,), np.float32)
    return nhwc(O.roi_align_forward(nchw(feat), rois, c.scale, c.PH, c.PW, c.sr))[:, ::c.step, ::c.step]


def oracle_backward(O, c, grad, rois):
    """bin_step > 1 is the full backward of a gradient that is zero on the bins that are not kept"""
    full = np.zeros((len(rois), c.PH, c.PW, c.C), np.float32)
    full[:, ::c.step, ::c.step] = grad
    return nhwc(O.roi_align_backward(nchw(full), rois, c.scale, c.PH, c.PW, c.B, c.C, c.H, c.W, c.sr))


# ------------------------------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize("sr", [0, 1, 2, 3])
@pytest.mark.parametrize("P", [(7, 7), (14, 14), (3, 5)])
@pytest.mark.parametrize("H,W", [(38, 63), (1, 1), (1, 9), (9, 1)])
def test_integer_taps_and_grids_equal_the_oracles(O, H, W, P, sr):
    rois = np.concatenate([R.edge_zoo(4, H, W, 0.0625), R.random_rois(4, H, W, 0.0625, 1024)])
    assert len(rois) >= 4096 + 30
    idx, grid = R.taps(rois, H, W, 0.0625, P[0], P[1], sr, 64)
    oidx, ogrid = O.roi_align_taps(rois, H, W, 0.0625, P[0], P[1], sr, 64)
    assert np.array_equal(grid, ogrid)
    assert np.array_equal(idx, oidx), f"first differing (k, bin, s, tap) = {np.argwhere(idx != oidx)[0]}"


def test_edge_zoo_rows_are_the_edges_they_name():
    """the named rows do what their names say on the model's map (7 bins, sampling_ratio 2 for the exact-coordinate rows)"""
    B, H, W, s = 2, 38, 63, 0.0625
    names, rois = R.edge_zoo_names(B, H, W, s), R.edge_zoo(B, H, W, s)
    row = {n: i for i, n in enumerate(names)}
    g = R.roi_geom(rois, s, 7, 7, 2)
    ay, ax = R.axis_taps(g.y0, g.bh, g.gh, 7, 1, H), R.axis_taps(g.x0, g.bw, g.gw, 7, 1, W)

    def coord(start, binsz, k, p, i):
        return np.float32(start[k] + np.float32(p) * binsz[k]) + np.float32(np.float32(i + 0.5) * binsz[k]) / np.float32(2)

    for n in ("outside_top", "outside_bottom"):
        assert not ay.ok[row[n]].any()
    for n in ("outside_left", "outside_right"):
        assert not ax.ok[row[n]].any()
    for n, a in (("straddle_top", ay), ("straddle_bottom", ay), ("straddle_left", ax), ("straddle_right", ax)):
        assert a.ok[row[n]].any() and not a.ok[row[n]].all()
    k = row["sample_at_minus_one_y"]
    assert coord(g.y0, g.bh, k, 0, 0) == np.float32(-1.0) and ay.ok[k, 0, 0] and ay.lo[k, 0, 0] == 0
    k = row["sample_at_minus_one_x"]
    assert coord(g.x0, g.bw, k, 0, 0) == np.float32(-1.0) and ax.ok[k, 0, 0]
    k = row["sample_at_H"]
    assert coord(g.y0, g.bh, k, 6, 0) == np.float32(H) and ay.ok[k, 6, 0] and not ay.ok[k, 6, 1] and ay.lo[k, 6, 0] == H - 1 and ay.lw[k, 6, 0] == 0
    k = row["sample_at_W"]
    assert coord(g.x0, g.bw, k, 6, 0) == np.float32(W) and ax.ok[k, 6, 0] and not ax.ok[k, 6, 1] and ax.lo[k, 6, 0] == W - 1
    k = row["integer_aligned"]
    assert ay.ok[k].all() and (ay.lw[k] == 0).all() and (ax.lw[k] == 0).all()
    for n in ("reversed_corners", "zero_size", "sub_pixel"):
        assert g.bh[row[n]] == np.float32(1) / np.float32(7) and g.bw[row[n]] == np.float32(1) / np.float32(7)
    ga = R.roi_geom(rois, s, 7, 7, 0)
    assert ga.gh[row["larger_than_image"]] >= 10 and ga.gw[row["larger_than_image"]] >= 10
    assert [int(ga.gh[row[n]] * ga.gw[row[n]]) for n in ("grid_32", "grid_33", "grid_64")] == [32, 33, 64]
    assert sum(n.startswith("same_roi_") for n in names) == 300
    lay = R.layouts(3, H, W, s)
    assert len(lay["empty"]) == 0 and len(lay["one_roi"]) == 1 and len(set(lay["one_image"][:, 0])) == 1


# ------------------------------------------------------------------------------------------------------------------------- honest float32
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_float32_oracle_stays_inside_the_bound(O, c):
    """the inputs of the GPU suite: an honest float32 forward and backward pass `check` against the float64 reference"""
    rois, feat = c.make_rois(), c.make_feat()
    want, S = R.forward(feat, rois, c.scale, c.PH, c.PW, c.sr, c.step)
    got = oracle_forward(O, c, feat, rois)
    print(f"RATIO fwd {c.id} {R.worst_ratio(got, want, S):.3e}")
    check(got, want, S, "oracle forward " + c.id)
    grad = c.make_grad(len(rois))
    want, S = R.backward(grad, rois, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, c.step)
    got = oracle_backward(O, c, grad, rois)
    print(f"RATIO bwd {c.id} {R.worst_ratio(got, want, S):.3e}")
    check(got, want, S, "oracle backward " + c.id, axes="b,y,x,c")


def test_float64_geometry_switch_matches_a_direct_float64_evaluation():
    """the `dtype` switch: with float64 geometry the reference equals a sample-by-sample float64 evaluation of the same formula to 1e-13 * S"""
    c = R.case(rois="zoo", C=2, B=2)
    rois, feat = c.make_rois()[:40], c.make_feat().astype(np.float64)
    want, S = R.forward(feat, rois, c.scale, 7, 7, 2, dtype=np.float64)
    got = np.zeros_like(want)
    for k, r in enumerate(rois.astype(np.float64)):
        y0, x0 = r[2] * c.scale, r[1] * c.scale
        bh, bw = max(r[4] * c.scale - y0, 1.0) / 7, max(r[3] * c.scale - x0, 1.0) / 7
        for ph in range(7):
            for pw in range(7):
                for iy in range(2):
                    for ix in range(2):
                        y, x = y0 + ph * bh + (iy + .5) * bh / 2, x0 + pw * bw + (ix + .5) * bw / 2
                        if y < -1 or y > c.H or x < -1 or x > c.W:
                            continue
                        y, x = max(y, 0.0), max(x, 0.0)
                        yl, xl = int(y), int(x)
                        if yl >= c.H - 1:
                            yl, y = c.H - 1, float(c.H - 1)
                        if xl >= c.W - 1:
                            xl, x = c.W - 1, float(c.W - 1)
                        yh, xh = min(yl + 1, c.H - 1), min(xl + 1, c.W - 1)
                        ly, lx = y - yl, x - xl
                        f = feat[int(r[0])]
                        got[k, ph, pw] += ((1 - ly) * (1 - lx) * f[yl, xl] + (1 - ly) * lx * f[yl, xh] + ly * (1 - lx) * f[yh, xl] + ly * lx * f[yh, xh]) / 4
    check(got, want, S, "float64 geometry", tol=1e-13)


# ------------------------------------------------------------------------------------------------------------------------- sensitivity
FULL = R.case(rois="full", B=5, C=256)   # the full-size RoI set (4 x 512 on 38 x 63) at 256 channels; image 4 has no RoI


@pytest.fixture(scope="module")
def full(O):
    c = FULL
    rois = np.concatenate([R.random_rois(4, c.H, c.W, c.scale, 512), R.outside(4, c.H, c.W, c.scale)])
    feat, grad = c.make_feat(), c.make_grad(len(rois))
    fw = R.forward(feat, rois, c.scale, 7, 7, 0)
    bw = R.backward(grad, rois, c.scale, 7, 7, 0, c.B, c.H, c.W)
    return dict(rois=rois, feat=feat, grad=grad, fw=fw, bw=bw, of=oracle_forward(O, c, feat, rois), ob=oracle_backward(O, c, grad, rois))


def _fails(got, want_S, what, **kw):
    with pytest.raises(AssertionError):
        check(got, *want_S, what, **kw)


def test_full_size_oracle_passes_and_every_mutation_is_caught(O, full):
    c, rois, feat, grad = FULL, full["rois"], full["feat"], full["grad"]
    print(f"RATIO fwd full {R.worst_ratio(full['of'], *full['fw']):.3e}")
    print(f"RATIO bwd full {R.worst_ratio(full['ob'], *full['bw']):.3e}")
    check(full["of"], *full["fw"], "full-size oracle forward")
    check(full["ob"], *full["bw"], "full-size oracle backward", axes="b,y,x,c")
    ft, bt = dict(), dict(axes="b,y,x,c")
    g = R.roi_geom(rois, c.scale, 7, 7, 0)
    k = int(np.nonzero((g.gh != g.gw) & (full["fw"][1].reshape(len(rois), -1).min(1) > 0))[0][0])   # an ordinary RoI inside the map

    # one RoI dropped
    m = full["of"].copy(); m[k] = 0
    _fails(m, full["fw"], "forward, RoI dropped", **ft)
    keep = np.arange(len(rois)) != k
    _fails(oracle_backward(O, c, grad[keep], rois[keep]), full["bw"], "backward, RoI dropped", **bt)
    # one RoI's taps one pixel to the right
    r2 = rois.copy(); r2[k, [1, 3]] += 1 / c.scale
    m = full["of"].copy(); m[k] = oracle_forward(O, c, feat, r2[k:k + 1])[0]
    _fails(m, full["fw"], "forward, taps shifted", **ft)
    _fails(oracle_backward(O, c, grad, r2), full["bw"], "backward, taps shifted", **bt)
    # count = gh * gh
    wrong = (g.gw / g.gh).astype(np.float32)[:, None, None, None]
    _fails(full["of"] * wrong, full["fw"], "forward, count gh * gh", **ft)
    _fails(oracle_backward(O, c, grad * wrong, rois), full["bw"], "backward, count gh * gh", **bt)
    # two 128-channel slices exchanged
    swap = np.r_[128:256, 0:128]
    _fails(full["of"][..., swap], full["fw"], "forward, slices exchanged", **ft)
    _fails(full["ob"][..., swap], full["bw"], "backward, slices exchanged", **bt)
    # one bin doubled
    m = full["of"].copy(); m[k, 3, 4] *= 2
    _fails(m, full["fw"], "forward, bin doubled", **ft)
    g2 = grad.copy(); g2[k, 3, 4] *= 2
    _fails(oracle_backward(O, c, g2, rois), full["bw"], "backward, bin's gradient doubled", **bt)
    # a stray write where no sample lands
    for got, (want, S), kw in ((full["of"], full["fw"], ft), (full["ob"], full["bw"], bt)):
        dead = np.argwhere(S == 0)
        assert len(dead), "the full-size set has elements no sample reaches: the fully-outside rows, the image without RoIs"
        m = got.copy(); m[tuple(dead[len(dead) // 2])] = 1e-3
        _fails(m, (want, S), "stray write", **kw)


def test_check_names_the_worst_element():
    want = np.ones((2, 3, 4, 5)); S = np.ones_like(want)
    got = want.copy(); got[1, 2, 0, 3] += 1e-3; got[0, 0, 0, 0] += 1e-5
    with pytest.raises(AssertionError, match=r"\(k,ph,pw,c\) = \(1, 2, 0, 3\)"):
        check(got, want, S, "x")
    got = want.copy(); got[0, 1, 1, 1] = np.nan
    with pytest.raises(AssertionError, match="non-finite"):
        check(got, want, S, "x")
    assert check(want + 5e-7, want, S, "x") == pytest.approx(5e-7)

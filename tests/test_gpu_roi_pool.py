"""ROIPool (abr_iod_amd/csrc/roi_pool.hip) against the numpy reference of tests/roi_pool_ref.py, through every route: `ops` (NHWC, float4
and scalar lanes), `_C` (NCHW, float and double) and autograd through layers.ROIPool.

A maximum has no rounding: forward values are EQUAL to the reference and argmax is equal everywhere.  The backward pass goes through
roi_align_ref.check with the tolerance max(TOL, (n + 8) 2^-24) * S per element (n = the element's addend count, S = the sum of their
magnitudes; tests/test_roi_pool_ref.py shows a float32 sum meets it), and is exactly 0 where nothing lands.

Cases (roi_pool_ref.POOL_CASES, B = 2): the 38 x 63 map with one RoI per length 1 .. 63 for P 7 and 14 -- among them the three rows where the
float32 bin borders differ from integer-exact ones --, corners that round half away from zero (+-8, +-24 image px at scale 1/16), malformed
boxes, boxes wholly outside (empty bins), an image without RoI, K = 0, C in {1, 3, 4, 5, 24, 256, 260} (both vector widths and C % 4 != 0),
pooling 3 x 5, random boxes, a constant map (every bin ties: argmax is the bin's first pixel), a map of -inf (-FLT_MAX and -1), one NaN pixel.
"""
import functools

import numpy as np
import pytest
import torch

import roi_align_ref as R
import roi_pool_ref as P
from roi_align_ref import TOL_F64, check
from roi_pool_ref import POOL_CASES, pool_case

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


@functools.lru_cache(maxsize=None)
def ref(c, dtype=np.float32):
    rois, feat = c.make_rois(), c.make_feat()
    want, arg = P.pool_forward(feat, rois, c.scale, c.PH, c.PW, dtype)
    grad = c.make_grad(len(rois))
    gwant, S, n = P.pool_backward(grad, rois, arg, c.B, c.H, c.W)
    return rois, feat, want, arg, grad, gwant, S, n


def same(got, want, arg_got, arg_want, what):
    assert got.shape == want.shape and arg_got.shape == arg_want.shape, what
    assert arg_got.dtype == np.int32
    bad = arg_got != arg_want
    assert not bad.any(), f"{what}: argmax differs at (k,ph,pw,c) = {np.argwhere(bad)[0]}: got {arg_got[bad][0]}, want {arg_want[bad][0]}; {int(bad.sum())} elements"
    bad = got.astype(np.float64) != want
    assert not bad.any(), f"{what}: value differs at (k,ph,pw,c) = {np.argwhere(bad)[0]}: got {got[bad][0]!r}, want {want[bad][0]!r}; {int(bad.sum())} elements"


# --------------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", POOL_CASES, ids=[c.id for c in POOL_CASES])
def test_forward(c):
    from abr_iod_amd import _C, ops
    rois, feat, want, arg = ref(c)[:4]
    out, am = ops.roi_pool_forward(T(feat), T(rois), c.scale, c.PH, c.PW)
    same(N(out), want, N(am), arg, "NHWC forward " + c.id)
    out, am = _C.roi_pool_forward(T(nchw(feat)), T(rois), c.scale, c.PH, c.PW)
    assert tuple(out.shape) == (len(rois), c.C, c.PH, c.PW)
    same(nhwc(N(out)), want, nhwc(N(am)), arg, "NCHW forward " + c.id)


@pytest.mark.parametrize("c", [pool_case("lengths", P=7), pool_case("lengths", P=14), pool_case(C=5), pool_case(feat="neginf"), pool_case(feat="nan"),
                               pool_case("empty")], ids=lambda c: c.id)
def test_forward_f64(c):
    from abr_iod_amd import _C
    rois, feat, want, arg = ref(c, np.float64)[:4]
    out, am = _C.roi_pool_forward(T(nchw(feat).astype(np.float64)), T(rois.astype(np.float64)), c.scale, c.PH, c.PW)
    assert out.dtype == torch.float64
    same(nhwc(N(out)), want, nhwc(N(am)), arg, "NCHW float64 forward " + c.id)


def test_the_discriminating_rows_are_reached():
    """length 57 over 7 bins: the last bin ends at 58 in float32 (57 exactly) -- on a map of -1 with one larger value in column 57, the
    RoI that covers columns 0 .. 56 still finds it"""
    from abr_iod_amd import ops
    feat = np.full((1, 2, 63, 4), -1.0, np.float32)
    feat[0, 0, 57] = 5.0
    rois = np.array([[0, 0, 0, 56 * 16, 0]], np.float32)
    out, am = ops.roi_pool_forward(T(feat), T(rois), 0.0625, 1, 7)
    assert N(out)[0, 0, 6].tolist() == [5.0] * 4 and N(am)[0, 0, 6].tolist() == [57] * 4
    want, arg = P.pool_forward(feat, rois, 0.0625, 1, 7)
    same(N(out), want, N(am), arg, "length 57")


@pytest.mark.parametrize("c", [pool_case(C=5), pool_case(C=24), pool_case("empty")], ids=lambda c: c.id)
def test_forward_out_writes_only_its_own_rows(c):
    from abr_iod_amd import ops
    rois, feat, want, arg = ref(c)[:4]
    K = len(rois)
    buf = torch.full((K + 2, c.PH, c.PW, c.C), SENTINEL, device="cuda")
    out, am = ops.roi_pool_forward(T(feat), T(rois), c.scale, c.PH, c.PW, out=buf[1:K + 1])
    assert out.data_ptr() == buf[1:K + 1].data_ptr()
    got = N(buf)
    assert (got[0] == SENTINEL).all() and (got[K + 1] == SENTINEL).all()
    same(got[1:K + 1], want, N(am), arg, "out= " + c.id)


# --------------------------------------------------------------------------------------------------------------------------- backward
def bwd_check(got, c, what, base=None):
    _, _, _, _, _, gwant, S, n = ref(c)
    if base is not None:
        gwant, S, n = gwant + base, S + np.abs(base), n + 1
    print(f"RATIO roi_pool bwd {what} {c.id} {R.worst_ratio(got, gwant, P.scaled(S, n)) / R.TOL:.3f} of the bound")
    check(got, gwant, P.scaled(S, n), f"{what} backward {c.id}", axes="b,y,x,c")


@pytest.mark.parametrize("c", POOL_CASES, ids=[c.id for c in POOL_CASES])
def test_backward(c):
    from abr_iod_amd import _C, layers, ops
    rois, feat, _, arg, grad = ref(c)[:5]
    bwd_check(N(ops.roi_pool_backward(T(grad), T(rois), T(arg), c.B, c.H, c.W)), c, "nhwc")
    x = T(nchw(feat))
    g = _C.roi_pool_backward(T(nchw(grad)), x, T(rois), T(nchw(arg)), c.scale, c.PH, c.PW, c.B, c.C, c.H, c.W)
    bwd_check(nhwc(N(g)), c, "nchw")
    x.requires_grad_(True)
    out = layers.ROIPool((c.PH, c.PW), c.scale)(x, T(rois))
    assert tuple(out.shape) == (len(rois), c.C, c.PH, c.PW)
    out.backward(T(nchw(grad)))
    bwd_check(nhwc(N(x.grad)), c, "autograd")


@pytest.mark.parametrize("c", [pool_case("lengths", P=14), pool_case(C=5), pool_case("empty")], ids=lambda c: c.id)
def test_backward_f64(c):
    from abr_iod_amd import _C
    rois, feat, _, arg, grad, gwant, S, _ = ref(c)
    g = _C.roi_pool_backward(T(nchw(grad).astype(np.float64)), T(nchw(feat).astype(np.float64)), T(rois.astype(np.float64)), T(nchw(arg)), c.scale,
                             c.PH, c.PW, c.B, c.C, c.H, c.W)
    assert g.dtype == torch.float64
    check(nhwc(N(g)), gwant, S, "NCHW float64 backward " + c.id, axes="b,y,x,c", tol=TOL_F64)


@pytest.mark.parametrize("c", [pool_case(C=5), pool_case("random", C=256), pool_case("empty")], ids=lambda c: c.id)
def test_backward_accumulates(c):
    from abr_iod_amd import ops
    rois, _, _, arg, grad = ref(c)[:5]
    base = np.random.default_rng(3).standard_normal((c.B, c.H, c.W, c.C)).astype(np.float32)
    out = T(base)
    got = ops.roi_pool_backward(T(grad), T(rois), T(arg), c.B, c.H, c.W, out=out)
    assert got.data_ptr() == out.data_ptr()
    bwd_check(N(out), c, "accumulate", base=base.astype(np.float64))


# --------------------------------------------------------------------------------------------------------------------------- the surface
def test_layer_tags_its_output_with_the_maps_amax():
    from abr_iod_amd import layers, ops
    from abr_iod_amd.layers._layout import from_nhwc
    c = pool_case("random", C=8)
    x = ops.amax_compute(T(c.make_feat()))
    assert ops.amax_of(x)[0] is not None
    out = layers.ROIPool(7, c.scale)(from_nhwc(x), T(c.make_rois()))
    assert ops.amax_of(out) == ops.amax_of(x)


def test_refusals():
    from abr_iod_amd import _C, _lib as L
    x, r = torch.zeros(1, 4, 6, 6, device="cuda"), torch.zeros(2, 5, device="cuda")
    with pytest.raises(RuntimeError, match="float16"):
        _C.roi_pool_forward(x.half(), r.half(), 1.0, 2, 2)
    with pytest.raises(RuntimeError, match="float64"):
        _C.deform_psroi_pooling_forward(x.double(), r.double(), x.new_empty(0), torch.zeros(2, 4, 2, 2, device="cuda", dtype=torch.float64),
                                        torch.zeros(2, 4, 2, 2, device="cuda", dtype=torch.float64), True, 1.0, 4, 1, 2, 2, 2, 0.0)
    with pytest.raises(RuntimeError, match="Output shape and bbox number wont match"):
        _C.deform_psroi_pooling_forward(x, r, x.new_empty(0), torch.zeros(3, 4, 2, 2, device="cuda"), torch.zeros(3, 4, 2, 2, device="cuda"), True, 1.0,
                                        4, 1, 2, 2, 2, 0.0)
    # K * C * PH * PW past int32: an error status before anything is launched (no pointer is touched)
    assert L.lib().abr_roi_pool_forward(None, None, 1 << 20, 1, 1024, 8, 8, 1.0, 7, 7, L.NHWC, None, None, None) != 0
    assert b"int32" in L.lib().abr_last_error()
    assert L.lib().abr_roi_pool_forward(None, None, 4, 1 << 10, 1 << 10, 1 << 6, 1 << 6, 1.0, 7, 7, L.NCHW, None, None, None) != 0
    assert b"int32" in L.lib().abr_last_error()
    assert L.lib().abr_roi_pool_forward(None, None, 0, 1, 8, 8, 8, 1.0, 7, 7, L.NHWC, None, None, None) == 0      # K == 0: nothing to do

"""Every RoIAlign route of abr_iod_amd/csrc/roi_align.hip against the float64 reference of tests/roi_align_ref.py, at its edges.

Every comparison goes through `check`: finite, |got - want| <= TOL * S element-wise with S the float64 sum of |addends|, and exactly 0 where
no sample lands.  Forward results are, in addition, bit-equal to oracle.ops.roi_align_forward (the kernels keep the reference's order).
tests/test_roi_align_ref.py shows on the CPU that the reference's taps are the oracle's and that an honest float32 implementation meets the
bound on these same inputs.  The cases are `roi_align_ref.CASES` ("mixed" = edge zoo + random RoIs) plus the few rows built below.

Which kernel and launch shape each row reaches (fwd shape = pick_shape's (tx, bpb); "sep" = roi_align_bwd_nhwc_sep, "direct" =
roi_align_bwd_nhwc; gather chunks = ceil(C / 256), xcd = the XCD mapping):

  kernel / instantiation                     reached by (CASES rows unless said otherwise)
  -----------------------------------------  -----------------------------------------------------------------------------------------
  roi_align_fwd_nchw<float>                  test_forward, every row with bin_step 1 (_C.roi_align_forward)
  roi_align_fwd_nchw<double>                 test_f64_nchw_pair (edge zoo)
  roi_align_fwd_nhwc<4>  cslices 1  (32, 8)  C = 4 ... 24, 8;   (64, 4) C = 252, 256;   (128, 2) C = 260, 512;
                                             (256, 1) C = 1024 on 5x5 (one pass) and C = 2048 on 5x5 (two passes);
                                             bpb cut to the bin count: pooled 1x1 (256, 1)
  roi_align_fwd_nhwc<4>  cslices 8           C = 1024 (32, 8), 1536 and 2048 (64, 4) on 38x63
  roi_align_fwd_nhwc<1>                      C = 1, 3, 5, 6 (32, 8);  C = 70 (128, 2);  C = 250 (256, 1);  C = 514 (256, 1, three passes)
  roi_align_bwd_nchw<float>                  test_backward[nchw], every row with bin_step 1;  accumulate = 1 in test_backward_accumulates
  roi_align_bwd_nchw<double>                 test_f64_nchw_pair
  roi_align_bwd_nhwc_sep<4>                  test_backward[scatter]: every C % 4 == 0 row with <= 8 kept bins per axis; channel chunks 1 (C <= 1024),
                                             2 (C = 1536, 2048)
  roi_align_bwd_nhwc_sep<1>                  test_backward[scatter]: C = 1, 3, 5, 6, 70, 250 (one chunk), 514 (three chunks)
  roi_align_bwd_nhwc<4>                      pooled 14x14 (C = 8, 12, 256) and 9x9 (C = 8);  the LDS limit: test_lds_limit (1000 x 1000 x 4, 8x8)
  roi_align_bwd_nhwc<1>                      pooled 9x9 at C = 5
  roi_bwd_tables_kernel,                     test_backward[gather] and [autograd]: every C % 4 == 0 row with <= 8 kept bins per axis;
  roi_tile_lists_kernel                      W = 1, 7, 8, 9, 21, 63 (x-tiles of 8: under, on and over one tile)
  roi_align_bwd_gather_kernel<4, 4>          bin_step 2 on 7x7 and 8x8 (4 bins), pooled 1x1;  xcd: C = 8, 256 (1 chunk), 512 (2)
  roi_align_bwd_gather_kernel<8, 4>          7x7, 8x8, 3x5, bin_step 2 on 14x14 (7 bins);  xcd: chunks 1 (C <= 256), 2 (C = 260, 512), 4 (1024), 8 (2048);
                                             the 3-D grid: 6 chunks (C = 1536);  full size in test_full_size_backward
  roi_align_taps_kernel                      tests/test_gpu_ops.py::test_roi_align_taps_bit_exact (unchanged)
"""
import functools

import numpy as np
import pytest
import torch

import roi_align_ref as R
from roi_align_ref import CASES, TOL_F64, case, check

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


def gatherable(c):
    return c.C % 4 == 0 and max(c.pooled) <= 8


@functools.lru_cache(maxsize=None)
def fwd_ref(c):
    from oracle import ops as O
    rois, feat = c.make_rois(), c.make_feat()
    want, S = R.forward(feat, rois, c.scale, c.PH, c.PW, c.sr, c.step)
    if len(rois):
        bits = nhwc(O.roi_align_forward(nchw(feat), rois, c.scale, c.PH, c.PW, c.sr))[:, ::c.step, ::c.step]
    else:
        bits = np.zeros(want.shape, np.float32)
    return rois, feat, want, S, np.ascontiguousarray(bits)


@functools.lru_cache(maxsize=None)
def bwd_ref(c):
    rois = c.make_rois()
    grad = c.make_grad(len(rois))
    want, S = R.backward(grad, rois, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, c.step)
    return rois, grad, want, S


def same_bits(got, bits, what):
    same = np.ascontiguousarray(got).view(np.int32) == bits.view(np.int32)
    assert same.all(), f"{what}: not bit-equal to the oracle at (k,ph,pw,c) = {np.argwhere(~same)[0]}, max |diff| {np.abs(got - bits).max():.3e}"


# --------------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("c", CASES, ids=[c.id for c in CASES])
def test_forward(c):
    from abr_iod_amd import _C, ops
    rois, feat, want, S, bits = fwd_ref(c)
    got = N(ops.roi_align_forward(T(feat), T(rois), c.scale, c.PH, c.PW, c.sr, bin_step=c.step))
    print(f"RATIO fwd nhwc {c.id} {R.worst_ratio(got, want, S):.3e}")
    check(got, want, S, "NHWC forward " + c.id)
    same_bits(got, bits, "NHWC forward " + c.id)
    if c.step == 1:
        got = nhwc(N(_C.roi_align_forward(T(nchw(feat)), T(rois), c.scale, c.PH, c.PW, c.sr)))
        assert got.shape == want.shape
        check(got, want, S, "NCHW forward " + c.id)
        same_bits(got, bits, "NCHW forward " + c.id)


@pytest.mark.parametrize("c", [case(C=5), case(C=24), case(C=1024, rois="random"), case(C=8, step=2), case(C=8, rois="empty")], ids=lambda c: c.id)
def test_forward_out_writes_only_its_own_rows(c):
    from abr_iod_amd import ops
    rois, feat, want, S, bits = fwd_ref(c)
    K, (po, qo) = len(rois), c.pooled
    buf = torch.full((K + 2, po, qo, c.C), SENTINEL, device="cuda")
    ret = ops.roi_align_forward(T(feat), T(rois), c.scale, c.PH, c.PW, c.sr, bin_step=c.step, out=buf[1:K + 1])
    assert ret.data_ptr() == buf[1:K + 1].data_ptr() or K == 0
    got = N(buf)
    assert (got[0] == SENTINEL).all() and (got[K + 1] == SENTINEL).all(), "the rows around `out` were written"
    check(got[1:K + 1], want, S, "forward out= " + c.id)
    same_bits(got[1:K + 1], bits, "forward out= " + c.id)


F64_CASES = [case(rois="zoo", C=3), case(rois="zoo", C=2, sr=2), case(rois="zoo", C=2, H=7, W=9, P=(3, 5)), case(rois="zoo", C=2, H=1, W=1, sr=3),
             case(rois="empty", C=2)]


@pytest.mark.parametrize("c", F64_CASES, ids=lambda c: c.id)
def test_f64_nchw_pair(c):
    """float64 tensors through _C: geometry, weights and sums in double; the reference with float64 geometry; 1e-12 * S"""
    from abr_iod_amd import _C
    rois, feat = c.make_rois(), c.make_feat().astype(np.float64)
    want, S = R.forward(feat, rois, c.scale, c.PH, c.PW, c.sr, dtype=np.float64)
    got = _C.roi_align_forward(T(nchw(feat)), T(rois.astype(np.float64)), c.scale, c.PH, c.PW, c.sr)
    assert got.dtype == torch.float64
    check(nhwc(N(got)), want, S, "f64 forward " + c.id, tol=TOL_F64)
    grad = c.make_grad(len(rois)).astype(np.float64)
    want, S = R.backward(grad, rois, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, dtype=np.float64)
    got = _C.roi_align_backward(T(nchw(grad)), T(rois.astype(np.float64)), c.scale, c.PH, c.PW, c.B, c.C, c.H, c.W, c.sr)
    assert got.dtype == torch.float64
    check(nhwc(N(got)), want, S, "f64 backward " + c.id, axes="b,y,x,c", tol=TOL_F64)


# --------------------------------------------------------------------------------------------------------------------------- backward
def run_backward(route, c, grad, rois, prior=None):
    """-> numpy [B, H, W, C].  `prior` (numpy, same shape) is accumulated into: the out= form of each route."""
    from abr_iod_amd import _C, _lib as L, layers, ops
    g, r = T(grad), T(rois)
    if route in ("scatter", "gather"):
        if route == "gather":
            assert gatherable(c)
        out = None if prior is None else T(prior)
        got = ops.roi_align_backward(g, r, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, c.C, bin_step=c.step, out=out, method=route)
        assert out is None or got.data_ptr() == out.data_ptr()
        return N(got)
    if route == "nchw":
        assert c.step == 1
        gn = T(nchw(grad))
        if prior is None:
            return nhwc(N(_C.roi_align_backward(gn, r, c.scale, c.PH, c.PW, c.B, c.C, c.H, c.W, c.sr)))
        out = T(nchw(prior))   # _C has no out=: the C ABI's accumulate flag on the NCHW layout
        L.check(L.lib().abr_roi_align_backward(L.ptr(gn), L.ptr(r), len(rois), c.B, c.C, c.H, c.W, c.scale, c.PH, c.PW, c.sr, 1, L.NCHW, 1,
                                               L.ptr(out), L.stream()), "roi_align_backward")
        return nhwc(N(out))
    assert route == "autograd"
    x = T(nchw(c.make_feat())).requires_grad_(True)
    if prior is not None:
        x.grad = T(nchw(prior))
    y = layers.ROIAlign((c.PH, c.PW), c.scale, c.sr)(x, r, bin_step=c.step)
    assert tuple(y.shape) == (len(rois), c.C) + c.pooled
    y.backward(T(nchw(grad)))
    return nhwc(N(x.grad))


def backward_rows(cases):
    rows = []
    for c in cases:
        for route in ("nchw", "scatter", "gather", "autograd"):
            if route == "nchw" and c.step != 1:
                continue    # the NCHW pair refuses bin_step > 1
            if route == "gather" and not gatherable(c):
                continue    # ops sends these to the scatter: the [scatter] row is that call
            rows.append(pytest.param(c, route, id=f"{route}-{c.id}"))
    return rows


@pytest.mark.parametrize("c,route", backward_rows(CASES))
def test_backward(c, route):
    rois, grad, want, S = bwd_ref(c)
    got = run_backward(route, c, grad, rois)
    print(f"RATIO bwd {route} {c.id} {R.worst_ratio(got, want, S):.3e}")
    check(got, want, S, f"{route} backward {c.id}", axes="b,y,x,c")
    if route == "gather":
        again = run_backward(route, c, grad, rois)
        assert np.array_equal(got.view(np.int32), again.view(np.int32)), "the gather is not bit-identical run to run"


ACC_CASES = [case(C=8), case(C=5), case(C=256), case(C=1536, rois="random"), case(C=8, step=2), case(C=8, P=14), case(C=8, H=7, W=9),
             case(C=8, rois="one_image", B=3), case(C=8, rois="empty")]


@pytest.mark.parametrize("c,route", backward_rows(ACC_CASES))
def test_backward_accumulates(c, route):
    """out= (the C ABI's accumulate flag; .grad for autograd): prior contents plus the reference, bounded on S + |prior|"""
    rois, grad, want, S = bwd_ref(c)
    prior = np.random.default_rng(5).standard_normal(want.shape).astype(np.float32)
    got = run_backward(route, c, grad, rois, prior=prior)
    check(got, want + prior, S + np.abs(prior), f"{route} accumulate {c.id}", axes="b,y,x,c")
    if len(rois) == 0:
        assert np.array_equal(got, prior), "K = 0 with out= must leave the buffer as it was"


def test_lds_limit_takes_the_direct_kernel_and_refuses_the_gather():
    """8 * (H + W) * 4 + 16 bytes of tables exceed the 60 KB of LDS: the scatter goes through roi_align_bwd_nhwc<4>; the gather, whose table
    builder needs them in LDS, raises and leaves the output as it was"""
    from abr_iod_amd import ops
    c = case(rois="lds", B=1, H=1000, W=1000, C=4, P=8)
    assert 4 * (c.PH * c.H + c.PW * c.W) + 16 > 60 * 1024
    # four RoIs in the map's corners (the last one past the far borders), and the four whose every sample is rejected
    rois = np.concatenate([R.random_rois(1, 55, 55, c.scale, 4, seed=3), R.outside(1, c.H, c.W, c.scale)])
    rois[:4, 1:] += np.float32([[0, 0, 0, 0], [900, 0, 900, 0], [0, 900, 0, 900], [945, 945, 945, 945]]) / np.float32(c.scale)
    assert len(rois) == 8
    grad = c.make_grad(8)
    want, S = R.backward(grad, rois, c.scale, 8, 8, 0, 1, c.H, c.W)
    assert (S > 0).any()
    got = N(ops.roi_align_backward(T(grad), T(rois), c.scale, 8, 8, 0, 1, c.H, c.W, c.C, method="scatter"))
    check(got, want, S, "direct atomic kernel past the LDS limit", axes="b,y,x,c")
    prior = torch.full((1, c.H, c.W, c.C), SENTINEL, device="cuda")
    with pytest.raises(RuntimeError, match="too large"):
        ops.roi_align_backward(T(grad), T(rois), c.scale, 8, 8, 0, 1, c.H, c.W, c.C, out=prior, method="gather")
    torch.cuda.synchronize()
    assert bool((prior == SENTINEL).all()), "the refused gather wrote into its output"


# --------------------------------------------------------------------------------------------------------------------------- poisoned output
def abi_backward(kind, c, grad, rois, buf):
    """the C ABI with accumulate = 0 into `buf` as it is"""
    from abr_iod_amd import _lib as L
    g, r, K = T(grad), T(rois), len(rois)
    if kind == "gather":
        nbytes = L.lib().abr_roi_align_backward_ws_bytes(K, c.B, c.H, c.W, c.PH, c.PW, c.step)
        ws = torch.empty((max(int(nbytes), 256),), dtype=torch.uint8, device="cuda")
        L.check(L.lib().abr_roi_align_backward_gather(L.ptr(g), L.ptr(r), K, c.B, c.C, c.H, c.W, c.scale, c.PH, c.PW, c.sr, c.step, 0, L.ptr(buf),
                                                      L.ptr(ws), ws.numel(), L.stream()), "roi_align_backward_gather")
    else:
        L.check(L.lib().abr_roi_align_backward(L.ptr(g), L.ptr(r), K, c.B, c.C, c.H, c.W, c.scale, c.PH, c.PW, c.sr, c.step, L.NHWC, 0, L.ptr(buf),
                                               L.stream()), "roi_align_backward")
    torch.cuda.synchronize()
    return N(buf)


POISON_CASES = [case(rois=lay, B=3, H=H, W=W, C=C, step=step)
                for lay in ("one_image", "one_roi", "empty") for (H, W, C, step) in ((38, 63, 8, 1), (7, 9, 256, 1), (13, 21, 260, 2), (5, 7, 1024, 1))]


@pytest.mark.parametrize("kind", ["gather", "scatter"])
@pytest.mark.parametrize("c", POISON_CASES, ids=lambda c: c.id)
def test_backward_overwrites_a_poisoned_output(c, kind):
    """accumulate = 0 into a buffer full of -12345: the gather claims to write every element exactly once with no zero-fill pass.  Images
    without RoIs, pixels outside every footprint and the pixels of RoIs whose every sample is rejected come back exactly 0."""
    rois = np.concatenate([c.make_rois(), R.outside(c.B, c.H, c.W, c.scale)])
    grad = c.make_grad(len(rois))
    want, S = R.backward(grad, rois, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, c.step)
    assert (S == 0).any(), "the layout leaves pixels that no sample reaches"
    buf = torch.full((c.B, c.H, c.W, c.C), SENTINEL, device="cuda")
    got = abi_backward(kind, c, grad, rois, buf)
    check(got, want, S, f"{kind} into a poisoned buffer {c.id}", axes="b,y,x,c")
    # no RoI at all
    buf.fill_(SENTINEL)
    got = abi_backward(kind, c, grad[:0], rois[:0], buf)
    assert (got == 0).all(), "K = 0 without accumulate must zero the output"


# --------------------------------------------------------------------------------------------------------------------------- workspace
def test_gather_workspace_is_per_stream_and_reused():
    """The gather backward keeps its workspace (weight tables, footprints, tile lists) between calls.  Two calls with different inputs, one on
    the current stream and one on a side stream, enqueued back to back, must each return the bits of the same call made alone (the gather is
    atomic-free, hence deterministic): they share nothing.  Two calls in a row on one stream reuse one workspace tensor."""
    from abr_iod_amd import _lib as L, ops
    K, B, H, W, C, P = 8, 1, 8, 8, 8, 7
    rng = np.random.default_rng(7)

    def inputs():
        lo, size = rng.uniform(-1, 5, (K, 2)), rng.uniform(.5, 6, (K, 2))
        rois = np.concatenate([np.zeros((K, 1)), lo, lo + size], 1).astype(np.float32)
        return T(rng.standard_normal((K, P, P, C)).astype(np.float32)), T(rois)

    def run(grad, rois):
        return ops.roi_align_backward(grad, rois, 1.0, P, P, 2, B, H, W, C, method="gather")

    def cached():
        return sorted((str(k), id(v)) for k, v in ops._roi_bwd_ws.items())

    (g0, r0), (g1, r1) = inputs(), inputs()
    alone0 = N(run(g0, r0))
    held = cached()
    alone1 = N(run(g1, r1))
    assert cached() == held and held, "a second call on the same stream must reuse the first one's workspace"
    assert np.abs(alone0).max() > 0 and not np.array_equal(alone0, alone1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())          # the inputs were uploaded on the current stream
    got0, ws0 = run(g0, r0), ops._roi_bwd_ws[(g0.device, L.stream())]
    with torch.cuda.stream(side):
        got1, ws1 = run(g1, r1), ops._roi_bwd_ws[(g1.device, L.stream())]
    torch.cuda.synchronize()
    assert ws0.data_ptr() != ws1.data_ptr(), "the side stream's call takes a workspace of its own"
    for got, alone, where in ((got0, alone0, "current"), (got1, alone1, "side")):
        assert np.array_equal(N(got).view(np.int32), alone.view(np.int32)), f"the call on the {where} stream differs from the same call made alone"


# --------------------------------------------------------------------------------------------------------------------------- full size
def test_full_size_forward():
    """B = 4, 38 x 63 x 1024, 512 RoIs per image through the 8 channel slices: against float64, and bit for bit against the oracle -- an
    exchanged slice or a dropped RoI shows in either"""
    from abr_iod_amd import ops
    c = case(rois="full", B=4, C=1024)
    rois, feat, want, S, bits = fwd_ref(c)
    assert len(rois) == 2048 and c.H * c.W * c.C * 4 > (2 << 20)
    got = N(ops.roi_align_forward(T(feat), T(rois), c.scale, c.PH, c.PW, c.sr))
    print(f"RATIO fwd nhwc full {R.worst_ratio(got, want, S):.3e}")
    check(got, want, S, "full-size NHWC forward")
    same_bits(got, bits, "full-size NHWC forward")
    fwd_ref.cache_clear()


@pytest.mark.parametrize("step", [1, 2])
def test_full_size_backward(step):
    """B = 4, 38 x 63 x 1024, 512 RoIs per image: the training step's call, gather and scatter each against float64"""
    c = case(rois="full", B=4, C=1024, step=step)
    rois = c.make_rois()
    assert len(rois) == 2048
    grad = c.make_grad(len(rois))
    want, S = R.backward(grad, rois, c.scale, c.PH, c.PW, c.sr, c.B, c.H, c.W, step)
    for route in ("gather", "scatter"):
        got = run_backward(route, c, grad, rois)
        print(f"RATIO bwd {route} full step{step} {R.worst_ratio(got, want, S):.3e}")
        check(got, want, S, f"full-size {route} backward, bin_step {step}", axes="b,y,x,c")

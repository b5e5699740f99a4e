"""The feature-pyramid pooler (abr_fpn_levels, abr_roi_align_pyramid_forward / _backward, modeling/poolers.py) against the level rule's
restatement, the CPU oracle's bits, the float64 reference and the reference implementation's own output (tests/golden/pooler_fpn.npz).

Every numeric comparison goes through roi_align_ref.check: finite, |got - want| <= 1e-6 * S with S the float64 sum of |addends|, exactly 0 where
nothing lands.  Forward results are in addition bit-equal to pooler_ref.expected_forward (oracle.ops.roi_align_forward per level, scattered
into zeros).  RoI sets: pooler_ref.roi_set -- the level rule's boundary rows, the rows without a level, random rows and ("zoo") the single-
level edge zoo rescaled to each level.  Pyramids: A = 256 x 384 with maps 64 x 96 ... 8 x 12; B = 200 x 300 with maps 50 x 75, 25 x 38,
13 x 19, 7 x 10 (no halves of one another); T = 64 x 96 with maps 16 x 24 ... 2 x 3 (the wide channel counts).  Two images everywhere.

Which kernel and launch shape each case reaches (fwd shape = pick_shape's (tx, bpb); chunks = channel chunks of the separable backward):

  kernel / instantiation            reached by
  --------------------------------  ------------------------------------------------------------------------------------------------
  fpn_levels_kernel                 test_levels (two blocks: K > 256 with the zoo)
  roi_align_pyramid_fwd<4>          (32, 8) C = 8;  (64, 4) C = 256;  (128, 2) C = 260;  (256, 1) C = 516 and, in two passes, C = 1028;
                                    pooled 14 x 14 and 3 x 5 at C = 8 (bins no multiple of bpb);  the no-level zero fill in every case
  roi_align_pyramid_fwd<1>          (32, 8) C = 5;  (128, 2) C = 70;  (256, 1) C = 514 (three passes)
  roi_align_pyramid_round           every backward: levels of different sizes back to back, accumulate 0 and 1
  roi_align_pyramid_bwd_sep<4>      pooled 7 x 7 and 3 x 5: one chunk C = 8, 256, 260, 516;  two chunks C = 1028
  roi_align_pyramid_bwd_sep<1>      one chunk C = 5, 70;  three chunks C = 514
  roi_align_pyramid_bwd<4>          pooled 14 x 14 at C = 8;  a level whose tables pass the LDS limit: test_lds_limit (2300 x 2 x 4)
  roi_align_pyramid_bwd<1>          pooled 14 x 14 at C = 5
"""
import ctypes
import functools
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import pooler_ref as P
from roi_align_ref import TOL, _seed, check

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
PYRAMIDS = {"A": ((256, 384), [(64, 96), (32, 48), (16, 24), (8, 12)]),
            "B": ((200, 300), [(50, 75), (25, 38), (13, 19), (7, 10)]),
            "T": ((64, 96), [(16, 24), (8, 12), (4, 6), (2, 3)])}
NB = 2
RULE = (P.K_MIN, P.K_MAX)


class Case(namedtuple("Case", "pyr C PH PW sr zoo")):
    @property
    def id(self):
        return f"{self.pyr}-C{self.C}-p{self.PH}x{self.PW}-sr{self.sr}{'-zoo' if self.zoo else ''}"

    @property
    def maps(self):
        return PYRAMIDS[self.pyr][1]

    @property
    def shapes(self):
        return [(NB, H, W, self.C) for H, W in self.maps]


def case(pyr, C, P_=7, sr=2, zoo=False):
    ph, pw = (P_, P_) if isinstance(P_, int) else P_
    return Case(pyr, C, ph, pw, sr, zoo)


CASES = [case(p, C, 7, sr, zoo=C <= 8) for p in "AB" for C in (5, 8, 256, 260) for sr in (2, 0)] + [
    case("A", 8, 14, 2, zoo=True), case("B", 8, 14, 0), case("B", 5, 14, 2),
    case("A", 8, (3, 5), 2, zoo=True), case("B", 8, (3, 5), 0),
    case("T", 70), case("T", 514, sr=0), case("T", 516), case("T", 1028, sr=0),
]
assert len({c.id for c in CASES}) == len(CASES)
ids = [c.id for c in CASES]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def rois_of(pyr, zoo):
    (ih, iw), maps = PYRAMIDS[pyr]
    rois, _ = P.roi_set(NB, ih, iw, maps, zoo=zoo)
    return rois, P.levels(rois)


@functools.lru_cache(maxsize=None)
def fwd_ref(c):
    rois, lv = rois_of(c.pyr, c.zoo)
    feats = P.make_feats(_seed("pooler_feats", *c), NB, c.C, c.maps)
    want, S = P.want_forward(feats, rois, lv, c.PH, c.PW, c.sr)
    exp = np.ascontiguousarray(P.expected_forward(feats, rois, lv, c.PH, c.PW, c.sr).transpose(0, 2, 3, 1))
    return rois, lv, feats, want, S, exp


@functools.lru_cache(maxsize=None)
def bwd_ref(c):
    rois, lv = rois_of(c.pyr, c.zoo)
    grad = np.random.default_rng(_seed("pooler_grad", *c)).standard_normal((len(rois), c.PH, c.PW, c.C)).astype(np.float32)
    return rois, lv, grad, P.want_backward(grad, rois, lv, c.shapes, c.PH, c.PW, c.sr)


def raw_backward(grad, rois, outs, PH, PW, sr, accumulate, scales=P.SCALES, rule=RULE):
    """abr_roi_align_pyramid_backward on the caller's own (prefilled) level tensors"""
    from abr_iod_amd import _lib as L
    n = len(outs)
    B, _, _, C = outs[0].shape
    ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    Hs, Ws = (ctypes.c_int * n)(*[o.shape[1] for o in outs]), (ctypes.c_int * n)(*[o.shape[2] for o in outs])
    sc = (ctypes.c_float * n)(*scales[:n])
    L.check(L.lib().abr_roi_align_pyramid_backward(L.ptr(grad), L.ptr(rois), rois.shape[0], B, C, Hs, Ws, sc, n, PH, PW, sr, rule[0], rule[1],
                                                   224.0, 4.0, 1e-6, int(accumulate), ptrs, L.stream()), "roi_align_pyramid_backward")
    torch.cuda.synchronize()


def fixture():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooler_fpn.npz"))
    maps = [tuple(int(v) for v in m) for m in d["maps"]]
    return d, P.make_feats(int(d["seed"]), int(d["B"]), int(d["C"]), maps)


# --------------------------------------------------------------------------------------------------------------------- 1. levels
@pytest.mark.parametrize("pyr,zoo", [("A", True), ("B", True), ("B", False)])
def test_levels(pyr, zoo):
    from abr_iod_amd import ops
    rois, lv = rois_of(pyr, zoo)
    assert (lv == -1).sum() == len(P.NO_LEVEL)
    got = ops.fpn_levels(T(rois), *RULE)
    assert got.dtype == torch.int32 and (N(got) == lv).all(), np.nonzero(N(got) != lv)[0]
    feats = [torch.zeros((NB, H, W, 4), device="cuda") for H, W in PYRAMIDS[pyr][1]]
    _, lo = ops.roi_align_pyramid_forward(feats, T(rois), P.SCALES, 7, 7, 2, *RULE, want_levels=True)
    assert lo.dtype == torch.int32 and (N(lo) == lv).all()


def test_levels_equal_the_reference_on_the_fixture():
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.poolers import LevelMapper
    from abr_iod_amd.structures.bounding_box import BoxList
    d, _ = fixture()
    ref = d["levels"]
    ok = (ref >= 0) & (ref <= 3)
    got = N(ops.fpn_levels(T(d["rois"]), *RULE))
    assert (got[ok] == ref[ok].astype(np.int64)).all() and (got[~ok] == -1).all()
    boxes = [BoxList(T(d["rois"][d["rois"][:, 0] == b, 1:]), (192, 128)) for b in range(2)]
    lm = LevelMapper(*RULE)(boxes)
    assert lm.dtype == torch.int64 and lm.is_cuda and (N(lm) == got).all()


# --------------------------------------------------------------------------------------------------------------------- 2. forward
@pytest.mark.parametrize("c", CASES, ids=ids)
def test_forward(c):
    from abr_iod_amd import ops
    rois, lv, feats, want, S, exp = fwd_ref(c)
    out, lo = ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), P.SCALES, c.PH, c.PW, c.sr, *RULE, want_levels=True)
    got = N(out)
    assert (N(lo) == lv).all()
    assert (bits(got[lv < 0]) == 0).all(), "rows without a level must be exactly zero"
    r = check(got, want, S, c.id)
    print(f"{c.id}: K = {len(rois)}, worst |err| / S = {r:.3e}")
    assert (bits(got) == bits(exp)).all(), f"{int((bits(got) != bits(exp)).sum())} elements differ from the oracle's bits"


def test_forward_out_writes_only_its_rows():
    from abr_iod_amd import ops
    c = CASES[ids.index("B-C5-p7x7-sr2-zoo")]
    rois, lv, feats, _, _, exp = fwd_ref(c)
    K = len(rois)
    buf = torch.full((K + 4, c.PH, c.PW, c.C), SENTINEL, device="cuda")
    ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), P.SCALES, c.PH, c.PW, c.sr, *RULE, out=buf[2:K + 2])
    got = N(buf)
    assert (got[:2] == SENTINEL).all() and (got[K + 2:] == SENTINEL).all()
    assert (bits(got[2:K + 2]) == bits(exp)).all()


def test_forward_no_rois():
    from abr_iod_amd import ops
    feats = [torch.randn((NB, H, W, 8), device="cuda") for H, W in PYRAMIDS["B"][1]]
    out, lo = ops.roi_align_pyramid_forward(feats, torch.zeros((0, 5), device="cuda"), P.SCALES, 7, 7, 2, *RULE, want_levels=True)
    assert tuple(out.shape) == (0, 7, 7, 8) and tuple(lo.shape) == (0,)


@pytest.mark.parametrize("layout", ["one_level", "one_image"])
def test_forward_layouts(layout):
    """every RoI on level 2 (the other maps unused), every RoI on the last image"""
    from abr_iod_amd import ops
    c = case("B", 8)
    rois, lv = rois_of("B", False)
    if layout == "one_level":
        rois = rois[lv == 2]
    else:
        rois = rois.copy()
        rois[:, 0] = NB - 1
    lv = P.levels(rois)
    feats = P.make_feats(7, NB, c.C, c.maps)
    exp = P.expected_forward(feats, rois, lv, 7, 7, 2).transpose(0, 2, 3, 1)
    got = N(ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), P.SCALES, 7, 7, 2, *RULE))
    assert len(rois) >= 8 and (bits(got) == bits(exp)).all()


def test_forward_single_level_is_roi_align():
    """L = 1: every row with a level is on level 0 and has the single-level operator's bits; the rows without a level are zero"""
    from abr_iod_amd import ops
    rois, lv = rois_of("B", True)
    feat = torch.randn((NB, 13, 19, 12), device="cuda")
    out, lo = ops.roi_align_pyramid_forward([feat], T(rois), (0.0625,), 7, 7, 2, 4.0, 4.0, want_levels=True)
    one = ops.roi_align_forward(feat, T(rois), 0.0625, 7, 7, 2)
    ok = lv >= 0
    assert (N(lo)[ok] == 0).all() and (N(lo)[~ok] == -1).all()
    assert (bits(N(out)[ok]) == bits(N(one)[ok])).all() and (bits(N(out)[~ok]) == 0).all()


# --------------------------------------------------------------------------------------------------------------------- 3. the fixture
def test_pooler_module_reproduces_the_reference_output():
    from abr_iod_amd.modeling.poolers import Pooler
    from abr_iod_amd.structures.bounding_box import BoxList
    d, feats = fixture()
    rois = d["rois"]
    boxes = [BoxList(T(rois[rois[:, 0] == b, 1:]), (192, 128)) for b in range(2)]
    assert [len(b) for b in boxes] == d["per_image"].tolist()
    x = [T(f).permute(0, 3, 1, 2) for f in feats]
    out = Pooler((7, 7), P.SCALES, 2)(x, boxes)
    assert tuple(out.shape) == d["out"].shape
    assert (bits(N(out)) == bits(d["out"])).all()


# --------------------------------------------------------------------------------------------------------------------- 4. backward
@pytest.mark.parametrize("c", CASES, ids=ids)
def test_backward(c):
    """Each level's gradient against the float64 transpose over that level's rows, 1e-6 relative to the sum of |addends|.

    MEASURED, MI355X, ten runs per zoo case: worst |err| / S = 1.9e-7 (B-C8-p7x7-sr0-zoo level 0), the same figure in every run.  The
    backward adds into float64 scratch and rounds once.  With float32 atomics (the first form of this kernel, and what
    ops.roi_align_backward(method="scatter") does on one level) A-C8-p3x5-sr2-zoo reached 1.07e-6 and 1.11e-6 on levels 0 and 1 in 9 runs of
    10 and B-C5-p7x7-sr0-zoo passed or failed with the order of the adds: at (b, y, x, c) = (1, 10, 32, 3) of level 1 three random rows add
    0.016, 0.129 and 0.259 and the 300 copies of the zoo's `same_roi` (the level-3 zoo lands on level 1; that pixel is the rim of its
    footprint) then add terms of mean magnitude 3.0e-7, each rounding at the ulp (3.0e-8) of a sum the three large terms set.  Adding the
    float64 addends in RoI order in float32 on the CPU gives that kernel's value to the bit, |err| / S = 1.1198e-6; in reverse order 1.3e-8."""
    rois, lv, grad, wants = bwd_ref(c)
    outs = [torch.full(s, SENTINEL, device="cuda") for s in c.shapes]
    raw_backward(T(grad), T(rois), outs, c.PH, c.PW, c.sr, accumulate=0)
    for l, (o, (want, S)) in enumerate(zip(outs, wants)):
        r = check(N(o), want, S, f"{c.id} level {l}", axes="b,y,x,c", tol=TOL)     # (exactly 0 where S == 0: the sentinel is gone)
        print(f"{c.id} level {l}: worst |err| / S = {r:.3e}")


def test_backward_unused_levels_are_zero_filled():
    c = case("B", 8)
    rois, lv = rois_of("B", False)
    rois = rois[lv == 1]
    grad = np.random.default_rng(3).standard_normal((len(rois), 7, 7, 8)).astype(np.float32)
    wants = P.want_backward(grad, rois, P.levels(rois), c.shapes, 7, 7, 2)
    outs = [torch.full(s, SENTINEL, device="cuda") for s in c.shapes]
    raw_backward(T(grad), T(rois), outs, 7, 7, 2, accumulate=0)
    for l, (o, (want, S)) in enumerate(zip(outs, wants)):
        if l != 1:
            assert (S == 0).all() and (bits(N(o)) == 0).all(), l
        check(N(o), want, S, f"level {l}", axes="b,y,x,c")


def test_backward_accumulates_into_out():
    from abr_iod_amd import ops
    c = CASES[ids.index("B-C8-p7x7-sr2-zoo")]
    rois, lv, grad, wants = bwd_ref(c)
    base = [np.random.default_rng(10 + l).standard_normal(s).astype(np.float32) for l, s in enumerate(c.shapes)]
    outs = [T(b) for b in base]
    res = ops.roi_align_pyramid_backward(T(grad), T(rois), P.SCALES, c.PH, c.PW, c.sr, c.shapes, *RULE, out=outs)
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs))
    for l, (o, b, (want, S)) in enumerate(zip(outs, base, wants)):
        check(N(o), want + b, S + np.abs(b), f"accumulate level {l}", axes="b,y,x,c")
    fresh = ops.roi_align_pyramid_backward(T(grad), T(rois), P.SCALES, c.PH, c.PW, c.sr, c.shapes, *RULE)
    for l, (o, (want, S)) in enumerate(zip(fresh, wants)):
        check(N(o), want, S, f"fresh level {l}", axes="b,y,x,c")


def test_backward_rows_without_a_level_add_nothing_and_no_rois_zero_fill():
    c = case("B", 8)
    rois, lv = rois_of("B", False)
    none = rois[lv < 0]
    assert len(none) == len(P.NO_LEVEL)
    for r in (none, np.zeros((0, 5), np.float32)):
        outs = [torch.full(s, SENTINEL, device="cuda") for s in c.shapes]
        raw_backward(torch.ones((len(r), 7, 7, 8), device="cuda"), T(r), outs, 7, 7, 2, accumulate=0)
        assert all((bits(N(o)) == 0).all() for o in outs)
        raw_backward(torch.ones((len(r), 7, 7, 8), device="cuda"), T(r), outs, 7, 7, 2, accumulate=1)
        assert all((bits(N(o)) == 0).all() for o in outs)


def test_lds_limit():
    """a level of 2300 x 2: its separable tables (7 * 2302 floats) pass the 60 KB limit, so every level takes the direct scatter kernel"""
    from abr_iod_amd import ops
    maps, scales, rule = [(2300, 2), (8, 8)], (0.25, 0.125), (2.0, 3.0)
    rng = np.random.default_rng(5)
    rows = [[0, 0.0, y, 7.0, y + h] for y, h in zip(rng.uniform(0, 9000, 12), rng.uniform(4, 100, 12))] + \
           [[0, x, y, x + 150, y + 140] for x, y in rng.uniform(-20, 40, (6, 2))] + [[0, 5.0, 5.0, 1.0, 9.0]]
    rois = np.array(rows, np.float32)
    lv = P.levels(rois, *rule)
    assert (lv == 0).sum() >= 6 and (lv == 1).sum() >= 6 and (lv == -1).sum() == 1
    shapes = [(1, H, W, 4) for H, W in maps]
    feats = P.make_feats(9, 1, 4, maps)
    exp = P.expected_forward(feats, rois, lv, 7, 7, 2, scales).transpose(0, 2, 3, 1)
    got = N(ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), scales, 7, 7, 2, *rule))
    assert (bits(got) == bits(exp)).all()
    grad = rng.standard_normal((len(rois), 7, 7, 4)).astype(np.float32)
    outs = [torch.full(s, SENTINEL, device="cuda") for s in shapes]
    raw_backward(T(grad), T(rois), outs, 7, 7, 2, 0, scales, rule)
    for l, (o, (want, S)) in enumerate(zip(outs, P.want_backward(grad, rois, lv, shapes, 7, 7, 2, scales))):
        check(N(o), want, S, f"lds limit level {l}", axes="b,y,x,c")


# --------------------------------------------------------------------------------------------------------------------- 5. autograd
def _module_inputs(c, rois, feats):
    from abr_iod_amd.structures.bounding_box import BoxList
    (ih, iw), _ = PYRAMIDS[c.pyr]
    order = np.argsort(rois[:, 0], kind="stable")
    boxes = [BoxList(T(rois[rois[:, 0] == b, 1:]), (iw, ih)) for b in range(NB)]
    x = [T(f).permute(0, 3, 1, 2).requires_grad_() for f in feats]
    return order, boxes, x


def test_pooler_autograd():
    from abr_iod_amd.modeling.poolers import Pooler
    c = CASES[ids.index("B-C8-p7x7-sr2-zoo")]
    rois, lv, feats, want, S, exp = fwd_ref(c)
    _, _, grad, _ = bwd_ref(c)
    order, boxes, x = _module_inputs(c, rois, feats)
    out = Pooler((c.PH, c.PW), P.SCALES, c.sr)(x, boxes)
    assert (bits(N(out.permute(0, 2, 3, 1))) == bits(exp[order])).all()
    out.backward(T(grad[order]).permute(0, 3, 1, 2))
    for l, (xl, (w, s)) in enumerate(zip(x, P.want_backward(grad[order], rois[order], lv[order], c.shapes, c.PH, c.PW, c.sr))):
        assert xl.grad is not None and tuple(xl.grad.shape) == tuple(xl.shape)
        check(N(xl.grad.permute(0, 2, 3, 1)), w, s, f"autograd level {l}", axes="b,y,x,c", tol=TOL)


def test_single_scale_pooler_is_roi_align():
    from abr_iod_amd.layers import ROIAlign
    from abr_iod_amd.modeling.poolers import Pooler
    rois, _ = rois_of("B", False)
    rois = rois[~np.isnan(rois).any(1)]
    x = torch.randn((NB, 13, 19, 12), device="cuda").permute(0, 3, 1, 2)
    a = Pooler((7, 7), (0.0625,), 2)([x], T(rois))
    b = ROIAlign((7, 7), 0.0625, 2)(x, T(rois))
    assert (bits(N(a)) == bits(N(b))).all()


# --------------------------------------------------------------------------------------------------------------------- 6. no host round trip
def test_pooler_makes_no_host_round_trip():
    from abr_iod_amd.modeling.poolers import Pooler
    c = case("B", 8)
    rois, _ = rois_of("B", False)
    feats = P.make_feats(1, NB, c.C, c.maps)
    pooler = Pooler((7, 7), P.SCALES, 2)
    g = torch.randn((len(rois), c.C, 7, 7), device="cuda")

    def step():
        _, boxes, x = _module_inputs(c, rois[np.argsort(rois[:, 0], kind="stable")], feats)
        torch.cuda.synchronize()
        return boxes, x

    boxes, x = step()
    pooler(x, boxes).backward(g)     # warm-up: library load, allocator
    boxes, x = step()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        pooler(x, boxes).backward(g)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    assert all(xl.grad is not None for xl in x)


# --------------------------------------------------------------------------------------------------------------------- 7. wrapper errors
def test_wrapper_errors_name_the_argument():
    from abr_iod_amd import ops
    rois = torch.zeros((3, 5), device="cuda")

    def maps(C=8, B=NB, n=4):
        return [torch.zeros((B, 8 >> min(l, 2), 8 >> min(l, 2), C), device="cuda") for l in range(n)]

    def fwd(feats, scales=P.SCALES):
        return ops.roi_align_pyramid_forward(feats, rois, scales, 7, 7, 2, *RULE)

    f = maps()
    f[2] = maps(C=12)[2]
    with pytest.raises(RuntimeError, match=r"C of feats\[2\]"):
        fwd(f)
    f = maps()
    f[1] = maps(B=3)[1]
    with pytest.raises(RuntimeError, match=r"B of feats\[1\]"):
        fwd(f)
    f = maps()
    f[3] = f[3].cpu()
    with pytest.raises(RuntimeError, match=r"feats\[3\] is a CPU tensor"):
        fwd(f)
    with pytest.raises(RuntimeError, match=r"feats has 9 levels"):
        fwd(maps(n=9), scales=(0.25,) * 9)
    with pytest.raises(RuntimeError, match="scales"):
        fwd(maps(), scales=P.SCALES[:3])

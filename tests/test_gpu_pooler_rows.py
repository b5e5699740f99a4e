"""The indexed feature-pyramid pooler (abr_roi_align_pyramid_rows_forward / _backward, ops.roi_align_pyramid_*(rows=), Pooler.forward(rows=)):
pooling SELECTED rows of a RoI table, the -1-padded positives list of the FPN mask head, in one launch each way.

Table and pyramid: the 74 RoIs, two images and four maps of tests/golden/pooler_fpn.npz (its two no-level rows, 6 and 42, are in the lists);
the maps are drawn per channel count by pooler_ref.make_feats.  Bounds: those of tests/test_gpu_pooler.py -- forward and backward through
roi_align_ref.check at 1e-6 of the float64 sum of |addends|, exactly 0 where nothing lands; forward in addition bit-equal to the unindexed
call's rows.

Which kernel each case reaches (the backward dispatcher has two routes: the separable kernel for pooled sides <= 8 whose tables fit LDS, the
direct scatter otherwise):

  roi_align_pyramid_rows_fwd<4> / <1>        C = 8 / C = 6, every pooled size
  roi_align_pyramid_rows_bwd_sep<4> / <1>    C = 8 / C = 6, pooled 7 x 7 (adaptive grid) and 1 x 1
  roi_align_pyramid_rows_bwd<4> / <1>        C = 8 / C = 6, pooled 14 x 14 (the mask head's own shape)
"""
import functools
import os

import numpy as np
import pytest
import torch

import pooler_ref as P
from roi_align_ref import TOL, _seed, check

pytestmark = pytest.mark.gpu

SENTINEL = -12345.0
RULE = (P.K_MIN, P.K_MAX)
GEOMS = [(14, 2), (7, 0), (1, 2)]
CASES = [(C, ph, sr) for C in (8, 6) for ph, sr in GEOMS]
case_ids = [f"C{C}-p{ph}-sr{sr}" for C, ph, sr in CASES]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def table():
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooler_fpn.npz"))
    rois = d["rois"]
    maps = [tuple(int(v) for v in m) for m in d["maps"]]
    lv = P.levels(rois)
    assert len(rois) == 74 and (np.nonzero(lv < 0)[0] == [6, 42]).all() and all((lv == l).sum() >= 8 for l in range(4))
    return rois, lv, maps, int(d["B"])


def row_lists():
    """name -> int64 rows; K = 74"""
    K = len(table()[0])
    tail = [0, 1, 2, 4, 6, 9, 16, 19, 20, 21, 26, 27, 33, 38, 42, 49, 50, 56, 59, 63, 73]      # ascending, all four levels, both no-level rows
    mixed = [-1, 73, -1, -1, 3, 3, 42, -1, 58, 1, -1, 19, 0, -7, 28, -1]                        # unordered, a repeat, other negatives
    return {"tail": np.array(tail + [-1] * 5, np.int64), "interleaved": np.array(mixed, np.int64), "all_padding": np.full(9, -1, np.int64),
            "empty": np.zeros(0, np.int64), "beyond": np.array([5, K, 70, 2 ** 40, -1, K - 1, 2 ** 31 + 3], np.int64)}


ROWS = sorted(row_lists())


def valid(rows):
    K = len(table()[0])
    return (rows >= 0) & (rows < K)


@functools.lru_cache(maxsize=None)
def fwd_ref(C, ph, sr):
    """the maps and the float64 pair of the WHOLE table, computed once per case and gathered by every row list"""
    rois, lv, maps, B = table()
    feats = P.make_feats(_seed("pooler_rows_feats", C), B, C, maps)
    want, S = P.want_forward(feats, rois, lv, ph, ph, sr)
    return feats, want, S


def shapes_of(C):
    _, _, maps, B = table()
    return [(B, H, W, C) for H, W in maps]


def gathered_backward_ref(grad, rows, C, ph, sr):
    """float64 (want, S) per level: the transpose over the gathered rows alone"""
    rois, lv, _, _ = table()
    ok = valid(rows)
    idx = rows[ok]
    return P.want_backward(grad[ok], rois[idx], lv[idx], shapes_of(C), ph, ph, sr)


def draw_grad(rows, C, ph, name, fill):
    g = np.random.default_rng(_seed("pooler_rows_grad", C, ph, name)).standard_normal((len(rows), ph, ph, C)).astype(np.float32)
    g[~valid(rows)] = fill
    return g


# --------------------------------------------------------------------------------------------------------------------- forward
@pytest.mark.parametrize("name", ROWS)
@pytest.mark.parametrize("C,ph,sr", CASES, ids=case_ids)
def test_forward(C, ph, sr, name):
    from abr_iod_amd import ops
    rois, lv, _, _ = table()
    rows = row_lists()[name]
    feats, want, S = fwd_ref(C, ph, sr)
    xs = [T(f) for f in feats]
    whole, whole_lv = ops.roi_align_pyramid_forward(xs, T(rois), P.SCALES, ph, ph, sr, *RULE, want_levels=True)
    buf = torch.full((len(rows) + 2, ph, ph, C), SENTINEL, device="cuda")
    out, lo = ops.roi_align_pyramid_forward(xs, T(rois), P.SCALES, ph, ph, sr, *RULE, want_levels=True, rows=T(rows), out=buf[1:len(rows) + 1])
    got, ok = N(out), valid(rows)
    assert tuple(got.shape) == (len(rows), ph, ph, C) and lo.dtype == torch.int32 and tuple(lo.shape) == (len(rows),)
    assert (N(buf[0]) == SENTINEL).all() and (N(buf[-1]) == SENTINEL).all(), "wrote outside its rows"
    assert (bits(got[ok]) == bits(N(whole)[rows[ok]])).all(), "a pooled row differs from the unindexed call's bits"
    assert (bits(got[~ok]) == 0).all(), "padding rows must be exactly zero"
    assert (N(lo)[ok] == N(whole_lv)[rows[ok]]).all() and (N(lo)[ok] == lv[rows[ok]]).all() and (N(lo)[~ok] == -1).all()
    w, s = np.zeros(got.shape), np.zeros(got.shape)
    w[ok], s[ok] = want[rows[ok]], S[rows[ok]]
    r = check(got, w, s, f"{name} C{C} p{ph} sr{sr}")
    print(f"{name} C{C} p{ph} sr{sr}: P = {len(rows)}, worst |err| / S = {r:.3e}")


def test_forward_without_rows_is_unchanged():
    """the fixture's recorded output of the reference Pooler, still to the bit, through the same wrapper"""
    from abr_iod_amd import ops
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pooler_fpn.npz"))
    rois, _, maps, B = table()
    feats = P.make_feats(int(d["seed"]), B, int(d["C"]), maps)
    got = N(ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), P.SCALES, 7, 7, 2, *RULE))
    assert (bits(got) == bits(d["out"].transpose(0, 2, 3, 1))).all()
    sel = row_lists()["tail"]
    part = N(ops.roi_align_pyramid_forward([T(f) for f in feats], T(rois), P.SCALES, 7, 7, 2, *RULE, rows=T(sel)))
    ok = valid(sel)
    assert (bits(part[ok]) == bits(d["out"].transpose(0, 2, 3, 1)[sel[ok]])).all() and (bits(part[~ok]) == 0).all()


def test_empty_table_is_all_padding():
    from abr_iod_amd import ops
    _, _, maps, B = table()
    xs = [torch.randn((B, H, W, 8), device="cuda") for H, W in maps]
    out, lo = ops.roi_align_pyramid_forward(xs, torch.zeros((0, 5), device="cuda"), P.SCALES, 14, 14, 2, *RULE, want_levels=True,
                                            rows=T(np.array([0, -1, 3], np.int64)))
    assert tuple(out.shape) == (3, 14, 14, 8) and (bits(N(out)) == 0).all() and (N(lo) == -1).all()


# --------------------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("name", ROWS)
@pytest.mark.parametrize("C,ph,sr", CASES, ids=case_ids)
def test_backward(C, ph, sr, name):
    """against the float64 transpose over the gathered rows; NaN in every padding row of grad changes nothing (both results meet the same
    bound: the order of the float64 atomics varies from run to run, so two runs are not compared bit for bit); every level is written whole
    (sentinel-filled outputs, exactly 0 where nothing lands -- for `all_padding` and `empty` that is every element of every level)"""
    from abr_iod_amd import _lib as L
    import ctypes
    rois, _, _, B = table()
    rows = row_lists()[name]
    wants = gathered_backward_ref(draw_grad(rows, C, ph, name, 0.0), rows, C, ph, sr)
    for fill in (0.0, np.nan):
        grad = T(draw_grad(rows, C, ph, name, fill))
        outs = [torch.full(s, SENTINEL, device="cuda") for s in shapes_of(C)]
        n = len(outs)
        ptrs = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
        Hs, Ws = (ctypes.c_int * n)(*[o.shape[1] for o in outs]), (ctypes.c_int * n)(*[o.shape[2] for o in outs])
        sc = (ctypes.c_float * n)(*P.SCALES)
        r_, t_ = T(rows), T(rois)
        L.check(L.lib().abr_roi_align_pyramid_rows_backward(L.ptr(grad), L.ptr(t_), L.ptr(r_), len(rows), len(rois), B, C, Hs, Ws, sc, n, ph, ph, sr,
                                                            RULE[0], RULE[1], 224.0, 4.0, 1e-6, 0, ptrs, L.stream()), "rows_backward")
        torch.cuda.synchronize()
        for l, (o, (want, S)) in enumerate(zip(outs, wants)):
            r = check(N(o), want, S, f"{name} C{C} p{ph} sr{sr} fill {fill} level {l}", axes="b,y,x,c", tol=TOL)
            print(f"{name} C{C} p{ph} sr{sr} fill {fill} level {l}: worst |err| / S = {r:.3e}")


@pytest.mark.parametrize("C,ph,sr", [(8, 14, 2), (6, 7, 0)], ids=["direct", "separable"])
def test_backward_accumulates_into_out(C, ph, sr):
    from abr_iod_amd import ops
    rois = table()[0]
    for name in ("tail", "all_padding", "empty"):
        rows = row_lists()[name]
        grad = draw_grad(rows, C, ph, name, np.nan)
        wants = gathered_backward_ref(grad, rows, C, ph, sr)
        base = [np.random.default_rng(10 + l).standard_normal(s).astype(np.float32) for l, s in enumerate(shapes_of(C))]
        outs = [T(b) for b in base]
        res = ops.roi_align_pyramid_backward(T(grad), T(rois), P.SCALES, ph, ph, sr, shapes_of(C), *RULE, out=outs, rows=T(rows))
        assert all(r.data_ptr() == o.data_ptr() for r, o in zip(res, outs))
        for l, (o, b, (want, S)) in enumerate(zip(outs, base, wants)):
            check(N(o), want + b, S + np.abs(b), f"{name} accumulate level {l}", axes="b,y,x,c")
            if not valid(rows).any():
                assert (bits(N(o)) == bits(b)).all(), "nothing to add must leave the buffer as it was"


def test_backward_writes_unreached_levels_whole():
    """rows on level 1 alone: the other three levels are exactly zero, not left as they were"""
    from abr_iod_amd import ops
    rois, lv, _, _ = table()
    rows = np.concatenate([np.nonzero(lv == 1)[0][:6], [-1, -1]]).astype(np.int64)
    grad = draw_grad(rows, 8, 14, "level1", np.nan)
    wants = gathered_backward_ref(grad, rows, 8, 14, 2)
    outs = ops.roi_align_pyramid_backward(T(grad), T(rois), P.SCALES, 14, 14, 2, shapes_of(8), *RULE, rows=T(rows))
    for l, (o, (want, S)) in enumerate(zip(outs, wants)):
        if l != 1:
            assert (S == 0).all() and (bits(N(o)) == 0).all(), l
        check(N(o), want, S, f"level {l}", axes="b,y,x,c")
    assert (wants[1][1] > 0).any()


# --------------------------------------------------------------------------------------------------------------------- the module
def test_pooler_rows_autograd_tag_and_no_host_round_trip():
    """Pooler.forward(x, table, rows): the op's rows forward, the indexed backward into every map, the levels' amax bound on the result, and no
    host synchronisation either way"""
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.poolers import Pooler
    C, ph, sr = 8, 14, 2
    rois = table()[0]
    rows = row_lists()["tail"]
    feats, _, _ = fwd_ref(C, ph, sr)
    grad = draw_grad(rows, C, ph, "module", 0.0)
    wants = gathered_backward_ref(grad, rows, C, ph, sr)
    pooler = Pooler((ph, ph), P.SCALES, sr)
    t_rois, t_rows, g = T(rois), T(rows), T(grad).permute(0, 3, 1, 2)
    g_nan = g.clone()
    g_nan[T(~valid(rows))] = float("nan")

    def maps(tagged=False):
        xs = [T(f.transpose(0, 3, 1, 2)).contiguous(memory_format=torch.channels_last) for f in feats]
        for t in xs if tagged else ():
            ops.amax_carry(t, ops.amax_compute(t.permute(0, 2, 3, 1)))
        return xs

    x = [t.requires_grad_() for t in maps()]
    pooler(x, t_rois, t_rows).backward(g)      # warm-up: library load, allocator
    x = [t.requires_grad_() for t in maps()]
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = pooler(x, t_rois, t_rows)
        out.backward(g_nan)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    torch.cuda.synchronize()
    direct = ops.roi_align_pyramid_forward([T(f) for f in feats], t_rois, P.SCALES, ph, ph, sr, *RULE, rows=t_rows)
    assert tuple(out.shape) == (len(rows), C, ph, ph) and (bits(N(out.permute(0, 2, 3, 1))) == bits(N(direct))).all()
    for l, (xl, (w, s)) in enumerate(zip(x, wants)):
        assert xl.grad is not None and tuple(xl.grad.shape) == tuple(xl.shape)
        check(N(xl.grad.permute(0, 2, 3, 1)), w, s, f"autograd level {l}", axes="b,y,x,c", tol=TOL)
    # a subset of the table's rows plus zeros keeps the bound the whole table's result carries
    assert ops.amax_of(pooler(maps(), t_rois, t_rows))[0] is None
    if ops.H3_TAGS:
        part, whole = pooler(maps(True), t_rois, t_rows), pooler(maps(True), t_rois)
        assert ops.amax_of(part)[0] is not None and ops.amax_of(whole)[0] is not None
        assert (N(part) == N(whole)[rows[valid(rows)].tolist() + [6] * int((~valid(rows)).sum())]).all()    # (row 6 has no level: zeros)


def test_single_level_pooler_takes_rows_too():
    """one scale: the rows go through the pyramid kernels with L = 1 and have the single-level operator's bits"""
    from abr_iod_amd.layers import ROIAlign
    from abr_iod_amd.modeling.poolers import Pooler
    rois = table()[0]
    rois = rois[~np.isnan(rois).any(1)]
    rows = np.array([3, -1, 0, 40, len(rois)], np.int64)
    x = torch.randn((2, 12, 13, 19), device="cuda").contiguous(memory_format=torch.channels_last)
    a = N(Pooler((7, 7), (0.0625,), 2)([x], T(rois), T(rows)))
    b = N(ROIAlign((7, 7), 0.0625, 2)(x, T(rois)))
    lv = P.levels(rois[[3, 0, 40]], 4.0, 4.0)
    assert (lv == 0).all() and (bits(a[[0, 2, 3]]) == bits(b[[3, 0, 40]])).all() and (bits(a[[1, 4]]) == 0).all()


def test_wrapper_errors_name_rows():
    from abr_iod_amd import ops
    _, _, maps, B = table()
    xs = [torch.zeros((B, H, W, 8), device="cuda") for H, W in maps]
    rois = torch.zeros((3, 5), device="cuda")
    with pytest.raises(RuntimeError, match="rows must be a one-dimensional int64"):
        ops.roi_align_pyramid_forward(xs, rois, P.SCALES, 7, 7, 2, *RULE, rows=torch.zeros(2, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="rows is on cpu"):
        ops.roi_align_pyramid_forward(xs, rois, P.SCALES, 7, 7, 2, *RULE, rows=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"grad \(3, 7, 7, 8\) is not \[2, 7, 7, 8\]"):
        ops.roi_align_pyramid_backward(torch.zeros((3, 7, 7, 8), device="cuda"), rois, P.SCALES, 7, 7, 2, [tuple(x.shape) for x in xs], *RULE,
                                       rows=torch.zeros(2, dtype=torch.int64, device="cuda"))

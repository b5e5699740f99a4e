"""CPU: the feature-pyramid pooler's references agree with the reference implementation's own run (tests/golden/pooler_fpn.npz, written by
tests/golden/make_golden_pooler.py from maskrcnn_benchmark/modeling/poolers.py), and the library declares, binds and validates its three
entry points.  No GPU: the argument checks return before any launch."""
import ctypes as C
import os
import re

import numpy as np

import pooler_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAMES = ("abr_fpn_levels", "abr_roi_align_pyramid_forward", "abr_roi_align_pyramid_backward")


def fixture():
    d = np.load(os.path.join(HERE, "golden", "pooler_fpn.npz"))
    maps = [tuple(int(v) for v in m) for m in d["maps"]]
    feats = P.make_feats(int(d["seed"]), int(d["B"]), int(d["C"]), maps)
    return d["rois"], d["levels"], d["out"], feats


def test_level_rule_equals_the_reference_on_the_fixture():
    rois, ref_levels, ref_out, _ = fixture()
    mine = P.levels(rois)
    in_range = (ref_levels >= 0) & (ref_levels <= P.K_MAX - P.K_MIN)
    assert in_range.sum() >= 60
    assert (mine[in_range] == ref_levels[in_range].astype(np.int64)).all(), np.nonzero(mine[in_range] != ref_levels[in_range])[0]
    # the reference's out-of-range rows are exactly the rows without a level, and their output is all zero
    assert ((mine == -1) == ~in_range).all()
    assert (~in_range).sum() == len(P.NO_LEVEL)
    assert (ref_out[~in_range] == 0).all()
    assert np.isfinite(ref_out).all()


def test_level_rule_at_its_boundaries():
    rows = {n: [0, x1, y1, x2, y2] for n, x1, y1, x2, y2 in P.edge_rows(128, 192)}
    lv = dict(zip(rows, P.levels(np.array(list(rows.values()), np.float32)).tolist()))
    # a square of side 2^k * 56 sits exactly on a boundary: the eps lifts it onto the upper level; 896 clamps to k_max
    assert [lv[f"square_{s}"] for s in (56, 112, 224, 448, 896)] == [0, 1, 2, 3, 3]
    assert lv["224x223"] == 1 and lv["448x447"] == 2
    assert lv["one_by_one"] == 0 and lv["area_zero"] == 0 and lv["both_sides_negative"] == 0
    assert lv["far_larger_than_image"] == 3
    assert lv["negative_area"] == -1 and lv["nan_coordinate"] == -1
    # no random row of a set lies within the margin of a boundary in float64, and float32 and float64 agree on every row with a level
    rois, _ = P.roi_set(2, 256, 384, [(64, 96), (32, 48), (16, 24), (8, 12)], zoo=True)
    v64 = P.level_value(rois, dtype=np.float64)
    ok = ~np.isnan(v64)
    got = P.levels(rois)
    assert (got[ok] == np.clip(np.floor(v64[ok]), P.K_MIN, P.K_MAX).astype(np.int64) - int(P.K_MIN)).all()
    assert (got[~ok] == -1).all()


def test_expected_forward_is_the_reference_output_bit_for_bit():
    rois, ref_levels, ref_out, feats = fixture()
    got = P.expected_forward(feats, rois, P.levels(rois), 7, 7, 2)
    assert got.dtype == ref_out.dtype == np.float32 and got.shape == ref_out.shape
    assert (got.view(np.uint32) == ref_out.view(np.uint32)).all()
    # and the float64 reference holds the reference's output within the project's bound
    want, S = P.want_forward(feats, rois, P.levels(rois), 7, 7, 2)
    P.R.check(ref_out.transpose(0, 2, 3, 1), want, S, "reference Pooler vs float64")


def test_symbols_declared_and_bound():
    from abr_iod_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "abr_iod_hip.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, src), f"{n} not declared"
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+ABR_MAX_PYRAMID_LEVELS\s+8\b", src)


def test_bad_arguments_return_minus_one_without_a_launch():
    from abr_iod_amd import _lib
    L = _lib.lib()
    H, W, sc = (C.c_int * 9)(*[8] * 9), (C.c_int * 9)(*[8] * 9), (C.c_float * 9)(*[0.25] * 9)
    ptrs = (C.c_void_p * 9)(*[0] * 9)     # (never dereferenced: every call below is refused first)
    rule = (2.0, 2.0, 224.0, 4.0, 1e-6)

    def fwd(feats=ptrs, L_=1, PH=7, K=4):
        return L.abr_roi_align_pyramid_forward(feats, H, W, sc, L_, None, K, 1, 8, PH, 7, 2, *rule, None, None, None)

    def bwd(gfeats=ptrs, L_=1, PH=7, K=4):
        return L.abr_roi_align_pyramid_backward(None, None, K, 1, 8, H, W, sc, L_, PH, 7, 2, *rule, 0, gfeats, None)

    for name, fn in (("roi_align_pyramid_forward", fwd), ("roi_align_pyramid_backward", bwd)):
        for kw in (dict(L_=0), dict(L_=9), dict(PH=0), {"feats" if fn is fwd else "gfeats": None}):
            assert fn(**kw) == -1, (name, kw)
            assert name.encode() in L.abr_last_error(), (name, kw, L.abr_last_error())
    # a null map at a level, K > 0
    assert fwd() == -1 and b"roi_align_pyramid_forward" in L.abr_last_error()
    assert bwd() == -1 and b"roi_align_pyramid_backward" in L.abr_last_error()
    # k_min .. k_max naming more levels than there are
    assert L.abr_roi_align_pyramid_forward(ptrs, H, W, sc, 2, None, 4, 1, 8, 7, 7, 2, 2.0, 5.0, 224.0, 4.0, 1e-6, None, None, None) == -1
    assert b"roi_align_pyramid_forward" in L.abr_last_error()
    # an extent that does not fit int32
    big = (C.c_int * 1)(1 << 20)
    assert L.abr_roi_align_pyramid_forward(ptrs, big, big, sc, 1, None, 4, 1, 8, 7, 7, 2, *rule, None, None, None) == -1
    assert b"int32" in L.abr_last_error()
    assert L.abr_fpn_levels(None, -1, 2.0, 5.0, 224.0, 4.0, 1e-6, None, None) == -1 and b"fpn_levels" in L.abr_last_error()
    assert L.abr_fpn_levels(None, 4, 2.0, 5.0, 224.0, 4.0, 1e-6, None, None) == -1 and b"fpn_levels" in L.abr_last_error()
    assert L.abr_fpn_levels(None, 0, 2.0, 5.0, 224.0, 4.0, 1e-6, None, None) == 0

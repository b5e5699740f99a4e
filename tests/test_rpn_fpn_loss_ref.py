"""CPU: the float64 restatement of the RPN loss over a feature pyramid (tests/rpn_fpn_loss_ref.py) against the golden written by the reference's
own AnchorGenerator, RPNLossComputation, Matcher, sampler and BoxCoder (tests/golden/make_golden_rpn_fpn_loss.py -> rpn_fpn_loss.npz), the order
of the concatenation, the one place where matching over all levels differs from matching level by level, and the argument checks of the two new
C entry points (no GPU involved)."""
import ctypes as C

import numpy as np
import pytest

import rpn_fpn_loss_ref as LR

HI, LO = 0.7, 0.3


@pytest.fixture(scope="module", params=[t for t, _ in LR.CASES])
def case(gold, request):
    return LR.golden_case(gold("rpn_fpn_loss"), gold("rpn_fpn"), request.param)


@pytest.fixture(scope="module")
def targets(case):
    return [LR.prepare_targets(case["boxes"], case["vis_cat"][i], case["gt"][i], HI, LO) for i in range(len(case["gt"]))]


def test_concatenation_order(case):
    """level-major, location row-major, the cell's anchors innermost: index g decodes to the level's own anchor row, and that row is the cell
    anchor shifted by the location's stride multiples"""
    n, offs, A = case["n"], case["offs"], case["A"]
    assert n == 6138 and offs.tolist() == [0, 4608, 5760, 6048, 6120, 6138]
    g = np.arange(2 * n)
    i, l, loc, a = LR.decode_index(g, n, offs, A)
    assert np.array_equal(i, g // n)
    for lev, ((H, W), anchors) in enumerate(zip(LR.MAPS, case["anchors"])):
        at = np.nonzero((l == lev) & (i == 1))[0]
        assert len(at) == H * W * A
        assert np.array_equal(case["boxes"][g[at] % n], anchors[loc[at] * A + a[at]])
        assert np.array_equal(loc[at] * A + a[at], np.arange(H * W * A))
        stride = 4 << lev
        cells = anchors.reshape(H, W, A, 4)
        assert np.array_equal(cells[1, 2] - cells[0, 0], np.tile(np.array([2, 1, 2, 1], np.float32) * stride, (A, 1)))
    obj, reg = LR.concat_predictions(case["ys"], A)
    assert obj.shape == (2, n) and reg.shape == (2, n, 4)
    assert obj[1, offs[2] + 7] == case["ys"][2][1, 7 // A, 7 % A] and np.array_equal(reg[0, offs[4] + 4], case["ys"][4][0, 1, A + 4: A + 8])


def test_restatement_reproduces_the_reference_targets(case, targets):
    for i, r in enumerate(targets):
        assert np.array_equal(r["matches"], case["matched"][i]), i
        assert np.array_equal(r["labels"], case["labels"][i]), i              # labels are exact
        assert np.all(np.abs(r["best"] - LO) > 1e-5) and np.all(np.abs(r["best"] - HI) > 1e-5)
    n = case["n"]
    tgt = np.concatenate([r["targets"] for r in targets]).reshape(-1, 4)
    bound = np.concatenate([r["target_bound"] for r in targets]).reshape(-1, 4)
    pa = case["pos_all"]
    assert len(pa) and np.all(np.abs(case["tgt_pos_all"] - tgt[pa]) <= bound[pa])
    if case["vis"][0][2].all():     # every anchor visible: the stored positives are this case's
        assert np.array_equal(pa, np.nonzero(case["labels"].reshape(-1) == 1)[0])
        _, lev, _, _ = LR.decode_index(case["pos"], n, case["offs"], case["A"])
        assert set(lev.tolist()) == {0, 1, 2, 3, 4}
    else:
        assert set(np.nonzero(case["labels"].reshape(-1) == 1)[0].tolist()) < set(pa.tolist())


def test_restatement_reproduces_the_reference_losses_and_gradients(case, targets):
    tgt = np.stack([r["targets"] for r in targets])
    ref = LR.losses(case["ys"], case["A"], case["labels"], tgt, case["pos"], case["samp"])
    LR.check_losses(case["loss_objectness"], case["loss_rpn_box_reg"], ref, "golden")
    assert ref["denom"] == len(case["samp"]) == 512
    d_obj, d_reg = LR.sampled_grads(ref["grads"], case["A"], case["n"], case["offs"], case["pos"], case["samp"])
    assert np.all(np.abs(d_obj - case["d_obj"]) <= 8 * LR.EPS * ref["obj_scale"])
    assert np.all(np.abs(d_reg - case["d_reg"]) <= 4 * LR.EPS * ref["box_scale"] * 10)
    assert sum(int((g != 0).sum()) for g in ref["grads"]) <= len(case["samp"]) + 4 * len(case["pos"])


def test_low_quality_matches_span_the_levels(case, targets):
    """Matcher's low-quality promotion takes a ground truth's best anchor over ALL levels: some level's own best anchor for some ground truth
    stays unmatched, which a matcher run level by level would have promoted"""
    found = 0
    for i, r in enumerate(targets):
        glob, local = LR.per_level_low_quality(r["iou"], case["offs"])
        for g in range(len(case["gt"][i])):
            for l, at in local[g].items():
                if l not in glob[g] and np.any(r["matches"][at] != g):
                    found += 1
    assert found > 0


def _tables(nlocs, ptr=True):
    nL = len(nlocs)
    return (C.c_void_p * max(nL, 1))(*([8] * nL)) if ptr else None, (C.c_int * max(nL, 1))(*nlocs)


@pytest.mark.parametrize("what,nL,Cf,null", [("L = 0", 0, 16, False), ("L = 9", 9, 16, False), ("Cf = 14", 2, 14, False), ("Cf = 18", 2, 18, False),
                                             ("null table", 2, 16, True)])
def test_entry_points_reject_bad_arguments(what, nL, Cf, null):
    from abr_iod_amd import _lib
    L = _lib.lib()
    y, nloc = _tables([4] * nL)
    rc = L.abr_rpn_pyramid_loss(y, None if null else nloc, nL, 2, 3, Cf, None, None, None, 4, None, 8, None, None, None, None, None)
    assert rc == -1 and b"rpn_pyramid_loss:" in L.abr_last_error(), (what, L.abr_last_error())
    if null:
        rc = L.abr_rpn_pyramid_loss(None, nloc, nL, 2, 3, Cf, None, None, None, 4, None, 8, None, None, None, None, None)
        assert rc == -1 and b"rpn_pyramid_loss:" in L.abr_last_error(), (what, L.abr_last_error())
    rc = L.abr_rpn_pyramid_loss_backward(None if null else nloc, nL, 2, 3, Cf, None, None, 4, 8, None, None, None, None)
    assert rc == -1 and b"rpn_pyramid_loss_backward:" in L.abr_last_error(), (what, L.abr_last_error())

"""GPU: the COCO scoring kernels (csrc/coco_eval.hip) against the host restatement (evaluation/coco/coco_eval_host.py, itself pinned by hand
in tests/test_coco_eval_host.py).  Box IoU: <= 1e-12 (values in [0,1] from a handful of correctly rounded float64 operations; contraction
into FMAs is the only possible difference, about a thousand times smaller) and the exactly representable ties bit-equal.  Matching:
index-exact on every output.  Mask IoU: equal."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from coco_eval_common import HAND_GROUPS, random_box_group, random_grid_group, tiny, tiny_predictions  # noqa: E402

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H  # noqa: E402

SIZES = (0, 1, 3, 65, 100)


def _box_groups():
    rng = np.random.default_rng(11)
    return list(HAND_GROUPS.values()) + [random_box_group(rng, D, G) for D in SIZES for G in SIZES]


def _flat(groups, key, shape):
    return np.concatenate([np.asarray(g[key]).reshape(shape) for g in groups])


def _counts(groups):
    return np.array([len(g["det_area"]) for g in groups]), np.array([len(g["gt_area"]) for g in groups])


@pytest.fixture(scope="module")
def box_ious():
    """(groups, device IoU per group, host IoU per group): computed once, shared, left unchanged"""
    from abr_iod_amd import ops
    groups = _box_groups()
    dc, gc = _counts(groups)
    iou, off = ops.coco_box_iou(_flat(groups, "det", (-1, 4)), _flat(groups, "gt", (-1, 4)), _flat(groups, "gt_crowd", (-1,)), dc, gc)
    assert iou.dtype == torch.float64 and iou.is_cuda and off[-1] == int((dc * gc).sum())
    flat = iou.cpu().numpy()
    got = [flat[off[k]: off[k + 1]].reshape(dc[k], gc[k]) for k in range(len(groups))]
    want = [H.box_iou(g["det"], g["gt"], g["gt_crowd"]) for g in groups]
    return groups, got, want


def test_box_iou_vs_host(box_ious):
    groups, got, want = box_ious
    worst = max([float(np.abs(a - b).max()) for a, b in zip(got, want) if a.size] + [0.0])
    print("coco_box_iou: max abs error", worst, "over", sum(a.size for a in got), "pairs")
    assert all(np.isfinite(a).all() for a in got)
    assert worst <= 1e-12
    names = list(HAND_GROUPS)
    assert got[names.index("iou_exactly_half")].tolist() == [[0.5]]
    assert got[names.index("iou_exactly_three_quarters")].tolist() == [[0.75]]
    assert got[names.index("equal_iou_two_gts")].tolist() == [[0.5, 0.5]]
    assert got[names.index("zero_area_boxes")].tolist() == [[0, 0], [0, 0], [1, 0]]
    assert any(g["gt_crowd"].any() for g in groups) and any((g["det_area"] == 0).any() for g in groups)


def _assert_match_equal(got, groups, iou_key):
    dc, gc = _counts(groups)
    d_off, g_off = np.concatenate(([0], np.cumsum(dc))), np.concatenate(([0], np.cumsum(gc)))
    for k, g in enumerate(groups):
        want = H.evaluate_img(g[iou_key], g["det_area"], g["gt_area"], g["gt_crowd"])
        ds, gs = slice(d_off[k], d_off[k + 1]), slice(g_off[k], g_off[k + 1])
        np.testing.assert_array_equal(got["dt_gt"][:, :, ds], want["dt_gt"], err_msg="dt_gt of group %d" % k)
        np.testing.assert_array_equal(got["dt_ig"][:, :, ds], want["dt_ig"], err_msg="dt_ig of group %d" % k)
        np.testing.assert_array_equal(got["gt_ig"][:, gs], want["gt_ig"], err_msg="gt_ig of group %d" % k)


def test_match_on_box_groups_index_exact(box_ious):
    """every hand case and the random box groups, matched on the DEVICE's IoUs left on the device"""
    from abr_iod_amd import ops
    groups, got_iou, _ = box_ious
    groups = [dict(g, iou=m) for g, m in zip(groups, got_iou)]
    dc, gc = _counts(groups)
    got = ops.coco_match(torch.from_numpy(_flat(groups, "iou", (-1,))).cuda(), dc, gc, _flat(groups, "det_area", (-1,)),
                         _flat(groups, "gt_area", (-1,)), _flat(groups, "gt_crowd", (-1,)), H.AREA_RNG, H.IOU_THRS)
    assert got["n_fallback"] == 0 and got["dt_gt"].dtype == np.int32 and got["dt_gt"].shape == (4, 10, int(dc.sum()))
    _assert_match_equal(got, groups, "iou")


def test_match_on_grid_ious_index_exact_with_fallback():
    """IoUs on the grid of multiples of 1/20 (ties and exact thresholds everywhere), D and G in {0, 1, 3, 65, 100}, G at the kernel's cap
    and one over it: that group comes back through the host restatement with the same answer, and is counted"""
    from abr_iod_amd import ops
    rng = np.random.default_rng(12)
    cap = ops.COCO_MATCH_MAX_GT
    shapes = [(D, G) for D in SIZES for G in SIZES] + [(7, cap), (7, cap + 1), (0, cap + 1), (100, 64)]
    groups = [random_grid_group(rng, D, G) for D, G in shapes]
    dc, gc = _counts(groups)
    got = ops.coco_match(_flat(groups, "iou", (-1,)), dc, gc, _flat(groups, "det_area", (-1,)), _flat(groups, "gt_area", (-1,)),
                         _flat(groups, "gt_crowd", (-1,)), H.AREA_RNG, H.IOU_THRS)
    assert got["n_fallback"] == 2
    _assert_match_equal(got, groups, "iou")
    assert (got["dt_gt"] >= 0).any() and got["dt_ig"].any() and (got["dt_gt"] >= 64).any()       # (the second state word is exercised)
    # another set of ranges and thresholds, as given
    one = ops.coco_match(groups[12]["iou"], dc[12:13], gc[12:13], groups[12]["det_area"], groups[12]["gt_area"], groups[12]["gt_crowd"],
                         [[0, 1e10]], [0.05, 1.0])
    want = H.evaluate_img(groups[12]["iou"], groups[12]["det_area"], groups[12]["gt_area"], groups[12]["gt_crowd"], [[0, 1e10]], [0.05, 1.0])
    np.testing.assert_array_equal(one["dt_gt"], want["dt_gt"])
    np.testing.assert_array_equal(one["dt_ig"], want["dt_ig"])
    empty = ops.coco_match(np.zeros(0), [], [], [], [], [], H.AREA_RNG, H.IOU_THRS)
    assert empty["dt_gt"].shape == (4, 10, 0) and empty["n_fallback"] == 0


@pytest.mark.parametrize("W", [63, 64, 65])
def test_mask_iou_with_a_crowd_equals_the_integer_ratio(W):
    from abr_iod_amd import ops
    rng = np.random.default_rng(W)
    pm, gm = rng.random((4, 9, W)) < 0.5, rng.random((3, 9, W)) < 0.4
    pm[3] = False                                # an empty prediction: 0, not 0 / 0
    pm[0, :, -1] = gm[0, :, -1] = True           # the last column of the row's last word
    crowd = np.array([False, True, False])
    pb, gb = ops.mask_pack_bits(torch.from_numpy(pm.astype(np.uint8)).cuda()), ops.mask_pack_bits(torch.from_numpy(gm.astype(np.uint8)).cuda())
    inter, area_p, area_t = ops.mask_pair_counts(pb, gb, W)
    got = ops.coco_mask_iou(inter, area_p, area_t, crowd).cpu().numpy()
    i = (pm.reshape(4, 1, -1) & gm.reshape(1, 3, -1)).sum(-1)
    ap, at = pm.reshape(4, -1).sum(-1), gm.reshape(3, -1).sum(-1)
    u = np.where(crowd[None, :], ap[:, None], ap[:, None] + at[None, :] - i)
    want = np.array([[float(i[p, t]) / float(u[p, t]) if i[p, t] else 0.0 for t in range(3)] for p in range(4)])
    assert got.dtype == np.float64 and (got == want).all(), (got, want)
    assert (got == H.mask_iou_from_counts(i, ap, at, crowd)).all() and (got[3] == 0).all()


def test_end_to_end_on_the_fixture_equals_the_host_route(tmp_path):
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import do_coco_evaluation, evaluate_predictions_on_coco
    ds = tiny(True, device="cuda")
    preds = tiny_predictions(ds, device="cuda", with_masks=True)
    results, coco_results = do_coco_evaluation(ds, preds, False, str(tmp_path), ("bbox", "segm"), (), 4)
    assert set(results.results) == {"bbox", "segm"} and len(coco_results["segm"]) == len(coco_results["bbox"]) == 9
    for iou_type in ("bbox", "segm"):
        dev = evaluate_predictions_on_coco(ds, coco_results[iou_type], iou_type, device="cuda")
        host = evaluate_predictions_on_coco(ds, coco_results[iou_type], iou_type, device="cpu")
        print(iou_type, dev.stats)
        np.testing.assert_array_equal(dev.stats, host.stats)
        np.testing.assert_array_equal(dev.precision, host.precision)
        np.testing.assert_array_equal(dev.recall, host.recall)
        assert [results.results[iou_type][m] for m in ("AP", "AP50", "AP75", "APs", "APm", "APl")] == dev.stats[:6].tolist()
        assert 0 < dev.stats[0] < 1 and dev.n_fallback == 0 and dev.n_groups == 5

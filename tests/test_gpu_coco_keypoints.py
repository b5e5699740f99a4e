"""GPU: the keypoint scoring kernels (csrc/coco_oks.hip, abr_coco_match_ig in csrc/coco_eval.hip) against the host restatement
(evaluation/coco/coco_eval_host.py, itself pinned by hand in tests/test_coco_keypoints_host.py).

OKS: the by-construction 1.0 and 0.0 entries bit-equal, every other entry within 2^-48 absolute.  The bound: both sides compute every e_k
with the same correctly rounded operations in the same order (contraction off), so only exp differs; both exps are within 1 ulp of the
true value by their libraries' documentation, so a term in (0, 1] differs by at most 2^-51; a serial sum of n such terms divided by n keeps
that order.  2^-48 leaves a factor 8.  Matching: index-exact on every output.  End to end on the fixture: equal tables (the CPU file's
margin check is what makes `==` safe)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from coco_eval_common import HAND_GROUPS, random_grid_group  # noqa: E402
from coco_kp_common import kp_tiny, kp_tiny_predictions, random_kp_group  # noqa: E402

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H  # noqa: E402

SIZES = (0, 1, 3, 65, 100)
BOUND = 2.0 ** -48


def _flat(groups, key, shape):
    return np.concatenate([np.asarray(g[key]).reshape(shape) for g in groups])


def _counts(groups):
    return np.array([len(g["det_area"]) for g in groups]), np.array([len(g["gt_area"]) for g in groups])


def _sigmas(K):
    return H.KPT_OKS_SIGMAS if K == 17 else np.array([0.05])


@pytest.fixture(scope="module")
def oks_groups():
    """{K: (groups, device OKS per group, host OKS per group)}: computed once, shared, left unchanged"""
    from abr_iod_amd import ops
    out = {}
    for K in (1, 17):
        rng = np.random.default_rng(20 + K)
        groups = [random_kp_group(rng, D, G, K) for D in SIZES for G in SIZES]
        for g in groups:
            g["det_area"] = H.keypoint_det_area(g["det_kp"])
        dc, gc = _counts(groups)
        oks, off = ops.coco_oks(_flat(groups, "det_kp", (-1, K, 3)), _flat(groups, "gt_kp", (-1, K, 3)), _flat(groups, "gt_box", (-1, 4)),
                                _flat(groups, "gt_area", (-1,)), _sigmas(K), dc, gc)
        assert oks.dtype == torch.float64 and oks.is_cuda and off[-1] == int((dc * gc).sum()) == oks.numel()
        flat = oks.cpu().numpy()
        got = [flat[off[k]: off[k + 1]].reshape(dc[k], gc[k]) for k in range(len(groups))]
        want = [H.oks(g["det_kp"], g["gt_kp"], g["gt_box"], g["gt_area"], _sigmas(K)) for g in groups]
        out[K] = (groups, got, want)
    return out


@pytest.mark.parametrize("K", [1, 17])
def test_oks_vs_host(oks_groups, K):
    groups, got, want = oks_groups[K]
    worst = max([float(np.abs(a - b).max()) for a, b in zip(got, want) if a.size] + [0.0])
    print("coco_oks K=%d: max abs error %.3e (2^-48 = %.3e) over %d pairs" % (K, worst, BOUND, sum(a.size for a in got)))
    assert all(np.isfinite(a).all() for a in got)
    n_one = n_zero = 0
    for g, a, b in zip(groups, got, want):
        for d, j in g["copies"]:
            assert a[d, j] == 1.0 and b[d, j] == 1.0, (d, j, a[d, j])
            n_one += 1
        for d in g["far"]:
            assert (a[d] == 0.0).all() and (b[d] == 0.0).all(), (d, a[d])
            n_zero += a.shape[1]
    assert n_one > 50 and n_zero > 500
    assert worst <= BOUND, worst
    # what the data was meant to hold
    assert any((g["gt_area"] == 0).any() for g in groups) and any(g["gt_ignore"].any() for g in groups)
    assert any(((g["gt_kp"][:, :, 2] > 0).sum(1) == 0).any() for g in groups)
    assert sum(int(((a > 0.01) & (a < 0.99)).sum()) for a in got) > (20 if K == 1 else 200)      # not only zeros and ones


def _assert_match_equal(got, groups, area_rng, thrs):
    dc, gc = _counts(groups)
    d_off, g_off = np.concatenate(([0], np.cumsum(dc))), np.concatenate(([0], np.cumsum(gc)))
    for k, g in enumerate(groups):
        want = H.evaluate_img(g["iou"], g["det_area"], g["gt_area"], g["gt_crowd"], area_rng, thrs, g["gt_ignore"])
        ds, gs = slice(d_off[k], d_off[k + 1]), slice(g_off[k], g_off[k + 1])
        np.testing.assert_array_equal(got["dt_gt"][:, :, ds], want["dt_gt"], err_msg="dt_gt of group %d" % k)
        np.testing.assert_array_equal(got["dt_ig"][:, :, ds], want["dt_ig"], err_msg="dt_ig of group %d" % k)
        np.testing.assert_array_equal(got["gt_ig"][:, gs], want["gt_ig"], err_msg="gt_ig of group %d" % k)


def _match(groups):
    from abr_iod_amd import ops
    dc, gc = _counts(groups)
    return ops.coco_match(_flat(groups, "iou", (-1,)), dc, gc, _flat(groups, "det_area", (-1,)), _flat(groups, "gt_area", (-1,)),
                          _flat(groups, "gt_crowd", (-1,)), H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=_flat(groups, "gt_ignore", (-1,)))


def test_match_with_gt_ignore_on_the_device_oks_index_exact(oks_groups):
    """the device's own OKS matrices (K = 17), an ignore flag that is not the crowd flag, the keypoint area ranges"""
    groups, got_oks, _ = oks_groups[17]
    groups = [dict(g, iou=m) for g, m in zip(groups, got_oks)]
    got = _match(groups)
    dc, _ = _counts(groups)
    assert got["n_fallback"] == 0 and got["dt_gt"].shape == (3, 10, int(dc.sum())) and got["gt_ig"].shape[0] == 3
    _assert_match_equal(got, groups, H.KP_AREA_RNG, H.IOU_THRS)
    assert any((g["gt_ignore"] != g["gt_crowd"]).any() for g in groups) and (got["dt_gt"] >= 0).any() and got["dt_ig"].any()


def test_match_with_gt_ignore_on_grid_matrices_index_exact_with_fallback():
    """matrices on the grid of multiples of 1/20 (ties and exact thresholds everywhere), gt_ignore drawn apart from gt_crowd, G at the
    kernel's cap and one over it: that group comes back through the host restatement with the flag passed on"""
    from abr_iod_amd import ops
    rng = np.random.default_rng(31)
    cap = ops.COCO_MATCH_MAX_GT
    shapes = [(D, G) for D in SIZES for G in SIZES] + [(7, cap), (7, cap + 1), (100, 64)]
    groups = [random_grid_group(rng, D, G) for D, G in shapes]
    for g in groups:
        g["gt_ignore"] = rng.random(len(g["gt_area"])) < 0.3
    assert any((g["gt_ignore"] & ~g["gt_crowd"]).any() for g in groups) and any((g["gt_crowd"] & ~g["gt_ignore"]).any() for g in groups)
    got = _match(groups)
    assert got["n_fallback"] == 1
    _assert_match_equal(got, groups, H.KP_AREA_RNG, H.IOU_THRS)
    # the flag is looked at: with gt_ignore = gt_crowd the answers differ somewhere
    dc, gc = _counts(groups)
    plain = ops.coco_match(_flat(groups, "iou", (-1,)), dc, gc, _flat(groups, "det_area", (-1,)), _flat(groups, "gt_area", (-1,)),
                           _flat(groups, "gt_crowd", (-1,)), H.KP_AREA_RNG, H.IOU_THRS)
    assert (plain["gt_ig"] != got["gt_ig"]).any() and (plain["dt_gt"] != got["dt_gt"]).any()


def test_match_without_gt_ignore_is_what_it_was_on_a_box_group():
    from abr_iod_amd import ops
    g = HAND_GROUPS["crowd_first_in_file"]
    iou = H.box_iou(g["det"], g["gt"], g["gt_crowd"])
    args = (iou, [2], [2], g["det_area"], g["gt_area"], g["gt_crowd"], H.AREA_RNG, H.IOU_THRS)
    none, same = ops.coco_match(*args, gt_ignore=None), ops.coco_match(*args, gt_ignore=g["gt_crowd"])
    want = H.evaluate_img(iou, g["det_area"], g["gt_area"], g["gt_crowd"])
    for key in ("dt_gt", "dt_ig", "gt_ig"):
        np.testing.assert_array_equal(none[key], want[key])
        np.testing.assert_array_equal(same[key], want[key])
    assert none["dt_gt"][0, 0].tolist() == [1, 0] and none["dt_ig"][0, 0].tolist() == [False, True]


def test_end_to_end_on_the_fixture_equals_the_host_route(tmp_path):
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import do_coco_evaluation, evaluate_predictions_on_coco
    ds = kp_tiny(device="cuda")
    preds = kp_tiny_predictions(ds, device="cuda")
    results, coco_results = do_coco_evaluation(ds, preds, False, str(tmp_path), ("keypoints",), (), 4, device="cuda")
    assert (tmp_path / "keypoints.json").exists() and len(coco_results["keypoints"]) == 38
    dev = evaluate_predictions_on_coco(ds, coco_results["keypoints"], "keypoints", device="cuda")
    host = evaluate_predictions_on_coco(ds, coco_results["keypoints"], "keypoints", device="cpu")
    print("keypoints", dev.stats)
    np.testing.assert_array_equal(dev.stats, host.stats)
    np.testing.assert_array_equal(dev.precision, host.precision)
    np.testing.assert_array_equal(dev.recall, host.recall)
    assert dev.stats.shape == (10,) and dev.n_fallback == 0 and dev.n_groups == 5 and 0 < dev.stats[0] < 1
    assert [results.results["keypoints"][m] for m in ("AP", "AP50", "AP75", "APm", "APl")] == dev.stats[:5].tolist()


def test_empty_inputs_launch_nothing():
    from abr_iod_amd import ops
    z = lambda *s: np.zeros(s)      # noqa: E731
    oks, off = ops.coco_oks(z(0, 17, 3), z(0, 17, 3), z(0, 4), z(0), H.KPT_OKS_SIGMAS, [], [])
    assert oks.numel() == 0 and oks.is_cuda and off.tolist() == [0]
    # groups, but no pair: detections without ground truths and the other way round
    oks, off = ops.coco_oks(z(2, 17, 3), z(3, 17, 3), z(3, 4), z(3), H.KPT_OKS_SIGMAS, [2, 0, 0], [0, 3, 0])
    assert oks.numel() == 0 and off.tolist() == [0, 0, 0, 0]
    empty = ops.coco_match(z(0), [], [], [], [], [], H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=[])
    assert empty["dt_gt"].shape == (3, 10, 0) and empty["n_fallback"] == 0
    with pytest.raises(RuntimeError):
        ops.coco_oks(z(0, 17, 3), z(0, 17, 3), z(0, 4), z(0), H.KPT_OKS_SIGMAS, [], [], device="cpu")
    with pytest.raises(RuntimeError):
        ops.coco_oks(z(1, 17, 3), z(0, 17, 3), z(0, 4), z(0), H.KPT_OKS_SIGMAS, [2], [0])      # counts that do not fit the arrays

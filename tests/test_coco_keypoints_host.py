"""CPU: the keypoint side of the host restatement of the COCO protocol (evaluation/coco/coco_eval_host.py: oks, the keypoint parameters,
evaluate_img's gt_ignore, summarize_keypoints) and the whole "keypoints" route of evaluation/coco/coco_eval.py with device="cpu", pinned on
answers worked out by hand.  Fixture: tests/golden/coco_kp_tiny.json (tests/coco_kp_common.py says what it holds)."""
import json
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

from coco_eval_common import HAND_GROUPS
from coco_kp_common import SHIFT_OF, kp_tiny, kp_tiny_predictions

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval as E
from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H

EPS = 1e-12          # pr = tp / (tp + fp + spacing(1)): a precision of "1" is 1 - 2.2e-16
SIG = H.KPT_OKS_SIGMAS


def _gt(K=17, vis=2, box=(10, 20, 40, 80), area=1600.0):
    kp = np.zeros((1, K, 3))
    kp[0, :, 0] = box[0] + np.arange(K) * 2.0
    kp[0, :, 1] = box[1] + np.arange(K) * 3.0
    kp[0, :, 2] = vis
    return kp, np.array([box], np.float64), np.array([area])


def test_keypoint_protocol_constants():
    assert H.KP_MAX_DETS == (20,)
    assert H.KP_AREA_RNG.tolist() == [[0, 1e10], [1024, 9216], [9216, 1e10]]
    assert H.KP_STAT_NAMES == ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
    assert SIG.shape == (17,) and SIG[0] == .26 / 10.0 and SIG[11] == 1.07 / 10.0 and SIG[16] == .89 / 10.0
    assert E.COCOResults.METRICS["keypoints"] == ["AP", "AP50", "AP75", "APm", "APl"]


def test_oks_of_a_copy_is_exactly_one_and_far_away_exactly_zero():
    kp, box, area = _gt()
    assert H.oks(kp, kp, box, area).tolist() == [[1.0]]
    # the detection's own v plays no part
    det = kp.copy()
    det[:, :, 2] = 0
    assert H.oks(det, kp, box, area).tolist() == [[1.0]]
    # 1e4 pixels away: e >= 1e8 / (2 * 0.107)^2 / 1600 / 2 > 6e5 > 745 for every keypoint, so every exp underflows to 0
    far = kp.copy()
    far[:, :, 0] += 1e4
    assert H.oks(far, kp, box, area).tolist() == [[0.0]]
    # only the labelled points count: moving an unlabelled one changes nothing, and n is their number
    kp2 = kp.copy()
    kp2[0, 5:, 2] = 0
    det = kp.copy()
    det[0, 5:, :2] += 1e4
    assert H.oks(det, kp2, box, area).tolist() == [[1.0]]


def test_oks_without_a_labelled_point_measures_the_distance_to_the_doubled_box():
    kp, box, area = _gt(vis=0)                      # box (10, 20, 40, 80): doubled about itself x in [-30, 90], y in [-60, 180]
    inside = np.zeros((1, 17, 3))
    inside[0, :, 0] = np.linspace(-30, 90, 17)      # both edges included
    inside[0, :, 1] = np.linspace(-60, 180, 17)
    assert H.oks(inside, kp, box, area).tolist() == [[1.0]]
    out = inside.copy()
    out[0, 0, 0] = -33.0                            # 3 left of x0
    out[0, 1, 1] = 184.0                            # 4 below y1
    out[0, 2, :2] = (95.0, -66.0)                   # 5 right of x1 and 6 above y0
    terms = [1.0] * 17
    terms[0] = math.exp(-(9.0 / (2 * SIG[0]) ** 2 / (1600.0 + 2.0 ** -52) / 2))
    terms[1] = math.exp(-(16.0 / (2 * SIG[1]) ** 2 / (1600.0 + 2.0 ** -52) / 2))
    terms[2] = math.exp(-(61.0 / (2 * SIG[2]) ** 2 / (1600.0 + 2.0 ** -52) / 2))
    want = 0.0
    for t in terms:
        want += t
    assert abs(H.oks(out, kp, box, area)[0, 0] - want / 17) <= 1e-15


def test_oks_of_one_visible_point_by_hand():
    # sigma 0.05 -> var 0.01; area 200; d^2 = 3^2 + 4^2 = 25: e = 25 / 0.01 / 200 / 2 = 6.25
    gt = np.array([[[10.0, 10.0, 2], [50.0, 50.0, 0]]])
    det = np.array([[[13.0, 14.0, 1], [0.0, 0.0, 1]]])
    got = H.oks(det, gt, [[0, 0, 20, 20]], [200.0], [0.05, 0.07])[0, 0]
    assert abs(got - math.exp(-25.0 / 0.05 ** 2 / 4 / 200.0 / 2)) <= 1e-15 and abs(got - math.exp(-6.25)) <= 1e-15


def test_oks_with_a_zero_area_ground_truth_has_no_nan():
    kp, box, _ = _gt()
    det = np.concatenate([kp, kp + [1.0, 0, 0]])
    got = H.oks(det, kp, box, [0.0])
    assert np.isfinite(got).all() and got.tolist() == [[1.0], [0.0]]     # e = 0 / (var * 2^-52) = 0; 1 / (var * 2^-52) / 2 > 745
    kp0, box0, _ = _gt(vis=0)
    assert np.isfinite(H.oks(det, kp0, box0, [0.0])).all()
    assert H.oks(np.zeros((0, 17, 3)), kp, box, [0.0]).shape == (0, 1) and H.oks(kp, np.zeros((0, 17, 3)), [], []).shape == (1, 0)


def test_keypoint_det_area_spans_all_points_whatever_v():
    kp = np.zeros((2, 3, 3))
    kp[0, :, 0], kp[0, :, 1] = (1, 5, 11), (2, 2, 9)          # (11 - 1) * (9 - 2); v is 0 everywhere
    kp[1, :, 0], kp[1, :, 1] = (3, 3, 3), (0, 8, 4)           # no width
    assert H.keypoint_det_area(kp).tolist() == [70.0, 0.0] and H.keypoint_det_area(np.zeros((0, 17, 3))).shape == (0,)


# ---------------------------------------------------------------------------------------------------- evaluate_img with gt_ignore
def test_a_ground_truth_without_keypoints_is_ignored_and_not_matched_twice_but_a_crowd_is():
    """two detections lie on one ground truth (similarity 1 each) that is ignored.  Ignored because num_keypoints == 0: the first takes
    it and is ignored, the second finds it taken and is a false positive (its own area is in range).  Ignored because it is a crowd:
    both match it."""
    sim = np.ones((2, 1))
    args = (sim, [2000.0, 2000.0], [3000.0], )
    r = H.evaluate_img(*args, [False], H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=[True])
    assert r["gt_ig"].tolist() == [[True]] * 3
    assert (r["dt_gt"][:, :, 0] == 0).all() and r["dt_ig"][:, :, 0].all()
    assert (r["dt_gt"][:, :, 1] == -1).all()
    assert r["dt_ig"][:, 0, 1].tolist() == [False, False, True]                   # unmatched: ignored by its own area (2000: all, medium)
    r = H.evaluate_img(*args, [True], H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=[True])
    assert (r["dt_gt"] == 0).all() and r["dt_ig"].all()
    # not ignored at all: the first is a true positive, the second a false one
    r = H.evaluate_img(*args, [False], H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=[False])
    assert r["gt_ig"][:, 0].tolist() == [False, False, True]
    assert (r["dt_gt"][:, :, 0] == 0).all() and (r["dt_gt"][:, :, 1] == -1).all() and not r["dt_ig"][0].any()


def test_a_labelled_ground_truth_is_preferred_to_an_ignored_one():
    # one detection, similarity 0.92 to an ignored ground truth (first in the file) and 0.6 to a labelled one: the labelled one is visited
    # first and, once it is matched, the walk stops at the first ignored ground truth
    r = H.evaluate_img([[0.92, 0.6]], [2000.0], [2000.0, 2000.0], [False, False], H.KP_AREA_RNG, H.IOU_THRS, gt_ignore=[True, False])
    # 0.5, 0.55, 0.6: the labelled one; 0.65 ... 0.9: only the ignored one is left; 0.95: none, and its own area (2000) is in range
    assert r["dt_gt"][0, :, 0].tolist() == [1, 1, 1] + [0] * 6 + [-1]
    assert r["dt_ig"][0, :, 0].tolist() == [False] * 3 + [True] * 6 + [False]


def test_gt_ignore_none_is_the_box_protocol():
    for name, g in HAND_GROUPS.items():
        iou = H.box_iou(g["det"], g["gt"], g["gt_crowd"])
        now = H.evaluate_img(iou, g["det_area"], g["gt_area"], g["gt_crowd"], gt_ignore=None)
        same = H.evaluate_img(iou, g["det_area"], g["gt_area"], g["gt_crowd"], gt_ignore=g["gt_crowd"])
        for key in ("dt_gt", "dt_ig", "gt_ig"):
            np.testing.assert_array_equal(now[key], same[key], err_msg=name)
    # and the answers are the ones test_coco_eval_host.py works out by hand
    g = HAND_GROUPS["crowd_first_in_file"]
    r = H.evaluate_img(H.box_iou(g["det"], g["gt"], g["gt_crowd"]), g["det_area"], g["gt_area"], g["gt_crowd"], gt_ignore=None)
    assert r["dt_gt"][0, 0].tolist() == [1, 0] and r["dt_ig"][0, 0].tolist() == [False, True]
    g = HAND_GROUPS["iou_exactly_half"]
    r = H.score_groups_host([dict(g, iou=H.box_iou(g["det"], g["gt"], g["gt_crowd"]))])[0]
    assert r["dt_gt"][0, :, 0].tolist() == [0] + [-1] * 9


# ---------------------------------------------------------------------------------------------------- the whole route on the fixture
def test_the_fixture_holds_what_the_tests_need():
    ds = kp_tiny()
    assert len(ds) == 5 and [len(ds.get_annotations(i)) for i in range(5)] == [3, 2, 2, 1, 0]
    anns = {a["id"]: a for i in range(5) for a in ds.get_annotations(i)}
    assert anns[3]["iscrowd"] == 1 and anns[5]["num_keypoints"] == 0 and anns[5]["iscrowd"] == 0 and anns[5]["bbox"][2] > 0
    assert [anns[i]["area"] for i in (7, 2, 1, 4, 6)] == [600.0, 32.0 ** 2, 5000.0, 96.0 ** 2, 20000.0]
    assert sum(v > 0 for v in anns[7]["keypoints"][2::3]) == 4 and "num_keypoints" not in anns[8]
    assert all(len(a["keypoints"]) == 51 for a in anns.values())


def test_perfect_predictions_score_one(tmp_path):
    ds = kp_tiny()
    results, coco_results = E.do_coco_evaluation(ds, kp_tiny_predictions(ds, perfect=True), False, str(tmp_path), ("keypoints",), (), 4,
                                                 device="cpu")
    assert list(results.results) == ["keypoints"] and list(results.results["keypoints"]) == ["AP", "AP50", "AP75", "APm", "APl"]
    # ids 1, 2, 4, 6, 7, 8 are predicted; medium holds ids 1, 2, 4, 8 and large ids 4, 6: every range has ground truths, all found
    assert len(coco_results["keypoints"]) == 6
    assert all(abs(v - 1) < EPS for v in results.results["keypoints"].values()), results
    res = E.evaluate_predictions_on_coco(ds, coco_results["keypoints"], "keypoints", device="cpu")
    assert res.stats.shape == (10,) and all(abs(v - 1) < EPS for v in res.stats)
    assert res.precision.shape == (10, 101, 1, 3, 1) and res.recall.shape == (10, 1, 3, 1) and res.n_groups == 4 and res.n_fallback == 0
    written = json.load(open(str(tmp_path / "keypoints.json")))
    assert len(written) == 6 and written[0]["keypoints"] == [float(v) for v in ds.get_annotations(0)[0]["keypoints"]]
    assert set(written[0]) == {"image_id", "category_id", "keypoints", "score"} and written[0]["category_id"] == 1
    text = res.text().splitlines()
    assert len(text) == 11 and text[0] == "COCO keypoints summary"
    assert text[1] == " Average Precision (AP) @[ IoU=0.50:0.95 | area=   all | maxDets= 20 ] = 1.000"
    assert text[10] == " Average Recall (AR) @[ IoU=0.50:0.95 | area= large | maxDets= 20 ] = 1.000"


def _shifted_oks(ann, shift):
    """a copy of `ann` moved by `shift` pixels in x: the mean over its labelled points of exp(-shift^2 / (2 sigma_k)^2 / area / 2)"""
    terms = [math.exp(-(shift * shift / (2 * s) ** 2 / (ann["area"] + 2.0 ** -52) / 2)) for s, v in zip(SIG, ann["keypoints"][2::3]) if v > 0]
    return sum(terms) / len(terms)


def test_shifted_predictions_by_hand_and_the_21st_detection_does_not_count():
    """SHIFTED (coco_kp_common.py).  Six ground truths count (ids 1, 2, 4, 6, 7, 8); id 3 is a crowd and id 5 has no labelled point.
    Every one of the six is followed by one detection, a copy moved by 1 to 10 pixels; every other similarity is far below 0.5.
      image 1: a figure in the bottom left corner (0.95): a false positive.  Two figures inside the crowd's doubled box (0.7, 0.6): OKS
               1 with the crowd, both match it, both ignored.
      image 2: two figures inside the doubled box of id 5 (0.61, 0.51): the first matches it and is ignored, the second finds it taken
               (it is not a crowd): a false positive.  A figure far away (0.31): a false positive.
      image 3: a figure far away (0.42): a false positive.
      image 4: 19 figures along the top edge (0.895 ... 0.715): false positives; the follower of id 8 is 20th (0.5); five exact copies of
               id 8 come 21st to 25th and must not count (they would be true positives at the thresholds the follower misses).
      image 5: no ground truth, one figure (0.852): a false positive.
    By score, at OKS 0.5 (T = true, F = false positive; the three ignored ones left out):
      F.95 T.92 T.91 T.9 F.895 F.885 F.875 F.865 F.855 F.852 F.845 F.835 F.825 T.82 F.815 F.805 T.8 F.795 ... F.715 (9) F.51 T.5 F.42 F.31
    Precision at the six true positives: 1/2, 2/3, 3/4, 4/14, 5/17, 6/28; made monotone from the right: 3/4 up to recall 3/6, 5/17 up to
    5/6, 6/28 up to 1.  Of the 101 recall thresholds 0.00 ... 0.50 are 51, 0.51 ... 0.83 are 33, 0.84 ... 1.00 are 17."""
    ds = kp_tiny()
    anns = {a["id"]: a for i in range(5) for a in ds.get_annotations(i)}
    follower = {i: _shifted_oks(anns[i], s) for i, s in SHIFT_OF.items()}
    assert all(v > 0.5 for v in follower.values()) and follower[6] < 0.95 and follower[8] < 0.95, follower
    results = E.prepare_for_coco_keypoint(kp_tiny_predictions(ds), ds)
    assert len(results) == 5 + 4 + 3 + 25 + 1
    res = E.evaluate_predictions_on_coco(ds, results, "keypoints", device="cpu")
    names = dict(zip(H.KP_STAT_NAMES, res.stats))
    ap50 = (51 * Fraction(3, 4) + 33 * Fraction(5, 17) + 17 * Fraction(6, 28)) / 101
    assert abs(names["AP50"] - float(ap50)) < EPS, (names["AP50"], float(ap50))
    # recall at a threshold: the ground truths whose follower reaches it, of six
    thrs = [min(t, 1 - 1e-10) for t in H.IOU_THRS.tolist()]
    recall = [sum(v >= t for v in follower.values()) / 6.0 for t in thrs]
    assert recall[0] == 1.0 and recall[-1] < 1.0
    assert abs(names["AR"] - sum(recall) / 10) < EPS and abs(names["AR50"] - 1.0) < EPS
    np.testing.assert_allclose(res.recall[:, 0, 0, 0], recall, rtol=0, atol=EPS)
    # medium: ids 1, 2, 4, 8; large: ids 4, 6
    assert abs(names["ARm"] - sum(sum(follower[i] >= t for i in (1, 2, 4, 8)) / 4.0 for t in thrs) / 10) < EPS
    assert abs(names["ARl"] - sum(sum(follower[i] >= t for i in (4, 6)) / 2.0 for t in thrs) / 10) < EPS
    # the 21st to 25th detection of image 4 change nothing ...
    cut = E.evaluate_predictions_on_coco(ds, E.prepare_for_coco_keypoint(kp_tiny_predictions(ds, keep=20), ds), "keypoints", device="cpu")
    np.testing.assert_array_equal(res.stats, cut.stats)
    np.testing.assert_array_equal(res.precision, cut.precision)
    np.testing.assert_array_equal(res.recall, cut.recall)
    # ... although a 20th that is an exact copy would: keep the 19 figures and the first copy
    preds = kp_tiny_predictions(ds)
    keep = torch.tensor(list(range(19)) + [20])
    preds[3] = preds[3][keep]
    other = E.evaluate_predictions_on_coco(ds, E.prepare_for_coco_keypoint(preds, ds), "keypoints", device="cpu")
    assert other.recall[-1, 0, 0, 0] > res.recall[-1, 0, 0, 0]


def test_margins_of_the_fixture_similarities():
    """what lets the device route be compared with `==` (tests/test_gpu_coco_keypoints.py): on the imperfect predictions no similarity
    lies within 1e-9 of a threshold, and no two entries of a row that could decide a match lie within 1e-9 of each other unless they are
    equal by construction (exactly 1 inside a doubled box).  An entry below the lowest threshold by more than the margin is never chosen,
    whatever its neighbours are, so pairs of such entries (the far-away ones, 1e-6 and less) are not compared."""
    ds = kp_tiny()
    results = E.prepare_for_coco_keypoint(kp_tiny_predictions(ds), ds)
    groups, _ = E.build_groups(ds, results, "keypoints", "cpu", n_keypoints=17)
    E.score_groups(groups, "keypoints", "cpu", sigmas=SIG)
    thrs = np.array([min(t, 1 - 1e-10) for t in H.IOU_THRS.tolist()])
    seen = 0
    for g in groups:
        assert len(g["scores"]) <= 20
        for row in g["iou"]:
            assert (np.abs(row[:, None] - thrs[None, :]) > 1e-9).all() or (row == 1.0).any(), row
            for v in row[row != 1.0]:
                assert (np.abs(v - thrs) > 1e-9).all(), v
            live = np.nonzero(row >= 0.5 - 1e-9)[0]
            for j in live:
                others = np.delete(row, j)
                assert ((np.abs(others - row[j]) > 1e-9) | (others == row[j])).all(), row
                seen += 1
    assert seen >= 9          # the six followers, the two on the crowd, the two on id 5


# ---------------------------------------------------------------------------------------------------- smaller checks
def test_prepare_for_coco_keypoint_resizes_back_to_the_file_size():
    ds = kp_tiny()
    at_file_size = E.prepare_for_coco_keypoint(kp_tiny_predictions(ds, perfect=True), ds)
    doubled = E.prepare_for_coco_keypoint(kp_tiny_predictions(ds, perfect=True, scale=2), ds)
    assert doubled == at_file_size and doubled[0]["keypoints"][:6] == [50.0, 30.0, 2.0, 53.0, 28.0, 2.0]
    assert [r["image_id"] for r in doubled] == [1, 1, 2, 3, 3, 4] and doubled[1]["score"] == 0.8


def test_a_prediction_without_the_field_and_a_wrong_keypoint_count_raise():
    ds = kp_tiny()
    preds = kp_tiny_predictions(ds, perfect=True)
    preds[0] = preds[0].copy_with_fields(["labels", "scores"])
    with pytest.raises(ValueError, match='"keypoints"'):
        E.prepare_for_coco_keypoint(preds, ds)
    with pytest.raises(ValueError, match='"keypoints"'):
        E.do_coco_evaluation(ds, preds, False, None, ("keypoints",), (), 4, device="cpu")
    five = [{"image_id": 1, "category_id": 1, "keypoints": [1.0, 2.0, 2.0] * 5, "score": 0.9}]
    with pytest.raises(ValueError, match="kpt_oks_sigmas"):
        E.evaluate_predictions_on_coco(ds, five, "keypoints", device="cpu")
    with pytest.raises(ValueError, match="holds 51 numbers"):        # the sigmas fit the result, the annotations have 17 points
        E.evaluate_predictions_on_coco(ds, five, "keypoints", device="cpu", kpt_oks_sigmas=[0.05] * 5)
    with pytest.raises(NotImplementedError):
        E.do_coco_evaluation(ds, kp_tiny_predictions(ds, perfect=True), True, None, ("keypoints",), (), 4, device="cpu")


def test_other_sigmas_are_used_as_given():
    ds = kp_tiny()
    results = E.prepare_for_coco_keypoint(kp_tiny_predictions(ds), ds)
    tight = E.evaluate_predictions_on_coco(ds, results, "keypoints", device="cpu", kpt_oks_sigmas=H.KPT_OKS_SIGMAS / 4)
    assert tight.stats[5] < E.evaluate_predictions_on_coco(ds, results, "keypoints", device="cpu").stats[5]


def test_box_and_keypoint_results_side_by_side(tmp_path):
    ds = kp_tiny()
    results, coco_results = E.do_coco_evaluation(ds, kp_tiny_predictions(ds, perfect=True), False, str(tmp_path), ("bbox", "keypoints"), (), 4,
                                                 device="cpu")
    assert list(results.results) == ["bbox", "keypoints"] and len(coco_results["bbox"]) == len(coco_results["keypoints"]) == 6
    assert (tmp_path / "bbox.json").exists() and (tmp_path / "keypoints.json").exists()
    assert 0 <= results.results["bbox"]["AP"] <= 1 and abs(results.results["keypoints"]["AP"] - 1) < EPS


def test_evaluate_takes_the_keywords_inference_passes():
    """engine.inference.inference ends in evaluate(dataset=, predictions=, output_folder=, box_only=, iou_types=, expected_results=,
    expected_results_sigma_tol=, alphabetical_order=): for a COCODataset that returns keypoint AP beside box AP"""
    from abr_iod_amd.data.datasets.evaluation import evaluate
    ds = kp_tiny()
    results, _ = evaluate(dataset=ds, predictions=kp_tiny_predictions(ds, perfect=True), output_folder=None, box_only=False,
                          iou_types=("bbox", "keypoints"), expected_results=[("keypoints", "AP", (1.0, 0.01))], expected_results_sigma_tol=4,
                          alphabetical_order=True, device="cpu")
    assert abs(results.results["keypoints"]["AP"] - 1) < EPS and "AP" in results.results["bbox"]


def test_ops_and_abi_carry_the_keypoint_kernels():
    from abr_iod_amd import _lib, ops
    assert "abr_coco_oks" in _lib.EXPORTS and "abr_coco_match_ig" in _lib.EXPORTS
    L = _lib.lib()
    # the argument checks run without a GPU
    assert L.abr_coco_oks(None, None, None, None, None, 17, None, None, None, 0, 0, None, None) == 0         # no groups: nothing to do
    assert L.abr_coco_oks(None, None, None, None, None, 17, None, None, None, 3, 0, None, None) == 0         # no pairs
    assert L.abr_coco_oks(None, None, None, None, None, 17, None, None, None, 3, 5, None, None) == -1 and b"coco_oks" in L.abr_last_error()
    assert L.abr_coco_oks(None, None, None, None, None, 17, None, None, None, -1, 0, None, None) == -1
    assert L.abr_coco_oks(None, None, None, None, None, 0, None, None, None, 0, 0, None, None) == -1
    assert L.abr_coco_match_ig(None, None, None, None, None, None, None, None, 0, 0, 0, None, 3, None, 10, None, None, None, None, None) == 0
    assert L.abr_coco_match_ig(None, None, None, None, None, None, None, None, 1, 0, 0, None, 9, None, 10, None, None, None, None, None) == -1
    assert L.abr_coco_match_ig(None, None, None, None, None, None, None, None, 1, 0, 0, None, 3, None, 10, None, None, None, None, None) == -1
    assert b"coco_match" in L.abr_last_error()
    with pytest.raises(RuntimeError):
        ops.coco_oks(np.zeros((0, 17, 3)), np.zeros((0, 17, 3)), np.zeros((0, 4)), [], SIG, [0], [0], device="cpu")
    with pytest.raises(RuntimeError):
        ops.coco_match(np.zeros(0), [0], [0], [], [], [], H.KP_AREA_RNG, H.IOU_THRS, device="cpu", gt_ignore=[])

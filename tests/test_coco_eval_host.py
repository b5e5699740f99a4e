"""CPU: the host restatement of the COCO protocol (evaluation/coco/coco_eval_host.py), COCODataset and the dispatch of evaluate(), pinned on
answers worked out by hand -- not on the restatement itself.  Fixture: tests/golden/coco_tiny.json (4 images, 3 categories, one crowd
run-length annotation, one image without annotations, one with a degenerate box only)."""
import logging

import numpy as np
import pytest
import torch

from coco_eval_common import HAND_GROUPS, tiny, tiny_predictions

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H

EPS = 1e-12          # pr = tp / (tp + fp + spacing(1)): a precision of "1" is 1 - 2.2e-16


def _match(name):
    g = HAND_GROUPS[name]
    iou = H.box_iou(g["det"], g["gt"], g["gt_crowd"])
    return iou, H.evaluate_img(iou, g["det_area"], g["gt_area"], g["gt_crowd"])


def _cell(r, scores):
    return dict(r, scores=np.asarray(scores, np.float64))


def test_protocol_constants():
    assert H.IOU_THRS.shape == (10,) and H.IOU_THRS[0] == 0.5 and H.IOU_THRS[5] == 0.75 and abs(H.IOU_THRS[9] - 0.95) < 1e-15
    assert H.REC_THRS.shape == (101,) and H.REC_THRS[50] == 0.5 and H.REC_THRS[100] == 1.0
    assert H.AREA_RNG.tolist() == [[0, 1e10], [0, 1024], [1024, 9216], [9216, 1e10]]


def test_box_iou_by_hand():
    # 10x10 inside 10x20: 100 / 200; 30x10 inside 40x10: 300 / 400 -- both exactly representable
    assert H.box_iou([[0, 0, 10, 10]], [[0, 0, 10, 20]], [0]).tolist() == [[0.5]]
    assert H.box_iou([[0, 0, 30, 10]], [[0, 0, 40, 10]], [0]).tolist() == [[0.75]]
    # no + 1: touching boxes do not meet; a crowd divides by the detection's area alone
    assert H.box_iou([[0, 0, 10, 10]], [[10, 0, 10, 10]], [0]).tolist() == [[0.0]]
    assert H.box_iou([[0, 0, 10, 10]], [[5, 0, 100, 100]], [1]).tolist() == [[0.5]]
    assert H.box_iou([[0, 0, 10, 10]], [[5, 0, 100, 100]], [0]).tolist() == [[50 / (100 + 10000 - 50)]]
    # zero-area boxes give 0, never 0 / 0
    g = HAND_GROUPS["zero_area_boxes"]
    iou = H.box_iou(g["det"], g["gt"], g["gt_crowd"])
    assert np.isfinite(iou).all() and iou.tolist() == [[0, 0], [0, 0], [1, 0]]


def test_mask_iou_from_counts_by_hand():
    iou = H.mask_iou_from_counts([[6, 3], [0, 0]], [12, 0], [6, 100], [0, 1])
    assert iou.tolist() == [[0.5, 0.25], [0.0, 0.0]]


def test_iou_exactly_at_a_threshold_matches_there_and_no_higher():
    _, r = _match("iou_exactly_half")
    assert r["dt_gt"][0, :, 0].tolist() == [0] + [-1] * 9
    _, r = _match("iou_exactly_three_quarters")
    assert r["dt_gt"][0, :, 0].tolist() == [0] * 6 + [-1] * 4


def test_equal_iou_takes_the_later_ground_truth():
    iou, r = _match("equal_iou_two_gts")
    assert iou.tolist() == [[0.5, 0.5]]
    assert r["dt_gt"][0, 0, 0] == 1


def test_crowd_semantics():
    # a detection lying only on a crowd: matched to it, ignored -- neither a true nor a false positive
    iou, r = _match("only_on_a_crowd")
    assert iou.tolist() == [[0.0, 1.0]]
    assert (r["dt_gt"][0, :, 0] == 1).all() and r["dt_ig"][0, :, 0].all()
    assert r["gt_ig"][0].tolist() == [False, True]
    acc = H.accumulate({0: [_cell(r, [0.9])]}, 1)
    assert (acc["recall"][:, 0, 0, 2] == 0).all() and (acc["precision"][:, :, 0, 0, 2] == 0).all()      # one gt, nothing counted
    # two detections on one crowd both match it
    _, r = _match("two_on_one_crowd")
    assert (r["dt_gt"][0] == 0).all() and r["dt_ig"][0].all()
    # the non-ignored ground truth is visited first although the crowd comes first in the file; the second detection finds it taken,
    # and goes to the crowd (IoU = 1 against a crowd that contains it)
    _, r = _match("crowd_first_in_file")
    assert r["dt_gt"][0, 0].tolist() == [1, 0] and r["dt_ig"][0, 0].tolist() == [False, True]


def test_area_exactly_32_squared_is_small_and_medium():
    _, r = _match("area_exactly_32_squared")
    assert r["gt_ig"][:, 0].tolist() == [False, False, False, True]
    assert (r["dt_gt"][:, :, 0] == 0).all()
    assert r["dt_ig"][:, 0, 0].tolist() == [False, False, False, True]     # matched to an ignored ground truth: ignored
    # an unmatched detection is ignored by its own area
    r = H.evaluate_img(np.zeros((1, 1)), [1024.0], [1024.0], [False])
    assert (r["dt_gt"] == -1).all() and r["dt_ig"][:, 0, 0].tolist() == [False, False, False, True]
    r = H.evaluate_img(np.zeros((1, 1)), [1025.0], [1024.0], [False])
    assert r["dt_ig"][:, 0, 0].tolist() == [False, True, False, True]


def test_empty_groups():
    for name, D, G in [("no_detections", 0, 1), ("no_ground_truth", 1, 0), ("nothing", 0, 0)]:
        _, r = _match(name)
        assert r["dt_gt"].shape == (4, 10, D) and r["gt_ig"].shape == (4, G) and (r["dt_gt"] == -1).all()


def test_equal_scores_keep_file_order():
    assert H.rank_detections([0.5, 0.9, 0.5, 0.9]).tolist() == [1, 3, 0, 2]
    assert H.rank_detections(np.linspace(1, 0, 101)).tolist() == list(range(100))
    # ... and in the merge across images: the first image's detection comes first at equal score.  Image 1: a false positive at 0.8,
    # image 2: a true positive at 0.8 -> precision at recall 1 is 1/2; swapped, it is 1
    fp = H.evaluate_img(np.zeros((1, 0)), [50.0], [], [])
    tp = H.evaluate_img(np.ones((1, 1)), [50.0], [50.0], [False])
    a = H.accumulate({0: [_cell(fp, [0.8]), _cell(tp, [0.8])]}, 1)
    b = H.accumulate({0: [_cell(tp, [0.8]), _cell(fp, [0.8])]}, 1)
    assert abs(a["precision"][0, 100, 0, 0, 2] - 0.5) < EPS and abs(b["precision"][0, 100, 0, 0, 2] - 1.0) < EPS


def test_two_ground_truths_one_exact_detection():
    """recall 0.5; precision 1 at the 51 recall thresholds <= 0.5, 0 above: AP = 51 / 101"""
    r = H.evaluate_img(np.array([[1.0, 0.0]]), [1600.0], [1600.0, 1800.0], [False, False])
    acc = H.accumulate({0: [_cell(r, [0.9])]}, 1)
    assert (acc["recall"][:, 0, 0, :] == 0.5).all()
    p = acc["precision"][:, :, 0, 0, 2]
    assert np.abs(p[:, :51] - 1).max() < EPS and (p[:, 51:] == 0).all()
    stats = H.summarize(acc)
    assert abs(stats[0] - 51 / 101) < EPS and abs(stats[1] - 51 / 101) < EPS and stats[8] == 0.5
    assert stats[3] == -1 and abs(stats[4] - 51 / 101) < EPS and stats[5] == -1       # both ground truths are medium


def test_only_the_first_100_of_101_detections_count():
    """101 ground truths, 101 detections, detection i exactly on ground truth i, scores descending: recall 100 / 101, and AR@1 / AR@10
    read the first 1 / 10 detections of the same matching"""
    scores = np.linspace(1, 0.5, 101)
    keep = H.rank_detections(scores[::-1])                      # given in ascending order: the LAST 100 of the file count
    assert keep.tolist() == list(range(100, 0, -1))
    r = H.evaluate_img(np.eye(101)[:100], np.full(100, 50.0), np.full(101, 50.0), np.zeros(101, bool))
    assert r["dt_gt"][0, 0].tolist() == list(range(100))
    acc = H.accumulate({0: [_cell(r, scores[:100])]}, 1)
    assert (acc["recall"][:, 0, 0, 0] == 1 / 101).all() and (acc["recall"][:, 0, 0, 1] == 10 / 101).all()
    assert (acc["recall"][:, 0, 0, 2] == 100 / 101).all()
    stats = H.summarize(acc)
    assert np.abs(stats[6:9] - np.array([1, 10, 100]) / 101).max() < EPS        # (a mean of ten equal numbers: not bit-exact)


def test_category_without_ground_truth_is_left_out_of_the_mean():
    tp = H.evaluate_img(np.ones((1, 1)), [50.0], [50.0], [False])
    fp = H.evaluate_img(np.zeros((1, 0)), [50.0], [], [])
    acc = H.accumulate({0: [_cell(tp, [0.9])], 1: [_cell(fp, [0.9])]}, 3)
    assert (acc["precision"][:, :, 1:] == -1).all() and (acc["recall"][:, 1:] == -1).all()
    stats = H.summarize(acc)
    assert abs(stats[0] - 1) < EPS and stats[8] == 1.0
    assert (H.summarize(H.accumulate({}, 3)) == -1).all()


# ------------------------------------------------------------------------------------------------ COCODataset
def test_dataset_maps_and_filter():
    ds = tiny(True, device="cpu")
    assert ds.json_category_id_to_contiguous_id == {3: 1, 5: 2, 9: 3} and ds.contiguous_category_id_to_json_id == {1: 3, 2: 5, 3: 9}
    assert ds.ids == [3, 7] and ds.id_to_img_map == {0: 3, 1: 7} and len(ds) == 2        # 11 has no annotation, 12 a degenerate box only
    assert tiny(False, device="cpu").ids == [3, 7, 11, 12]
    assert ds.get_img_info(1) == {"id": 7, "width": 200, "height": 150, "file_name": "seven.png"}


def test_dataset_targets_drop_the_crowd_and_the_evaluator_sees_it():
    ds = tiny(True, device="cpu", with_masks=True)
    t = ds.get_target(1)
    assert len(t) == 2 and t.get_field("labels").tolist() == [1, 2] and t.mode == "xyxy" and t.size == (200, 150)
    assert t.bbox.tolist() == [[10, 10, 129, 109], [150, 20, 181, 51]]         # xywh -> xyxy: x + w - 1
    masks = t.get_field("masks")
    assert type(masks).__name__ == "PolygonList" and len(masks) == 2
    anns = ds.get_annotations(1)
    assert [a["id"] for a in anns] == [101, 102, 103] and anns[2]["iscrowd"] == 1
    gt = ds.get_groundtruth(1)
    assert gt.get_field("iscrowd").tolist() == [0, 0, 1] and gt.get_field("area").tolist() == [12000, 1024, 3000]
    m = ds.annotation_masks(1, "cpu", packed=False)
    assert tuple(m.shape) == (3, 150, 200) and int(m[2].sum()) == 3000 and bool(m[2, 80:140, 140:190].all())
    assert int(m[0].sum()) > 0 and int(m[0, :10].sum()) == 0
    # an image without annotations gives an empty target
    t = tiny(False, device="cpu").get_target(2)
    assert len(t) == 0 and t.get_field("labels").numel() == 0


# ------------------------------------------------------------------------------------------------ the whole route on the host
def test_perfect_detections_score_one_in_every_populated_cell():
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval as E
    ds = tiny(True, device="cpu")
    res = E.evaluate_predictions_on_coco(ds, E.prepare_for_coco_detection(tiny_predictions(ds, perfect=True), ds), "bbox", device="cpu")
    # small (400, 1024), medium (1024, 1600, 1800) and large (12000) all occur.  AR@1 is the one number that cannot be 1: "kite" has two
    # ground truths in one image and one detection per image counts, so its recall there is 1/2 and the mean over categories 5/6
    want = np.ones(12)
    want[6] = 5 / 6
    assert np.abs(res.stats - want).max() < EPS, res.stats
    assert res.n_groups == 4 and res.n_fallback == 0
    pop = res.precision > -1
    assert np.abs(res.precision[..., 1:][pop[..., 1:]] - 1).max() < EPS          # (maxDets 10 and 100)
    assert (res.recall[..., 1:][res.recall[..., 1:] > -1] == 1).all() and res.recall[:, :, 0, 0].tolist() == [[1, 1, 0.5]] * 10
    assert not pop[:, :, 2, 1].any() and not pop[:, :, 2, 3].any()       # "kite" has medium ground truths only


def test_fixture_by_hand():
    """category 9 ("kite"): two ground truths, one exact detection -> AP 51 / 101; category 3: a detection on the crowd only -> not counted,
    and the exact one -> AP 1; category 5: nothing detected -> AP 0"""
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval as E
    ds = tiny(True, device="cpu")
    results = [{"image_id": 3, "category_id": 9, "bbox": [5, 5, 40, 40], "score": 0.9},
               {"image_id": 7, "category_id": 3, "bbox": [150, 90, 30, 40], "score": 0.99},
               {"image_id": 7, "category_id": 3, "bbox": [10, 10, 120, 100], "score": 0.5}]
    res = E.evaluate_predictions_on_coco(ds, results, "bbox", device="cpu")
    ap = [H._mean_valid(res.precision[:, :, k, 0, 2]) for k in range(3)]
    assert abs(ap[0] - 1) < EPS and ap[1] == 0 and abs(ap[2] - 51 / 101) < EPS
    assert abs(res.stats[0] - (1 + 0 + 51 / 101) / 3) < EPS
    with pytest.raises(ValueError):
        E.evaluate_predictions_on_coco(ds, [dict(results[0], image_id=11)], "bbox", device="cpu")


def test_evaluate_routes_a_coco_dataset_to_the_coco_protocol(tmp_path):
    from abr_iod_amd.data.datasets.evaluation import evaluate
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import COCOResults
    ds = tiny(True, device="cpu")
    results, coco_results = evaluate(ds, tiny_predictions(ds, perfect=True), str(tmp_path), box_only=False, iou_types=("bbox",),
                                     expected_results=[("bbox", "AP", (1.0, 0.01))], expected_results_sigma_tol=4, device="cpu")
    assert isinstance(results, COCOResults) and list(results.results) == ["bbox"]
    assert list(results.results["bbox"]) == ["AP", "AP50", "AP75", "APs", "APm", "APl"]
    assert all(abs(v - 1) < EPS for v in results.results["bbox"].values())
    assert len(coco_results["bbox"]) == 5 and coco_results["bbox"][0]["category_id"] in (3, 5, 9)
    assert (tmp_path / "bbox.json").exists() and (tmp_path / "coco_results.pth").exists()


def test_evaluate_routes_a_voc_dataset_where_it_went_before(monkeypatch):
    import abr_iod_amd.data.datasets.evaluation as ev
    seen = []
    monkeypatch.setattr(ev, "voc_evaluation", lambda **kw: seen.append(("voc", sorted(kw))) or "voc")
    monkeypatch.setattr(ev, "voc_evaluation_inst", lambda **kw: seen.append(("inst", sorted(kw))) or "inst")
    monkeypatch.setattr(ev, "coco_evaluation", lambda **kw: seen.append(("coco", sorted(kw))) or "coco")

    class NotCoco(object):
        pass

    assert ev.evaluate(NotCoco(), [], None, iou_types=("bbox",)) == "voc"
    assert ev.evaluate(NotCoco(), [], None, iou_types=("bbox", "segm")) == "inst"
    assert ev.evaluate(NotCoco(), [], None) == "voc"
    assert ev.evaluate(tiny(True, device="cpu"), [], None, iou_types=("bbox", "segm")) == "coco"
    assert [s[0] for s in seen] == ["voc", "inst", "voc", "coco"]
    assert seen[0][1] == ["dataset", "iou_types", "output_folder", "predictions"]


def test_check_expected_results_logs_pass_and_fail(caplog):
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import COCOResults, check_expected_results
    r = COCOResults("bbox")
    r.results["bbox"]["AP"] = 0.30
    with caplog.at_level(logging.INFO, logger="maskrcnn_benchmark.inference"):
        check_expected_results(r, [("bbox", "AP", (0.31, 0.01))], 4)
        check_expected_results(r, [("bbox", "AP", (0.40, 0.01))], 4)
    text = [rec.getMessage() for rec in caplog.records]
    assert text[0].startswith("PASS") and text[1].startswith("FAIL")


def test_ops_and_abi_carry_the_coco_kernels():
    from abr_iod_amd import _lib, ops
    for name in ("abr_coco_box_iou", "abr_coco_mask_iou", "abr_coco_match", "abr_coco_match_max_gt"):
        assert name in _lib.EXPORTS
    assert _lib.lib().abr_coco_match_max_gt() == ops.COCO_MATCH_MAX_GT == 128
    # the argument checks run without a GPU: one lane per (area range, threshold)
    assert _lib.lib().abr_coco_match(None, None, None, None, None, None, None, 1, 0, 0, None, 9, None, 10, None, None, None, None, None) == -1
    assert b"coco_match" in _lib.lib().abr_last_error()
    with pytest.raises(RuntimeError):
        ops.coco_match(np.zeros(0), [0], [0], [], [], [], H.AREA_RNG, H.IOU_THRS, device="cpu")

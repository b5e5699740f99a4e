"""CPU: the host restatement of proposal recall (coco_eval_host.proposal_recall_host = the reference's evaluate_box_proposals) on cases
worked out by hand, against the reference's inner loop written out again here on seeded random cases, and through do_coco_evaluation
(box_only=True, device="cpu") on the tiny COCO fixture."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coco_eval_common import tiny  # noqa: E402
from proposal_recall_common import HAND, bits, random_image  # noqa: E402

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H  # noqa: E402

KEYS = ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]


def _recalls(hits, num_pos):
    return (torch.tensor(hits, dtype=torch.float32) / float(num_pos)).tolist()


def test_iou_exactly_half_counts_at_the_first_threshold():
    r = H.proposal_recall_host(HAND["iou_exactly_half"])
    assert r["gt_overlaps"].tolist() == [0.5] and r["num_pos"] == 1
    assert r["thresholds"][0].item() == 0.5 and len(r["thresholds"]) == 10
    assert r["recalls"].tolist() == [1.0] + [0.0] * 9
    assert r["ar"].item() == torch.tensor([1.0] + [0.0] * 9).mean().item()
    assert set(r) == {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}


def test_identical_and_disjoint_boxes():
    r = H.proposal_recall_host(HAND["identical"])
    assert r["gt_overlaps"].tolist() == [1.0] and r["recalls"].tolist() == [1.0] * 10 and r["ar"].item() == 1.0
    r = H.proposal_recall_host(HAND["disjoint"])
    assert r["gt_overlaps"].tolist() == [0.0] and r["recalls"].tolist() == [0.0] * 10 and r["ar"].item() == 0.0 and r["num_pos"] == 1


def test_fewer_proposals_than_ground_truths_leaves_zeros_that_count():
    r = H.proposal_recall_host(HAND["fewer_proposals_than_gts"])
    assert r["gt_overlaps"].tolist() == [0.0, 0.0, 1.0] and r["num_pos"] == 3
    assert r["recalls"].tolist() == _recalls([1] * 10, 3)


def test_more_proposals_than_ground_truths():
    r = H.proposal_recall_host(HAND["more_proposals_than_gts"])
    assert r["gt_overlaps"].tolist() == [1.0] and r["num_pos"] == 1


def test_limit_cuts_before_the_cover():
    ims = HAND["limit_cuts_before_the_cover"]
    assert H.proposal_recall_host(ims, limit=1)["gt_overlaps"].tolist() == [0.0]
    assert H.proposal_recall_host(ims, limit=2)["gt_overlaps"].tolist() == [1.0]
    assert H.proposal_recall_host(ims)["gt_overlaps"].tolist() == [1.0]


def test_area_range_ends_are_inclusive():
    ims = HAND["area_exactly_32_squared"]
    assert [H.proposal_recall_host(ims, area=a)["num_pos"] for a in ("all", "small", "medium", "large")] == [1, 1, 1, 0]


def test_areas_are_rounded_to_float32_before_they_are_compared():
    ims = HAND["area_just_above_32_squared"]
    assert ims[0]["gt_area"][0] > 1024 and np.float32(ims[0]["gt_area"][0]) == 1024
    r = H.proposal_recall_host(ims, area="small")
    assert r["num_pos"] == 1 and r["gt_overlaps"].tolist() == [1.0]


def test_crowd_annotations_are_ignored():
    r = H.proposal_recall_host(HAND["crowd_is_ignored"])
    assert r["num_pos"] == 1 and r["gt_overlaps"].tolist() == [1.0]
    # an image whose only annotations are crowds is skipped like one without annotations
    only = [dict(HAND["crowd_is_ignored"][0], gt_crowd=[True, True])]
    assert H.proposal_recall_host(only)["num_pos"] == 0


def test_image_without_proposals_adds_to_num_pos_only():
    r = H.proposal_recall_host(HAND["image_without_proposals"])
    assert r["num_pos"] == 3 and r["gt_overlaps"].tolist() == [1.0]
    assert r["recalls"].tolist() == _recalls([1] * 10, 3)


def test_empty_range_gives_nan():
    r = H.proposal_recall_host(HAND["empty_range"], area="large")
    assert r["num_pos"] == 0 and r["gt_overlaps"].numel() == 0
    assert math.isnan(r["ar"].item()) and all(math.isnan(v) for v in r["recalls"].tolist())


def test_ties_go_to_the_lowest_ground_truth_then_the_lowest_rank():
    im = HAND["tie_between_ground_truths"][0]
    gt, _ = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
    assert H.proposal_iou(im["boxes"], gt).tolist() == [[0.5, 0.5], [0.25, 0.0]]
    assert H.proposal_cover(im["boxes"], gt).tolist() == [0.5, 0.0]
    im = HAND["tie_between_proposals"][0]
    gt, _ = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
    late = (torch.tensor(20.0) / torch.tensor(230.0)).item()
    assert H.proposal_iou(im["boxes"], gt).tolist() == [[0.5, 0.0], [0.5, late]]
    assert H.proposal_cover(im["boxes"], gt).tolist() == [0.5, late]
    im = HAND["duplicates"][0]
    gt, _ = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
    assert H.proposal_cover(im["boxes"], gt).tolist() == [1.0, 1.0, 0.5]


def test_unsorted_objectness_is_ranked_stably():
    ims = HAND["unsorted_objectness"]
    assert H.proposal_rank(ims[0]["objectness"]).tolist() == [1, 2, 0]
    assert H.proposal_recall_host(ims, limit=1)["gt_overlaps"].tolist() == [0.0]
    assert H.proposal_recall_host(ims, limit=2)["gt_overlaps"].tolist() == [1.0]


def _reference_loop(prop, gt):
    """coco_eval.py:316-334 written out again: numpy float32 IoU in boxlist_iou's operation order, then the loop on a clone.  The loop is
    the reference's text and so is coco_eval_host.proposal_cover's: what the agreement pins independently is the IoU arithmetic (numpy
    against torch) and the ranking / limit / range plumbing around the cover.  The tie rule is pinned by the hand cases above."""
    p, g = prop.numpy().astype(np.float32), gt.numpy().astype(np.float32)
    one = np.float32(1)
    area1 = (p[:, 2] - p[:, 0] + one) * (p[:, 3] - p[:, 1] + one)
    area2 = (g[:, 2] - g[:, 0] + one) * (g[:, 3] - g[:, 1] + one)
    lt = np.maximum(p[:, None, :2], g[None, :, :2])
    rb = np.minimum(p[:, None, 2:], g[None, :, 2:])
    wh = np.maximum(rb - lt + one, np.float32(0))
    inter = wh[:, :, 0] * wh[:, :, 1]
    overlaps = torch.from_numpy(inter / (area1[:, None] + area2[None, :] - inter)).clone()
    assert overlaps.dtype == torch.float32
    out = torch.zeros(len(g))
    for j in range(min(len(p), len(g))):
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_ovr, gt_ind = max_overlaps.max(dim=0)
        box_ind = argmax_overlaps[gt_ind]
        out[j] = overlaps[box_ind, gt_ind]
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return out


def test_agrees_with_the_reference_loop_on_random_cases_bit_for_bit():
    rng = np.random.default_rng(7)
    seen_ties = 0
    for case in range(200):
        P, G = int(rng.integers(1, 40)), int(rng.integers(1, 12))
        im = random_image(rng, P, G, fractional=case % 4 == 3)
        gt, area = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
        if len(gt) == 0:
            continue
        limit = int(rng.integers(1, P + 1))
        ranked = im["boxes"][H.proposal_rank(im["objectness"], limit)]
        want = _reference_loop(ranked, gt)
        iou = H.proposal_iou(ranked, gt)
        seen_ties += int((iou == iou.max()).sum() > 1)
        assert np.array_equal(bits(H.proposal_cover(ranked, gt)), bits(want)), case
        r = H.proposal_recall_host([im], limit=limit)
        assert r["num_pos"] == len(gt)
        assert np.array_equal(bits(r["gt_overlaps"]), bits(torch.sort(want)[0])), case
        # and one area range
        valid = (area >= 0) & (area <= 1024)
        rs = H.proposal_recall_host([im], limit=limit, area="small")
        assert rs["num_pos"] == int(valid.sum())
        if valid.any():
            assert np.array_equal(bits(rs["gt_overlaps"]), bits(torch.sort(_reference_loop(ranked, gt[valid]))[0])), case
    assert seen_ties > 50, seen_ties       # the generator does produce exact ties at the maximum


# ------------------------------------------------------------------------------------------------ through do_coco_evaluation
def _fixture_predictions(ds, shifted):
    """the fixture's non-crowd ground truths as proposals (objectness descending in file order); shifted: each one shortened so that its
    IoU with its own ground truth is h' / h (or w' / w) exactly and it meets no other ground truth"""
    from abr_iod_amd.structures.bounding_box import BoxList
    cut = {(5, 5, 40, 40): (5, 5, 40, 31), (60, 2, 20, 20): (60, 2, 20, 10), (10, 10, 120, 100): (10, 10, 120, 92),
           (150, 20, 32, 32): (150, 20, 32, 16)}
    preds = []
    for index in range(len(ds)):
        info = ds.get_img_info(index)
        boxes = [tuple(a["bbox"]) for a in ds.get_annotations(index) if not a.get("iscrowd", 0)]
        if shifted:
            boxes = [cut.get(b, b) for b in boxes]
        bl = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (info["width"], info["height"]), mode="xywh").convert("xyxy")
        bl.add_field("objectness", torch.tensor([0.9 - 0.1 * k for k in range(len(boxes))], dtype=torch.float32))
        preds.append(bl)
    return preds


def test_box_only_on_the_tiny_fixture(tmp_path):
    from abr_iod_amd.data.datasets.evaluation import evaluate
    ds = tiny()
    # the fixture: areas 1600, 1800 (medium), 400 (small) | 12000 (large), 1024 (small and medium), one crowd: every range is populated
    results, second = evaluate(ds, _fixture_predictions(ds, False), str(tmp_path), box_only=True, iou_types=("bbox",), device="cpu")
    assert second is None
    assert list(results.results["box_proposal"]) == KEYS
    assert all(v == 1.0 for v in results.results["box_proposal"].values())
    saved = torch.load(str(tmp_path / "box_proposals.pth"), weights_only=False)
    assert saved.results == results.results
    # shifted: overlaps 0.775, 1, 0.5 | 0.92, 0.5 -> how many reach 0.5, 0.55, ..., 0.95, over the ground truths of the range
    results, _ = evaluate(ds, _fixture_predictions(ds, True), None, box_only=True, iou_types=("bbox",), device="cpu")
    hand = {"AR": ([5, 3, 3, 3, 3, 3, 2, 2, 2, 1], 5), "ARs": ([2] + [0] * 9, 2), "ARm": ([3, 2, 2, 2, 2, 2, 1, 1, 1, 1], 3), "ARl": ([1] * 9 + [0], 1)}
    for key, (hits, num_pos) in hand.items():
        want = (torch.tensor(hits, dtype=torch.float32) / float(num_pos)).mean().item()
        for limit in (100, 1000):
            assert results.results["box_proposal"]["{}@{}".format(key, limit)] == want, key


def test_evaluate_box_proposals_has_the_references_signature():
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import evaluate_box_proposals
    ds = tiny()
    r = evaluate_box_proposals(_fixture_predictions(ds, True), ds, area="large", limit=100, device="cpu")
    assert r["num_pos"] == 1 and r["gt_overlaps"].tolist() == [(torch.tensor(11040.0) / torch.tensor(12000.0)).item()]
    with pytest.raises(AssertionError, match="Unknown area range"):
        evaluate_box_proposals(_fixture_predictions(ds, True), ds, area="huge", device="cpu")


def test_a_prediction_without_objectness_names_the_image_and_its_fields():
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import do_coco_evaluation
    ds = tiny()
    preds = _fixture_predictions(ds, False)
    bare = preds[1].copy_with_fields([])
    bare.add_field("scores", torch.ones(len(bare)))
    with pytest.raises(ValueError, match=r"image {}.*objectness.*scores".format(ds.id_to_img_map[1])):
        do_coco_evaluation(ds, [preds[0], bare], True, None, ("bbox",), (), 4, device="cpu")

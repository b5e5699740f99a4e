"""Shared by tests/test_coco_eval_host.py and tests/test_gpu_coco_eval.py: the tiny COCO fixture, the hand-made groups whose answers are
worked out in the tests, seeded random groups, and predictions for the fixture."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_tiny.json")


def tiny(remove=True, **kw):
    from abr_iod_amd.data.datasets.coco import COCODataset
    return COCODataset(FIXTURE, os.path.dirname(FIXTURE), remove, **kw)


def box_group(det, gt, crowd=None, gt_area=None):
    """a group of xywh boxes; gt_area defaults to w * h"""
    det, gt = np.asarray(det, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    crowd = np.zeros(len(gt), bool) if crowd is None else np.asarray(crowd, bool)
    return {"det": det, "gt": gt, "gt_crowd": crowd, "det_area": det[:, 2] * det[:, 3],
            "gt_area": gt[:, 2] * gt[:, 3] if gt_area is None else np.asarray(gt_area, np.float64)}


# name -> group; the answers are in test_coco_eval_host.py
HAND_GROUPS = {
    "iou_exactly_half": box_group([[0, 0, 10, 10]], [[0, 0, 10, 20]]),
    "iou_exactly_three_quarters": box_group([[0, 0, 30, 10]], [[0, 0, 40, 10]]),
    "equal_iou_two_gts": box_group([[0, 0, 10, 10]], [[0, 0, 10, 20], [0, -10, 10, 20]]),
    "only_on_a_crowd": box_group([[0, 0, 10, 10]], [[100, 100, 10, 10], [0, 0, 20, 20]], crowd=[0, 1]),
    "two_on_one_crowd": box_group([[0, 0, 10, 10], [5, 5, 10, 10]], [[0, 0, 20, 20]], crowd=[1]),
    "crowd_first_in_file": box_group([[0, 0, 10, 10], [1, 0, 10, 10]], [[0, 0, 20, 20], [0, 0, 10, 10]], crowd=[1, 0]),
    "area_exactly_32_squared": box_group([[0, 0, 32, 32]], [[0, 0, 32, 32]]),
    "zero_area_boxes": box_group([[5, 5, 0, 0], [0, 0, 10, 0], [0, 0, 10, 10]], [[0, 0, 10, 10], [5, 5, 0, 0]], crowd=[0, 1]),
    "no_detections": box_group([], [[0, 0, 10, 10]]),
    "no_ground_truth": box_group([[0, 0, 10, 10]], []),
    "nothing": box_group([], []),
}


def random_box_group(rng, D, G):
    """integer-ish boxes with crowds, repeated boxes and zero-area boxes"""
    def boxes(n):
        b = np.concatenate([rng.integers(0, 60, (n, 2)), rng.integers(0, 50, (n, 2))], axis=1).astype(np.float64)
        b[rng.random(n) < 0.3] += 0.25
        return b
    det, gt = boxes(D), boxes(G)
    if D and G:
        k = min(D, G)
        det[:k:3] = gt[:k:3]                    # exact copies: IoU 1
    return box_group(det, gt, crowd=rng.random(G) < 0.2)


def random_grid_group(rng, D, G):
    """a group given by its IoU matrix: multiples of 1/20, so ties and exact thresholds are frequent and nothing is within 1e-9 of a
    threshold without being equal to it"""
    iou = rng.integers(0, 21, (D, G)).astype(np.float64) / 20.0
    iou[rng.random((D, G)) < 0.5] = 0.0
    area = lambda n: rng.choice([10.0, 1024.0, 1025.0, 5000.0, 9216.0, 9217.0, 20000.0], n)      # noqa: E731
    return {"iou": iou, "det_area": area(D), "gt_area": area(G), "gt_crowd": rng.random(G) < 0.2}


def tiny_predictions(dataset, device="cpu", with_masks=False, perfect=False):
    """one BoxList per image of the (filtered) fixture: the non-crowd annotations (perfect=True), or those shifted, one false positive
    per image and a detection lying on the crowd"""
    from abr_iod_amd.structures.bounding_box import BoxList
    preds = []
    rng = np.random.default_rng(3)
    for index in range(len(dataset)):
        info = dataset.get_img_info(index)
        w, h = info["width"], info["height"]
        anns = [a for a in dataset.get_annotations(index) if not a.get("iscrowd", 0)]
        boxes = [list(a["bbox"]) for a in anns]
        labels = [dataset.json_category_id_to_contiguous_id[a["category_id"]] for a in anns]
        scores = [0.9 - 0.1 * k for k in range(len(anns))]
        if not perfect:
            for b in boxes:
                b[0] += int(rng.integers(-3, 4))
                b[2] -= int(rng.integers(0, 6))
            boxes += [[2, 2, 12, 9], [150, 90, 30, 40]]
            labels += [labels[0] if labels else 1, 1]
            scores += [0.95, 0.5]
        bl = BoxList(torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4), (w, h), mode="xywh")
        # xywh -> xyxy here is x + w - 1: prepare_for_coco_detection's convert("xywh") adds the 1 back
        bl = bl.convert("xyxy")
        bl.add_field("labels", torch.tensor(labels, dtype=torch.int64))
        bl.add_field("scores", torch.tensor(scores, dtype=torch.float64))
        if with_masks:
            m = torch.zeros((len(boxes), 1, h, w), dtype=torch.uint8)
            for k, (x, y, bw, bh) in enumerate(boxes):
                m[k, 0, int(y): int(y + bh), int(x): int(x + bw)] = 1
            bl.add_field("mask", m)
        preds.append(bl.to(device))
    return preds

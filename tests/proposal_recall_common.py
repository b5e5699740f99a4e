"""Shared by tests/test_proposal_recall_host.py and tests/test_gpu_proposal_recall.py: images in the form coco_eval_host's proposal-recall
section takes, the hand-made cases whose answers are worked out in the host test, and seeded random images."""
import numpy as np
import torch


def image(boxes, gt_xywh, objectness=None, gt_area=None, gt_crowd=None):
    """boxes: xyxy proposals at the original image size; objectness defaults to descending in the given order; gt_area to w * h"""
    boxes = torch.tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    gt = [list(map(float, g)) for g in gt_xywh]
    return {"boxes": boxes,
            "objectness": torch.tensor([1.0 - 0.001 * k for k in range(len(boxes))] if objectness is None else objectness, dtype=torch.float32),
            "gt_boxes": gt, "gt_area": [g[2] * g[3] for g in gt] if gt_area is None else list(gt_area),
            "gt_crowd": [False] * len(gt) if gt_crowd is None else list(gt_crowd)}


GT = [0, 0, 10, 10]                # xywh: the box [0,0,9,9], area 100
HALF, SAME, AWAY = [0, 0, 9, 4], [0, 0, 9, 9], [20, 20, 29, 29]          # xyxy proposals: IoU with GT 0.5, 1, 0

# name -> list of images; the answers are in test_proposal_recall_host.py
HAND = {
    "iou_exactly_half": [image([HALF], [GT])],
    "identical": [image([SAME], [GT])],
    "disjoint": [image([AWAY], [GT])],
    "fewer_proposals_than_gts": [image([[30, 0, 39, 9]], [GT, [30, 0, 10, 10], [60, 0, 10, 10]])],
    "more_proposals_than_gts": [image([HALF, SAME, AWAY], [GT])],
    "limit_cuts_before_the_cover": [image([AWAY, SAME], [GT])],
    "area_exactly_32_squared": [image([[0, 0, 31, 31]], [[0, 0, 32, 32]])],
    "area_just_above_32_squared": [image([[0, 0, 31, 31]], [[0, 0, 32, 32]], gt_area=[1024.00001])],
    "crowd_is_ignored": [image([SAME], [GT, [30, 0, 10, 10]], gt_crowd=[False, True])],
    "image_without_proposals": [image([SAME], [GT]), image([], [GT, [30, 0, 10, 10]])],
    "empty_range": [image([SAME], [GT])],
    # both ground truths have their best overlap, 0.5, with proposal 0: the tie goes to ground truth 0, ground truth 1 is left with nothing
    # (the other way round ground truth 0 would still get 0.25 from proposal 1)
    "tie_between_ground_truths": [image([[0, 0, 9, 9], [0, 10, 9, 14]], [[0, 0, 10, 20], [0, 0, 20, 10]])],
    # ground truth 0 has 0.5 with proposals 0 and 1: proposal 0 retires, so ground truth 1 still finds proposal 1 (20 / 230)
    "tie_between_proposals": [image([[0, 0, 9, 4], [0, 5, 9, 9]], [GT, [0, 8, 10, 20]])],
    "duplicates": [image([HALF, HALF, SAME, SAME], [GT, GT, GT])],
    # rank order is 1, 2, 0: of the two proposals with objectness 0.9 the first one (disjoint) comes first
    "unsorted_objectness": [image([SAME, AWAY, SAME], [GT], objectness=[0.5, 0.9, 0.9])],
}


def random_image(rng, P, G, fractional=False, crowds=True):
    """P proposals and exactly G NON-CROWD ground truths: integer-valued boxes in a 64 x 64 window (exact IoU ties are frequent), repeated
    boxes, tied objectness and areas on the range borders; crowds: about G / 10 crowd annotations (at least one) on top of the G, at random
    places among them, which the protocol drops again; fractional: quarter-pixel coordinates instead"""
    n_crowd = max(1, int(rng.binomial(G, 0.1))) if crowds else 0
    n_gt, G = G, G + n_crowd
    def xyxy(n):
        x1, y1 = rng.integers(0, 48, n), rng.integers(0, 48, n)
        b = np.stack([x1, y1, x1 + rng.integers(0, 16, n), y1 + rng.integers(0, 16, n)], 1).astype(np.float64)
        if fractional:
            b += rng.integers(0, 4, (n, 4)) * 0.25
            b[:, 2:] = np.maximum(b[:, 2:], b[:, :2])
        return b
    prop, gt = xyxy(P), xyxy(G)
    if P and G:
        k = min(P, G)
        prop[:k:3] = gt[:k:3]                                   # exact copies: IoU 1
    if P > 3:
        prop[P // 2] = prop[0]                                   # repeated proposals
        prop[P - 1] = prop[1]
    if G > 3:
        gt[G - 1] = gt[0]                                        # repeated ground truths
    gt_xywh = np.concatenate([gt[:, :2], gt[:, 2:] - gt[:, :2] + 1], 1)
    area = rng.choice([10.0, 1024.0, 1024.00001, 1025.0, 5000.0, 9216.0, 9217.0, 20000.0], G)
    crowd = np.zeros(G, bool)
    crowd[rng.permutation(G)[:n_crowd]] = True
    assert int((~crowd).sum()) == n_gt
    return image(prop.tolist(), gt_xywh.tolist(), objectness=(rng.integers(0, 8, P) / 8.0).tolist(), gt_area=area.tolist(),
                 gt_crowd=crowd.tolist())


def bits(t):
    """float32 tensor / array -> its bit patterns (int32 numpy)"""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, np.float32).view(np.int32)

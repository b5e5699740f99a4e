"""Shared by tests/test_coco_keypoints_host.py and tests/test_gpu_coco_keypoints.py: the person-keypoint fixture
(tests/golden/coco_kp_tiny.json), predictions for it whose scores are worked out by hand in the CPU test, and seeded random keypoint groups.

The fixture (5 images of 400 x 300, one category, 17 keypoints):
  image 1: id 1 (area 5000, all visible), id 2 (area 1024 = 32^2, all labelled), id 3 (a crowd: no keypoints, box [250,100,120,150])
  image 2: id 4 (area 9216 = 96^2), id 5 (num_keypoints 0 but a box [200,50,50,60]; not a crowd)
  image 3: id 6 (area 20000), id 7 (area 600, four labelled points: shoulders and hips)
  image 4: id 8 (area 2500, twelve labelled points, no num_keypoints key)
  image 5: nothing
It is loaded with remove_images_without_annotations=False."""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "coco_kp_tiny.json")

# where a keypoint sits in an instance's box, as fractions of its width and height (the fixture's annotations use the same figure)
FIGURE = [(.5, .1), (.55, .08), (.45, .08), (.6, .1), (.4, .1), (.7, .25), (.3, .25), (.8, .4), (.2, .4), (.85, .55), (.15, .55), (.65, .6),
          (.35, .6), (.65, .8), (.35, .8), (.65, .95), (.35, .95)]


def kp_tiny(**kw):
    from abr_iod_amd.data.datasets.coco import COCODataset
    kw.setdefault("device", "cpu")
    return COCODataset(FIXTURE, os.path.dirname(FIXTURE), False, **kw)


def figure(box):
    """17 keypoints (x, y, 2) laid into an xywh box"""
    return [[round(box[0] + box[2] * fx), round(box[1] + box[3] * fy), 2] for fx, fy in FIGURE]


# The imperfect predictions, per image index: (annotation id to copy or None, shift in x or the box to lay a figure into, score).
# No two scores are equal.  What each one does is said where the CPU test works the answer out.
SHIFTED = {
    0: [(None, [0, 250, 40, 40], 0.95), (1, 3, 0.9), (2, 2, 0.8), (None, [260, 110, 60, 100], 0.7), (None, [300, 150, 50, 80], 0.6)],
    1: [(4, 1, 0.91), (None, [205, 55, 40, 50], 0.61), (None, [210, 60, 30, 40], 0.51), (None, [330, 200, 50, 80], 0.31)],
    2: [(6, 10, 0.92), (7, 1, 0.82), (None, [200, 20, 60, 100], 0.42)],
    3: [(None, [5 + 15 * i, 5, 30, 40], 0.895 - 0.01 * i) for i in range(19)] + [(8, 2, 0.5)] + [(8, 0, s) for s in (0.4, 0.35, 0.3, 0.25, 0.2)],
    4: [(None, [100, 100, 40, 60], 0.852)],
}
SHIFT_OF = {1: 3, 2: 2, 4: 1, 6: 10, 7: 1, 8: 2}       # annotation id -> the shift of the one detection that follows it


def kp_tiny_predictions(dataset, device="cpu", perfect=False, keep=None, scale=1):
    """one BoxList per image with "labels", "scores" and a PersonKeypoints "keypoints" field.  perfect=True: a copy of every annotation
    that is not a crowd and has labelled keypoints; else SHIFTED, of image 4 only the `keep` best-scored when keep is given.
    scale: the predictions live on an image `scale` times the file's size (prepare_for_coco_keypoint resizes them back)."""
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    preds = []
    for index in range(len(dataset)):
        info = dataset.get_img_info(index)
        size = (info["width"] * scale, info["height"] * scale)
        anns = {a["id"]: a for a in dataset.get_annotations(index)}
        kps, scores = [], []
        if perfect:
            for k, a in enumerate(a for a in anns.values() if not a["iscrowd"] and any(v > 0 for v in a["keypoints"][2::3])):
                kps.append(np.array(a["keypoints"], np.float64).reshape(17, 3))
                scores.append(0.9 - 0.1 * k)
        else:
            for src, how, score in SHIFTED[index]:
                kp = np.array(figure(how) if src is None else anns[src]["keypoints"], np.float64).reshape(17, 3)
                if src is not None:
                    kp[kp[:, 2] > 0, 0] += how
                kps.append(kp)
                scores.append(score)
            if keep is not None and index == 3:
                kps, scores = kps[:keep], scores[:keep]
        kp = torch.tensor(np.array(kps).reshape(-1, 17, 3) * [scale, scale, 1], dtype=torch.float32)
        x, y = kp[:, :, 0], kp[:, :, 1]
        box = torch.stack([x.min(1).values, y.min(1).values, x.max(1).values, y.max(1).values], dim=1) if len(kps) else torch.zeros((0, 4))
        bl = BoxList(box, size, mode="xyxy")
        bl.add_field("labels", torch.ones(len(kps), dtype=torch.int64))
        bl.add_field("scores", torch.tensor(scores, dtype=torch.float64))
        bl.add_field("keypoints", PersonKeypoints(kp, size))
        preds.append(bl.to(device))
    return preds


def random_kp_group(rng, D, G, K):
    """seeded keypoint group: visibilities in {0,1,2}, some ground truths with none visible, some detections copied from ground truths
    (OKS exactly 1: every e_k is 0), the last detection 1e7 pixels away (exactly 0 against every ground truth: every e_k > 745, where exp
    underflows), some areas 0.  -> dict with det_kp, gt_kp, gt_box, gt_area, gt_crowd, gt_ignore and the index lists `copies` [(d, g)] and
    `far` [d]"""
    gt_box = np.concatenate([rng.uniform(0, 300, (G, 2)), rng.uniform(5, 120, (G, 2))], axis=1)
    gt_kp = np.zeros((G, K, 3))
    gt_kp[:, :, 0] = gt_box[:, None, 0] + gt_box[:, None, 2] * rng.random((G, K))
    gt_kp[:, :, 1] = gt_box[:, None, 1] + gt_box[:, None, 3] * rng.random((G, K))
    gt_kp[:, :, 2] = rng.integers(0, 3, (G, K))
    gt_kp[rng.random(G) < 0.25, :, 2] = 0                     # none visible: the doubled-box branch
    gt_area = gt_box[:, 2] * gt_box[:, 3] * rng.uniform(0.3, 0.9, G)
    gt_area[rng.random(G) < 0.15] = 0.0
    det_kp = np.zeros((D, K, 3))
    det_kp[:, :, :2] = rng.uniform(0, 420, (D, K, 2))
    det_kp[:, :, 2] = 1
    copies, far = [], []
    if D and G:
        for d in range(1, D, 2):                               # near a ground truth: e_k around 0.1 ... 4, where exp has something to do
            j = int(rng.integers(0, G))
            det_kp[d, :, :2] = gt_kp[j, :, :2] + rng.normal(0, 0.1 * np.sqrt(gt_area[j] + 1.0), (K, 2))
        for d in range(0, min(D - 1 if D > 1 else D, G), 3):   # (the last detection is the far one)
            det_kp[d, :, :2] = gt_kp[d, :, :2]
            if not (gt_kp[d, :, 2] > 0).any():                 # none visible: every point inside the doubled box, OKS 1 too
                det_kp[d, :, 0] = gt_box[d, 0] + gt_box[d, 2] * 0.5
                det_kp[d, :, 1] = gt_box[d, 1] + gt_box[d, 3] * 0.5
            copies.append((d, d))
        if D > 1:
            det_kp[D - 1, :, :2] = 1e7                         # e > 745 for every keypoint against every ground truth: exp underflows to 0
            far.append(D - 1)
    crowd = rng.random(G) < 0.2
    return {"det_kp": det_kp, "gt_kp": gt_kp, "gt_box": gt_box, "gt_area": gt_area, "gt_crowd": crowd,
            "gt_ignore": crowd | ~(gt_kp[:, :, 2] > 0).any(1), "copies": copies, "far": far}

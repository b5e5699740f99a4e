"""TEST INFRASTRUCTURE ONLY -- the float64 model of the FPN mask head and the fixture its suites share (tests/test_mask_head_fpn_config.py on
the CPU, tests/test_gpu_mask_head_fpn.py on the GPU, tests/golden/make_golden_mask_head_fpn.py where the reference tree exists).  Nothing here
imports the library under test.

MODEL: the four-level pooler (tests/pooler_ref.py's float64 forward and transpose, wrapped as tests/detector_fpn_ref.py's autograd Function)
at 14 x 14, sampling ratio 2 -> n x relu(conv3x3 + bias) -> mask_ref.mask_branch -> mask_ref.mask_loss, in torch float64 on the CPU; autograd
gives every gradient, the maps' included.

FIXTURE: the maps and the 74-row RoI table of tests/golden/pooler_fpn.npz.  POSITIVES names the rows of that table that are positives, each
matched to a ground-truth box equal to itself (IoU 1) that carries a label and an ellipse mask drawn from a seed; the -1-padded list is what
ops.mask_compact_pos gives for those labels at P_MAX."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import detector_fpn_ref as DR
import mask_ref
import pooler_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "mask_head_fpn.npz")
POOLED = os.path.join(HERE, "golden", "pooler_fpn.npz")

GOLDEN_SEED = 20251
RES, SAMPLING, M = 14, 2, 28
LAYERS = (8, 8)
NUM_CLASSES = 3
P_MAX = 16
# rows of the table: image 0, then image 1; levels 0, 1 and 2; row 0 is square_56 (the k_min boundary), row 37 square_112 (levels 0 | 1)
POSITIVES = (0, 9, 20, 24, 27, 37, 45, 49, 55, 63)
BOUNDARY_ROWS = (0, 37)
PARAMS = ("mask_fcn1", "mask_fcn2", "conv5_mask", "mask_fcn_logits")
# the tiny R-50-FPN + mask detector: tests/golden/make_golden_box_head_fpn.py's DETECTOR widths with the mask head on
MASK_CFG = ["MODEL.MASK_ON", True, "MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor",
            "MODEL.ROI_MASK_HEAD.PREDICTOR", "MaskRCNNC4Predictor", "MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
            "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", RES, "MODEL.ROI_MASK_HEAD.POOLER_SCALES", P.SCALES,
            "MODEL.ROI_MASK_HEAD.POOLER_SAMPLING_RATIO", SAMPLING, "MODEL.ROI_MASK_HEAD.RESOLUTION", M,
            "MODEL.ROI_MASK_HEAD.CONV_LAYERS", LAYERS]


def fixture():
    """dict: rois [74,5], lv, feats (NHWC float32 list), maps, B, C, image (h, w), labels int64 [74] (0 = not a positive), pos_rows int64 [P_MAX],
    n_pos, gt_boxes / gt_labels / gt_masks per image (uint8 [n,h,w])"""
    pg = np.load(POOLED)
    B, C = int(pg["B"]), int(pg["C"])
    maps = [tuple(int(v) for v in m) for m in pg["maps"]]
    img_h, img_w = (int(v) for v in pg["image"])
    rois = pg["rois"]
    lv = P.levels(rois)
    rng = np.random.default_rng(GOLDEN_SEED)
    labels = np.zeros(len(rois), np.int64)
    labels[list(POSITIVES)] = rng.integers(1, NUM_CLASSES, len(POSITIVES))
    pos_rows = np.full(P_MAX, -1, np.int64)
    pos_rows[:len(POSITIVES)] = POSITIVES
    ys, xs = np.mgrid[0:img_h, 0:img_w]
    gt_boxes, gt_labels, gt_masks = [], [], []
    for b in range(B):
        rows = [r for r in POSITIVES if rois[r, 0] == b]
        boxes = rois[rows, 1:].copy()
        masks = []
        for x1, y1, x2, y2 in boxes:       # an ellipse inside the part of the box that is inside the image, off-centre
            cx, cy = np.clip((x1 + x2) / 2, 8, img_w - 8) + rng.uniform(-4, 4), np.clip((y1 + y2) / 2, 8, img_h - 8) + rng.uniform(-4, 4)
            rx, ry = rng.uniform(0.2, 0.45) * min(x2 - x1, img_w), rng.uniform(0.2, 0.45) * min(y2 - y1, img_h)
            masks.append((((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0).astype(np.uint8))
        gt_boxes.append(boxes)
        gt_labels.append(labels[rows])
        gt_masks.append(np.stack(masks))
    return dict(rois=rois, lv=lv, feats=P.make_feats(int(pg["seed"]), B, C, maps), maps=maps, B=B, C=C, image=(img_h, img_w), labels=labels,
                pos_rows=pos_rows, n_pos=len(POSITIVES), gt_boxes=gt_boxes, gt_labels=gt_labels, gt_masks=gt_masks)


def check_fixture(fx):
    """the conditions the suites rely on"""
    rois, lv, rows = fx["rois"], fx["lv"], fx["pos_rows"]
    pos = rows[rows >= 0]
    assert all((rois[pos, 0] == b).any() for b in range(fx["B"])), "an image without a positive"
    assert len(set(lv[pos].tolist())) >= 3 and (lv[pos] >= 0).all(), "the positives reach fewer than three levels"
    assert (rows < 0).any(), "no padding entry"
    edge = {tuple(np.float32(v) for v in r[1:]) for r in P.edge_rows(*fx["image"]) if r[0].startswith("square_")}
    on_edge = [int(r) for r in pos if tuple(rois[r, 1:]) in edge]
    assert on_edge and set(BOUNDARY_ROWS) <= set(on_edge), "no positive on a level-boundary row"
    assert (np.diff(pos) > 0).all() and (np.diff(rois[pos, 0]) >= 0).all()       # compaction order: ascending rows, image by image


def params64(g):
    """golden (reference layout) -> {name: (weight, bias)} as float64 leaf tensors"""
    return {n: (torch.from_numpy(g["w_" + n].astype(np.float64)).requires_grad_(), torch.from_numpy(g["b_" + n].astype(np.float64)).requires_grad_())
            for n in PARAMS}


def conv_stack(pooled, p, names=("mask_fcn1", "mask_fcn2")):
    """-> the activations after each relu(conv3x3 + bias)"""
    acts, x = [], pooled
    for n in names:
        x = F.relu(F.conv2d(x, p[n][0], p[n][1], padding=1))
        acts.append(x)
    return acts


def model(fx, p, rows=None):
    """float64 forward on the positives (rows: default the fixture's, padding dropped) -> dict(maps (leaf tensors, logical NCHW), pooled, acts,
    logits [n_pos,K,M,M])"""
    rows = fx["pos_rows"] if rows is None else rows
    rows = rows[rows >= 0]
    maps = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2)).astype(np.float64)).requires_grad_() for f in fx["feats"]]
    pooled = DR._Pool.apply(fx["rois"][rows], fx["lv"][rows], RES, SAMPLING, *maps)
    pooled.retain_grad()
    acts = conv_stack(pooled, p)
    logits = mask_ref.mask_branch(acts[-1], *p["conv5_mask"], *p["mask_fcn_logits"])
    return dict(maps=maps, pooled=pooled, acts=acts, logits=logits)


def loss_of(logits, labels_pos, targets):
    return mask_ref.mask_loss(logits, torch.as_tensor(labels_pos), torch.as_tensor(np.asarray(targets, np.float64)))


def unpack_targets(g):
    """the reference's mask targets of the positives, stored as packed bits -> float64 [n_pos,M,M]"""
    n = int(g["n_pos"])
    return np.unpackbits(g["targets_bits"])[: n * M * M].reshape(n, M, M).astype(np.float64)


# --------------------------------------------------------------------------------------------------------------------- the detector
class MaskDetectorRef(DR.DetectorFPNRef):
    """tests/detector_fpn_ref.py's float64 R-50-FPN detector + the unshared mask branch"""

    def mask_head(self, ps, rois):
        """ps: P2..P6 (the mask pooler reads the first four), rois [n,5] -> (logits [n,K,2r,2r], levels)"""
        pooled, lv = DR.pool(list(ps[:4]), rois, res=RES, sr=SAMPLING)
        fe, pr = "roi_heads.mask.feature_extractor", "roi_heads.mask.predictor"
        x, i = pooled, 1
        while f"{fe}.mask_fcn{i}.weight" in self.p:
            x = F.relu(F.conv2d(x, self.p[f"{fe}.mask_fcn{i}.weight"], self.p[f"{fe}.mask_fcn{i}.bias"], padding=1))
            i += 1
        logits = mask_ref.mask_branch(x, self.p[f"{pr}.conv5_mask.weight"], self.p[f"{pr}.conv5_mask.bias"],
                                      self.p[f"{pr}.mask_fcn_logits.weight"], self.p[f"{pr}.mask_fcn_logits.bias"])
        return logits, lv


def mask_step(model, images, pos_rois, pos_labels, mask_targets, **box_and_rpn):
    """detector_fpn_ref.step (RPN + box head, no distillation) and the mask loss on the positives.  The gradient of a sum is the sum of the
    gradients: the box / RPN total is back-propagated by `step`, the mask loss through a second forward of the body -- both add into the same
    leaves.  -> step's dict with losses["loss_mask"], mask_logits, mask_levels and the total including the mask loss."""
    out = DR.step(model, images, **box_and_rpn)
    logits, lv = model.mask_head(model.features(images), np.ascontiguousarray(pos_rois, np.float32))
    lm = loss_of(logits, np.asarray(pos_labels, np.int64), mask_targets)
    lm.backward()
    out["losses"]["loss_mask"] = float(lm.detach())
    out["total"] += float(lm.detach())
    out.update(mask_logits=logits.detach().numpy(), mask_levels=lv)
    return out


def ellipse_masks(seed, boxes, h, w):
    """one uint8 [h,w] ellipse per ground-truth box, inside it and off-centre, from a seed (never stored)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w]
    out = []
    for x1, y1, x2, y2 in np.asarray(boxes, np.float64):
        cx, cy = (x1 + x2) / 2 + rng.uniform(-0.1, 0.1) * (x2 - x1), (y1 + y2) / 2 + rng.uniform(-0.1, 0.1) * (y2 - y1)
        rx, ry = rng.uniform(0.25, 0.4) * (x2 - x1), rng.uniform(0.25, 0.4) * (y2 - y1)
        out.append((((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0).astype(np.uint8))
    return np.stack(out)

"""TEST INFRASTRUCTURE ONLY -- the float64 model of the FPN keypoint head and the scene its suites share (tests/test_keypoint_fpn_config.py on
the CPU, tests/test_gpu_keypoint_head_fpn.py on the GPU, tests/golden/make_golden_keypoint_fpn.py where the reference tree exists).  Nothing
here imports the library under test.

MODEL: the four-level pooler (tests/pooler_ref.py's float64 forward and transpose, wrapped as tests/detector_fpn_ref.py's autograd Function) at
6 x 6, sampling ratio 2 -> n x relu(conv3x3 + bias) -> conv_transpose2d(4, 2, 1) -> tests/keypoint_ref.py's upsample2x -> cross-entropy over
the valid rows, in torch float64 on the CPU; autograd gives every gradient, the maps' included.  The selection and the heat-map targets are
tests/keypoint_ref.py's select_targets.

SCENE: 2 images of 640 x 512, maps of 16 channels at strides 4, 8, 16 and 32 drawn from a seed, a sampled set of 16 RoIs per image
(BATCH_SIZE_PER_IMAGE 16, POSITIVE_FRACTION 0.5: P_MAX = 16).  Image 0 holds a live positive on every level -- boxes of side 60, 150, 224,
300, 448 and 480 px, the 224 and the 448 ones exactly on a level boundary -- a positive whose instance has no visible keypoint, and a labelled
point far outside its box.  Every labelled point of image 1 lies outside its box: all of its positives are dropped.  The rest of P_MAX is
padding."""
import os

import numpy as np
import torch
import torch.nn.functional as F

import detector_fpn_ref as DR
import keypoint_ref as R
import pooler_ref as P

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden", "keypoint_head_fpn.npz")
SHAPES = os.path.join(HERE, "golden", "keypoint_fpn_state_dict_shapes.json")

GOLDEN_SEED = 20252
FEAT_SEED = 77
B, C, IMG_H, IMG_W = 2, 16, 512, 640
MAPS = tuple((IMG_H // s, IMG_W // s) for s in (4, 8, 16, 32))
RES, SAMPLING, M = 6, 2, 24
LAYERS = (16, 16)
KS = (5, 17)
PER_IMAGE, P_MAX = 16, 16
BLOCKS = ("conv_fcn1", "conv_fcn2")

# image 0: (x1, y1, x2, y2), side = x2 - x1 + 1 (the level rule's TO_REMOVE = 1)
GT0 = np.array([[10, 10, 69, 69],            # 60 px: P2
                [80, 10, 229, 159],          # 150 px: P3
                [400, 10, 623, 233],         # sqrt(area) exactly 224: the P3 | P4 boundary, P4 by the rule's eps
                [10, 200, 309, 499],         # 300 px: P4
                [180, 40, 627, 487],         # sqrt(area) exactly 448: the P4 | P5 boundary, P5
                [100, 16, 579, 495],         # 480 px: P5
                [330, 250, 389, 330]],       # nothing visible: its positive is dropped
               np.float32)
NOTHING_VISIBLE = 6
GT1 = np.array([[40, 40, 139, 159], [300, 100, 459, 299], [500, 300, 619, 479]], np.float32)
BOUNDARY_SIDES = (224, 448)
# the tiny R-50-FPN + keypoint detector: tests/golden/make_golden_box_head_fpn.py's DETECTOR widths with upstream's keypoint settings
# (e2e_keypoint_rcnn_R_50_FPN_1x) at CONV_LAYERS (8, 8)
DET_RES, DET_LAYERS = 14, (8, 8)
KEYPOINT_CFG = ["MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.FEATURE_EXTRACTOR", "KeypointRCNNFeatureExtractor",
                "MODEL.ROI_KEYPOINT_HEAD.PREDICTOR", "KeypointRCNNPredictor", "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
                "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", DET_RES, "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", P.SCALES,
                "MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", 2, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 4 * DET_RES,
                "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", DET_LAYERS]


def head_cfg_list(K):
    """the head alone at the scene's sizes, as a merge_from_list list"""
    return ["MODEL.BACKBONE.CONV_BODY", "R-50-FPN", "MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
            "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", RES, "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", P.SCALES,
            "MODEL.ROI_KEYPOINT_HEAD.POOLER_SAMPLING_RATIO", SAMPLING, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", M,
            "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", LAYERS, "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", K,
            "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", PER_IMAGE, "MODEL.ROI_HEADS.POSITIVE_FRACTION", 0.5]


def keypoints_for(gt, K, img):
    """[n,K,3] float32: point k of instance j at a fixed fraction of its box, the first two on opposite corners (the v == hi rule), every
    fourth one not labelled"""
    n = gt.shape[0]
    kp = np.zeros((n, K, 3), np.float32)
    for j in range(n):
        x1, y1, x2, y2 = gt[j]
        for k in range(K):
            fx, fy = ((7 * k + 3 * j) % 11 + 0.5) / 11, ((5 * k + 2 * j) % 13 + 0.5) / 13
            kp[j, k] = (x1 + fx * (x2 - x1), y1 + fy * (y2 - y1), 2)
        kp[j, 0, :2] = (x1, y1)
        kp[j, 1, :2] = (x2, y2)
        for k in range(K):
            if (j + k) % 4 == 3:
                kp[j, k] = 0
    if img == 0:
        kp[0, 2, :2] += 500.0                       # one labelled point far outside its box
        kp[NOTHING_VISIBLE, :, 2] = 0               # an instance with nothing visible
    else:
        kp[:, :, :2] += 1000.0                      # every point outside: all of this image's positives are dropped
    return kp


def _small_boxes(rng, n, avoid):
    """n boxes of 16..40 px inside the image whose IoU with every box of `avoid` is below 0.3: the negatives of the sampled set"""
    out = []
    while len(out) < n:
        w, h = rng.uniform(16, 40, 2)
        x1, y1 = rng.uniform(0, IMG_W - w - 1), rng.uniform(0, IMG_H - h - 1)
        b = np.array([x1, y1, x1 + w, y1 + h], np.float32)
        if max(R.box_iou_f32(g, b) for g in avoid) < 0.3:
            out.append(b)
    return np.stack(out)


def scene(K):
    """dict: rois [32,5] float32 (the sampled set's table, image 0's rows first), labels int64 [32] (> 0: a positive), gt_boxes, keypoints
    ([n,K,3] per image), feats (NHWC float32 list), lv (the level of every row), sel (keypoint_ref.select_targets at P_MAX)"""
    rng = np.random.default_rng(FEAT_SEED)
    jit = lambda b: (b + rng.uniform(-3, 3, 4)).astype(np.float32)       # noqa: E731
    # image 0: the six instances' own boxes (IoU 1: the boundary boxes keep their exact sides), a second box on the 150 px instance, the
    # positive of the instance without a visible point; the rest negatives
    pos0 = [GT0[i].copy() for i in range(6)] + [jit(GT0[1]), GT0[NOTHING_VISIBLE].copy()]
    neg0 = _small_boxes(rng, PER_IMAGE - len(pos0), GT0)
    order0 = [("p", 0), ("n", 0), ("p", 1), ("p", 2), ("n", 1), ("n", 2), ("p", 3), ("p", 7), ("p", 4), ("n", 3), ("p", 5), ("n", 4), ("p", 6), ("n", 5),
              ("n", 6), ("n", 7)]
    rows0 = [(pos0[i] if kind == "p" else neg0[i], 1 + i % 3 if kind == "p" else 0) for kind, i in order0]
    pos1 = [jit(GT1[0]), jit(GT1[1]), jit(GT1[2])]
    neg1 = _small_boxes(rng, PER_IMAGE - len(pos1), GT1)
    rows1 = [(neg1[0], 0), (pos1[0], 2), (pos1[1], 1)] + [(b, 0) for b in neg1[1:7]] + [(pos1[2], 3)] + [(b, 0) for b in neg1[7:]]
    rois = np.array([[i, *b] for i, rows in enumerate((rows0, rows1)) for b, _ in rows], np.float32)
    labels = np.array([l for rows in (rows0, rows1) for _, l in rows], np.int64)
    gt_boxes = [GT0, GT1]
    keypoints = [keypoints_for(GT0, K, 0), keypoints_for(GT1, K, 1)]
    sel = R.select_targets(rois, labels, gt_boxes, keypoints, M, P_MAX)
    return dict(K=K, rois=rois, labels=labels, gt_boxes=gt_boxes, keypoints=keypoints, feats=P.make_feats(FEAT_SEED, B, C, MAPS), lv=P.levels(rois),
                sel=sel, image=(IMG_H, IMG_W))


def check_scene(sc):
    """the conditions the suites rely on"""
    rois, labels, lv, sel = sc["rois"], sc["labels"], sc["lv"], sc["sel"]
    rows = sel["pos_rows"]
    live = rows[rows >= 0]
    assert len(rois) == B * PER_IMAGE and len(rows) == P_MAX == min(len(rois), B * PER_IMAGE // 2)
    assert sel["n_pos"] == len(live) and (np.diff(live) > 0).all()
    assert sorted(set(lv[live].tolist())) == [0, 1, 2, 3], "a level without a live positive"
    side = np.sqrt((rois[live, 3] - rois[live, 1] + 1.0) * (rois[live, 4] - rois[live, 2] + 1.0))
    for s, l in zip(BOUNDARY_SIDES, (2, 3)):
        on = live[side == s]
        assert len(on) == 1 and lv[on[0]] == l, "no live positive of sqrt(area) exactly %d on level %d" % (s, l)
    pos = np.nonzero(labels > 0)[0]
    dropped = sorted(set(pos.tolist()) - set(live.tolist()))
    assert any(rois[r, 0] == 0 for r in dropped), "no dropped positive next to live ones (the instance without a visible point)"
    assert (rois[live, 0] == 0).all() and (rois[pos, 0] == 1).sum() >= 2, "image 1's positives are not all dropped"
    kp0, g0 = sc["keypoints"][0], sc["gt_boxes"][0]
    outside = (kp0[:, :, 2] > 0) & ((kp0[:, :, 0] > g0[:, None, 2]) | (kp0[:, :, 1] > g0[:, None, 3]))
    assert outside[:NOTHING_VISIBLE].any(), "no labelled point outside its box"
    n = sel["n_pos"]
    assert (sel["valid"][:n].sum(1) > 0).all() and not sel["valid"][:n].all() and not sel["valid"][n:].any()
    assert (rows[n:] == -1).all() and n < P_MAX, "no padding row"


def params64(g, K):
    """golden (reference layout) -> {name: (weight, bias)} as float64 leaf tensors; the deconvolution under "kps_score_lowres" """
    leaf = lambda a: torch.from_numpy(np.asarray(a, np.float64)).requires_grad_()       # noqa: E731
    p = {n: (leaf(g["w_" + n]), leaf(g["b_" + n])) for n in BLOCKS}
    p["kps_score_lowres"] = (leaf(g["w%d_kps_score_lowres" % K]), leaf(g["b%d_kps_score_lowres" % K]))
    return p


def conv_stack(pooled, p, names=BLOCKS):
    acts, x = [], pooled
    for n in names:
        x = F.relu(F.conv2d(x, p[n][0], p[n][1], padding=1))
        acts.append(x)
    return acts


def head(pooled, p):
    """pooled [n,C,r,r] -> (acts, logits [n,K,4r,4r]): the stack, ConvTranspose2d(4, 2, 1) and the bilinear doubling"""
    acts = conv_stack(pooled, p, [n for n in p if n != "kps_score_lowres"])
    low = F.conv_transpose2d(acts[-1], *p["kps_score_lowres"], stride=2, padding=1)
    return acts, R.upsample2x(low)


def loss_of(logits, targets, valid):
    """logits [n,K,M,M], targets / valid [n,K] -> mean cross-entropy over the valid rows (0 without one: keypoint_head/loss.py:162-169)"""
    v = torch.as_tensor(np.asarray(valid)).reshape(-1).bool()
    if not bool(v.any()):
        return logits.sum() * 0
    n, K, h, w = logits.shape
    return F.cross_entropy(logits.reshape(n * K, h * w)[v], torch.as_tensor(np.asarray(targets, np.int64)).reshape(-1)[v])


def model(sc, p, feats=None, res=RES, sr=SAMPLING):
    """float64 forward on the live rows of the scene's selection -> dict(maps (leaf tensors, logical NCHW), pooled, acts, logits, loss)"""
    rows = sc["sel"]["pos_rows"]
    rows = rows[rows >= 0]
    n = len(rows)
    feats = sc["feats"] if feats is None else feats
    maps = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2)).astype(np.float64)).requires_grad_() for f in feats]
    pooled = DR._Pool.apply(sc["rois"][rows], sc["lv"][rows], res, sr, *maps)
    pooled.retain_grad()
    acts, logits = head(pooled, p)
    return dict(maps=maps, pooled=pooled, acts=acts, logits=logits, loss=loss_of(logits, sc["sel"]["targets"][:n], sc["sel"]["valid"][:n]))

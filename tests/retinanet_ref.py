"""RetinaNet's inference half restated without the library: numpy for the post-processor (candidates, decode, class-wise NMS, the cut), torch on
the CPU in float64 for LastLevelP6P7 (forward and backward) and RetinaNetHead's forward.  tests/test_retinanet_ref.py checks the restatement
against the reference's own output (tests/golden/retinanet.npz); the GPU tests check the library against both.

Where the reference leaves an order open the rules are the library's: equal scores inside an (image, level) segment go by ascending flat index
loc * A * C + a * C + c (torch.topk(sorted=False) there), equal scores inside a class by ascending candidate position level * pre + rank.

The ORDER inside a class is such a case.  The reference's _C.nms hands back the survivors' indices in ascending order (nms_cpu.cpp:66,
nms.cu:127-130), so a class's detections come out in candidate order: level by level, and inside a level in whatever order
topk(sorted=False) left -- nothing a second implementation can reproduce.  The library emits every class by descending score.  The golden
stores the reference's output as it came; `canonical` puts it into the library's order (its scores are all different, so that is one
well-defined permutation), and the comparisons are exact from there: the same members, the same labels, the same order."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import rpn_fpn_ref as F  # noqa: E402
from oracle import ops as O  # noqa: E402

# the golden's geometry (tests/golden/make_golden_retinanet.py)
STRIDES = (8, 16, 32, 64, 128)
SIZES = (16, 32, 64, 128, 256)
RATIOS = (0.5, 1.0, 2.0)
OCTAVE, SCALES_PER_OCTAVE = 2.0, 3
IMAGE_SIZES = ((128, 192), (112, 160))               # (h, w)
MAPS = ((16, 24), (8, 12), (4, 6), (2, 3), (1, 2))
A, C = 9, 4
PRE, NMS_TH, TH = 100, 0.4, 0.05
CAPS = (30, 1000)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)


def level_sizes(sizes=SIZES, octave=OCTAVE, per_octave=SCALES_PER_OCTAVE):
    """anchor_generator.py:149-155, in double precision as python computes it"""
    return tuple(tuple(octave ** (i / float(per_octave)) * s for i in range(per_octave)) for s in sizes)


def pyramid_anchors(maps=MAPS, strides=STRIDES, sizes=SIZES, ratios=RATIOS, image_hw=IMAGE_SIZES[0]):
    """per level the [H*W*A,4] anchors from the oracle's C restatement"""
    return [O.grid_anchors(O.cell_anchors(stride=st, sizes=s, ratios=ratios), H, W, st, image_hw)[0]
            for (H, W), st, s in zip(maps, strides, level_sizes(sizes))]


def segment_ref(cls, reg, anchors, A, C, image_hw, th, pre, min_size=0, weights=WEIGHTS, score_fn=F.torch_sigmoid):
    """One (image, level): cls [nloc, >= A*C] logits (column a * C + c), reg [nloc, >= 4A] deltas, anchors [nloc*A,4] -> dict of the kept
    candidates in rank order: flat, scores, labels, boxes (inference.py:73-123)"""
    cls, reg = np.asarray(cls, np.float32), np.asarray(reg, np.float32)
    nloc = cls.shape[0]
    scores = score_fn(np.ascontiguousarray(cls[:, :A * C]).reshape(1, -1))[0]
    cand = np.nonzero(scores > np.float32(th))[0]
    order = cand[np.lexsort((cand, -scores[cand].astype(np.float64)))][:pre]
    a_idx, labels = order // C, order % C + 1
    deltas = np.ascontiguousarray(reg[:, :4 * A]).reshape(nloc * A, 4)[a_idx]
    boxes = O.box_decode(deltas, np.ascontiguousarray(anchors[a_idx], np.float32), weights) if len(order) else np.zeros((0, 4), np.float32)
    h, w = image_hw
    boxes[:, 0::2] = np.clip(boxes[:, 0::2], 0, w - 1)
    boxes[:, 1::2] = np.clip(boxes[:, 1::2], 0, h - 1)
    if min_size > 0:
        ok = (boxes[:, 2] - boxes[:, 0] + 1 >= min_size) & (boxes[:, 3] - boxes[:, 1] + 1 >= min_size)
        order, labels, boxes = order[ok], labels[ok], boxes[ok]
    return dict(flat=order, scores=scores[order], labels=labels.astype(np.int64), boxes=boxes, n_cand=len(cand))


def image_ref(segments, C, pre, nms_th, det):
    """segments: one image's levels (segment_ref's output) -> dict boxes, scores, labels, src (candidate position level * pre + rank), n_nms
    (survivors before the cut): class by class, descending score, ties by ascending position; NMS `>=`; the detections cut keeps ties
    (inference.py:131-174)"""
    boxes = np.concatenate([s["boxes"] for s in segments]).reshape(-1, 4)
    scores = np.concatenate([s["scores"] for s in segments]).astype(np.float32)
    labels = np.concatenate([s["labels"] for s in segments])
    pos = np.concatenate([l * pre + np.arange(len(s["flat"])) for l, s in enumerate(segments)]).astype(np.int64)
    keep = []
    for j in range(1, C + 1):
        idx = np.nonzero(labels == j)[0]
        idx = idx[np.lexsort((pos[idx], -scores[idx].astype(np.float64)))]
        if len(idx):
            keep.append(idx[F.nms64(boxes[idx], nms_th, len(idx) + 1)])
    keep = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    n_nms = len(keep)
    if det > 0 and n_nms > det:
        kth = np.sort(scores[keep])[::-1][det - 1]
        keep = keep[scores[keep] >= kth]
    return dict(boxes=boxes[keep], scores=scores[keep], labels=labels[keep], src=pos[keep], n_nms=n_nms)


def detect_ref(cls, reg, anchors, A, C, image_sizes, th, pre, nms_th, det, min_size=0, weights=WEIGHTS, score_fn=F.torch_sigmoid):
    """cls / reg: lists of L arrays [N, nloc_l, ld]; anchors: list of L [nloc_l*A,4] -> per image image_ref's dict (plus `segments`)"""
    out = []
    for i, hw in enumerate(image_sizes):
        segs = [segment_ref(cls[l][i], reg[l][i], anchors[l], A, C, hw, th, pre, min_size, weights, score_fn) for l in range(len(cls))]
        d = image_ref(segs, C, pre, nms_th, det)
        d["segments"] = segs
        out.append(d)
    return out


def canonical(boxes, scores, labels):
    """the reference's detections of one image in the library's order: class by class (as they are), each class by descending score"""
    order = np.lexsort((-np.asarray(scores, np.float64), labels))
    assert np.array_equal(np.asarray(labels)[order], labels), "the reference emits class by class"
    return boxes[order], scores[order], labels[order]


def same_label_ious(segments):
    """the IoUs (float64) of every pair of one image's candidates that share a label"""
    boxes = np.concatenate([s["boxes"] for s in segments]).reshape(-1, 4)
    labels = np.concatenate([s["labels"] for s in segments])
    if len(boxes) < 2:
        return np.zeros(0)
    iou = F.iou64(boxes)
    same = np.triu(labels[:, None] == labels[None, :], 1)
    return iou[same]


# ------------------------------------------------------------------------------------------------------------ golden inputs
def golden_inputs(seed):
    """The golden's head outputs as integer codes (logit = code / 1024, delta = code / 16): every logit whose sigmoid passes TH is a different
    member of rpn_fpn_ref.LOGIT_GRID across the whole batch, the others are drawn (with repeats) from the grid below it.
    -> (cls_code: list of L int16 [N, nloc, A*C], reg_code: list of L int8 [N, nloc, 4A])"""
    rng = np.random.default_rng(seed)
    N = len(IMAGE_SIZES)
    grid = np.round(F.LOGIT_GRID.astype(np.float64) * 1024).astype(np.int64)
    passing = grid[F.torch_sigmoid(F.LOGIT_GRID.reshape(1, -1))[0] > np.float32(TH) + np.float32(1e-3)]
    below = grid[F.torch_sigmoid(F.LOGIT_GRID.reshape(1, -1))[0] < np.float32(TH) - np.float32(1e-3)]
    pool = rng.permutation(passing)
    want = ((150, 60), (90, 80), (70, 60), (30, 25), (10, 0))      # candidates per (level, image): one over PRE, one segment empty
    used = 0
    cls_code, reg_code = [], []
    for l, (H, W) in enumerate(MAPS):
        nloc = H * W
        cc = rng.choice(below, size=(N, nloc, A * C)).astype(np.int16)
        for i in range(N):
            n = want[l][i]
            classes = C if i == 0 else C - 1                         # image 1: the last class has no candidate
            cells = rng.choice(nloc * A * classes, size=n, replace=False)
            loc_a, c = cells // classes, cells % classes
            if n >= 8:
                # the same anchor under two labels (both survive) and neighbouring scales of one ratio under one label (NMS takes one)
                loc_a[1], c[1] = loc_a[0], (c[0] + 1) % classes
                a0 = loc_a[2] % A
                loc_a[3], c[3] = loc_a[2] - a0 + (a0 // 3) * 3 + (a0 % 3 + 1 if a0 % 3 < 2 else 1), c[2]
                flat = loc_a * C + c
                _, first = np.unique(flat, return_index=True)
                loc_a, c = loc_a[np.sort(first)], c[np.sort(first)]
            n = len(loc_a)
            cc[i].reshape(-1)[loc_a * C + c] = pool[used:used + n].astype(np.int16)
            used += n
        cls_code.append(cc)
        reg_code.append(rng.integers(-16, 17, size=(N, nloc, 4 * A)).astype(np.int8))
    assert used <= len(pool)
    return cls_code, reg_code


def golden_arrays(cls_code, reg_code):
    return ([c.astype(np.float32) / np.float32(1024) for c in cls_code], [r.astype(np.float32) / np.float32(16) for r in reg_code])


def golden_conditions(cls, reg, anchors):
    """the properties the golden's seed loop redraws for; returns the list of those that FAIL (empty: the draw is good)"""
    bad = []
    res = {cap: detect_ref(cls, reg, anchors, A, C, IMAGE_SIZES, TH, PRE, NMS_TH, cap) for cap in CAPS}
    r30, r1000 = res[30], res[1000]
    allsc = np.concatenate([F.torch_sigmoid(np.ascontiguousarray(c[:, :, :A * C]).reshape(1, -1))[0] for c in cls])
    if np.any(np.abs(allsc.astype(np.float64) - TH) < 1e-6):
        bad.append("a sigmoid within 1e-6 of the threshold")
    if not r30[0]["segments"][0]["n_cand"] > PRE:
        bad.append("image 0 / level 0 has no more than PRE candidates")
    if not any(s["n_cand"] == 0 for d in r30 for s in d["segments"]):
        bad.append("no empty segment")
    lab1 = np.concatenate([s["labels"] for s in r30[1]["segments"]])
    if not any(np.sum(lab1 == j) == 0 for j in range(1, C + 1)):
        bad.append("every class has a candidate in image 1")
    for i, d in enumerate(r1000):
        segs = d["segments"]
        if np.any(np.abs(same_label_ious(segs) - NMS_TH) < 1e-5):
            bad.append("image %d: an equal-label pair within 1e-5 of NMS_TH" % i)
        n_cand = sum(len(s["flat"]) for s in segs)
        if not d["n_nms"] < n_cand:
            bad.append("image %d loses no box to NMS" % i)
        b, lab = d["boxes"], d["labels"]
        same_box = np.all(b[:, None, :] == b[None, :, :], 2) & (lab[:, None] != lab[None, :])
        if not same_box.any():
            bad.append("image %d keeps no same-box pair of different labels" % i)
        if not r30[i]["n_nms"] > 30 or not len(r30[i]["scores"]) < r30[i]["n_nms"]:
            bad.append("image %d: the 30-cap is not active" % i)
        if not d["n_nms"] <= 1000 or len(d["scores"]) != d["n_nms"]:
            bad.append("image %d: the 1000-cap is active" % i)
    return bad, res


# ------------------------------------------------------------------------------------------------------------ neck and head, float64
def p6p7_ref(w6, b6, w7, b7, x, grads=None):
    """LastLevelP6P7 on its input x (C5, or P5 with use_P5) in float64: OIHW weights -> (p6, p7) and, with grads = (g6 or None, g7 or None),
    also (dx, dw6, db6, dw7, db7) of sum(p6 * g6) + sum(p7 * g7) (zeros where a gradient is None)"""
    import torch
    import torch.nn.functional as Fn
    t = [torch.tensor(np.asarray(v, np.float64), requires_grad=grads is not None) for v in (w6, b6, w7, b7, x)]
    p6 = Fn.conv2d(t[4], t[0], t[1], stride=2, padding=1)
    p7 = Fn.conv2d(Fn.relu(p6), t[2], t[3], stride=2, padding=1)
    if grads is None:
        return p6.numpy(), p7.numpy()
    loss = sum((p * torch.tensor(np.asarray(g, np.float64))).sum() for p, g in zip((p6, p7), grads) if g is not None)
    loss.backward()
    gr = [v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape)) for v in (t[4], t[0], t[1], t[2], t[3])]
    return (p6.detach().numpy(), p7.detach().numpy()), tuple(gr)


def head_ref(sd, xs, num_convs):
    """RetinaNetHead.forward in float64: sd = {state-dict key: OIHW array}, xs = list of [N,C,H,W] -> (list of logits, list of deltas)"""
    import torch
    import torch.nn.functional as Fn
    g = {k: torch.tensor(np.asarray(v, np.float64)) for k, v in sd.items()}
    logits, deltas = [], []
    for x in xs:
        outs = []
        for tower, last in (("cls_tower", "cls_logits"), ("bbox_tower", "bbox_pred")):
            t = torch.tensor(np.asarray(x, np.float64))
            for n in range(num_convs):
                t = Fn.relu(Fn.conv2d(t, g["%s.%d.weight" % (tower, 2 * n)], g["%s.%d.bias" % (tower, 2 * n)], padding=1))
            outs.append(Fn.conv2d(t, g[last + ".weight"], g[last + ".bias"], padding=1).numpy())
        logits.append(outs[0])
        deltas.append(outs[1])
    return logits, deltas

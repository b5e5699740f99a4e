"""Restatement of the RPN proposal selection over a feature pyramid (maskrcnn_benchmark/modeling/rpn/inference.py:76-176) in plain numpy.

Nothing here imports the library.  Decode comes from the oracle's C restatement (oracle.ops.box_decode, what oracle.torch_ref.rpn_post_process
uses); `cross_check_level` runs that function itself on one level as a second opinion.  What this file fixes where the reference leaves it open:

  * ranking: tests/ranking_ref.topk_ref's order (descending float32 sigmoid, equal scores by ascending anchor index);
  * NMS: greedy, suppress at IoU >= thr, IoU in float64.  A float32 IoU can land on the other side of the threshold, so `near_threshold`
    lets the set builders REDRAW any case where a kept box and one behind it lie within 1e-5 of it (or a box side within 1e-3 of MIN_SIZE)
    at build time; every case
    that is then compared is compared, none is skipped;
  * the cross-level cut (torch.topk leaves tie groups undefined): the library's documented rule, equal scores by ascending candidate
    position (level * post + rank within the level), image-major in the per-batch mode.

Per-batch mode (training with FPN_POST_NMS_PER_BATCH) emits each image's chosen candidates in candidate order, the per-image mode by
descending score."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import ranking_ref as R  # noqa: E402
from oracle import ops as O  # noqa: E402

# the golden's geometry (tests/golden/make_golden_rpn_fpn.py)
STRIDES = (4, 8, 16, 32, 64)
SIZES = (32, 64, 128, 256, 512)
RATIOS = (0.5, 1.0, 2.0)
IMAGE_SIZES = ((128, 192), (112, 160))               # (h, w): the second image is smaller, so clipping differs
MAPS = ((32, 48), (16, 24), (8, 12), (4, 6), (2, 3))
PRE, POST, FPN_POST, NMS_THRESH, MIN_SIZE = 200, 60, 100, 0.7, 16
# logits of the golden: multiples of 2^-10 in [-6, 6], each used at most once in the whole batch (test_rpn_fpn_ref checks the spacing)
LOGIT_GRID = (np.arange(-6 * 1024, 6 * 1024 + 1, dtype=np.int64) / 1024.0).astype(np.float32)


def pyramid_anchors(maps=MAPS, strides=STRIDES, sizes=SIZES, ratios=RATIOS, image_hw=IMAGE_SIZES[0]):
    """per level ([H*W*A,4] anchors, [H*W*A] uint8 visibility for image_hw) from the oracle's C restatement"""
    out = []
    for (H, W), st, s in zip(maps, strides, sizes):
        cell = O.cell_anchors(stride=st, sizes=s if isinstance(s, (tuple, list)) else (s,), ratios=ratios)
        out.append(O.grid_anchors(cell, H, W, st, image_hw))
    return out


def iou64(b):
    """pairwise IoU of xyxy boxes [n,4] in float64 (boxlist_ops.py:51-87, TO_REMOVE = 1)"""
    b = np.asarray(b, np.float64)
    area = (b[:, 2] - b[:, 0] + 1) * (b[:, 3] - b[:, 1] + 1)
    lt = np.maximum(b[:, None, :2], b[None, :, :2])
    rb = np.minimum(b[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt + 1, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    with np.errstate(invalid="ignore", divide="ignore"):
        return inter / (area[:, None] + area[None, :] - inter)


def nms64(boxes, thr, max_keep):
    """greedy NMS over boxes already in descending score order: positions kept, at most max_keep (nms_cpu.cpp: suppress at IoU >= thr)"""
    iou = iou64(boxes)
    alive = np.ones(len(boxes), bool)
    keep = []
    for i in range(len(boxes)):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) == max_keep:
            break
        alive[i + 1:] &= ~(iou[i, i + 1:] >= thr)
    return np.array(keep, np.int64)


def decode_clip(reg_rows, anchor_rows, image_hw):
    props = O.box_decode(np.ascontiguousarray(reg_rows, np.float32), np.ascontiguousarray(anchor_rows, np.float32), (1.0, 1.0, 1.0, 1.0))
    h, w = image_hw
    props[:, 0::2] = np.clip(props[:, 0::2], 0, w - 1)
    props[:, 1::2] = np.clip(props[:, 1::2], 0, h - 1)
    return props


def torch_sigmoid(flat):
    """the reference's own float32 sigmoid (torch on the CPU, on the [N, n] matrix inference.py:87-88 applies it to): what its stored scores
    are, to the bit; ranking_ref.sigmoid32 is the correctly rounded value and may differ from it in the last place"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(flat, np.float32)).sigmoid().numpy()


def level_ref(y, A, anchors, image_sizes, pre, post, thr, min_size, score_fn=None):
    """One level: y [N,nloc,ld] fused head output (columns 0..A-1 logits, A+4a.. deltas).  Per image a dict: idx (ranked anchor ids), ranked
    (decoded boxes of all of them), alive (positions in `ranked` that pass remove_small_boxes), boxes / scores (those, in rank order) and
    keep (positions in `boxes` after NMS, at most post).  The order is always topk_ref's; score_fn replaces the REPORTED scores."""
    y = np.asarray(y, np.float32)
    N, nloc, _ = y.shape
    k = min(pre, nloc * A)
    idx, top = R.topk_ref(y, A, k)
    if score_fn is not None:
        top = np.take_along_axis(score_fn(y[:, :, :A].reshape(N, -1)), idx, 1)
    out = []
    for i in range(N):
        reg = y[i, :, A:5 * A].reshape(nloc * A, 4)
        ranked = decode_clip(reg[idx[i]], anchors[idx[i]], image_sizes[i])
        ws, hs = ranked[:, 2] - ranked[:, 0] + 1, ranked[:, 3] - ranked[:, 1] + 1
        alive = np.nonzero((ws >= min_size) & (hs >= min_size))[0] if min_size > 0 else np.arange(k)
        boxes, scores = ranked[alive], top[i][alive]
        out.append(dict(idx=idx[i], ranked=ranked, alive=alive, boxes=boxes, scores=scores, keep=nms64(boxes, thr, post)))
    return out


def near_threshold(levels, thr, min_size):
    """True when some decision of `levels` (list over levels of level_ref's output) hangs on less than a float32 evaluation can promise"""
    for lev in levels:
        for d in lev:
            if len(d["boxes"]) > 1:                     # the sweep's decisions: a KEPT box against every box ranked behind it
                iou = iou64(d["boxes"])[d["keep"]]
                behind = np.arange(iou.shape[1])[None, :] > d["keep"][:, None]
                if np.any(behind & (np.abs(iou - thr) < 1e-5)):
                    return True
            if min_size > 0:
                r = d["ranked"]
                sides = np.concatenate([r[:, 2] - r[:, 0] + 1, r[:, 3] - r[:, 1] + 1])
                if np.any(np.abs(sides - min_size) < 1e-3):
                    return True
    return False


def order_key(scores):
    """uint32 key that orders like the float (ranking_ref.sort_desc_ref's)"""
    b = np.ascontiguousarray(scores, np.float32).view(np.uint32).astype(np.int64)
    return np.where(b >> 31, 0xFFFFFFFF - b, b + 0x80000000)


def select_ref(cand_scores, cand_pos, per_img, fpn_post, per_batch):
    """cand_scores / cand_pos: per image the candidates' scores and positions (level * post + rank), in candidate order; per_img = L * post.
    -> per image the positions chosen, in emission order."""
    N = len(cand_scores)
    if per_batch:
        key = np.concatenate([order_key(s) for s in cand_scores]) if N else np.zeros(0, np.int64)
        gpos = np.concatenate([i * per_img + np.asarray(p, np.int64) for i, p in enumerate(cand_pos)]) if N else np.zeros(0, np.int64)
        chosen = np.sort(gpos[np.lexsort((gpos, -key))[:min(fpn_post, len(key))]])
        return [chosen[(chosen >= i * per_img) & (chosen < (i + 1) * per_img)] - i * per_img for i in range(N)]
    out = []
    for s, p in zip(cand_scores, cand_pos):
        p = np.asarray(p, np.int64)
        out.append(p[np.lexsort((p, -order_key(s)))[:min(fpn_post, len(p))]])
    return out


def pyramid_ref(ys, As, anchors, image_sizes, pre, post, fpn_post, thr, min_size=0, per_batch=False, gt_boxes=None, levels=None):
    """ys: list of L fused head outputs [N,nloc_l,ld_l]; anchors: list of L [nloc_l*A_l,4].  -> per image (boxes, scores, src) with
    src = level * post + rank of every emitted proposal (-1 for appended ground truth).  One level: no cross-level cut (inference.py:139-140)."""
    L, N = len(ys), len(image_sizes)
    if levels is None:
        levels = [level_ref(ys[l], As[l], anchors[l], image_sizes, pre, post, thr, min_size) for l in range(L)]
    cs, cp, cb = [], [], []
    for i in range(N):
        s, p, b = [], [], []
        for l in range(L):
            d = levels[l][i]
            s.append(d["scores"][d["keep"]])
            b.append(d["boxes"][d["keep"]])
            p.append(l * post + np.arange(len(d["keep"])))
        cs.append(np.concatenate(s)); cp.append(np.concatenate(p)); cb.append(np.concatenate(b, 0).reshape(-1, 4))
    chosen = select_ref(cs, cp, L * post, fpn_post, per_batch) if L > 1 else cp
    out = []
    for i in range(N):
        at = np.searchsorted(cp[i], chosen[i])            # candidate positions ascend within an image
        boxes, scores, src = cb[i][at], cs[i][at], chosen[i].astype(np.int64)
        if gt_boxes is not None:
            g = np.asarray(gt_boxes[i], np.float32).reshape(-1, 4)
            boxes = np.concatenate([boxes, g], 0)
            scores = np.concatenate([scores, np.ones(len(g), np.float32)])
            src = np.concatenate([src, np.full(len(g), -1, np.int64)])
        out.append((boxes, scores, src))
    return out


def cross_check_level(y, A, H, W, anchors, image_sizes, pre, post, thr, min_size):
    """oracle.torch_ref.rpn_post_process on one level (torch.topk's order: use on inputs without tied scores) -> per image (boxes, scores)"""
    import torch
    from oracle import torch_ref as T
    y = np.asarray(y, np.float32)
    N = y.shape[0]
    nchw = torch.from_numpy(np.ascontiguousarray(y.reshape(N, H, W, -1).transpose(0, 3, 1, 2)))
    return T.rpn_post_process(nchw[:, :A], nchw[:, A:5 * A], [anchors] * N, image_sizes, pre, post, thr, min_size)


# --------------------------------------------------------------------------------------------------------------- input builders
def fused_from(obj, reg, ld=None, rng=None):
    """obj [N,nloc,A] logits, reg [N,nloc,A,4] deltas -> fused [N,nloc,ld] (ld >= 5A; further columns are decoys when rng is given)"""
    N, nloc, A = obj.shape
    ld = 5 * A if ld is None else ld
    y = np.zeros((N, nloc, ld), np.float32)
    if rng is not None and ld > 5 * A:
        y[:, :, 5 * A:] = np.where(rng.random((N, nloc, ld - 5 * A)) < 0.5, np.float32(9.0), np.float32(np.nan))
    y[:, :, :A] = obj
    y[:, :, A:5 * A] = reg.reshape(N, nloc, 4 * A)
    return y


def golden_inputs(seed):
    """the golden's head outputs: every logit a different member of LOGIT_GRID across the whole batch, deltas multiples of 1/16 in [-1, 1]
    -> (obj_code int16 list, reg_code int8 list): logit = code / 1024, delta = code / 16"""
    rng = np.random.default_rng(seed)
    N, A = len(IMAGE_SIZES), len(RATIOS)
    total = sum(N * H * W * A for H, W in MAPS)
    codes = rng.permutation(len(LOGIT_GRID))[:total].astype(np.int64) - 6 * 1024
    obj, reg, at = [], [], 0
    for H, W in MAPS:
        n = N * H * W * A
        obj.append(codes[at:at + n].reshape(N, H * W, A).astype(np.int16))
        reg.append(rng.integers(-16, 17, size=(N, H * W, A, 4)).astype(np.int8))
        at += n
    return obj, reg


def golden_fused(obj_code, reg_code):
    return [fused_from(o.astype(np.float32) / np.float32(1024), r.astype(np.float32) / np.float32(16)) for o, r in zip(obj_code, reg_code)]


def tie_heavy_inputs(seed, maps, A, image_sizes, pre, post, thr, min_size, value_set="halves", ld=16):
    """head outputs whose logits come from a small value set (long tie groups inside and across levels), redrawn until no NMS or MIN_SIZE
    decision is near its threshold -> (ys, anchors, levels)"""
    strides = STRIDES[:len(maps)]
    anchors = [a for a, _ in pyramid_anchors(maps, strides, SIZES[:len(maps)], RATIOS[:A], image_sizes[0])]
    for attempt in range(64):
        rng = np.random.default_rng(seed + 1000 * attempt)
        N = len(image_sizes)
        ys = [fused_from(R.draw(rng, value_set, (N, H * W, A)), (rng.integers(-8, 9, size=(N, H * W, A, 4)) / 8.0).astype(np.float32), ld, rng)
              for H, W in maps]
        levels = [level_ref(ys[l], A, anchors[l], image_sizes, pre, post, thr, min_size) for l in range(len(maps))]
        if not near_threshold(levels, thr, min_size):
            return ys, anchors, levels
    raise RuntimeError("no draw without a near-threshold decision in 64 attempts")

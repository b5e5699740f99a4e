"""RetinaNet's loss restated in float64 without the library (numpy): IoU with the +1 convention, the Matcher with low-quality matches (the
first maximum wins), the labels and the box encoding, the mathematical sigmoid focal loss and smooth-L1 with their normalisers, and closed-form
gradients.  tests/test_retinanet_loss_ref.py checks the restatement against the reference's own RetinaNetLossComputation
(tests/golden/retinanet_loss.npz); the GPU tests check the library against it.

Layout, as the library's: level l's class output is [N, nloc_l, ldc] with column a * C + c the logit of anchor loc * A + a and class c + 1, its
box output [N, nloc_l, ldr] with columns 4a .. 4a+3; an image's anchors are the levels' concatenated (n = A * sum nloc_l), labels [N, n]
(class / 0 background / -1 ignored), targets [N, n, 4].

IoU, Matcher and the encoding are rpn_fpn_loss_ref's (iou64, match, encode64): the same rpn/loss.py code serves both losses in the reference."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import retinanet_ref as R  # noqa: E402
import rpn_fpn_loss_ref as FL  # noqa: E402

EPS, TOL = FL.EPS, FL.TOL
HI, LO = 0.5, 0.4                   # MODEL.RETINANET.FG_IOU_THRESHOLD / BG_IOU_THRESHOLD
GAMMA, ALPHA = 2.0, 0.25            # LOSS_GAMMA / LOSS_ALPHA
BETA, NORM = 0.11, 4.0              # BBOX_REG_BETA / BBOX_REG_WEIGHT
WEIGHTS = R.WEIGHTS


# ------------------------------------------------------------------------------------------------------------------ targets
def image_targets(anchors, gt, gt_labels, hi=HI, lo=LO, weights=WEIGHTS):
    """one image over the concatenated anchors [n,4] -> dict(labels int64 [n], targets float64 [n,4], target_bound, matches, best, iou, lq: the
    anchors that are positive only through a low-quality match).  No ground truth: every anchor background, zero targets."""
    anchors = np.asarray(anchors, np.float32)
    n = anchors.shape[0]
    gt = np.asarray(gt, np.float32).reshape(-1, 4)
    if gt.shape[0] == 0:
        z = np.zeros((n, 4))
        return dict(labels=np.zeros(n, np.int64), targets=z, target_bound=z, matches=np.full(n, -1, np.int64), best=np.zeros(n),
                    iou=np.zeros((0, n)), lq=np.zeros(n, bool))
    iou = FL.iou64(gt, anchors)
    matches, best = FL.match(iou, hi, lo, True)
    lab = np.asarray(gt_labels, np.int64)[np.clip(matches, 0, None)]       # generate_retinanet_labels over matched_idxs.clamp(min=0)
    lab[matches == -1] = 0
    lab[matches == -2] = -1                                                # discard_cases = ['between_thresholds'] only
    tgt, bound = FL.encode64(gt[np.clip(matches, 0, None)], anchors, weights)
    return dict(labels=lab, targets=tgt, target_bound=bound, matches=matches, best=best, iou=iou, lq=(matches >= 0) & (best < hi))


def batch_targets(anchors, gt_boxes, gt_labels, hi=HI, lo=LO, weights=WEIGHTS):
    per = [image_targets(anchors, b, l, hi, lo, weights) for b, l in zip(gt_boxes, gt_labels)]
    return dict(labels=np.stack([p["labels"] for p in per]), targets=np.stack([p["targets"] for p in per]),
                target_bound=np.stack([p["target_bound"] for p in per]), per_image=per,
                n_pos=int(sum((p["labels"] > 0).sum() for p in per)))


def threshold_margin(per_image, hi=HI, lo=LO):
    """the smallest distance of any anchor's best IoU from a threshold (a redraw keeps it above 1e-5)"""
    best = np.concatenate([p["best"] for p in per_image if p["iou"].shape[0]] or [np.ones(1)])
    return float(min(np.abs(best - hi).min(), np.abs(best - lo).min()))


# ------------------------------------------------------------------------------------------------------------------ losses
def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def focal(x, positive, gamma=GAMMA, alpha=ALPHA):
    """sigmoid focal loss of logits x (float64) -> (value, derivative): positive entries -alpha (1-p)^gamma log p, the others
    -(1-alpha) p^gamma log(1-p), with log p = -softplus(-x), log(1-p) = -softplus(x)"""
    x = np.asarray(x, np.float64)
    p = FL.sigmoid(x)
    q = FL.sigmoid(-x)                                    # 1 - p without cancellation
    logp, logq = -softplus(-x), -softplus(x)
    vp, gp = -alpha * q ** gamma * logp, -alpha * q ** gamma * (q - gamma * p * logp)
    vn, gn = -(1 - alpha) * p ** gamma * logq, -(1 - alpha) * p ** gamma * (gamma * q * logq - p)
    return np.where(positive, vp, vn), np.where(positive, gp, gn)


def anchor_view(t, A, width):
    """[N, nloc, ld] -> [N, nloc * A, width]: the first A * width columns, anchor-major"""
    N, nloc = t.shape[:2]
    return np.asarray(t[:, :, :A * width], np.float64).reshape(N, nloc * A, width)


def losses(cls, reg, A, C, labels, targets, gamma=GAMMA, alpha=ALPHA, beta=BETA, norm=NORM, g_cls=1.0, g_reg=1.0):
    """cls / reg: lists of L arrays [N, nloc_l, ld] (fp32 values; pad columns are never looked at); labels [N,n], targets [N,n,4]
    -> dict(cls, reg: the two losses; cls_addends, reg_addends: sum of |addends| / denominator, what their bound scales with (check_losses);
    d_cls, d_reg: lists of L float64 arrays shaped like the inputs = d(g_cls * cls + g_reg * reg), zero in pad columns; n_pos; cls_den, reg_den)"""
    N = cls[0].shape[0]
    x = np.concatenate([anchor_view(c, A, C) for c in cls], 1)             # [N, n, C]
    d = np.concatenate([anchor_view(r, A, 4) for r in reg], 1)             # [N, n, 4]
    lab, tgt = np.asarray(labels, np.int64), np.asarray(targets, np.float64)
    assert lab.shape == x.shape[:2] and tgt.shape == d.shape
    n_pos = int((lab > 0).sum())
    cls_den, reg_den = float(n_pos + N), float(max(1.0, n_pos * norm))
    positive = lab[:, :, None] == np.arange(1, C + 1)[None, None, :]
    live = (lab >= 0)[:, :, None]
    v, gv = focal(x, positive, gamma, alpha)
    v, gv = np.where(live, v, 0.0), np.where(live, gv, 0.0)
    pos = (lab > 0)[:, :, None]
    diff = np.where(pos, d - tgt, 0.0)
    sv, sg = FL.sl1(diff, beta)
    sv, sg = np.where(pos, sv, 0.0), np.where(pos, sg, 0.0)
    out = dict(cls=float(v.sum()) / cls_den, reg=float(sv.sum()) / reg_den, n_pos=n_pos, cls_den=cls_den, reg_den=reg_den,
               cls_addends=float(np.where(live, v + np.abs(np.where(live, x, 0.0)) + 1, 0.0).sum()) / cls_den,
               reg_addends=float(np.where(pos, sv + np.minimum(np.abs(diff), beta) / beta * (np.abs(d) + np.abs(tgt)), 0.0).sum()) / reg_den,
               cls_scale=abs(g_cls) / cls_den, reg_scale=abs(g_reg) / reg_den)
    gx, gd = gv * (g_cls / cls_den), sg * (g_reg / reg_den)
    d_cls, d_reg, o = [], [], 0
    for c, r in zip(cls, reg):
        nloc = c.shape[1]
        dc, dr = np.zeros(c.shape), np.zeros(r.shape)
        dc[:, :, :A * C] = gx[:, o:o + nloc * A].reshape(N, nloc, A * C)
        dr[:, :, :A * 4] = gd[:, o:o + nloc * A].reshape(N, nloc, A * 4)
        d_cls.append(dc)
        d_reg.append(dr)
        o += nloc * A
    out["d_cls"], out["d_reg"] = d_cls, d_reg
    return out


def check_losses(got_cls, got_reg, ref, what=""):
    """rpn_fpn_loss_ref.check_losses' rule: a loss is within TOL * (sum of |addends| / denominator) of float64"""
    assert np.isfinite(got_cls) and np.isfinite(got_reg), f"{what}: non-finite loss {got_cls} {got_reg}"
    print(f"{what}: cls {got_cls!r} vs {ref['cls']!r} (bound {TOL * ref['cls_addends']:.3e}), reg {got_reg!r} vs {ref['reg']!r} "
          f"(bound {TOL * ref['reg_addends']:.3e})")
    assert abs(got_cls - ref["cls"]) <= TOL * ref["cls_addends"], \
        f"{what}: focal loss {got_cls!r} vs float64 {ref['cls']!r}: |d| = {abs(got_cls - ref['cls']):.3e} > {TOL * ref['cls_addends']:.3e}"
    assert abs(got_reg - ref["reg"]) <= TOL * ref["reg_addends"], \
        f"{what}: box loss {got_reg!r} vs float64 {ref['reg']!r}: |d| = {abs(got_reg - ref['reg']):.3e} > {TOL * ref['reg_addends']:.3e}"


def check_d_reg(got, ref, what=""):
    """rpn_fpn_loss_ref.check_grads' smooth-L1 bound (4 EPS * scale * 10), and exactly zero wherever float64 is zero (off the positives, pads)"""
    for l, (g, r) in enumerate(zip(got, ref["d_reg"])):
        g = np.asarray(g, np.float64).reshape(r.shape)
        assert np.isfinite(g).all(), f"{what}: level {l}: non-finite gradient"
        assert np.all(g[r == 0] == 0), f"{what}: level {l}: {int((g[r == 0] != 0).sum())} elements off the positives are not exactly 0"
        err = np.abs(g - r)
        assert np.all(err <= 4 * EPS * ref["reg_scale"] * 10), f"{what}: level {l}: smooth-L1 gradient off by {err.max():.3e}"


# ------------------------------------------------------------------------------------------------------------------ golden inputs
GOLDEN_G = (6, 4)                   # ground truths per image


def golden_inputs(seed):
    """The golden's inputs at retinanet_ref's tiny pyramid (MAPS, A = 9, C = 4, two images): per image integer-grid ground-truth boxes with
    labels 1 .. C -- sizes spread over the levels' anchor scales, one of them a 5 : 1 sliver no anchor overlaps by half (a positive through a
    low-quality match only) -- and head outputs as integer codes (logit = code / 256, delta = code / 16).
    -> (gt_boxes: list of fp32 [G_i,4], gt_labels: list of int64 [G_i], cls_code: list of L int16 [N, nloc, A*C], reg_code: list of L int8)"""
    rng = np.random.default_rng(seed)
    gt_boxes, gt_labels = [], []
    for i, (h, w) in enumerate(R.IMAGE_SIZES):
        boxes = []
        for k in range(GOLDEN_G[i]):
            side = float(rng.choice([14, 22, 36, 60, 90, 110]))
            bw, bh = (side * 2.2, side / 2.2) if k == 0 else (side * rng.uniform(0.7, 1.4), side * rng.uniform(0.7, 1.4))
            bw, bh = min(int(round(bw)), w - 2), min(int(round(bh)), h - 2)
            x1, y1 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
            boxes.append([x1, y1, x1 + bw, y1 + bh])
        gt_boxes.append(np.asarray(boxes, np.float32))
        gt_labels.append(rng.integers(1, R.C + 1, size=GOLDEN_G[i]).astype(np.int64))
    cls_code = [rng.integers(-6 * 256, 3 * 256, size=(len(R.IMAGE_SIZES), H * W, R.A * R.C)).astype(np.int16) for H, W in R.MAPS]
    reg_code = [rng.integers(-24, 25, size=(len(R.IMAGE_SIZES), H * W, 4 * R.A)).astype(np.int8) for H, W in R.MAPS]
    return gt_boxes, gt_labels, cls_code, reg_code


def golden_arrays(cls_code, reg_code):
    return ([c.astype(np.float32) / np.float32(256) for c in cls_code], [r.astype(np.float32) / np.float32(16) for r in reg_code])


def golden_conditions(anchors_per_level, gt_boxes, gt_labels):
    """what the golden's seed loop redraws for; returns (the list of conditions that FAIL, the batch's targets)"""
    anchors = np.concatenate(anchors_per_level)
    tg = batch_targets(anchors, gt_boxes, gt_labels)
    offs = np.concatenate([[0], np.cumsum([len(a) for a in anchors_per_level])])
    bad = []
    lab = tg["labels"]
    levels = {int(np.searchsorted(offs, j, side="right") - 1) for j in np.nonzero((lab > 0).any(0))[0]}
    if len(levels) < 3:
        bad.append("positives on %d levels only" % len(levels))
    if not any(p["lq"].any() for p in tg["per_image"]):
        bad.append("no positive through a low-quality match only")
    if not (lab < 0).any():
        bad.append("no ignored anchor")
    if threshold_margin(tg["per_image"]) < 1e-5:
        bad.append("an IoU within 1e-5 of a threshold")
    return bad, tg


def golden_sample(n_entries, count, seed):
    """the fixed sample of flat entries of one level's output whose gradient the golden stores"""
    return np.sort(np.random.default_rng(seed).choice(n_entries, size=min(count, n_entries), replace=False))


# ------------------------------------------------------------------------------------------------------------------ the head, float64
def head_ref_grads(sd, xs, num_convs, g_cls, g_reg):
    """retinanet_ref.head_ref extended with float64 gradients: sd = {state-dict key: OIHW array}, xs = list of [N,C,H,W], g_cls / g_reg = lists
    of output gradients shaped like the logits / deltas (NCHW) -> (logits, deltas, {key: d sum_l (<logits_l, g_cls_l> + <deltas_l, g_reg_l>) /
    d parameter}, list of input gradients): the parameters are shared by the levels, so their gradients add"""
    import torch
    import torch.nn.functional as Fn
    p = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in sd.items()}
    ts = [torch.tensor(np.asarray(x, np.float64), requires_grad=True) for x in xs]
    logits, deltas, total = [], [], 0.0
    for l, x in enumerate(ts):
        outs = []
        for tower, last in (("cls_tower", "cls_logits"), ("bbox_tower", "bbox_pred")):
            t = x
            for n in range(num_convs):
                t = Fn.relu(Fn.conv2d(t, p["%s.%d.weight" % (tower, 2 * n)], p["%s.%d.bias" % (tower, 2 * n)], padding=1))
            outs.append(Fn.conv2d(t, p[last + ".weight"], p[last + ".bias"], padding=1))
        total = total + (outs[0] * torch.tensor(np.asarray(g_cls[l], np.float64))).sum() + (outs[1] * torch.tensor(np.asarray(g_reg[l], np.float64))).sum()
        logits.append(outs[0].detach().numpy())
        deltas.append(outs[1].detach().numpy())
    total.backward()
    return logits, deltas, {k: v.grad.numpy() for k, v in p.items()}, [t.grad.numpy() for t in ts]

"""Reference-side restatements for the mask head tests (numpy / torch on the CPU; no product kernels): the mask branch for autograd, the
float64 paste the paste tests excuse near-threshold pixels with, the oracle model with a mask branch, and plain restatements of the
kernels of csrc/mask.hip (compaction, row gather, depth-to-space + bias + ReLU and its backward, mask targets, select + sigmoid) with the
paste cases that tests/test_mask_ref.py (CPU) and tests/test_gpu_mask_kernels.py (GPU) share."""
import functools

import numpy as np
import torch
import torch.nn.functional as F


def mask_branch(x, w5, b5, wl, bl):
    """MaskRCNNC4Predictor (roi_mask_predictors.py:10-32): x [P,C,h,w], w5 [C,Cm,2,2], wl [K,Cm,1,1] -> logits [P,K,2h,2w]"""
    return F.conv2d(F.relu(F.conv_transpose2d(x, w5, b5, stride=2)), wl, bl)


def mask_loss(logits, labels_pos, targets):
    """mask_head/loss.py:117-128 on the positives' logits [P,K,M,M]"""
    if targets.numel() == 0:
        return logits.sum() * 0
    return F.binary_cross_entropy_with_logits(logits[torch.arange(logits.shape[0]), labels_pos], targets)


def paste_f64(prob, box, im_h, im_w, padding=1):
    """paste_mask_in_image (inference.py:119-159) with the integer box arithmetic in float32 / int32 as there and the INTERPOLATION in float64:
    -> (values float64 [im_h, im_w], written bool [im_h, im_w]); the pasted mask is values > threshold where written, 0 elsewhere"""
    M = prob.shape[-1]
    scale = float(M + 2 * padding) / M
    padded = torch.zeros((M + 2 * padding, M + 2 * padding), dtype=torch.float32)
    padded[padding:-padding, padding:-padding] = prob.float()
    b = box.float()
    w_half, h_half = (b[2] - b[0]) * .5, (b[3] - b[1]) * .5
    x_c, y_c = (b[2] + b[0]) * .5, (b[3] + b[1]) * .5
    w_half = w_half * scale
    h_half = h_half * scale
    bi = torch.stack([x_c - w_half, y_c - h_half, x_c + w_half, y_c + h_half]).to(torch.int32)
    w = max(int(bi[2] - bi[0] + 1), 1)
    h = max(int(bi[3] - bi[1] + 1), 1)
    vals = torch.zeros((im_h, im_w), dtype=torch.float64)
    written = torch.zeros((im_h, im_w), dtype=torch.bool)
    bx0, by0, bx2, by3 = (int(v) for v in bi)
    x_0, x_1, y_0, y_1 = max(bx0, 0), min(bx2 + 1, im_w), max(by0, 0), min(by3 + 1, im_h)
    if x_1 <= x_0 or y_1 <= y_0:
        return vals, written
    # float32 source coordinates as torch computes them -- ONE fused multiply-add, as csrc/mask_bilinear.h records: the float64 product of a
    # float32 and a small half-integer is exact, so rounding product - 0.5 once is that FMA (unfused, a coordinate that is 1.5e-8 there
    # becomes an exact 0 and a pixel that torch pastes at threshold 0 is lost) -- and float64 taps; only the rows and columns that land
    # on the canvas are interpolated (every output pixel is a function of its own taps alone, and a box can be thousands of pixels wide)
    def taps(out, inp, lo, hi):
        sc = torch.tensor(inp, dtype=torch.float32) / torch.tensor(out, dtype=torch.float32)
        s = (sc.double() * (torch.arange(lo, hi, dtype=torch.float64) + 0.5) - 0.5).float()
        s = s.clamp(min=0)
        i0 = s.floor().long().clamp(max=inp - 1)
        l1 = (s - i0.float()).clamp(0, 1)
        i1 = i0 + (i0 < inp - 1).long()
        return i0, i1, l1.double()
    y0, y1, ly = taps(h, M + 2 * padding, y_0 - by0, y_1 - by0)
    x0, x1, lx = taps(w, M + 2 * padding, x_0 - bx0, x_1 - bx0)
    p = padded.double()
    r0 = p[y0][:, x0] * (1 - lx) + p[y0][:, x1] * lx
    r1 = p[y1][:, x0] * (1 - lx) + p[y1][:, x1] * lx
    vals[y_0:y_1, x_0:x_1] = r0 * (1 - ly)[:, None] + r1 * ly[:, None]
    written[y_0:y_1, x_0:x_1] = True
    return vals, written


def ref_model_with_mask():
    """oracle.model_ref.RefModel + the mask branch on the box head's layer4 output"""
    from oracle.model_ref import RefModel, _RoiAlignRef

    class MaskRefModel(RefModel):
        def head_features(self, feat, rois, sr=0, res=7, scale=0.0625):
            x = _RoiAlignRef.apply(feat, rois, scale, res, res, sr)
            pooled = x
            for i in range(3):
                x = self._block(x, f"roi_heads.box.feature_extractor.head.layer4.{i}", 2 if i == 0 else 1)
            return pooled, x

        def box_predictor(self, x):
            v = F.adaptive_avg_pool2d(x, 1).flatten(1)
            pr = "roi_heads.box.predictor"
            return (F.linear(v, self.p[f"{pr}.cls_score.weight"], self.p[f"{pr}.cls_score.bias"]),
                    F.linear(v, self.p[f"{pr}.bbox_pred.weight"], self.p[f"{pr}.bbox_pred.bias"]))

        def mask_predictor(self, x):
            pr = "roi_heads.mask.predictor"
            return mask_branch(x, self.p[f"{pr}.conv5_mask.weight"], self.p[f"{pr}.conv5_mask.bias"], self.p[f"{pr}.mask_fcn_logits.weight"],
                               self.p[f"{pr}.mask_fcn_logits.bias"])

    return MaskRefModel


# ------------------------------------------------------------------------------------------------ the kernels of csrc/mask.hip, restated
def compact_ref(labels, p_max):
    """labels int64 [K] -> (pos_rows [p_max], pos_labels [p_max], inv [K], n_pos): rows with labels > 0 in ascending order cut at p_max, the
    tail -1; inv[rows[p]] = p, else -1"""
    labels = np.asarray(labels, dtype=np.int64)
    nz = np.nonzero(labels > 0)[0]
    rows = nz[:p_max]
    pos_rows = np.full((p_max,), -1, np.int64)
    pos_labels = np.full((p_max,), -1, np.int64)
    pos_rows[:len(rows)] = rows
    pos_labels[:len(rows)] = labels[rows]
    inv = np.full((len(labels),), -1, np.int64)
    inv[rows] = np.arange(len(rows))
    return pos_rows, pos_labels, inv, min(len(nz), p_max)


def gather_ref(x, rows):
    """x [n_src, ...] -> out[p] = x[rows[p]] where 0 <= rows[p] < n_src, else zeros"""
    out = np.zeros((len(rows),) + x.shape[1:], x.dtype)
    for p, r in enumerate(rows):
        if 0 <= int(r) < x.shape[0]:
            out[p] = x[int(r)]
    return out


def d2s_ref(y, bias):
    """y [P,h,w,4*Cm] float32, bias [Cm] -> out[n, 2y+dy, 2x+dx, c] = y[n, y, x, (dy*2+dx)*Cm + c] + bias[c] (one float32 addition), then
    where(v < 0, 0, v)"""
    P, h, w, c4 = y.shape
    Cm = c4 // 4
    out = torch.empty((P, 2 * h, 2 * w, Cm), dtype=torch.float32)
    for dy in range(2):
        for dx in range(2):
            q = dy * 2 + dx
            out[:, dy::2, dx::2, :] = y[..., q * Cm:(q + 1) * Cm] + bias
    return torch.where(out < 0, torch.zeros_like(out), out)


def d2s_backward_ref(g, out):
    """g, out [P,2h,2w,Cm] -> gy [P,h,w,4*Cm]: where(out > 0, g, 0) scattered back to the (dy, dx, c) columns"""
    P, h2, w2, Cm = out.shape
    gm = torch.where(out > 0, g, torch.zeros_like(g))
    gy = torch.empty((P, h2 // 2, w2 // 2, 4 * Cm), dtype=torch.float32)
    for dy in range(2):
        for dx in range(2):
            q = dy * 2 + dx
            gy[..., q * Cm:(q + 1) * Cm] = gm[:, dy::2, dx::2, :]
    return gy


def iou_f32(gt, b):
    """structures/boxlist_ops.py:53-88 (TO_REMOVE = 1) in float32: gt [G,4], b [4] -> [G]"""
    gt, b = gt.float(), b.float()
    area1 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    area2 = (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    lt = torch.max(gt[:, :2], b[:2])
    rb = torch.min(gt[:, 2:], b[2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    return inter / (area1 + area2 - inter)


def targets_ref(masks, gts, rois, pos_rows, M):
    """masks: per-image CPU tensors [n,H,W]; gts: per-image [n,4]; rois [K,5]; pos_rows [P] -> ([P,M,M] float32, matched instance per row or
    -1): per RoI the first maximum of the float32 IoU (np.argmax), then crop + resize through the CPU SegmentationMask API (pinned to the
    reference by tests/test_mask_config.py).  Rows outside [0, K), image indices outside [0, N) and images without instances give zeros."""
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    K, N = len(rois), len(masks)
    out = torch.zeros((len(pos_rows), M, M), dtype=torch.float32)
    matched = []
    for p, row in enumerate(int(r) for r in pos_rows):
        matched.append(-1)
        if not 0 <= row < K:
            continue
        img = int(rois[row, 0])
        if not 0 <= img < N or len(masks[img]) == 0:
            continue
        b = torch.as_tensor(rois[row, 1:5])
        bi = int(np.argmax(iou_f32(torch.as_tensor(gts[img]), b).numpy()))
        H, W = masks[img].shape[1:]
        out[p] = SegmentationMask(masks[img][bi], (W, H)).crop(b).resize((M, M)).get_mask_tensor().float()
        matched[-1] = bi
    return out, matched


def resize_four_weight(mask, M):
    """[h,w] 0/1 mask -> [M,M] float32 in the operation order of the four-weight form (csrc/mask_bilinear.h, bilinear_mix): the source index
    is one fused multiply-add, the four weights are products of float32 factors, the taps accumulate in a chain of fused multiply-adds.
    Exact for 0/1 taps: a float64 product of two float32 is exact, and so is the float64 sum of such a product with a float32 up to one
    final rounding (innocuous double rounding of a sum, 53 >= 2 * 24 + 2)."""
    f32 = np.float32

    def taps(inp, out):
        scale = f32(inp) / f32(out)
        s = np.maximum((np.float64(scale) * (np.arange(out, dtype=np.float64) + 0.5) - 0.5).astype(f32), f32(0))
        i0 = np.minimum(np.floor(s).astype(np.int64), inp - 1)
        return i0, i0 + (i0 < inp - 1), np.clip(s - i0.astype(f32), f32(0), f32(1)).astype(f32)

    m = np.asarray(mask).astype(f32)
    assert ((m == 0) | (m == 1)).all()
    y0, y1, ly = taps(m.shape[0], M)
    x0, x1, lx = taps(m.shape[1], M)
    ly, lx = ly[:, None], lx[None, :]
    wx0, wy0 = f32(1) - lx, f32(1) - ly

    def fma(a, b, c):
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)
    return fma(ly * lx, m[y1][:, x1], fma(ly * wx0, m[y1][:, x0], fma(wy0 * lx, m[y0][:, x1], (wy0 * wx0) * m[y0][:, x0])))


def select_sigmoid_ref(logits, num_classes, labels):
    """logits [D,M,M,ldk], labels [D] -> float64 [D,1,M,M]: sigmoid of channel labels[d]; zeros where the label is outside [0, num_classes)"""
    D, M1, M2, _ = logits.shape
    out = torch.zeros((D, 1, M1, M2), dtype=torch.float64)
    for d, l in enumerate(int(v) for v in labels):
        if 0 <= l < num_classes:
            out[d, 0] = torch.sigmoid(logits[d, :, :, l].double())
    return out


# ------------------------------------------------------------------------------------------------ paste cases
PASTE_THRESHOLDS = (0.0, 0.25, 0.5, 0.9)
PASTE_CANVASES = ((1, 1), (1, 97), (61, 1), (33, 64), (5, 3))
PASTE_PROBS = ("zeros", "ones", "corners", "random")
# how far the two boxes below stick out: chosen (like every number here) so that on the canvases of fewer than 1000 pixels no product of
# edge weights lands within 1e-6 of a threshold (a condition on the inputs that tests/test_mask_ref.py checks)
_OFF = (2.5, 1.5, 7.5, 4.5)
_CIN = (5, 2)      # centre of the box whose expanded corners are (-0.5, -0.6)


def paste_boxes(H, W, M):
    """name -> box for a canvas of H x W at resolution M.  The paste expands a box about its centre by (M + 2) / M before truncating, so the
    boxes that aim at a pixel boundary are stated through that scale."""
    s = float(M + 2) / M
    return [
        ("outside left", (-40.0, -1.0, -30.0, H)), ("outside right", (W + 30.0, -1.0, W + 40.0, H)),
        ("outside above", (-1.0, -40.0, W, -30.0)), ("outside below", (-1.0, H + 30.0, W, H + 40.0)),
        # expanded x range (-9.5, 0.5): only column 0;  expanded y range (H - 0.5, H + 9.5): only row H - 1
        ("one column at the left", (-4.5 - 5.0 / s, 0.3, -4.5 + 5.0 / s, H - 0.6)),
        ("one row at the bottom", (0.2, H + 4.5 - 5.0 / s, W - 0.7, H + 4.5 + 5.0 / s)),
        ("reversed", (0.6 * W + 3, 0.7 * H + 3, 0.2 * W, 0.1 * H)),
        ("zero size", (W // 2, H // 2, W // 2, H // 2)),
        ("sub-pixel", (W / 3 + 0.2, H / 3 + 0.3, W / 3 + 0.6, H / 3 + 0.9)),
        # expanded corners (-0.5, -0.6): truncation toward zero gives 0, a floor would give -1
        ("corners in (-1, 0)", (_CIN[0] - (_CIN[0] + 0.5) / s, _CIN[1] - (_CIN[1] + 0.6) / s, _CIN[0] + (_CIN[0] + 0.5) / s, _CIN[1] + (_CIN[1] + 0.6) / s)),
        ("huge", (-1000.0, -1000.0, 2000.0, 2000.0)),
        ("inside, not square", (0.1 * W + 0.3, 0.2 * H + 0.1, 0.8 * W + 1.4, 0.7 * H + 2.2)),
        ("over the top left", (-0.3 * W - _OFF[0], -0.2 * H - _OFF[1], 0.5 * W + 0.3, 0.6 * H + 1.4)),
        ("over the bottom right", (0.4 * W + 0.2, 0.5 * H + 0.1, 1.3 * W + _OFF[2], 1.2 * H + _OFF[3])),
    ]


def _paste_prob(kind, M, gen):
    if kind == "zeros":
        return torch.zeros(M, M)
    if kind == "ones":
        return torch.ones(M, M)
    if kind == "corners":    # a different value in each corner: an x / y swap or a flip moves them (M = 1: one pixel)
        p = torch.zeros(M, M)
        p[0, 0], p[0, M - 1], p[M - 1, 0], p[M - 1, M - 1] = 0.3, 0.6, 0.8, 0.95
        return p
    return torch.rand(M, M, generator=gen)


class PasteCase(object):
    def __init__(self, name, M, H, W, boxes, prob, kinds):
        self.name, self.M, self.H, self.W, self.kinds = name, M, H, W, kinds
        self.boxes = torch.tensor(boxes, dtype=torch.float32).view(-1, 4)
        self.prob = prob
        self.D = len(self.boxes)


@functools.lru_cache(maxsize=None)
def paste_cases():
    """every M x canvas with all 14 boxes x 4 probability patterns (D = 56, D H W % 4 == 0), and short lists of boxes that all reach the
    canvas with random probabilities, whose D H W % 4 is 1, 2 and 3: the last pack is a tail, and on the 5 x 3 canvas with D = 7 four-pixel
    packs straddle detections with different boxes"""
    cases = []
    for M in (1, 7, 14, 28):
        for H, W in PASTE_CANVASES:
            gen = torch.Generator().manual_seed(1000 * M + 10 * H + W)
            named = paste_boxes(H, W, M)
            boxes, probs, kinds = [], [], []
            for kind in PASTE_PROBS:
                for bname, b in named:
                    boxes.append(b)
                    probs.append(_paste_prob(kind, M, gen))
                    kinds.append(bname + " / " + kind)
            cases.append(PasteCase("M%d-%dx%d-D%d" % (M, H, W, len(boxes)), M, H, W, boxes, torch.stack(probs)[:, None], kinds))
    reach = ("inside, not square", "over the top left", "over the bottom right", "corners in (-1, 0)", "huge", "zero size", "sub-pixel")
    for (H, W), D in (((1, 1), 1), ((1, 1), 2), ((1, 1), 3), ((5, 3), 7), ((5, 3), 2), ((5, 3), 1), ((1, 97), 3), ((61, 1), 2)):
        M = 14
        gen = torch.Generator().manual_seed(7000 + 100 * H + 10 * W + D)
        named = dict(paste_boxes(H, W, M))
        cases.append(PasteCase("M%d-%dx%d-D%d-rem%d" % (M, H, W, D, D * H * W % 4), M, H, W, [named[k] for k in reach[:D]],
                               torch.rand(D, 1, M, M, generator=gen), [k + " / random" for k in reach[:D]]))
    return tuple(cases)


@functools.lru_cache(maxsize=None)
def paste_reference(name):
    """-> (values float64 [D,H,W], written bool [D,H,W]) of the named case, computed once"""
    c = next(c for c in paste_cases() if c.name == name)
    out = [paste_f64(c.prob[d, 0], c.boxes[d], c.H, c.W) for d in range(c.D)]
    return torch.stack([v for v, _ in out]), torch.stack([w for _, w in out])


def paste_expected(vals, written, thresh):
    """-> (want uint8, excused bool): the pasted mask is values > thresh where written; a pixel is excused where the float64 value lies
    within 1e-6 of the threshold (threshold 0: only 0 < v <= 1e-6 -- an exact zero is a zero in float32 too)"""
    want = (written & (vals > thresh)).to(torch.uint8)
    near = (vals - thresh).abs() <= 1e-6
    if thresh == 0:
        near = near & (vals > 0)
    return want, written & near

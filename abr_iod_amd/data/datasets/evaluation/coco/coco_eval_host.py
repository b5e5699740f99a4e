"""The COCO detection protocol on the host, in float64 numpy: what pycocotools' COCOeval computes -- bbIou / rleIou, evaluateImg,
accumulate, summarize, and for the "keypoints" iou type computeOks with the keypoint parameters -- restated from the protocol
(DESIGN.md §4).  pycocotools cannot be installed where this project is built, so compatibility rests on this restatement and its
answers worked out by hand (tests/test_coco_eval_host.py, tests/test_coco_keypoints_host.py), as it does for run-length masks and polygons.  Three users: the groups the match kernel leaves to the host (more ground truths than ops.COCO_MATCH_MAX_GT), the
accumulation behind both routes, and the tests of csrc/coco_eval.hip.

A GROUP is one (image, category) pair: its detections in rank order (score descending, stable, the first maxDets[-1]) and its ground
truths in file order.

One deliberate difference: a match is recorded by the ground truth's ROW in its group, -1 = none.  pycocotools stores annotation ids
and tests them with `> 0` / `== 0`, so an annotation (or detection) whose id is 0 reads as unmatched; that quirk is not reproduced.

The last section restates proposal recall (evaluate_box_proposals, the box_only metric of RPN proposals) in torch float32, the
arithmetic the reference runs it in: the yardstick of csrc/proposal_recall.hip and what device="cpu" scores with."""
import numpy as np

IOU_THRS = np.linspace(.5, 0.95, int(np.round((0.95 - .5) / .05)) + 1, endpoint=True)
REC_THRS = np.linspace(.0, 1.00, int(np.round((1.00 - .0) / .01)) + 1, endpoint=True)
MAX_DETS = (1, 10, 100)
AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
AREA_LABELS = ("all", "small", "medium", "large")
STAT_NAMES = ("AP", "AP50", "AP75", "APs", "APm", "APl", "AR1", "AR10", "AR100", "ARs", "ARm", "ARl")
# the keypoint protocol's own parameters (COCOeval's Params.setKpParams): one maxDets, no "small" range, a sigma per person keypoint
KP_MAX_DETS = (20,)
KP_AREA_RNG = np.array([[0 ** 2, 1e5 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2]], np.float64)
KP_AREA_LABELS = ("all", "medium", "large")
KP_STAT_NAMES = ("AP", "AP50", "AP75", "APm", "APl", "AR", "AR50", "AR75", "ARm", "ARl")
KPT_OKS_SIGMAS = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def rank_detections(scores, max_det=MAX_DETS[-1]):
    """indices of the detections that count, in rank order: a stable sort by score descending (equal scores keep their order), cut at max_det"""
    return np.argsort(-np.asarray(scores, np.float64), kind="mergesort")[:max_det]


def box_iou(det, gt, gt_crowd):
    """bbIou: det [D,4], gt [G,4] xywh -> float64 [D,G].  area = w * h (no + 1); a pair whose intersection has no positive width or height
    gets 0; else i / (a_d + a_g - i), or i / a_d when the ground truth is a crowd"""
    det, gt = np.asarray(det, np.float64).reshape(-1, 4), np.asarray(gt, np.float64).reshape(-1, 4)
    crowd = np.asarray(gt_crowd).astype(bool).reshape(-1)
    dx, dy, dw, dh = (det[:, k, None] for k in range(4))
    gx, gy, gw, gh = (gt[None, :, k] for k in range(4))
    w = np.minimum(dw + dx, gw + gx) - np.maximum(dx, gx)
    h = np.minimum(dh + dy, gh + gy) - np.maximum(dy, gy)
    i = w * h
    da = np.broadcast_to(dw * dh, i.shape)
    u = np.where(crowd[None, :], da, da + gw * gh - i)
    out = np.zeros(i.shape, np.float64)
    np.divide(i, u, out=out, where=(w > 0) & (h > 0))
    return out


def mask_iou_from_counts(inter, area_p, area_t, gt_crowd):
    """rleIou from pixel counts: inter [P,T], area_p [P], area_t [T] integers -> float64 [P,T]; 0 where the masks do not meet"""
    inter = np.asarray(inter, np.int64)
    area_p, area_t = np.asarray(area_p, np.int64).reshape(-1), np.asarray(area_t, np.int64).reshape(-1)
    crowd = np.asarray(gt_crowd).astype(bool).reshape(-1)
    u = np.where(crowd[None, :], area_p[:, None], area_p[:, None] + area_t[None, :] - inter)
    out = np.zeros(inter.shape, np.float64)
    np.divide(inter.astype(np.float64), u.astype(np.float64), out=out, where=inter > 0)
    return out


def keypoint_det_area(det_kp):
    """loadRes' area of a keypoint result: det_kp [D,K,3] -> [D], (max x - min x) * (max y - min y) over all K points, whatever v is"""
    kp = np.asarray(det_kp, np.float64)
    if kp.size == 0:
        return np.zeros(len(kp), np.float64)
    kp = kp.reshape(len(kp), -1, 3)
    x, y = kp[:, :, 0], kp[:, :, 1]
    return (x.max(1) - x.min(1)) * (y.max(1) - y.min(1))


def oks(det_kp, gt_kp, gt_box, gt_area, sigmas=KPT_OKS_SIGMAS):
    """computeOks: det_kp [D,K,3], gt_kp [G,K,3] (x, y, v), gt_box [G,4] xywh, gt_area [G], sigmas [K] -> float64 [D,G].  With k1 = the
    ground truth's keypoints of v > 0: the mean of exp(-e_k) over them, e_k = (dx_k^2 + dy_k^2) / (2 sigma_k)^2 / (area + 2^-52) / 2; with
    k1 == 0 the mean over all K, dx and dy being the distances to the box doubled about itself.  Crowds get no special value.
    The sum runs serially in keypoint order (np.sum, which pycocotools uses, adds pairwise and can differ in the last bits)."""
    var = (np.asarray(sigmas, np.float64).reshape(-1) * 2) ** 2
    K = len(var)
    det_kp, gt_kp = np.asarray(det_kp, np.float64).reshape(-1, K, 3), np.asarray(gt_kp, np.float64).reshape(-1, K, 3)
    gt_box, gt_area = np.asarray(gt_box, np.float64).reshape(-1, 4), np.asarray(gt_area, np.float64).reshape(-1)
    G = gt_kp.shape[0]
    if K < 1 or len(gt_box) != G or len(gt_area) != G:
        raise ValueError("oks: {} sigmas, {} boxes and {} areas for {} ground truths".format(K, len(gt_box), len(gt_area), G))
    D = det_kp.shape[0]
    out = np.zeros((D, G), np.float64)
    z = np.zeros((D, K))
    xd, yd = det_kp[:, :, 0], det_kp[:, :, 1]
    for j in range(G):
        xg, yg, vg = gt_kp[j, :, 0], gt_kp[j, :, 1], gt_kp[j, :, 2]
        k1 = np.count_nonzero(vg > 0)
        if k1 > 0:
            dx, dy = xd - xg, yd - yg
        else:
            bb = gt_box[j]
            x0, x1, y0, y1 = bb[0] - bb[2], bb[0] + bb[2] * 2, bb[1] - bb[3], bb[1] + bb[3] * 2
            dx = np.maximum(z, x0 - xd) + np.maximum(z, xd - x1)
            dy = np.maximum(z, y0 - yd) + np.maximum(z, yd - y1)
        with np.errstate(over="ignore", divide="ignore"):
            e = (dx * dx + dy * dy) / var / (gt_area[j] + np.spacing(1)) / 2
        if k1 > 0:
            e = e[:, vg > 0]
        t = np.exp(-e)
        acc = np.zeros(D, np.float64)
        for k in range(t.shape[1]):
            acc = acc + t[:, k]
        out[:, j] = acc / t.shape[1]
    return out


def evaluate_img(iou, det_area, gt_area, gt_crowd, area_rng=AREA_RNG, thrs=IOU_THRS, gt_ignore=None):
    """evaluateImg of one group for every area range and IoU threshold.  iou float64 [D,G] (detections in rank order, ground truths in
    file order) -> {"dt_gt": int32 [A,T,D] matched ground-truth row or -1, "dt_ig": bool [A,T,D], "gt_ig": bool [A,G]}.
    gt_ignore [G] is the protocol's `ignore` flag of a ground truth: None = its crowd flag (boxes, masks); keypoints pass crowd or
    num_keypoints == 0.  A ground truth is ignored when the flag is set or its area is outside the range; the crowd flag alone lets a
    matched ground truth be matched again."""
    det_area, gt_area = np.asarray(det_area, np.float64).reshape(-1), np.asarray(gt_area, np.float64).reshape(-1)
    crowd = np.asarray(gt_crowd).astype(bool).reshape(-1)
    flag = crowd if gt_ignore is None else np.asarray(gt_ignore).astype(bool).reshape(-1)
    area_rng, thrs = np.asarray(area_rng, np.float64).reshape(-1, 2), np.asarray(thrs, np.float64).reshape(-1)
    D, G, A, T = len(det_area), len(gt_area), len(area_rng), len(thrs)
    iou = np.asarray(iou, np.float64).reshape(D, G)
    dt_gt = np.full((A, T, D), -1, np.int32)
    dt_ig = np.zeros((A, T, D), bool)
    gt_ig = np.zeros((A, G), bool)
    rows = iou.tolist()
    for a, (lo, hi) in enumerate(area_rng):
        ig = flag | (gt_area < lo) | (gt_area > hi)
        gt_ig[a] = ig
        order = np.argsort(ig, kind="mergesort").tolist()       # the non-ignored first, stable
        ig_l, crowd_l = ig.tolist(), crowd.tolist()
        d_out = ((det_area < lo) | (det_area > hi)).tolist()
        for t, thr in enumerate(thrs.tolist()):
            taken = [False] * G
            for d in range(D):
                best, m = min(thr, 1 - 1e-10), -1
                row = rows[d]
                for g in order:
                    if taken[g] and not crowd_l[g]:
                        continue
                    if m > -1 and not ig_l[m] and ig_l[g]:
                        break
                    if row[g] < best:
                        continue
                    best, m = row[g], g
                if m == -1:
                    dt_ig[a, t, d] = d_out[d]
                    continue
                taken[m] = True
                dt_gt[a, t, d] = m
                dt_ig[a, t, d] = ig_l[m]
    return {"dt_gt": dt_gt, "dt_ig": dt_ig, "gt_ig": gt_ig}


def accumulate(cells, n_cats, n_areas=len(AREA_RNG), n_thrs=len(IOU_THRS), max_dets=MAX_DETS, rec_thrs=REC_THRS):
    """cells: {category index k: [group results in image order]}, a group result = {"scores": [D] in rank order, "dt_gt", "dt_ig", "gt_ig"}
    (an (image, category) pair without detections and without ground truths has no entry, as evaluateImg returns None for it).
    -> {"precision": [T,R,K,A,M], "recall": [T,K,A,M]}, -1 where a cell has no non-ignored ground truth"""
    rec_thrs = np.asarray(rec_thrs, np.float64)
    T, R, K, A, M = n_thrs, len(rec_thrs), n_cats, n_areas, len(max_dets)
    precision = -np.ones((T, R, K, A, M))
    recall = -np.ones((T, K, A, M))
    for k in range(K):
        E = cells.get(k, [])
        if not E:
            continue
        for a in range(A):
            gt_ig = np.concatenate([e["gt_ig"][a] for e in E])
            npig = np.count_nonzero(~gt_ig)
            if npig == 0:
                continue
            for m, max_det in enumerate(max_dets):
                scores = np.concatenate([np.asarray(e["scores"], np.float64)[:max_det] for e in E])
                inds = np.argsort(-scores, kind="mergesort")
                dtm = np.concatenate([e["dt_gt"][a][:, :max_det] >= 0 for e in E], axis=1)[:, inds]
                dt_ig = np.concatenate([e["dt_ig"][a][:, :max_det] for e in E], axis=1)[:, inds]
                tp_sum = np.cumsum(dtm & ~dt_ig, axis=1).astype(np.float64)
                fp_sum = np.cumsum(~dtm & ~dt_ig, axis=1).astype(np.float64)
                for t, (tp, fp) in enumerate(zip(tp_sum, fp_sum)):
                    nd = len(tp)
                    rc = tp / npig
                    pr = tp / (fp + tp + np.spacing(1))
                    q = np.zeros((R,))
                    recall[t, k, a, m] = rc[-1] if nd else 0
                    if nd:
                        pr = np.maximum.accumulate(pr[::-1])[::-1]       # monotone from the right
                        at = np.searchsorted(rc, rec_thrs, side="left")
                        ok = at < nd
                        q[ok] = pr[at[ok]]
                    precision[t, :, k, a, m] = q
    return {"precision": precision, "recall": recall}


def _mean_valid(s):
    s = s[s > -1]
    return -1.0 if s.size == 0 else float(np.mean(s))


def summarize(acc, thrs=IOU_THRS, max_dets=MAX_DETS):
    """the 12 numbers of COCOeval.summarize for bbox / segm, in STAT_NAMES' order"""
    P, Rc = acc["precision"], acc["recall"]
    last = len(max_dets) - 1

    def ap(a=0, thr=None):
        s = P[:, :, :, a, last]
        return _mean_valid(s if thr is None else s[np.where(thr == thrs)[0]])

    def ar(a=0, m=last):
        return _mean_valid(Rc[:, :, a, m])

    return np.array([ap(), ap(thr=.5), ap(thr=.75), ap(1), ap(2), ap(3), ar(m=0), ar(m=1), ar(m=2), ar(1), ar(2), ar(3)], np.float64)


def summarize_keypoints(acc, thrs=IOU_THRS):
    """the 10 numbers of COCOeval.summarize for keypoints, in KP_STAT_NAMES' order; acc was accumulated with KP_AREA_RNG and KP_MAX_DETS"""
    P, Rc = acc["precision"], acc["recall"]

    def ap(a=0, thr=None):
        s = P[:, :, :, a, 0]
        return _mean_valid(s if thr is None else s[np.where(thr == thrs)[0]])

    def ar(a=0, thr=None):
        s = Rc[:, :, a, 0]
        return _mean_valid(s if thr is None else s[np.where(thr == thrs)[0]])

    return np.array([ap(), ap(thr=.5), ap(thr=.75), ap(1), ap(2), ar(), ar(thr=.5), ar(thr=.75), ar(1), ar(2)], np.float64)


def summary_text(stats, iou_type):
    """the lines COCOeval.summarize prints"""
    rows = [("Average Precision", "AP", "0.50:0.95", "all", 100), ("Average Precision", "AP", "0.50", "all", 100),
            ("Average Precision", "AP", "0.75", "all", 100), ("Average Precision", "AP", "0.50:0.95", "small", 100),
            ("Average Precision", "AP", "0.50:0.95", "medium", 100), ("Average Precision", "AP", "0.50:0.95", "large", 100),
            ("Average Recall", "AR", "0.50:0.95", "all", 1), ("Average Recall", "AR", "0.50:0.95", "all", 10),
            ("Average Recall", "AR", "0.50:0.95", "all", 100), ("Average Recall", "AR", "0.50:0.95", "small", 100),
            ("Average Recall", "AR", "0.50:0.95", "medium", 100), ("Average Recall", "AR", "0.50:0.95", "large", 100)]
    if iou_type == "keypoints":
        rows = [(title, kind, iou, area, KP_MAX_DETS[0]) for title, kind in (("Average Precision", "AP"), ("Average Recall", "AR"))
                for iou, area in (("0.50:0.95", "all"), ("0.50", "all"), ("0.75", "all"), ("0.50:0.95", "medium"), ("0.50:0.95", "large"))]
    lines = ["COCO {} summary".format(iou_type)]
    for (title, kind, iou, area, md), v in zip(rows, stats):
        lines.append(" {:<18} @[ IoU={:<9} | area={:>6s} | maxDets={:>3d} ] = {:0.3f}".format(title + " (" + kind + ")", iou, area, md, v))
    return "\n".join(lines)


def score_groups_host(groups, area_rng=AREA_RNG, thrs=IOU_THRS):
    """groups: list of {"iou" [D,G], "det_area", "gt_area", "gt_crowd" and, for keypoints, "gt_ignore"} -> list of evaluate_img results"""
    return [evaluate_img(g["iou"], g["det_area"], g["gt_area"], g["gt_crowd"], area_rng, thrs, g.get("gt_ignore")) for g in groups]


# ------------------------------------------------------------------------------------------------ proposal recall
# evaluate_box_proposals (maskrcnn_benchmark's coco_eval.py:245-356) restated line for line, in torch float32 as the reference computes
# it.  An IMAGE is a dict: "boxes" [P,4] xyxy at the original image size and "objectness" [P] (the proposals, in any order), "gt_boxes"
# [G,4] xywh, "gt_area" [G] and "gt_crowd" [G] (the annotations, in file order).  Nothing here knows a dataset.
PROPOSAL_LIMITS = (100, 1000)
PROPOSAL_AREAS = {"all": 0, "small": 1, "medium": 2, "large": 3, "96-128": 4, "128-256": 5, "256-512": 6, "512-inf": 7}
PROPOSAL_AREA_RNG = [[0 ** 2, 1e5 ** 2], [0 ** 2, 32 ** 2], [32 ** 2, 96 ** 2], [96 ** 2, 1e5 ** 2], [96 ** 2, 128 ** 2],
                     [128 ** 2, 256 ** 2], [256 ** 2, 512 ** 2], [512 ** 2, 1e5 ** 2]]
PROPOSAL_METRICS = [("AR{}@{:d}".format(s, lim), lim, a) for lim in PROPOSAL_LIMITS for a, s in (("all", ""), ("small", "s"), ("medium", "m"), ("large", "l"))]


def proposal_thresholds():
    import torch
    return torch.arange(0.5, 0.95 + 1e-5, 0.05, dtype=torch.float32)


def proposal_rank(objectness, limit=None):
    """indices of the proposals in rank order: objectness descending, equal values in their incoming order, cut at limit"""
    import torch
    inds = torch.sort(torch.as_tensor(objectness).reshape(-1), descending=True, stable=True)[1]
    return inds if limit is None else inds[:limit]


def proposal_ground_truth(gt_boxes, gt_area, gt_crowd):
    """the non-crowd annotations -> (float32 [G,4] xyxy with the reference's + 1 convention: x2 = x + max(w - 1, 0); float32 [G] areas: the
    annotations' `area` fields ROUNDED to float32, as torch.as_tensor(list) leaves them before they are compared with a range)"""
    import torch
    keep = [i for i, c in enumerate(gt_crowd) if not c]
    box = torch.as_tensor(np.asarray(gt_boxes, np.float64).reshape(-1, 4)[keep], dtype=torch.float32).reshape(-1, 4)
    x, y, w, h = box.unbind(-1)
    xyxy = torch.stack((x, y, x + (w - 1).clamp(min=0), y + (h - 1).clamp(min=0)), -1)
    return xyxy, torch.as_tensor(np.asarray(gt_area, np.float64).reshape(-1)[keep], dtype=torch.float32).reshape(-1)


def proposal_iou(prop, gt):
    """boxlist_iou: float32 [P,4] x [G,4] xyxy -> [P,G], one rounding per operation, in the reference's operation order"""
    import torch
    area1 = (prop[:, 2] - prop[:, 0] + 1) * (prop[:, 3] - prop[:, 1] + 1)
    area2 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    lt = torch.max(prop[:, None, :2], gt[:, :2])
    rb = torch.min(prop[:, None, 2:], gt[:, 2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, :, 0] * wh[:, :, 1]
    return inter / (area1[:, None] + area2 - inter)


def proposal_cover(prop, gt):
    """the cover of coco_eval.py:316-334: float32 [G], the min(P, G) recorded overlaps in round order, then zeros.  Each round takes the
    largest remaining overlap (Tensor.max: the first maximal index, so ties go to the lowest ground truth, then the lowest proposal
    rank) and retires its proposal and its ground truth.  P > 0 and G > 0."""
    import torch
    overlaps = proposal_iou(prop, gt)
    out = torch.zeros(len(gt))
    for j in range(min(len(prop), len(gt))):
        max_overlaps, argmax_overlaps = overlaps.max(dim=0)
        gt_ovr, gt_ind = max_overlaps.max(dim=0)
        assert gt_ovr >= 0
        box_ind = argmax_overlaps[gt_ind]
        out[j] = overlaps[box_ind, gt_ind]
        assert out[j] == gt_ovr
        overlaps[box_ind, :] = -1
        overlaps[:, gt_ind] = -1
    return out


def proposal_summary(gt_overlaps, hits, num_pos, thresholds):
    """the reference's result dict from the sorted overlaps, the counts of overlaps >= threshold and num_pos (coco_eval.py:344-356)"""
    import torch
    recalls = torch.zeros_like(thresholds)
    for i in range(len(thresholds)):
        recalls[i] = torch.tensor(int(hits[i])).float() / float(num_pos)
    return {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "gt_overlaps": gt_overlaps, "num_pos": num_pos}


def proposal_recall_host(images, thresholds=None, area="all", limit=None, area_range=None):
    """evaluate_box_proposals over `images` (see above) -> {"ar", "recalls", "thresholds", "gt_overlaps", "num_pos"}.
    area: a key of PROPOSAL_AREAS, or give area_range = (lo, hi) itself; a ground truth is in the range when lo <= area <= hi.
    One deviation: a range without a ground truth in the whole dataset (the reference raises from torch.cat([])) gives ar = nan, nan
    recalls and an empty gt_overlaps; with ground truths but no image that has proposals too, the recalls are 0."""
    import torch
    if area_range is None:
        assert area in PROPOSAL_AREAS, "Unknown area range: {}".format(area)
        area_range = PROPOSAL_AREA_RNG[PROPOSAL_AREAS[area]]
    gt_overlaps = []
    num_pos = 0
    for im in images:
        boxes = torch.as_tensor(im["boxes"], dtype=torch.float32).reshape(-1, 4)
        inds = proposal_rank(im["objectness"])
        boxes = boxes[inds]
        gt_boxes, gt_areas = proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
        if len(gt_boxes) == 0:
            continue
        valid_gt_inds = (gt_areas >= area_range[0]) & (gt_areas <= area_range[1])
        gt_boxes = gt_boxes[valid_gt_inds]
        num_pos += len(gt_boxes)
        if len(gt_boxes) == 0:
            continue
        if len(boxes) == 0:
            continue
        if limit is not None and len(boxes) > limit:
            boxes = boxes[:limit]
        gt_overlaps.append(proposal_cover(boxes, gt_boxes))
    gt_overlaps = torch.sort(torch.cat(gt_overlaps, dim=0))[0] if gt_overlaps else torch.zeros(0)
    if thresholds is None:
        thresholds = proposal_thresholds()
    thresholds = torch.as_tensor(thresholds, dtype=torch.float32)
    recalls = torch.zeros_like(thresholds)
    for i, t in enumerate(thresholds):
        recalls[i] = (gt_overlaps >= t).float().sum() / float(num_pos)
    return {"ar": recalls.mean(), "recalls": recalls, "thresholds": thresholds, "gt_overlaps": gt_overlaps, "num_pos": num_pos}

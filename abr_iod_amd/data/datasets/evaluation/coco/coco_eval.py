"""COCO box, mask and keypoint AP / AR (mirror of maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py: do_coco_evaluation, the
prepare_for_coco_* functions, COCOResults, check_expected_results).  The reference hands the scoring to pycocotools' COCOeval, a host loop
over every image, category, area range and IoU threshold.  Here the protocol is restated and split in two:
  * the per-image work runs on the device for the whole dataset at once: pairwise IoU with crowd semantics (ops.coco_box_iou; for masks
    ops.mask_pair_counts + ops.coco_mask_iou over run-length results decoded by ops.rle_decode; for keypoints the object keypoint similarity,
    ops.coco_oks) and the greedy matching for all area ranges and thresholds (ops.coco_match);
  * the short accumulation and the summary numbers (12; 10 for keypoints) stay on the host in float64 (coco_eval_host.py).
device="cpu" scores everything with the host restatement instead: the yardstick of the tests, never chosen silently.
"keypoints" scores the "keypoints" field the keypoint head (MODEL.KEYPOINT_ON) puts on the detections, under the keypoint protocol's
own parameters: at most 20 detections per image, the area ranges all / medium / large, ground truths without a labelled keypoint ignored.
box_only (predictions that carry an "objectness" field: RPN proposals) scores proposal recall instead, the reference's
evaluate_box_proposals: AR at 100 and 1000 proposals for all / small / medium / large ground truths.  The greedy
cover of every image, limit and area range runs in one launch (ops.proposal_cover); the restatement (coco_eval_host.proposal_recall_host, float32 as the reference computes it) is what device="cpu" runs."""
import json
import logging
import os
from collections import OrderedDict

import numpy as np
import torch

from ..voc.coco_results import prepare_for_coco_segmentation  # noqa: F401
from . import coco_eval_host as H


class MissingObjectness(ValueError, NotImplementedError):
    """box_only was asked of predictions that carry no "objectness" field: a bad value for the caller, and, for detections, a score this
    module does not produce (their boxes are not ranked as proposals).  Callers written while box_only was not carried at all caught
    NotImplementedError for exactly this call; they keep working."""


def do_coco_evaluation(dataset, predictions, box_only, output_folder, iou_types, expected_results, expected_results_sigma_tol, device="cuda"):
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    if box_only:
        logger.info("Evaluating bbox proposals")
        res = COCOResults("box_proposal")
        areas = ("all", "small", "medium", "large")
        cells, n_fallback = score_proposals(proposal_images(predictions, dataset), H.PROPOSAL_LIMITS,
                                            [H.PROPOSAL_AREA_RNG[H.PROPOSAL_AREAS[a]] for a in areas], None, device)
        for key, limit, area in H.PROPOSAL_METRICS:          # the eight cells come out of ONE ops.proposal_cover call
            res.results["box_proposal"][key] = cells[H.PROPOSAL_LIMITS.index(limit)][areas.index(area)]["ar"].item()
        if n_fallback:
            logger.info("{} images were left to the host restatement (more proposals or ground truths than the kernel holds)".format(n_fallback))
        logger.info(res)
        check_expected_results(res, expected_results, expected_results_sigma_tol)
        if output_folder:
            torch.save(res, os.path.join(output_folder, "box_proposals.pth"))
        return res, None
    unknown = [t for t in iou_types if t not in ("bbox", "segm", "keypoints")]
    if unknown:
        raise NotImplementedError("COCO evaluation of {} is not carried (bbox, segm and keypoints are)".format(unknown))
    logger.info("Preparing results for COCO format")
    coco_results = {}
    if "bbox" in iou_types:
        logger.info("Preparing bbox results")
        coco_results["bbox"] = prepare_for_coco_detection(predictions, dataset)
    if "segm" in iou_types:
        logger.info("Preparing segm results")
        coco_results["segm"] = prepare_for_coco_segmentation(predictions, dataset)       # (encoded on the device whatever `device` scores)
    if "keypoints" in iou_types:
        logger.info("Preparing keypoints results")
        coco_results["keypoints"] = prepare_for_coco_keypoint(predictions, dataset)
    results = COCOResults(*iou_types)
    logger.info("Evaluating predictions")
    for iou_type in iou_types:
        if output_folder:
            with open(os.path.join(output_folder, iou_type + ".json"), "w") as f:
                json.dump(coco_results[iou_type], f)
        res = evaluate_predictions_on_coco(dataset, coco_results[iou_type], iou_type, device=device)
        logger.info(res.text())
        results.update(res)
    logger.info(results)
    check_expected_results(results, expected_results, expected_results_sigma_tol)
    if output_folder:
        torch.save(results, os.path.join(output_folder, "coco_results.pth"))
    return results, coco_results


def prepare_for_coco_detection(predictions, dataset):
    """predictions (BoxLists in dataset order) -> [{"image_id", "category_id", "bbox": xywh at the original image size, "score"}]"""
    coco_results = []
    for image_id, prediction in enumerate(predictions):
        original_id = dataset.id_to_img_map[image_id]
        if len(prediction) == 0:
            continue
        info = dataset.get_img_info(image_id)
        prediction = prediction.copy_with_fields(["labels", "scores"]).resize((info["width"], info["height"])).convert("xywh")
        boxes = prediction.bbox.tolist()
        scores = prediction.get_field("scores").tolist()
        labels = [dataset.contiguous_category_id_to_json_id[i] for i in prediction.get_field("labels").tolist()]
        coco_results.extend({"image_id": original_id, "category_id": labels[k], "bbox": box, "score": scores[k]} for k, box in enumerate(boxes))
    return coco_results


def prepare_for_coco_keypoint(predictions, dataset):
    """predictions (BoxLists with a "keypoints" field, in dataset order) -> [{"image_id", "category_id", "keypoints": [x, y, v] * K at the
    original image size, "score": the box score}]"""
    coco_results = []
    for image_id, prediction in enumerate(predictions):
        original_id = dataset.id_to_img_map[image_id]
        if len(prediction) == 0:
            continue
        if not prediction.has_field("keypoints"):
            raise ValueError('image {}: the prediction has no "keypoints" field (its fields: {}); keypoint scoring needs a model with '
                             'MODEL.KEYPOINT_ON'.format(original_id, prediction.fields()))
        info = dataset.get_img_info(image_id)
        size = (info["width"], info["height"])
        prediction = prediction.copy_with_fields(["labels", "scores", "keypoints"]).resize(size)
        scores = prediction.get_field("scores").tolist()
        labels = [dataset.contiguous_category_id_to_json_id[i] for i in prediction.get_field("labels").tolist()]
        keypoints = prediction.get_field("keypoints").resize(size)        # (BoxList.resize has resized the field: a ratio of 1, as in the reference)
        keypoints = keypoints.keypoints.reshape(keypoints.keypoints.shape[0], -1).tolist()
        coco_results.extend({"image_id": original_id, "category_id": labels[k], "keypoints": kp, "score": scores[k]} for k, kp in enumerate(keypoints))
    return coco_results


# ------------------------------------------------------------------------------------------------ proposal recall
def proposal_images(predictions, dataset):
    """predictions (BoxLists with an "objectness" field, in dataset order) -> the images coco_eval_host's proposal-recall section takes:
    the proposals resized to the original image size (BoxList.resize) and ALL annotations of the image as the file gives them"""
    images = []
    for image_id, prediction in enumerate(predictions):
        original_id = dataset.id_to_img_map[image_id]
        if not prediction.has_field("objectness"):
            raise MissingObjectness('image {}: the prediction has no "objectness" field (its fields: {}); proposal recall (box_only) scores '
                                    'RPN proposals'.format(original_id, prediction.fields()))
        info = dataset.get_img_info(image_id)
        prediction = prediction.copy_with_fields(["objectness"]).resize((info["width"], info["height"])).convert("xyxy")
        anno = dataset.get_annotations(image_id)
        images.append({"boxes": prediction.bbox.detach().to("cpu", torch.float32).reshape(-1, 4),
                       "objectness": prediction.get_field("objectness").detach().cpu().reshape(-1),
                       "gt_boxes": [obj["bbox"] for obj in anno], "gt_area": [obj["area"] for obj in anno],
                       "gt_crowd": [obj.get("iscrowd", 0) != 0 for obj in anno]})
    return images


def score_proposals(images, limits, area_ranges, thresholds=None, device="cuda"):
    """The dataset-free core of proposal recall: images (see coco_eval_host) x limits [L] x area_ranges [A] of (lo, hi) ->
    ([L][A] result dicts of evaluate_box_proposals, the number of images the kernel left to the host).  device "cuda": one
    ops.proposal_cover launch for all L x A cells; "cpu": the host restatement, cell by cell."""
    from ..... import ops
    device = torch.device(device)
    thresholds = H.proposal_thresholds() if thresholds is None else torch.as_tensor(thresholds, dtype=torch.float32).reshape(-1)
    limits = [int(v) for v in limits]
    if device.type != "cuda":
        return [[H.proposal_recall_host(images, thresholds, limit=lim, area_range=tuple(r)) for r in area_ranges] for lim in limits], 0
    props, gts, areas = [], [], []
    for im in images:
        boxes = torch.as_tensor(im["boxes"], dtype=torch.float32).reshape(-1, 4)
        props.append(boxes[H.proposal_rank(im["objectness"], max(limits))])
        g, a = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
        gts.append(g)
        areas.append(a)
    cat = lambda ts, shape: (torch.cat(ts) if ts else torch.zeros((0,) + shape[1:])).reshape(shape)      # noqa: E731
    out = ops.proposal_cover(cat(props, (-1, 4)), cat(gts, (-1, 4)), cat(areas, (-1,)), [len(p) for p in props], [len(g) for g in gts],
                             np.asarray(area_ranges, np.float32).reshape(-1, 2), limits, thresholds, device)
    cells = []
    for li in range(len(limits)):
        row = []
        for a in range(len(area_ranges)):
            v = torch.from_numpy(out["overlaps"][li, a])
            row.append(H.proposal_summary(torch.sort(v[v >= 0])[0], out["hits"][li, a], int(out["num_pos"][a]), thresholds))
        cells.append(row)
    return cells, out["n_fallback"]


def evaluate_box_proposals(predictions, dataset, thresholds=None, area="all", limit=None, device="cuda"):
    """the reference's evaluate_box_proposals (coco_eval.py:245-356) plus `device` -> {"ar", "recalls", "thresholds", "gt_overlaps",
    "num_pos"}; limit None: every proposal counts.  See coco_eval_host.proposal_recall_host for the protocol and its one deviation.
    Where device="cuda" differs from "cpu": more than 16 thresholds raise (ops.proposal_cover takes at most 16), and an image with more
    proposals inside the limit than ops.PROPOSAL_COVER_MAX_PROP (1024; only limit None or a limit above it lets that happen) or more than
    ops.COCO_MATCH_MAX_GT non-crowd ground truths is scored by the host restatement inside the call -- same numbers, host speed."""
    assert area in H.PROPOSAL_AREAS, "Unknown area range: {}".format(area)
    images = proposal_images(predictions, dataset)
    if torch.device(device).type != "cuda":
        return H.proposal_recall_host(images, thresholds, area=area, limit=limit)
    lim = max([len(im["boxes"]) for im in images] + [1]) if limit is None else limit
    return score_proposals(images, [lim], [H.PROPOSAL_AREA_RNG[H.PROPOSAL_AREAS[area]]], thresholds, device)[0][0][0]


class COCOEvalResult(object):
    """what one iou_type's evaluation leaves: stats (the numbers of COCOeval.summarize: 12 in coco_eval_host.STAT_NAMES' order, for
    keypoints 10 in KP_STAT_NAMES'), the precision [T,R,K,A,M] and recall [T,K,A,M] tables, and how the groups were scored"""

    def __init__(self, iou_type, stats, acc, n_groups, n_fallback):
        self.iou_type, self.stats, self.precision, self.recall = iou_type, stats, acc["precision"], acc["recall"]
        self.n_groups, self.n_fallback = n_groups, n_fallback

    def text(self):
        return H.summary_text(self.stats, self.iou_type)


class COCOResults(object):
    METRICS = {"bbox": ["AP", "AP50", "AP75", "APs", "APm", "APl"], "segm": ["AP", "AP50", "AP75", "APs", "APm", "APl"],
               "keypoints": ["AP", "AP50", "AP75", "APm", "APl"],
               "box_proposal": ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]}

    def __init__(self, *iou_types):
        assert all(t in COCOResults.METRICS for t in iou_types), iou_types
        self.results = OrderedDict((t, OrderedDict((m, -1) for m in COCOResults.METRICS[t])) for t in iou_types)

    def update(self, coco_eval):
        if coco_eval is None:
            return
        assert isinstance(coco_eval, COCOEvalResult)
        res = self.results[coco_eval.iou_type]
        for idx, metric in enumerate(COCOResults.METRICS[coco_eval.iou_type]):
            res[metric] = float(coco_eval.stats[idx])

    def __repr__(self):
        return repr(self.results)


def check_expected_results(results, expected_results, sigma_tol):
    """expected_results: [(task, metric, (mean, std))]; logs PASS / FAIL for mean - sigma_tol * std < value < mean + sigma_tol * std"""
    if not expected_results:
        return
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    for task, metric, (mean, std) in expected_results:
        actual = results.results[task][metric]
        lo, hi = mean - sigma_tol * std, mean + sigma_tol * std
        ok = lo < actual < hi
        msg = "{} > {} sanity check (actual vs. expected): {:.3f} vs. mean={:.4f}, std={:.4}, range=({:.4f}, {:.4f})".format(
            task, metric, actual, mean, std, lo, hi)
        if ok:
            logger.info("PASS: " + msg)
        else:
            logger.error("FAIL: " + msg)


# ------------------------------------------------------------------------------------------------ groups
def _image_mask_iou(dets, anns, size, masks_of, device):
    """one image: result dicts with run-length "segmentation"s x annotations -> (float64 [P,T] IoU, [P] pixel counts), pairs of different
    categories 0"""
    from ..... import ops
    width, height = size
    P, T = len(dets), len(anns)
    crowd = np.array([bool(a.get("iscrowd", 0)) for a in anns], bool)
    dl = np.array([d["category_id"] for d in dets], np.int64)
    gl = np.array([a["category_id"] for a in anns], np.int64)
    rles = [d["segmentation"] for d in dets]
    if device.type == "cuda":
        pb = ops.rle_decode(rles, (height, width), device, packed=True)
        if T == 0:
            area_p = ops.mask_pair_counts(pb, pb[:1], width)[1] if P else torch.zeros((0,), dtype=torch.int32)
            return np.zeros((P, 0)), area_p.cpu().numpy().astype(np.int64)
        gb = masks_of(device, True)
        inter, area_p, area_t = ops.mask_pair_counts(pb, gb, width, torch.from_numpy(dl), torch.from_numpy(gl))
        return ops.coco_mask_iou(inter, area_p, area_t, crowd).cpu().numpy(), area_p.cpu().numpy().astype(np.int64)
    pm = ops.rle_decode(rles, (height, width), "cpu").numpy().reshape(P, -1).astype(np.int64)
    area_p = pm.sum(1)
    if T == 0:
        return np.zeros((P, 0)), area_p
    gm = masks_of(device, False).numpy().reshape(T, -1).astype(np.int64)
    inter = (pm @ gm.T) * (dl[:, None] == gl[None, :])
    return H.mask_iou_from_counts(inter, area_p, gm.sum(1), crowd), area_p


def _keypoint_rows(items, K, what):
    """the "keypoints" lists of results or annotations -> float64 [n,K,3]"""
    for it in items:
        if len(it.get("keypoints", ())) != 3 * K:
            raise ValueError('{} of image {}: "keypoints" holds {} numbers, {} keypoints need {}'.format(
                what, it["image_id"], len(it.get("keypoints", ())), K, 3 * K))
    return np.array([it["keypoints"] for it in items], np.float64).reshape(-1, K, 3)


def build_groups(dataset, coco_results, iou_type, device, n_keypoints=None):
    """-> (groups, cat_ids).  A group: {"k": category index, "scores" (rank order), "det_area", "gt_area", "gt_crowd", and "det" / "gt"
    xywh boxes (bbox), "iou" float64 [D,G] (segm) or "det_kp" / "gt_kp" [.,K,3], "gt_box" and "gt_ignore" (keypoints, K = n_keypoints;
    ranked detections cut at 20; gt_ignore = crowd or num_keypoints == 0, the annotation's own count or else its v > 0)}, images in
    dataset order, categories ascending inside an image"""
    device = torch.device(device)
    max_det = H.KP_MAX_DETS[-1] if iou_type == "keypoints" else H.MAX_DETS[-1]
    cat_ids = sorted(dataset.json_category_id_to_contiguous_id)
    cat_index = {c: k for k, c in enumerate(cat_ids)}
    by_image = {}
    for r in coco_results:
        by_image.setdefault(r["image_id"], []).append(r)
    known = set(dataset.id_to_img_map.values())
    stray = [i for i in by_image if i not in known]
    if stray:
        raise ValueError("results for image ids the dataset does not hold: {}".format(sorted(stray)[:5]))
    groups = []
    for index in range(len(dataset)):
        dets = by_image.get(dataset.id_to_img_map[index], [])
        anns = dataset.get_annotations(index)
        if not dets and not anns:
            continue
        if iou_type == "segm" and dets:
            info = dataset.get_img_info(index)
            iou_img, area_img = _image_mask_iou(dets, anns, (int(info["width"]), int(info["height"])),
                                                lambda dev, packed: dataset.annotation_masks(index, dev, packed), device)
        for c in sorted(set(d["category_id"] for d in dets) | set(a["category_id"] for a in anns)):
            if c not in cat_index:
                raise ValueError("category id {} is not in the annotation file".format(c))
            rows = np.array([i for i, d in enumerate(dets) if d["category_id"] == c], np.int64)
            cols = np.array([j for j, a in enumerate(anns) if a["category_id"] == c], np.int64)
            rows = rows[H.rank_detections([dets[i]["score"] for i in rows], max_det)]
            g = {"k": cat_index[c], "scores": np.array([dets[i]["score"] for i in rows], np.float64),
                 "gt_area": np.array([anns[j]["area"] for j in cols], np.float64),
                 "gt_crowd": np.array([bool(anns[j].get("iscrowd", 0)) for j in cols], bool)}
            if iou_type == "bbox":
                g["det"] = np.array([dets[i]["bbox"] for i in rows], np.float64).reshape(-1, 4)
                g["gt"] = np.array([anns[j]["bbox"] for j in cols], np.float64).reshape(-1, 4)
                g["det_area"] = g["det"][:, 2] * g["det"][:, 3]
            elif iou_type == "keypoints":
                gts = [anns[j] for j in cols]
                g["det_kp"] = _keypoint_rows([dets[i] for i in rows], n_keypoints, "a result")
                g["gt_kp"] = _keypoint_rows(gts, n_keypoints, "an annotation")
                g["gt_box"] = np.array([a["bbox"] for a in gts], np.float64).reshape(-1, 4)
                g["det_area"] = H.keypoint_det_area(g["det_kp"])
                labelled = np.array([a["num_keypoints"] if "num_keypoints" in a else np.count_nonzero(kp[:, 2] > 0)
                                     for a, kp in zip(gts, g["gt_kp"])], np.int64)
                g["gt_ignore"] = g["gt_crowd"] | (labelled == 0)
            else:
                g["iou"] = iou_img[np.ix_(rows, cols)] if len(rows) else np.zeros((0, len(cols)))
                g["det_area"] = area_img[rows].astype(np.float64) if len(rows) else np.zeros((0,))
            groups.append(g)
    return groups, cat_ids


def score_groups(groups, iou_type, device, area_rng=None, thrs=H.IOU_THRS, sigmas=None):
    """-> (per-group evaluateImg results, number of groups the match kernel left to the host).  area_rng None: the protocol's own
    (H.KP_AREA_RNG for keypoints, else H.AREA_RNG); sigmas [K]: the per-keypoint constants of OKS (keypoints only)"""
    from ..... import ops
    device = torch.device(device)
    kp = iou_type == "keypoints"
    if area_rng is None:
        area_rng = H.KP_AREA_RNG if kp else H.AREA_RNG
    if device.type != "cuda":
        for g in groups:
            if iou_type == "bbox":
                g["iou"] = H.box_iou(g["det"], g["gt"], g["gt_crowd"])
            elif kp:
                g["iou"] = H.oks(g["det_kp"], g["gt_kp"], g["gt_box"], g["gt_area"], sigmas)
        return H.score_groups_host(groups, area_rng, thrs), 0
    if not groups:
        return [], 0
    dc = np.array([len(g["scores"]) for g in groups], np.int64)
    gc = np.array([len(g["gt_area"]) for g in groups], np.int64)
    cat = lambda key, shape: np.concatenate([np.asarray(g[key]).reshape(shape) for g in groups])      # noqa: E731
    crowd = cat("gt_crowd", (-1,))
    if iou_type == "bbox":
        iou, _ = ops.coco_box_iou(cat("det", (-1, 4)), cat("gt", (-1, 4)), crowd, dc, gc, device)
    elif kp:
        K = len(sigmas)
        iou, _ = ops.coco_oks(cat("det_kp", (-1, K, 3)), cat("gt_kp", (-1, K, 3)), cat("gt_box", (-1, 4)), cat("gt_area", (-1,)), sigmas, dc, gc, device)
    else:
        iou = cat("iou", (-1,))
    out = ops.coco_match(iou, dc, gc, cat("det_area", (-1,)), cat("gt_area", (-1,)), crowd, area_rng, thrs, device,
                         gt_ignore=cat("gt_ignore", (-1,)) if kp else None)
    d_off, g_off = np.concatenate(([0], np.cumsum(dc))), np.concatenate(([0], np.cumsum(gc)))
    res = [{"dt_gt": out["dt_gt"][:, :, d_off[i]: d_off[i + 1]], "dt_ig": out["dt_ig"][:, :, d_off[i]: d_off[i + 1]],
            "gt_ig": out["gt_ig"][:, g_off[i]: g_off[i + 1]]} for i in range(len(groups))]
    return res, out["n_fallback"]


def _keypoint_sigmas(dataset, coco_results, kpt_oks_sigmas):
    """the OKS constants, one per keypoint: COCO's 17 person-keypoint sigmas unless given; K is read off the first result or annotation"""
    first = next((r for r in coco_results if "keypoints" in r), None)
    if first is None:
        first = next((a for index in range(len(dataset)) for a in dataset.get_annotations(index) if "keypoints" in a), None)
    K = len(first["keypoints"]) // 3 if first is not None else len(H.KPT_OKS_SIGMAS)
    if kpt_oks_sigmas is None:
        if K != len(H.KPT_OKS_SIGMAS):
            raise ValueError("keypoint scoring: {} keypoints per instance and no kpt_oks_sigmas given; the default sigmas are those of COCO's "
                             "{} person keypoints".format(K, len(H.KPT_OKS_SIGMAS)))
        return H.KPT_OKS_SIGMAS
    sigmas = np.asarray(kpt_oks_sigmas, np.float64).reshape(-1)
    if len(sigmas) != K:
        raise ValueError("keypoint scoring: {} kpt_oks_sigmas for {} keypoints per instance".format(len(sigmas), K))
    return sigmas


def evaluate_predictions_on_coco(dataset, coco_results, iou_type="bbox", device="cuda", kpt_oks_sigmas=None):
    if iou_type != "keypoints":
        groups, cat_ids = build_groups(dataset, coco_results, iou_type, device)
        scored, n_fallback = score_groups(groups, iou_type, device)
    else:
        sigmas = _keypoint_sigmas(dataset, coco_results, kpt_oks_sigmas)
        groups, cat_ids = build_groups(dataset, coco_results, iou_type, device, n_keypoints=len(sigmas))
        scored, n_fallback = score_groups(groups, iou_type, device, sigmas=sigmas)
    cells = {}
    for g, r in zip(groups, scored):
        cells.setdefault(g["k"], []).append(dict(r, scores=g["scores"]))
    if iou_type == "keypoints":
        acc = H.accumulate(cells, len(cat_ids), n_areas=len(H.KP_AREA_RNG), max_dets=H.KP_MAX_DETS)
        return COCOEvalResult(iou_type, H.summarize_keypoints(acc), acc, len(groups), n_fallback)
    acc = H.accumulate(cells, len(cat_ids))
    return COCOEvalResult(iou_type, H.summarize(acc), acc, len(groups), n_fallback)

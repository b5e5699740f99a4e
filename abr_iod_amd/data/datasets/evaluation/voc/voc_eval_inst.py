"""PASCAL VOC box AND instance-mask AP over the IoU thresholds 0.5:0.05:0.9 ("mAP OD" / "mAP IS").

Mirror of maskrcnn_benchmark/data/datasets/evaluation/voc/voc_eval_inst.py:14-217 (same function names, return values and result.txt).
The file has two parts:
  * a DEVICE part, which turns one image's predicted and ground-truth masks into integer pixel counts (ops.mask_resize_pack_bits,
    ops.mask_pack_bits, ops.mask_pair_counts) -- the reference's masklist_iou (:89-105) is a Python double loop over full-image float
    tensors, run again for each of the 9 thresholds; here the counts are exact integers, computed once per image and reused;
  * a pure-numpy part (matching, precision / recall, AP) that takes those counts and needs no GPU.
The reference's rules are kept: box IoU on +1 corners through boxlist_iou (:150-158), no "difficult" handling, detections sorted by score
per class per image (:133), argmax takes the first maximum (:160-161), unmatched iff max < thresh (:164-165), a ground truth is claimed by
the first detection that reaches it (:169-189)."""
import os

import numpy as np
import torch

from .voc_eval import calc_detection_voc_ap

IOU_THRESHOLDS = np.arange(0.5, 0.95, 0.05).tolist()     # (:26)
POSTPROCESS_KEY = "MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS"


# ------------------------------------------------------------------------------------------------ device part
def _prediction_bits(field, size, device):
    """the "mask" field of one prediction -> packed bits [n,H,Wq] on `device` at size = (width, height)"""
    from ..... import ops
    from .....structures.segmentation_mask import PackedMasks, SegmentationMask
    width, height = int(size[0]), int(size[1])
    if isinstance(field, PackedMasks):
        return field.resize((width, height)).bits.to(device)
    if isinstance(field, torch.Tensor):
        if field.dtype != torch.uint8:
            raise ValueError("the predictions' 'mask' field is a bare {} tensor of shape {}: mask probabilities per RoI, not masks pasted "
                             "into the image.  Mask AP needs {} = True".format(field.dtype, tuple(field.shape), POSTPROCESS_KEY))
        masks = field.reshape((field.shape[0],) + tuple(field.shape[-2:]))      # [n,1,H,W] as the mask head returns it (inference.py:70-79)
    elif isinstance(field, SegmentationMask):
        masks = field.masks
    else:
        raise TypeError("cannot score a 'mask' field of type {}".format(type(field).__name__))
    masks = masks.to(device)
    if masks.dtype == torch.uint8:
        return ops.mask_resize_pack_bits(masks, height, width)
    if tuple(masks.shape[1:]) != (height, width):
        raise TypeError("float32 masks are packed at their own size only; resize them first or hold them as uint8")
    return ops.mask_pack_bits(masks)


def image_mask_counts(prediction, gt_boxlist, size, device=None):
    """One image -> {"inter": [P,T], "area_p": [P], "area_t": [T]} int64 numpy pixel counts, rows in the prediction's own order and columns
    in the ground truth's.  Pairs of different labels are not compared (the metric never looks at them) and hold 0."""
    from ..... import ops
    field = prediction.get_field("mask")
    if device is None:
        held = field.bits if hasattr(field, "bits") else (field.masks if hasattr(field, "masks") else field)
        device = held.device if held.is_cuda else torch.device("cuda")
    pred_bits = _prediction_bits(field, size, device)
    gt = gt_boxlist.get_field("masks").instances
    if hasattr(gt, "poly_offsets"):     # PolygonList: rasterised straight into bits on the device
        gt = gt.to(device).pack()
    if hasattr(gt, "bits"):     # PackedMasks (decoded from run-length annotations straight into bits)
        assert tuple(gt.size) == (int(size[0]), int(size[1])), "ground-truth masks {} are not at the image's size {}".format(gt, size)
        gt_bits = gt.bits.to(device)
    else:
        gt_masks = gt.masks
        assert tuple(gt_masks.shape[1:]) == (int(size[1]), int(size[0])), "ground-truth masks {} are not at the image's size {}".format(
            tuple(gt_masks.shape), size)
        gt_bits = ops.mask_pack_bits(gt_masks.to(device))
    inter, area_p, area_t = ops.mask_pair_counts(pred_bits, gt_bits, size[0], prediction.get_field("labels"), gt_boxlist.get_field("labels"))
    return {"inter": inter.cpu().numpy().astype(np.int64), "area_p": area_p.cpu().numpy().astype(np.int64),
            "area_t": area_t.cpu().numpy().astype(np.int64)}


# ------------------------------------------------------------------------------------------------ numpy part
def mask_iou_from_counts(inter, area_p, area_t):
    """float64 [P,T]: inter / union, 0.0 where the union is empty (:100-104; the reference's `break` there leaves zeros in the rest of
    the row, which an empty predicted mask has anyway)"""
    inter = np.asarray(inter, np.int64)
    union = np.asarray(area_p, np.int64)[:, None] + np.asarray(area_t, np.int64)[None, :] - inter
    out = np.zeros(inter.shape, np.float64)
    np.divide(inter, union, out=out, where=union > 0)
    return out


def _box_iou(pred_bbox_l, gt_bbox_l, size):
    from .....structures.bounding_box import BoxList
    from .....structures.boxlist_ops import boxlist_iou
    p, g = pred_bbox_l.copy(), gt_bbox_l.copy()
    p[:, 2:] += 1          # "VOC evaluation follows integer typed bounding boxes" (:150-154)
    g[:, 2:] += 1
    return boxlist_iou(BoxList(torch.from_numpy(p), size), BoxList(torch.from_numpy(g), size)).numpy()


def _claim(iou, iou_thresh):
    """detections in score order x ground truths -> 1 for the first detection whose best ground truth it is, else 0 (:160-189)"""
    gt_index = iou.argmax(axis=1)
    gt_index[iou.max(axis=1) < iou_thresh] = -1
    taken = np.zeros(iou.shape[1], dtype=bool)
    out = []
    for g in gt_index:
        out.append(1 if g >= 0 and not taken[g] else 0)
        if g >= 0:
            taken[g] = True
    return out


def image_record(prediction, gt_boxlist, mask_iou):
    """what the matching needs of one image, on the host: boxes, labels, scores and the [P,T] mask IoU matrix"""
    return {"pred_bbox": prediction.bbox.cpu().numpy(), "pred_label": prediction.get_field("labels").cpu().numpy(),
            "pred_score": prediction.get_field("scores").cpu().numpy(), "gt_bbox": gt_boxlist.bbox.cpu().numpy(),
            "gt_label": gt_boxlist.get_field("labels").cpu().numpy(), "size": gt_boxlist.size, "mask_iou": np.asarray(mask_iou, np.float64)}


def calc_detection_voc_prec_rec(records, iou_thresh=0.5):
    """records: image_record per image -> (prec, rec, mask_prec, mask_rec), lists indexed by class id (:107-217)"""
    n_pos, score, match, mask_match = {}, {}, {}, {}
    for r in records:
        pred_label, gt_label = r["pred_label"], r["gt_label"]
        for l in np.unique(np.concatenate((pred_label, gt_label)).astype(int)):
            rows = np.nonzero(pred_label == l)[0]
            rows = rows[r["pred_score"][rows].argsort()[::-1]]       # sort by score (:133)
            cols = np.nonzero(gt_label == l)[0]
            n_pos[l] = n_pos.get(l, 0) + len(cols)
            score.setdefault(l, []).extend(r["pred_score"][rows])
            match.setdefault(l, [])
            mask_match.setdefault(l, [])
            if len(rows) == 0:
                continue
            if len(cols) == 0:
                match[l].extend((0,) * len(rows))
                mask_match[l].extend((0,) * len(rows))
                continue
            match[l].extend(_claim(_box_iou(r["pred_bbox"][rows], r["gt_bbox"][cols], r["size"]), iou_thresh))
            mask_match[l].extend(_claim(r["mask_iou"][np.ix_(rows, cols)], iou_thresh))
    n_fg_class = max(n_pos.keys()) + 1
    prec, rec, mask_prec, mask_rec = ([None] * n_fg_class for _ in range(4))
    for l in n_pos:
        order = np.array(score[l]).argsort()[::-1]
        match_l = np.array(match[l], dtype=np.int8)[order]
        mask_match_l = np.array(mask_match[l], dtype=np.int8)[order]
        tp, fp = np.cumsum(match_l == 1), np.cumsum(match_l == 0)
        mask_tp, mask_fp = np.cumsum(mask_match_l == 1), np.cumsum(mask_match_l == 0)
        prec[l] = tp / (fp + tp)
        mask_prec[l] = mask_tp / (mask_fp + mask_tp)
        if n_pos[l] > 0:
            rec[l] = tp / n_pos[l]
            mask_rec[l] = mask_tp / n_pos[l]
    return prec, rec, mask_prec, mask_rec


def eval_detection_voc(records, iou_thresh=0.5, use_07_metric=False):
    """-> {"ap_box", "ap_mask": per-class arrays (index 0 = background), "map_box", "map_mask"}  (:68-87)"""
    prec, rec, mask_prec, mask_rec = calc_detection_voc_prec_rec(records, iou_thresh)
    ap_box = calc_detection_voc_ap(prec, rec, use_07_metric=use_07_metric)
    ap_mask = calc_detection_voc_ap(mask_prec, mask_rec, use_07_metric=use_07_metric)
    return {"ap_box": ap_box, "ap_mask": ap_mask, "map_box": np.nanmean(ap_box), "map_mask": np.nanmean(ap_mask)}


def summarise(dataset, records, output_folder, logger):
    """the 9 thresholds over prepared records -> the reference's return value, log lines, prints and result.txt (:26-65)"""
    n_classes = len(dataset.new_classes) + len(dataset.old_classes)
    ap_boxes = np.zeros((len(IOU_THRESHOLDS), n_classes))
    ap_masks = np.zeros((len(IOU_THRESHOLDS), n_classes))
    for idx, iou_thresh in enumerate(IOU_THRESHOLDS):
        result = eval_detection_voc(records, iou_thresh=iou_thresh, use_07_metric=False)
        ap_masks[idx] = result["ap_mask"][1:]
        ap_boxes[idx] = result["ap_box"][1:]
    ap_05_95_mask = ap_masks.mean(axis=0)
    ap_05_95_box = ap_boxes.mean(axis=0)
    result_str_box = "mAP OD\n {:.4f}\n".format(np.mean(ap_05_95_box))
    result_str_mask = "mAP IS\n {:.4f}\n".format(np.mean(ap_05_95_mask))
    for i, ap in enumerate(ap_05_95_box):
        result_str_box += "{:<16}: {:.4f}\n".format(dataset.map_class_id_to_class_name(i + 1), ap)
    for i, ap in enumerate(ap_05_95_mask):
        result_str_mask += "{:<16}: {:.4f}\n".format(dataset.map_class_id_to_class_name(i + 1), ap)
    print("BOX", end=": ")
    print(",".join([str(x) for x in ap_05_95_box]))
    print("MSK", end=": ")
    print(",".join([str(x) for x in ap_05_95_mask]))
    logger.info(result_str_box)
    logger.info(result_str_mask)
    if output_folder:
        with open(os.path.join(output_folder, "result.txt"), "w") as fid:
            fid.write(result_str_box)
            fid.write(result_str_mask)
    return {"mask": ap_05_95_mask, "box": result_str_box}, ap_boxes, ap_masks


def prepare_records(dataset, predictions, device=None):
    """device part over the dataset: every prediction's boxes resized to the original image size (:17-24), its masks resized and packed
    there, counted against the ground truth once"""
    records = []
    for image_id, prediction in enumerate(predictions):
        info = dataset.get_img_info(image_id)
        size = (info["width"], info["height"])
        gt_boxlist = dataset.get_groundtruth(image_id)
        boxes = prediction.copy_with_fields(["labels", "scores"]).resize(size)
        counts = image_mask_counts(prediction, gt_boxlist, size, device)
        records.append(image_record(boxes, gt_boxlist, mask_iou_from_counts(counts["inter"], counts["area_p"], counts["area_t"])))
    return records


def do_voc_evaluation_inst(dataset, predictions, output_folder, logger):
    return summarise(dataset, prepare_records(dataset, predictions), output_folder, logger)[0]

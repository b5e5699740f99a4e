"""Golden vectors for the instance-mask evaluation from the REFERENCE's own voc_eval_inst.py (run by hand where the reference tree exists;
see ref_harness.py) -> mask_eval.npz, data only:
    inputs      per image: predictions at the network's scale (boxes, labels, scores, uint8 masks), ground truth at the original size
    miou_i_l    masklist_iou of image i, class l (rows: that class's detections in descending score order; columns: its ground truths)
    prec / rec  calc_detection_voc_prec_rec for box and mask at each of the 9 thresholds
    ap tables   eval_detection_voc at each threshold, and do_voc_evaluation_inst's return value and result.txt
The cases the fixture must hold are asserted at the end."""
import copy
import logging
import os
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness  # noqa: E402

NAMES = ["__background__", "aeroplane", "bicycle", "bird"]
# original (width, height) and network (width, height): non-integer ratios both ways, one identity; widths below 64 and off multiples of 64
SIZES = [((150, 100), (211, 141)), ((45, 80), (33, 59)), ((130, 97), (173, 129)), ((200, 120), (147, 88)), ((70, 64), (70, 64)), ((100, 100), (137, 137))]


def ellipse(w, h, cx, cy, rx, ry):
    ys, xs = np.mgrid[0:h, 0:w]
    return ((((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2) <= 1.0).astype(np.uint8)


def box_of(m):
    ys, xs = np.nonzero(m)
    if len(ys) == 0:
        return [2.0, 2.0, 6.0, 6.0]
    return [float(xs.min()), float(ys.min()), float(xs.max()), float(ys.max())]


def build_inputs():
    images = []
    for i, ((w, h), (nw, nh)) in enumerate(SIZES):
        sx, sy = nw / w, nh / h
        gt, det = [], []      # (label, mask at original size) / (label, score, mask at network size)

        def detect(label, score, cx, cy, rx, ry):
            det.append((label, score, ellipse(nw, nh, cx * sx, cy * sy, rx * sx, ry * sy)))

        if i == 0:      # two detections on one ground truth; a detected class without ground truth here (3)
            gt += [(1, ellipse(w, h, 40, 40, 25, 20)), (2, ellipse(w, h, 110, 60, 30, 25))]
            detect(1, 0.9, 41, 41, 24, 20)
            detect(1, 0.8, 38, 42, 26, 19)
            detect(2, 0.7, 105, 58, 27, 27)
            detect(3, 0.6, 75, 20, 10, 10)
        elif i == 1:    # two ground truths with equal IoU to one detection (identical masks): the first maximum wins
            m = ellipse(w, h, 22, 40, 15, 25)
            gt += [(1, m.copy()), (1, m.copy()), (2, ellipse(w, h, 20, 15, 12, 9))]
            detect(1, 0.85, 22, 41, 14, 24)
            detect(1, 0.55, 22, 40, 15, 25)
            detect(2, 0.65, 24, 18, 12, 9)
        elif i == 2:    # an all-zero prediction against an all-zero ground truth of its class (masklist_iou's break), then a real pair
            gt += [(2, np.zeros((h, w), np.uint8)), (2, ellipse(w, h, 60, 50, 35, 30)), (3, ellipse(w, h, 100, 30, 18, 14))]
            det.append((2, 0.95, np.zeros((nh, nw), np.uint8)))
            detect(2, 0.75, 62, 49, 33, 31)
            detect(1, 0.35, 20, 80, 12, 10)
        elif i == 3:    # down-scaled network; a poor detection that passes only the low thresholds
            gt += [(1, ellipse(w, h, 60, 60, 40, 35)), (2, ellipse(w, h, 150, 50, 30, 40)), (3, ellipse(w, h, 100, 100, 25, 12))]
            detect(1, 0.88, 66, 63, 36, 30)
            detect(2, 0.77, 150, 52, 29, 38)
            detect(2, 0.45, 140, 60, 35, 30)
            detect(1, 0.30, 160, 20, 12, 12)
        elif i == 4:    # identity resize: a pair whose mask IoU is exactly 1 / 2
            two = np.zeros((h, w), np.uint8)
            two[30, 20:22] = 1
            one = np.zeros((nh, nw), np.uint8)
            one[30, 20] = 1
            gt += [(1, two), (2, ellipse(w, h, 45, 35, 18, 20))]
            det.append((1, 0.5, one))
            detect(2, 0.66, 44, 36, 17, 19)
        else:           # no detections at all
            gt += [(1, ellipse(w, h, 50, 50, 30, 30)), (3, ellipse(w, h, 70, 30, 15, 20))]
        images.append({"size": (w, h), "net": (nw, nh), "gt": gt, "det": det})
    return images


class Dataset(object):
    new_classes = NAMES[2:]
    old_classes = NAMES[1:2]

    def __init__(self, gts):
        self.gts = gts

    def get_img_info(self, i):
        return {"width": self.gts[i].size[0], "height": self.gts[i].size[1]}

    def get_groundtruth(self, i):
        return self.gts[i]

    def map_class_id_to_class_name(self, i):
        return NAMES[i]


def main():
    ref_harness.setup()
    import importlib.util     # the package __init__ chain needs torchvision (absent here); the file itself only needs structures/
    spec = importlib.util.spec_from_file_location(
        "ref_voc_eval_inst", os.path.join(ref_harness.REF, "maskrcnn_benchmark/data/datasets/evaluation/voc/voc_eval_inst.py"))
    R = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(R)
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

    images = build_inputs()
    out = {"n_images": np.int64(len(images)), "names": np.array(NAMES), "n_new": np.int64(2), "n_old": np.int64(1)}
    preds, gts = [], []
    for i, im in enumerate(images):
        (w, h), (nw, nh) = im["size"], im["net"]
        gm = np.stack([m for _, m in im["gt"]])
        gb = np.array([box_of(m) for _, m in im["gt"]], np.float32)
        gl = np.array([l for l, _ in im["gt"]], np.int64)
        if im["det"]:
            dm = np.stack([m for _, _, m in im["det"]])
            db = np.array([box_of(m) for _, _, m in im["det"]], np.float32)
        else:
            dm, db = np.zeros((0, nh, nw), np.uint8), np.zeros((0, 4), np.float32)
        dl = np.array([l for l, _, _ in im["det"]], np.int64)
        ds = np.array([s for _, s, _ in im["det"]], np.float32)
        out.update({"size%d" % i: np.array([w, h]), "net%d" % i: np.array([nw, nh]), "gm%d" % i: gm, "gb%d" % i: gb, "gl%d" % i: gl,
                    "dm%d" % i: dm, "db%d" % i: db, "dl%d" % i: dl, "ds%d" % i: ds})
        g = BoxList(torch.from_numpy(gb.copy()), (w, h))
        g.add_field("labels", torch.from_numpy(gl.copy()))
        g.add_field("masks", SegmentationMask(torch.from_numpy(gm.copy()), (w, h), mode="mask"))
        p = BoxList(torch.from_numpy(db.copy()), (nw, nh))
        p.add_field("labels", torch.from_numpy(dl.copy()))
        p.add_field("scores", torch.from_numpy(ds.copy()))
        p.add_field("mask", SegmentationMask(torch.from_numpy(dm.copy()), (nw, nh), mode="mask"))
        preds.append(p)
        gts.append(g)

    # (BinaryMaskList.resize unsqueezes its tensor IN PLACE, segmentation_mask.py:126: a prediction can be resized once, so work on copies)
    resized = [copy.deepcopy(p).resize(g.size) for p, g in zip(preds, gts)]
    half = False
    for i, (p, g) in enumerate(zip(resized, gts)):
        pl, ps, gl = p.get_field("labels").numpy(), p.get_field("scores").numpy(), g.get_field("labels").numpy()
        pm, gm = p.get_field("mask").instances.masks.numpy(), g.get_field("masks").instances.masks.numpy()
        out["rb%d" % i] = p.bbox.numpy().copy()
        for l in np.unique(np.concatenate((pl, gl)).astype(int)):
            sel = pl == l
            order = ps[sel].argsort()[::-1]
            if sel.sum() and (gl == l).sum():
                m = R.masklist_iou(gm[gl == l], pm[sel][order])
                out["miou_%d_%d" % (i, l)] = m
                half |= bool((m == 0.5).any())
    assert half, "no pair with mask IoU exactly 0.5"

    thresholds = np.arange(0.5, 0.95, 0.05).tolist()
    out["thresholds"] = np.array(thresholds)
    K = len(NAMES) - 1
    ap_box, ap_mask = np.zeros((len(thresholds), K)), np.zeros((len(thresholds), K))
    for k, t in enumerate(thresholds):
        prs = R.calc_detection_voc_prec_rec(gt_boxlists=gts, pred_boxlists=resized, iou_thresh=t)
        for tag, lst in zip(("prec", "rec", "mprec", "mrec"), prs):
            out["n_%s_%d" % (tag, k)] = np.int64(len(lst))
            for l, v in enumerate(lst):
                if v is not None:
                    out["%s_%d_%d" % (tag, k, l)] = np.asarray(v, np.float64)
        r = R.eval_detection_voc(pred_boxlists=resized, gt_boxlists=gts, iou_thresh=t, use_07_metric=False)
        ap_box[k], ap_mask[k] = r["ap_box"][1:], r["ap_mask"][1:]
    out["ap_box"], out["ap_mask"] = ap_box, ap_mask
    with tempfile.TemporaryDirectory() as d:
        res = R.do_voc_evaluation_inst(Dataset(gts), preds, d, logging.getLogger("golden"))
        out["result_txt"] = np.array(open(os.path.join(d, "result.txt")).read())
    out["ret_mask"], out["ret_box"] = np.asarray(res["mask"], np.float64), np.array(res["box"])
    assert np.array_equal(out["ret_mask"], ap_mask.mean(axis=0))
    assert len(images[5]["det"]) == 0 and "miou_2_2" in out and out["miou_2_2"][0].max() == 0.0
    assert out["miou_1_1"][0, 0] == out["miou_1_1"][0, 1] > 0.5
    assert not (out["ap_mask"] == out["ap_box"]).all(), "box and mask AP never differ: the fixture does not tell them apart"
    np.savez_compressed(os.path.join(HERE, "mask_eval.npz"), **out)
    print("wrote mask_eval.npz (%d bytes)" % os.path.getsize(os.path.join(HERE, "mask_eval.npz")))
    print("ap_box\n", ap_box, "\nap_mask\n", ap_mask)


if __name__ == "__main__":
    main()

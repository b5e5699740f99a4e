"""Shared by test_mask_eval.py (CPU) and test_gpu_mask_eval.py: tests/golden/mask_eval.npz as BoxLists, a dataset stub, and the fixture's
per-class IoU matrices laid out as the [P,T] matrices the numpy part of voc_eval_inst.py takes."""
import numpy as np
import torch

from abr_iod_amd.structures.bounding_box import BoxList
from abr_iod_amd.structures.segmentation_mask import SegmentationMask


class FakeInstDataset(object):
    def __init__(self, gts, names, n_new, n_old):
        self.gts, self.names = gts, list(names)
        self.new_classes = self.names[1 + n_old:1 + n_old + n_new]
        self.old_classes = self.names[1:1 + n_old]

    def __len__(self):
        return len(self.gts)

    def get_img_info(self, i):
        return {"width": self.gts[i].size[0], "height": self.gts[i].size[1]}

    def get_groundtruth(self, i):
        return self.gts[i]

    def map_class_id_to_class_name(self, i):
        return self.names[i]


def lists(g, device="cpu"):
    """-> (predictions at the network's scale, ground truths at the original size, dataset)"""
    preds, gts = [], []
    for i in range(int(g["n_images"])):
        size, net = tuple(int(v) for v in g["size%d" % i]), tuple(int(v) for v in g["net%d" % i])
        p = BoxList(torch.from_numpy(g["db%d" % i]).to(device), net)
        p.add_field("labels", torch.from_numpy(g["dl%d" % i]).to(device))
        p.add_field("scores", torch.from_numpy(g["ds%d" % i]).to(device))
        p.add_field("mask", SegmentationMask(torch.from_numpy(g["dm%d" % i]).to(device), net))
        t = BoxList(torch.from_numpy(g["gb%d" % i]), size)
        t.add_field("labels", torch.from_numpy(g["gl%d" % i]))
        t.add_field("masks", SegmentationMask(torch.from_numpy(g["gm%d" % i]), size))
        preds.append(p)
        gts.append(t)
    return preds, gts, FakeInstDataset(gts, [str(n) for n in g["names"]], int(g["n_new"]), int(g["n_old"]))


def class_blocks(g, i):
    """image i: [(label, rows in descending score order, columns, the reference's masklist_iou block)]"""
    dl, ds, gl = g["dl%d" % i], g["ds%d" % i], g["gl%d" % i]
    out = []
    for l in np.unique(np.concatenate((dl, gl)).astype(int)):
        key = "miou_%d_%d" % (i, l)
        if key in g.files:
            rows = np.nonzero(dl == l)[0]
            rows = rows[ds[rows].argsort()[::-1]]
            out.append((l, rows, np.nonzero(gl == l)[0], g[key]))
    return out


def reference_mask_iou(g, i):
    """the [P,T] matrix of image i filled from the reference's per-class blocks (pairs of different classes: 0, never looked at)"""
    full = np.zeros((len(g["dl%d" % i]), len(g["gl%d" % i])), np.float64)
    for _l, rows, cols, block in class_blocks(g, i):
        full[np.ix_(rows, cols)] = block
    return full


def check_tables(g, records, atol=1e-12):
    """prec / rec for box and mask at each threshold and both AP tables against the fixture"""
    from abr_iod_amd.data.datasets.evaluation.voc import voc_eval_inst as V
    for k, t in enumerate(g["thresholds"].tolist()):
        assert t == V.IOU_THRESHOLDS[k]
        got = V.calc_detection_voc_prec_rec(records, iou_thresh=t)
        for tag, lst in zip(("prec", "rec", "mprec", "mrec"), got):
            assert len(lst) == int(g["n_%s_%d" % (tag, k)])
            for l, v in enumerate(lst):
                key = "%s_%d_%d" % (tag, k, l)
                assert (v is None) == (key not in g.files), key
                if v is not None:
                    np.testing.assert_allclose(v, g[key], rtol=0, atol=atol, equal_nan=True, err_msg=key)
        r = V.eval_detection_voc(records, iou_thresh=t)
        np.testing.assert_allclose(r["ap_box"][1:], g["ap_box"][k], rtol=0, atol=atol)
        np.testing.assert_allclose(r["ap_mask"][1:], g["ap_mask"][k], rtol=0, atol=atol)
        assert abs(r["map_mask"] - np.nanmean(r["ap_mask"])) < atol and abs(r["map_box"] - np.nanmean(r["ap_box"])) < atol

"""Golden vectors for the mask head from the REFERENCE's own code (run by hand where the reference tree exists; see ref_harness.py):
    mask_defaults.json            MODEL.ROI_MASK_HEAD of config/defaults.py
    mask_state_dict_shapes.json   build_detection_model(MASK_ON).state_dict() names and shapes (duplicate shared-extractor keys included)
    mask_segmentation.npz         SegmentationMask crop / resize / transpose / index, uint8 and float32
    mask_head.npz                 project_masks_on_boxes, MaskRCNNLossComputation, MaskRCNNC4Predictor, MaskPostProcessor, Masker
The files hold data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness  # noqa: E402
from mask_ref import paste_f64  # noqa: E402

W, H = 97, 61
# (x1, y1, x2, y2): corners ending in .5 with even and odd integer parts, boxes outside the image on each side, narrower than a pixel,
# crops smaller and larger than every M
TARGET_BOXES = [
    (10.5, 11.5, 40.5, 41.5), (11.5, 10.5, 41.5, 40.5), (0.5, 1.5, 2.5, 3.5), (12.5, 20.5, 13.5, 21.5),
    (-20.0, 5.0, 30.0, 50.0), (60.0, -15.0, 90.0, 20.0), (70.0, 30.0, 130.0, 58.0), (20.0, 40.0, 50.0, 90.0),
    (-30.0, -30.0, 140.0, 100.0), (30.2, 30.1, 30.6, 45.0), (50.0, 20.3, 80.0, 20.4), (3.0, 3.0, 6.0, 6.0),
    (5.0, 5.0, 9.0, 17.0), (0.0, 0.0, 96.0, 60.0), (1.49, 2.51, 60.5, 33.5), (44.0, 22.0, 44.0, 22.0),
    (96.0, 60.0, 120.0, 80.0), (-10.0, -10.0, 0.4, 0.4), (33.3, 7.7, 64.9, 52.2), (15.0, 15.0, 43.0, 29.0),
]


def _instances(rng, n, dtype):
    ys, xs = np.mgrid[0:H, 0:W]
    out = []
    for i in range(n):
        cx, cy, rx, ry = rng.uniform(15, W - 15), rng.uniform(10, H - 10), rng.uniform(6, 45), rng.uniform(5, 30)
        m = (((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1.0)
        if dtype == np.float32:
            m = m * rng.uniform(0.05, 1.0, size=m.shape)
        out.append(m.astype(dtype))
    return np.stack(out)


def main():
    ref_harness.setup()
    from maskrcnn_benchmark.config import cfg as ref_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.inference import Masker, MaskPostProcessor
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.loss import MaskRCNNLossComputation, project_masks_on_boxes
    from maskrcnn_benchmark.modeling.roi_heads.mask_head.roi_mask_predictors import MaskRCNNC4Predictor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.segmentation_mask import SegmentationMask

    def plain(v):
        return list(v) if isinstance(v, (tuple, list)) else v

    with open(os.path.join(HERE, "mask_defaults.json"), "w") as f:
        json.dump({k: plain(v) for k, v in ref_cfg.MODEL.ROI_MASK_HEAD.items()}, f, indent=1, sort_keys=True)

    cfg = ref_cfg.clone()
    cfg.merge_from_list(["MODEL.MASK_ON", True, "MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21])
    sd = build_detection_model(cfg).state_dict()
    with open(os.path.join(HERE, "mask_state_dict_shapes.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f, indent=1, sort_keys=True)

    rng = np.random.default_rng(7)
    out = {}
    # ---- SegmentationMask API
    seg = {}
    for tag, dt in (("u8", np.uint8), ("f32", np.float32)):
        inst = _instances(rng, 3, dt)
        seg[tag + "_masks"] = inst
        sm = SegmentationMask(torch.from_numpy(inst.copy()), (W, H), mode="mask")
        for i, b in enumerate([(10.5, 11.5, 40.5, 41.5), (-5.0, 3.2, 50.7, 70.0), (30.2, 30.1, 30.6, 45.0)]):
            c = sm.crop(list(b))
            seg["%s_crop%d" % (tag, i)] = c.instances.masks.numpy().copy()
            seg["%s_crop%d_resize" % (tag, i)] = c.resize((14, 9)).instances.masks.numpy().copy()
        seg[tag + "_flip0"] = sm.transpose(0).instances.masks.numpy().copy()
        seg[tag + "_flip1"] = sm.transpose(1).instances.masks.numpy().copy()
        seg[tag + "_index"] = sm[torch.tensor([2, 0])].instances.masks.numpy().copy()
        seg[tag + "_resize"] = SegmentationMask(torch.from_numpy(inst.copy()), (W, H), mode="mask").resize((50, 40)).instances.masks.numpy().copy()
    seg["crop_boxes"] = np.array([(10.5, 11.5, 40.5, 41.5), (-5.0, 3.2, 50.7, 70.0), (30.2, 30.1, 30.6, 45.0)], np.float32)
    np.savez_compressed(os.path.join(HERE, "mask_segmentation.npz"), **seg)

    # ---- mask targets: one instance per box (box i crops instance i)
    boxes = torch.tensor(TARGET_BOXES, dtype=torch.float32)
    out["t_boxes"] = boxes.numpy()
    for tag, dt in (("u8", np.uint8), ("f32", np.float32)):
        inst = _instances(rng, len(TARGET_BOXES), dt)
        out["t_masks_" + tag] = inst
        for M in (8, 14, 28):
            sm = SegmentationMask(torch.from_numpy(inst.copy()), (W, H), mode="mask")
            out["t_%s_M%d" % (tag, M)] = project_masks_on_boxes(sm, BoxList(boxes.clone(), (W, H), "xyxy"), M).numpy()

    # ---- MaskRCNNLossComputation: 2 images, matching through the ROI_HEADS thresholds
    M, K = 14, 6
    ev = MaskRCNNLossComputation(Matcher(0.5, 0.5, allow_low_quality_matches=False), M)
    props, tgts, n_rows = [], [], 0
    for i in range(2):
        gtb = torch.tensor([[8.0, 6.0, 50.0, 40.0], [40.0, 20.0, 90.0, 58.0], [5.0, 35.0, 30.0, 59.0]][: 3 - i], dtype=torch.float32)
        gl = torch.tensor([3, 5, 1][: 3 - i])
        inst = _instances(rng, len(gtb), np.uint8)
        t = BoxList(gtb, (W, H), "xyxy")
        t.add_field("labels", gl)
        t.add_field("masks", SegmentationMask(torch.from_numpy(inst.copy()), (W, H), mode="mask"))
        jit = torch.from_numpy(rng.uniform(-4, 4, size=(4 * len(gtb), 4)).astype(np.float32))
        pb = torch.cat([gtb.repeat(4, 1) + jit, torch.tensor([[60.0, 1.0, 75.0, 9.0], [1.0, 1.0, 9.0, 9.0]])])
        props.append(BoxList(pb, (W, H), "xyxy"))
        tgts.append(t)
        out["l_gt%d" % i], out["l_gtlabels%d" % i], out["l_masks%d" % i], out["l_props%d" % i] = gtb.numpy(), gl.numpy(), inst, pb.numpy()
        n_rows += len(pb)
    labels, mask_targets = ev.prepare_targets(props, tgts)
    pos_props = [p[l > 0] for p, l in zip(props, labels)]      # (ROIMaskHead.forward hands the loss the positives only, mask_head.py:62-77)
    labels = torch.cat(labels)
    n_pos = int((labels > 0).sum())
    logits = torch.from_numpy(rng.standard_normal((n_pos, K, M, M)).astype(np.float32) * 3)
    out["l_labels"], out["l_targets"], out["l_logits"] = labels.numpy(), torch.cat(mask_targets).numpy(), logits.numpy()
    out["l_loss"] = np.float64(ev(pos_props, logits, tgts).double().item())

    # ---- MaskRCNNC4Predictor
    pc = ref_cfg.clone()
    pc.merge_from_list(["MODEL.RESNETS.RES2_OUT_CHANNELS", 8, "MODEL.ROI_MASK_HEAD.CONV_LAYERS", (16, 16, 16, 16), "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 5])
    torch.manual_seed(3)
    pred = MaskRCNNC4Predictor(pc, 64)
    with torch.no_grad():
        pred.conv5_mask.bias.normal_(0, 0.1)
        pred.mask_fcn_logits.bias.normal_(0, 0.1)
        x = torch.randn(6, 64, 4, 4)
        out["p_x"], out["p_logits"] = x.numpy(), pred(x).numpy()
    for k, v in pred.state_dict().items():
        out["p_" + k] = v.numpy()

    # ---- MaskPostProcessor + Masker
    D, M, K = 9, 14, 5
    x = torch.from_numpy(rng.standard_normal((D, K, M, M)).astype(np.float32) * 2)
    pbox = torch.tensor([(10.0, 8.0, 60.0, 50.0), (-12.3, -7.9, 30.5, 25.1), (70.2, 40.7, 110.0, 75.0), (33.0, 20.0, 33.0, 20.0), (5.5, 5.5, 6.4, 30.0),
                         (0.0, 0.0, 96.0, 60.0), (20.7, 30.2, 45.1, 31.0), (80.0, 2.0, 96.9, 20.0), (40.0, 50.0, 70.0, 66.0)], dtype=torch.float32)
    plab = torch.tensor([1, 4, 2, 3, 1, 2, 4, 3, 0])
    b = BoxList(pbox, (W, H), "xyxy")
    b.add_field("labels", plab)
    b.add_field("scores", torch.ones(D))
    with torch.no_grad():
        prob = MaskPostProcessor(None)(x, [b])[0].get_field("mask")
        pasted = MaskPostProcessor(Masker(threshold=0.5, padding=1))(x, [b])[0].get_field("mask")
    out["e_logits"], out["e_boxes"], out["e_labels"], out["e_prob"], out["e_pasted"] = x.numpy(), pbox.numpy(), plab.numpy(), prob.numpy(), pasted.numpy()
    excused = 0
    for d in range(D):
        vals, written = paste_f64(prob[d, 0], pbox[d], H, W)
        near = written & ((vals - 0.5).abs() <= 1e-6)
        excused += int(near.sum())
        want = ((vals > 0.5) & written).to(torch.uint8)
        assert torch.equal(want[~near], pasted[d, 0][~near]), "float64 restatement of paste_mask_in_image differs from the reference (detection %d)" % d
    assert excused <= 1e-3 * D * H * W, "more than 0.1 %% of the fixture's pixels sit within 1e-6 of the threshold (%d)" % excused
    np.savez_compressed(os.path.join(HERE, "mask_head.npz"), **out)
    print("wrote mask goldens; excused paste pixels:", excused)


if __name__ == "__main__":
    main()

"""Golden vectors for the keypoint head from the REFERENCE's own code (run by hand where the reference tree exists; see ref_harness.py):
    keypoint_defaults.json            MODEL.ROI_KEYPOINT_HEAD of config/defaults.py
    keypoint_state_dict_shapes.json   build_detection_model(KEYPOINT_ON, SHARE_BOX_FEATURE_EXTRACTOR False).state_dict() names and shapes
    keypoint_head.npz                 PersonKeypoints resize / transpose / index, keypoints_to_heat_map, KeypointRCNNLossComputation
                                      (prepare_targets' labels and __call__'s loss), KeypointRCNNFeatureExtractor's conv stack and
                                      KeypointRCNNPredictor at small sizes (8 input channels, CONV_LAYERS (16, 16), pooler 6 -> 24, K = 5 and 17;
                                      of the K = 17 logits the first three RoIs are kept, for the file's size)
heatmaps_to_keypoints is not recorded: it needs cv2.  The files hold data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness  # noqa: E402

W, H = 320, 256
GT = [np.array([[10, 10, 50, 60], [100, 20, 180, 90], [200, 200, 260, 250]], np.float32),
      np.array([[30, 30, 90, 120]], np.float32),
      np.array([[5, 5, 45, 45], [60, 60, 61, 100]], np.float32)]
ROIS = np.array([[0, 10, 10, 50, 60], [0, 12, 8, 48, 63], [0, 300, 200, 318, 250], [0, 98, 22, 182, 88], [0, 200, 200, 260, 250],
                 [1, 30, 30, 90, 120], [1, 28, 33, 88, 118], [1, 200, 100, 250, 180],
                 [2, 5, 5, 45, 45], [2, 60, 60, 60, 100], [2, 60, 60, 61, 100], [2, 7, 3, 44, 47], [0, 101, 19, 179, 91],
                 [0, 14, 12, 52, 58], [0, 105, 25, 175, 85], [1, 35, 28, 95, 115], [2, 3, 8, 47, 42], [2, 100, 100, 140, 150],
                 [0, 11, 9, 49.5, 61], [1, 31, 29, 89, 121]], np.float32)


def keypoints_for(gt, K, img):
    """fixed points: on the box corners, inside at fractions, outside, and every fourth one not labelled"""
    n = gt.shape[0]
    kp = np.zeros((n, K, 3), np.float32)
    for j in range(n):
        x1, y1, x2, y2 = gt[j]
        for k in range(K):
            fx, fy = ((7 * k + 3 * j) % 11 + 0.5) / 11, ((5 * k + 2 * j) % 13 + 0.5) / 13
            kp[j, k] = (x1 + fx * (x2 - x1), y1 + fy * (y2 - y1), 2)
        kp[j, 0, :2] = (x1, y1)
        kp[j, 1 % K, :2] = (x2, y2)
        if K > 3:
            kp[j, 3, :2] = (x2 + 5, y1 + 3)          # labelled but outside the box
        for k in range(K):
            if (j + k) % 4 == 3:
                kp[j, k] = 0
    if img == 0:
        kp[2, :, 2] = 0                              # an instance with nothing visible
    if img == 1:
        kp[0, :, :2] += 400                          # every point outside: all of this image's positives are dropped
    return kp


def main():
    ref_harness.setup()
    from maskrcnn_benchmark.config import cfg as ref_cfg
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import make_roi_keypoint_loss_evaluator
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.roi_keypoint_feature_extractors import KeypointRCNNFeatureExtractor
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.roi_keypoint_predictors import KeypointRCNNPredictor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.keypoint import PersonKeypoints, keypoints_to_heat_map

    def plain(v):
        return list(v) if isinstance(v, (tuple, list)) else v

    with open(os.path.join(HERE, "keypoint_defaults.json"), "w") as f:
        json.dump({k: plain(v) for k, v in ref_cfg.MODEL.ROI_KEYPOINT_HEAD.items()}, f, indent=1, sort_keys=True)

    cfg = ref_cfg.clone()
    cfg.merge_from_list(["MODEL.KEYPOINT_ON", True, "MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21,
                         "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 56])
    sd = build_detection_model(cfg).state_dict()
    with open(os.path.join(HERE, "keypoint_state_dict_shapes.json"), "w") as f:
        json.dump({k: list(v.shape) for k, v in sd.items()}, f, indent=1, sort_keys=True)

    out = {"gt_counts": np.array([g.shape[0] for g in GT]), "gt": np.concatenate(GT), "rois": ROIS}
    g = torch.Generator().manual_seed(3)
    # ---- the Keypoints API
    kp17 = PersonKeypoints(torch.from_numpy(keypoints_for(GT[0], 17, 0)), (W, H))
    out["api_in"] = kp17.keypoints.numpy()
    out["api_resize"] = kp17.resize((200, 300)).keypoints.numpy()
    out["api_flip"] = kp17.transpose(0).keypoints.numpy()
    out["api_index"] = kp17[torch.tensor([2, 0])].keypoints.numpy()
    out["flip_inds"] = PersonKeypoints.FLIP_INDS.numpy()
    out["connections"] = np.array(PersonKeypoints.CONNECTIONS)
    for K in (5, 17):
        kps = [keypoints_for(gt, K, i) for i, gt in enumerate(GT)]
        out["kp%d" % K] = np.concatenate(kps)
        cfgk = ref_cfg.clone()
        cfgk.merge_from_list(["MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 24, "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 6,
                              "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", (16, 16), "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", K,
                              "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 64])
        ev = make_roi_keypoint_loss_evaluator(cfgk)
        proposals, targets = [], []
        for i, gt in enumerate(GT):
            t = BoxList(torch.from_numpy(gt), (W, H), mode="xyxy")
            t.add_field("labels", torch.arange(1, gt.shape[0] + 1))
            t.add_field("keypoints", PersonKeypoints(torch.from_numpy(kps[i]), (W, H)))
            targets.append(t)
            proposals.append(BoxList(torch.from_numpy(ROIS[ROIS[:, 0] == i, 1:]), (W, H), mode="xyxy"))
        labels, _ = ev.prepare_targets(proposals, targets)
        out["labels%d" % K] = torch.cat(labels).numpy()          # (in per-image order: images 0, 1, 2)
        kept = ev.subsample(proposals, targets)
        out["kept_boxes%d" % K] = torch.cat([p.bbox for p in kept]).numpy()
        out["kept_counts%d" % K] = np.array([len(p) for p in kept])
        for M in (8, 24, 56):
            hm, va = zip(*[keypoints_to_heat_map(p.get_field("keypoints").keypoints, p.bbox, M) for p in kept if len(p)])
            out["heat%d_M%d" % (K, M)] = torch.cat(hm).numpy()
            out["valid%d_M%d" % (K, M)] = torch.cat(va).numpy()
        # ---- the head behind the pooler
        ext = KeypointRCNNFeatureExtractor(cfgk, 8)
        pred = KeypointRCNNPredictor(cfgk, 16)
        with torch.no_grad():
            for p in list(ext.parameters()) + list(pred.parameters()):
                if p.dim() == 1:
                    p.normal_(0.0, 0.1, generator=g)
        P = sum(len(p) for p in kept)
        pooled = torch.randn(P, 8, 6, 6, generator=g)
        x = pooled
        for name in ext.blocks:
            x = torch.relu(getattr(ext, name)(x))
        logits = pred(x)
        loss = ev(kept, logits)
        grads = torch.autograd.grad(loss, list(ext.parameters()) + list(pred.parameters()))
        out["pooled%d" % K], out["features%d" % K], out["logits%d" % K] = pooled.numpy(), x.detach().numpy(), logits.detach().numpy()[:12 if K == 5 else 3]
        out["loss%d" % K] = np.array(loss.item())
        names = [n for n, _ in ext.named_parameters()] + ["predictor." + n for n, _ in pred.named_parameters()]
        for n, p, gr in zip(names, list(ext.parameters()) + list(pred.parameters()), grads):
            out["param%d.%s" % (K, n)], out["grad%d.%s" % (K, n)] = p.detach().numpy(), gr.numpy()
    np.savez_compressed(os.path.join(HERE, "keypoint_head.npz"), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == "__main__":
    main()

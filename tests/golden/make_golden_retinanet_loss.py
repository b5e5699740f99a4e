#!/usr/bin/env python3
"""RetinaNet loss golden FROM THE REFERENCE (in-container only; see ref_harness.py): the reference's own RetinaNetLossComputation
(rpn/retinanet/loss.py over rpn/loss.py, Matcher, BoxCoder, concat_box_prediction_layers, smooth_l1_loss, sigmoid_focal_loss_cpu) run on the
CPU at tests/retinanet_ref.py's tiny pyramid -- MAPS, A = 9, C = 4, two images -- on the inputs of retinanet_loss_ref.golden_inputs(seed).

    retinanet_loss.npz   results only (the inputs come back from the seed):
      seed; labels int8 [N, n]; pos [P, 2] (image, anchor) of the labels > 0 and targets [P, 4] there; losses [2] = (cls, reg);
      per level l: idx_cls_l / idx_reg_l (retinanet_loss_ref.golden_sample's flat entries of the level's [N, nloc, A*C] / [N, nloc, 4A] output)
      and grad_cls_l / grad_reg_l, autograd's gradient of cls + reg there; grad_cls_pos [P, C] / grad_reg_pos [P, 4] at the positives.
    The seed is advanced until retinanet_loss_ref.golden_conditions holds.

Two lines of this fork's loss do not run as written, and the harness steps around them without touching the arithmetic: its
RPNLossComputation.prepare_targets returns four lists where RetinaNetLossComputation.__call__ unpacks two (the subclass below drops the last
two), and sigmoid_focal_loss_cpu indexes gamma[0] / alpha[0] (they are passed as one-element tuples)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import retinanet_loss_ref as RL  # noqa: E402
import retinanet_ref as R  # noqa: E402

SAMPLE = 96


class _Images(object):
    image_sizes = R.IMAGE_SIZES


def main():
    rh.setup()
    ref_cfg = rh.default_cfg()
    from maskrcnn_benchmark.layers import SigmoidFocalLoss
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.rpn.anchor_generator import make_anchor_generator_retinanet
    from maskrcnn_benchmark.modeling.rpn.retinanet.loss import RetinaNetLossComputation, generate_retinanet_labels
    from maskrcnn_benchmark.structures.bounding_box import BoxList

    class Loss(RetinaNetLossComputation):
        def prepare_targets(self, anchors, targets):
            return super().prepare_targets(anchors, targets)[:2]

    cfg = ref_cfg.clone()
    cfg.merge_from_list(["MODEL.RETINANET.ANCHOR_SIZES", R.SIZES, "MODEL.RETINANET.ANCHOR_STRIDES", R.STRIDES, "MODEL.RETINANET.ASPECT_RATIOS", R.RATIOS,
                         "MODEL.RETINANET.NUM_CLASSES", R.C + 1])
    r = cfg.MODEL.RETINANET
    assert (r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, r.LOSS_GAMMA, r.LOSS_ALPHA, r.BBOX_REG_BETA, r.BBOX_REG_WEIGHT) == \
        (RL.HI, RL.LO, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)
    N = len(R.IMAGE_SIZES)
    ag = make_anchor_generator_retinanet(cfg)
    anchors = ag(_Images(), [torch.zeros(N, 1, H, W) for H, W in R.MAPS])
    grids = [anchors[0][l].bbox.numpy() for l in range(len(R.MAPS))]
    for seed in range(4100, 4400):
        gt_boxes, gt_labels, cls_code, reg_code = RL.golden_inputs(seed)
        bad, tg = RL.golden_conditions(grids, gt_boxes, gt_labels)
        if not bad:
            break
        print("seed", seed, bad)
    else:
        raise RuntimeError("no seed meets the golden's conditions")
    cls, reg = RL.golden_arrays(cls_code, reg_code)
    box_cls = [torch.from_numpy(np.ascontiguousarray(c.reshape(N, H, W, R.A * R.C).transpose(0, 3, 1, 2))).requires_grad_(True)
               for c, (H, W) in zip(cls, R.MAPS)]
    box_reg = [torch.from_numpy(np.ascontiguousarray(d.reshape(N, H, W, R.A * 4).transpose(0, 3, 1, 2))).requires_grad_(True)
               for d, (H, W) in zip(reg, R.MAPS)]
    targets = []
    for i, (h, w) in enumerate(R.IMAGE_SIZES):
        t = BoxList(torch.from_numpy(gt_boxes[i]), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(gt_labels[i]))
        targets.append(t)
    ev = Loss(Matcher(r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, allow_low_quality_matches=True), BoxCoder(weights=R.WEIGHTS),
              generate_retinanet_labels, SigmoidFocalLoss((r.LOSS_GAMMA,), (r.LOSS_ALPHA,)), bbox_reg_beta=r.BBOX_REG_BETA,
              regress_norm=r.BBOX_REG_WEIGHT)
    # the labels and targets the loss draws, through the same call
    from maskrcnn_benchmark.structures.boxlist_ops import cat_boxlist
    labels, reg_targets = ev.prepare_targets([cat_boxlist(a) for a in anchors], targets)
    labels = torch.stack(labels).numpy()
    reg_targets = torch.stack(reg_targets).numpy()
    loss_cls, loss_reg = ev(anchors, box_cls, box_reg, targets)
    (loss_cls + loss_reg).backward()
    out = dict(seed=np.int64(seed), labels=labels.astype(np.int8), losses=np.array([loss_cls.item(), loss_reg.item()], np.float32))
    assert np.array_equal(out["labels"].astype(np.float32), labels)
    pos = np.argwhere(labels > 0)
    out["pos"] = pos.astype(np.int32)
    out["targets"] = reg_targets[pos[:, 0], pos[:, 1]].astype(np.float32)
    gc, gr = [], []
    for l, (H, W) in enumerate(R.MAPS):
        g_cls = box_cls[l].grad.permute(0, 2, 3, 1).reshape(N, H * W, R.A * R.C).numpy()
        g_reg = box_reg[l].grad.permute(0, 2, 3, 1).reshape(N, H * W, R.A * 4).numpy()
        for name, g in (("cls", g_cls), ("reg", g_reg)):
            idx = RL.golden_sample(g.size, SAMPLE, 100 + l)
            out["idx_%s_%d" % (name, l)] = idx.astype(np.int32)
            out["grad_%s_%d" % (name, l)] = g.reshape(-1)[idx].astype(np.float32)
        gc.append(g_cls.reshape(N, H * W * R.A, R.C))
        gr.append(g_reg.reshape(N, H * W * R.A, 4))
    gc, gr = np.concatenate(gc, 1), np.concatenate(gr, 1)
    out["grad_cls_pos"] = gc[pos[:, 0], pos[:, 1]].astype(np.float32)
    out["grad_reg_pos"] = gr[pos[:, 0], pos[:, 1]].astype(np.float32)
    path = os.path.join(HERE, "retinanet_loss.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "positives", len(pos), "ignored", int((labels < 0).sum()), "losses", out["losses"], "bytes", os.path.getsize(path),
          "retinanet.npz", os.path.getsize(os.path.join(HERE, "retinanet.npz")))
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "retinanet.npz"))


if __name__ == "__main__":
    main()

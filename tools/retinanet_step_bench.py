"""First measurements of RetinaNet's training half (modeling/rpn/retinanet.py, csrc/retinanet_loss.hip) at R-50-FPN-RETINANET shapes: an
800 x 1344 image, B = 2, P3..P7 of 256 channels (100 x 168 down to 7 x 11), A = 9 anchors per location, 80 foreground classes, NUM_CONVS 4.

  (a) the anchor targets of the whole batch: ops.retina_targets over the 201 600 concatenated anchors (two launches), synthetic boxes;
  (b) the loss alone on head-shaped tensors: ops.retina_loss (one read of the ~32 M logits) and ops.retina_loss_backward (one read, one
      write): us per call, GB/s of the bytes each must move, and that as a fraction of the 8.0 TB/s HBM peak;
  (c) the head alone: RetinaNetHead.forward_train over the five levels and its backward (output gradients of the loss's shape);
  (d) one training step of the whole detector (forward, backward, FusedSGD.step) in the default arithmetic.

Device events around --reps back-to-back calls.  Nothing here is a threshold.  Prints the tables, then one JSON line.

    python tools/retinanet_step_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IMG_H, IMG_W, C, A, CLASSES = 2, 800, 1344, 256, 9, 81
MAPS = ((100, 168), (50, 84), (25, 42), (13, 21), (7, 11))
HBM_PEAK = 8.0e12
RETINA_CFG = ["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", "R-50-FPN-RETINANET", "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", C,
              "MODEL.RETINANET.NUM_CLASSES", CLASSES]


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3   # us


def _batch():
    from abr_iod_amd.engine.synthetic import synthetic_batch
    from abr_iod_amd.structures.image_list import ImageList
    images, targets = synthetic_batch(B, IMG_H, IMG_W, seed=5, label_range=(1, CLASSES))
    return ImageList(images, [(IMG_H, IMG_W)] * B), targets


def _anchors(cfg):
    from abr_iod_amd.modeling.rpn.retinanet import make_anchor_generator_retinanet

    class Images(object):
        image_sizes = [(IMG_H, IMG_W)] * B
    gen = make_anchor_generator_retinanet(cfg).cuda()
    return gen(Images(), [torch.zeros(B, 1, h, w, device="cuda") for h, w in MAPS])


def targets_row(cfg, targets, reps):
    from abr_iod_amd import ops
    anchors = _anchors(cfg)
    boxes = torch.cat([a.bbox for a in anchors[0]]).contiguous()
    gtb, gtl = [t.bbox for t in targets], [t.get_field("labels") for t in targets]
    out = ops.retina_targets(boxes, gtb, gtl, 0.5, 0.4)
    us = timed(lambda: ops.retina_targets(boxes, gtb, gtl, 0.5, 0.4), reps)
    return {"anchors_per_image": int(boxes.shape[0]), "gt_per_image": [int(b.shape[0]) for b in gtb], "n_pos": int(out[2].item()), "us": round(us, 1)}, out


def loss_rows(tg, reps):
    from abr_iod_amd import ops
    labels, reg_targets, n_pos = tg
    g = torch.Generator(device="cuda").manual_seed(2)
    n_cls = A * (CLASSES - 1)
    cls = [torch.randn(B, h, w, n_cls, device="cuda", generator=g) * 2 - 4 for h, w in MAPS]
    reg = [torch.randn(B, h, w, 4 * A, device="cuda", generator=g) * 0.5 for h, w in MAPS]
    one = torch.ones(1, device="cuda")
    nums = (A, CLASSES - 1, labels, reg_targets, n_pos, 2.0, 0.25, 0.11, 4.0)
    bufs = (torch.empty(sum(c.numel() for c in cls), device="cuda"), torch.empty(sum(r.numel() for r in reg), device="cuda"))
    logits, deltas = sum(c.numel() for c in cls), sum(r.numel() for r in reg)
    side = labels.numel() * 4                                                  # the labels; the targets are read at the positives only
    rows = []
    for name, fn, nbytes in (("retina_loss", lambda: ops.retina_loss(cls, reg, *nums), 4 * (logits + deltas) + side),
                             ("retina_loss_backward", lambda: ops.retina_loss_backward(cls, reg, *nums, one, one, out=bufs),
                              8 * (logits + deltas) + side)):
        us = timed(fn, reps)
        rows.append({"op": name, "logits": logits, "us": round(us, 1), "GBps": round(nbytes / us / 1e3, 1),
                     "hbm_peak_fraction": round(nbytes / (us * 1e-6) / HBM_PEAK, 3)})
    return rows


def head_rows(cfg, reps):
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetHead
    math = {"f32": ops.MATH_F32, "bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3}[ops.DEFAULT_CONV_MATH]
    head = RetinaNetHead(cfg, C).cuda()
    set_conv_math(head, math)
    g = torch.Generator(device="cuda").manual_seed(3)
    feats = [torch.randn(B, h, w, C, device="cuda", generator=g).clamp_(min=0).permute(0, 3, 1, 2).requires_grad_(True) for h, w in MAPS]
    gouts = None

    def fwd():
        return head.forward_train(feats)

    def fwd_bwd():
        cls, reg = fwd()
        torch.autograd.backward(cls + reg, gouts)
        ops.join_side_stream()

    cls, reg = fwd()
    gouts = [torch.randn_like(t) * 1e-3 for t in cls + reg]
    f = timed(fwd, reps)
    fb = timed(fwd_bwd, reps)
    return [{"op": "head forward (5 levels)", "math": ops.DEFAULT_CONV_MATH, "us": round(f, 1)},
            {"op": "head backward (5 levels)", "math": ops.DEFAULT_CONV_MATH, "us": round(fb - f, 1)}]


def step_row(cfg, batch, reps):
    from abr_iod_amd.engine.synthetic import build_models
    from abr_iod_amd.solver.build import FusedSGD
    _, model = build_models(None, cfg, seed=0, need_source=False)
    opt = FusedSGD(model, 0.002, 0.9, 1e-4, 2.0, 0.0)
    images, targets = batch
    model.train()
    last = {}

    def step():
        opt.zero_grad()
        losses = model(images, targets)[0]
        sum(losses.values()).backward()
        opt.step()
        last.update(losses)

    for _ in range(3):
        step()
    us = timed(step, reps)
    return {"ms_per_step": round(us / 1e3, 3), "conv_math": model.conv_math, "losses": {k: round(float(v), 4) for k, v in last.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--skip-step", action="store_true", help="leave out (d), the whole detector's training step")
    a = ap.parse_args()
    from abr_iod_amd.engine.synthetic import make_cfgs
    torch.cuda.set_device(0)
    cfg = make_cfgs("15-5", overrides=RETINA_CFG)[1]
    batch = _batch()
    out = {"shape": {"B": B, "image": [IMG_H, IMG_W], "maps": [list(m) for m in MAPS], "C": C, "A": A, "classes": CLASSES - 1}}
    out["targets"], tg = targets_row(cfg, batch[1], a.reps)
    print("(a) anchor targets: %(anchors_per_image)d anchors per image, ground truths %(gt_per_image)s, %(n_pos)d positives: %(us).1f us" % out["targets"])
    out["loss"] = loss_rows(tg, a.reps)
    print("(b) the loss alone, %d logits" % out["loss"][0]["logits"])
    for r in out["loss"]:
        print("    %-22s %9.1f us  %8.1f GB/s  %.3f of the HBM peak" % (r["op"], r["us"], r["GBps"], r["hbm_peak_fraction"]))
    out["head"] = head_rows(cfg, max(a.reps // 2, 3))
    print("(c) the head alone, %d channels, NUM_CONVS %d" % (C, cfg.MODEL.RETINANET.NUM_CONVS))
    for r in out["head"]:
        print("    %-26s %-6s %10.1f us" % (r["op"], r["math"], r["us"]))
    if not a.skip_step:
        out["step"] = step_row(cfg, batch, max(a.reps // 2, 3))
        print("(d) R-50-FPN-RETINANET training step: %(ms_per_step).3f ms (%(conv_math)s), losses %(losses)s" % out["step"])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()

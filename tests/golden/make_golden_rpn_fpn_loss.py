#!/usr/bin/env python3
"""Multi-level RPN loss golden FROM THE REFERENCE (in-container only): the reference's own modeling/rpn/anchor_generator.py `AnchorGenerator`,
modeling/rpn/loss.py `RPNLossComputation` (cat_boxlist over the levels, concat_box_prediction_layers), `Matcher`, `BoxCoder` and
`BalancedPositiveNegativeSampler` run on the CPU over the pyramid of tests/rpn_fpn_ref.py: N = 2, images 128 x 192 and 112 x 160, strides
4 .. 64, sizes 32 .. 512, maps 32 x 48 down to 2 x 3, A = 3, n = 6138 anchors per image.  The head outputs are those of tests/golden/rpn_fpn.npz
(exact fp32 codes: logit = int16 / 1024, delta = int8 / 16), so both sides read identical inputs; its seed is stored and compared.

Two cases: STRADDLE_THRESH = -1 (every anchor visible, all five levels take part) and 0 (no anchor of levels 2-4 lies inside these images).
The ground truth spans the levels' anchor sizes (sides of about 32 .. 512, the large ones reaching outside the image: the loss never clips),
every box shifted by (+0.3, +0.6, +0.1, +0.7) so that no IoU is a ratio of small integers.

The generator aborts unless: in the -1 case every level holds a sampled positive in the batch and the sampled negatives come from at least
three levels (in the 0 case only levels 0 and 1 have a visible anchor, so neither can hold there); no anchor's best IoU lies within 1e-5 of
0.3 or 0.7; at least one ground truth's low-quality match lies on another level than a matcher run level by level would promote; the
reference's fp32 losses lie within rpn_fpn_loss_ref.TOL x addends of the float64 restatement.

The sampler's draw is the reference's own (torch.manual_seed(SEED)), recorded by wrapping the sampler object.

Stored as tests/golden/rpn_fpn_loss.npz (data only): seed_rpn_fpn, gt_i, matched int8 [N, n] (Matcher output; the same for both cases), and per
case c in (m1, 0): labels_c int8 [N, n], pos_c / neg_c int64 (the draw, flat batch indices), loss_objectness_c, loss_rpn_box_reg_c, d_obj_c (the
gradient of the sum of both losses at the sampled logits, in the order pos_c then neg_c) and d_reg_c [#pos, 4]; pos_all int64 (the anchors labelled
positive in the -1 case) with their fp32 regression targets tgt_pos_all.  The reference's gradient is zero everywhere else (asserted here)."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import rpn_fpn_loss_ref as LR  # noqa: E402
import rpn_fpn_ref as F  # noqa: E402

SHIFT = np.array([0.3, 0.6, 0.1, 0.7], np.float32)
GT = [np.array([[100, 64, 131, 95], [60, 20, 123, 83], [30, 0, 157, 127], [-32, -64, 223, 191], [-160, -192, 351, 319]], np.float32) + SHIFT,
      np.array([[20, 40, 51, 71], [90, 10, 153, 73], [-40, -60, 215, 195], [-180, -200, 331, 311]], np.float32) + SHIFT]
SEED = 20251
BATCH, FRACTION, HI, LO = 256, 0.5, 0.7, 0.3
CASES = (("m1", -1), ("0", 0))


class _Images(object):
    image_sizes = F.IMAGE_SIZES


class _Recorder(object):
    """wraps the reference's sampler: same call, the draw kept"""

    def __init__(self, sampler):
        self.sampler, self.pos, self.neg = sampler, None, None

    def __call__(self, *a, **k):
        self.pos, self.neg = self.sampler(*a, **k)
        return self.pos, self.neg


def flat_order(t, A):
    """[N, A*k, H, W] gradient or prediction -> [N, H*W*A, k] (permute_and_flatten, rpn/utils.py:10-14)"""
    t = t.detach().numpy()
    N, C, H, W = t.shape
    return t.reshape(N, A, C // A, H, W).transpose(0, 3, 4, 1, 2).reshape(N, H * W * A, C // A)


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
    from maskrcnn_benchmark.modeling.box_coder import BoxCoder
    from maskrcnn_benchmark.modeling.matcher import Matcher
    from maskrcnn_benchmark.modeling.rpn.anchor_generator import AnchorGenerator
    from maskrcnn_benchmark.modeling.rpn.loss import RPNLossComputation, generate_rpn_labels
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.boxlist_ops import cat_boxlist
    N, A, nL = len(F.IMAGE_SIZES), len(F.RATIOS), len(F.MAPS)
    fpn = np.load(os.path.join(HERE, "rpn_fpn.npz"))
    obj_code, reg_code = [fpn["obj_%d" % l] for l in range(nL)], [fpn["reg_%d" % l] for l in range(nL)]
    ys = F.golden_fused(obj_code, reg_code)
    offs = LR.level_offsets([H * W for H, W in F.MAPS], A)
    n = int(offs[-1])
    out = dict(seed_rpn_fpn=fpn["seed"])
    for i, g in enumerate(GT):
        out["gt_%d" % i] = g
    targets = [BoxList(torch.from_numpy(g.copy()), (w, h), mode="xyxy") for g, (h, w) in zip(GT, F.IMAGE_SIZES)]
    feats = [torch.zeros(N, 1, H, W) for H, W in F.MAPS]
    for tag, straddle in CASES:
        ag = AnchorGenerator(sizes=F.SIZES, aspect_ratios=F.RATIOS, anchor_strides=F.STRIDES, straddle_thresh=straddle)
        anchors = ag(_Images(), feats)
        for per_image in anchors:    # STRADDLE_THRESH < 0 gives a uint8 mask of ones (anchor_generator.py:103), a boolean mask in the torch the
            for b in per_image:      # reference was written for; today's torch takes `~mask` of a uint8 as arithmetic: hand it the same mask as bool
                b.add_field("visibility", b.get_field("visibility").bool())
        cat = [cat_boxlist(a) for a in anchors]
        boxes = cat[0].bbox.numpy()
        assert boxes.shape == (n, 4) and np.array_equal(boxes, np.concatenate([fpn["anchors_%d" % l] for l in range(nL)])), "concatenation order"
        rec = _Recorder(BalancedPositiveNegativeSampler(BATCH, FRACTION))
        ev = RPNLossComputation(Matcher(HI, LO, allow_low_quality_matches=True), rec, BoxCoder((1.0, 1.0, 1.0, 1.0)), generate_rpn_labels)
        labels, reg_t, _, matched = ev.prepare_targets(cat, targets)
        objectness, regression = [], []
        for (H, W), y in zip(F.MAPS, ys):
            nchw = torch.from_numpy(np.ascontiguousarray(y.reshape(N, H, W, 5 * A).transpose(0, 3, 1, 2)))
            objectness.append(nchw[:, :A].clone().requires_grad_(True))
            regression.append(nchw[:, A:].clone().requires_grad_(True))
        torch.manual_seed(SEED)
        lo, lb = ev(anchors, objectness, regression, targets)
        (lo + lb).backward()
        pos = torch.nonzero(torch.cat(rec.pos)).squeeze(1).numpy().astype(np.int64)
        neg = torch.nonzero(torch.cat(rec.neg)).squeeze(1).numpy().astype(np.int64)
        samp = np.concatenate([pos, neg])
        lab = torch.stack(labels).numpy()
        tgt = torch.stack(reg_t).numpy()
        mat = torch.stack(matched).numpy()
        # ---- the restatement agrees before anything is stored
        glob_differs = False
        for i in range(N):
            vis = cat[i].get_field("visibility").numpy()
            r = LR.prepare_targets(boxes, vis, GT[i], HI, LO)
            assert np.array_equal(r["matches"], mat[i]) and np.array_equal(r["labels"], lab[i]), "restatement vs reference: matching"
            assert np.all(np.abs(r["best"] - LO) > 1e-5) and np.all(np.abs(r["best"] - HI) > 1e-5), "a best IoU within 1e-5 of a threshold: nudge the GT"
            assert np.all(np.abs(tgt[i] - r["targets"]) <= r["target_bound"]), "restatement vs reference: regression targets"
            glob, local = LR.per_level_low_quality(r["iou"], offs)
            for g in range(len(GT[i])):      # a level-by-level matcher would promote an anchor the matcher over all levels leaves unmatched
                for l, at in local[g].items():
                    if l not in glob[g] and np.any(mat[i][at] != g):
                        glob_differs = True
        assert glob_differs, "no ground truth whose low-quality match depends on matching across the levels"
        il, ll, _, _ = LR.decode_index(pos, n, offs, A)
        pos_levels = [np.bincount(ll[il == i], minlength=nL).tolist() for i in range(N)]
        neg_levels = np.bincount(LR.decode_index(neg, n, offs, A)[1], minlength=nL)
        print(tag, "labelled positives per image and level", [np.bincount(np.searchsorted(offs, np.nonzero(lab[i] == 1)[0], side="right") - 1,
                                                                         minlength=nL).tolist() for i in range(N)])
        print(tag, "sampled positives per image and level", pos_levels, "sampled negatives per level", neg_levels.tolist())
        if straddle < 0:
            assert all(sum(p[l] for p in pos_levels) > 0 for l in range(nL)), "a level without a sampled positive"
            assert (neg_levels > 0).sum() >= 3, "sampled negatives from fewer than three levels"
            out["pos_all"] = np.nonzero(lab.reshape(-1) == 1)[0].astype(np.int64)
            out["tgt_pos_all"] = tgt.reshape(-1, 4)[out["pos_all"]]
            out["matched"] = mat.astype(np.int8)
        else:
            assert np.array_equal(out["matched"], mat.astype(np.int8)), "the matcher does not see the visibility"
        ref = LR.losses(ys, A, lab, tgt, pos, samp)
        LR.check_losses(lo.item(), lb.item(), ref, "reference fp32 vs float64 restatement, case " + tag)
        d_obj = np.concatenate([flat_order(o.grad, A) for o in objectness], 1).reshape(N * n)
        d_reg = np.concatenate([flat_order(r.grad, A) for r in regression], 1).reshape(N * n, 4)
        mask = np.zeros(N * n, bool)
        mask[samp] = True
        assert np.all(d_obj[~mask] == 0), "reference gradient outside the sampled logits"
        mask[:] = False
        mask[pos] = True
        assert np.all(d_reg[~mask] == 0), "reference gradient outside the sampled positives' deltas"
        out.update({"labels_" + tag: lab.astype(np.int8), "pos_" + tag: pos, "neg_" + tag: neg,
                    "loss_objectness_" + tag: np.float32(lo.item()), "loss_rpn_box_reg_" + tag: np.float32(lb.item()),
                    "d_obj_" + tag: d_obj[samp].astype(np.float32), "d_reg_" + tag: d_reg[pos].astype(np.float32)})
        print(tag, "losses", lo.item(), lb.item(), "float64", ref["obj"], ref["box"], "#pos", len(pos), "#neg", len(neg))
    path = os.path.join(HERE, "rpn_fpn_loss.npz")
    np.savez_compressed(path, **out)
    print("bytes", os.path.getsize(path), "(rpn_fpn.npz:", os.path.getsize(os.path.join(HERE, "rpn_fpn.npz")), ")")
    assert os.path.getsize(path) <= os.path.getsize(os.path.join(HERE, "rpn_fpn.npz"))


if __name__ == "__main__":
    main()

"""GPU: the whole R-50-FPN detector (tiny widths, configuration "15-5": ID + ARD over the 64 soften proposals per image) against the float64
model tests/detector_fpn_ref.py on IDENTICAL weights, images and sampler draws, in the three fp32-accurate arithmetics.

  * test_fpn_train_step_losses_and_grads_vs_float64: the trainer's sequence; the GPU's own draws are read back and fed to the float64 model.
    Exact: anchor labels (rpn_fpn_loss_ref.prepare_targets), box-head labels (oracle.ops.matcher), RoI levels (pooler_ref.levels).  Values:
    P2..P6 and the RPN outputs within 1e-4 of max |ref|, the six losses and the total within 1e-4 max(1, |ref|), the gradient of each of the 72
    trainable tensors within e2e_fpn_common.GRAD_MAX_REL / GRAD_REL_L2.
  * test_fpn_reference_draws_reproduce_reference_losses: the draws of tests/golden/e2e_fpn_tiny.npz (the reference's own run) injected.
  * test_fpn_step_then_forward_follows_the_weights: one FusedSGD step, then the same comparison on the weights after the step.
  * test_fpn_eval_detections_vs_float64: eval mode; the GPU's proposals through the float64 box head and float64 post-processing.

What the pieces' own tests cannot see and these can: the RPN's and the pooler's gradients summed into P2..P5, P6's gradient returning into P5,
the top-down path, three RoI passes adding into the same maps, the level / image order of the concatenated RPN predictions, which tensors
train, and derived weight copies after a step (tests/test_detector_fpn_ref.py shows the inputs react to each)."""
import os
import random

import numpy as np
import pytest
import torch

import box_head_fpn_ref as HR
import detector_fpn_ref as D
import e2e_fpn_common as E
import pooler_ref as P
import rpn_fpn_loss_ref as LR
from detect_ref import softmax_decode_f64

pytestmark = pytest.mark.gpu

MATHS = ("bf16x6", "f16x3", "f32")
N_TRAINABLE = len(D.trainable_keys(E.shapes_json()["shapes"]))      # 72, from the reference's own key list


def N(t):
    return t.detach().cpu().numpy()


def _close(a, b, tol=1e-4):
    return abs(a - b) <= tol * max(1.0, abs(b))


def _near(got, want, what):
    want = np.asarray(want, np.float64)
    err, lim = float(np.abs(np.asarray(got, np.float64) - want).max()), 1e-4 * float(np.abs(want).max())
    print("%-28s err %.3e  limit %.3e" % (what, err, lim))
    assert err <= lim, (what, err, lim)


@pytest.fixture(scope="module", params=MATHS)
def S(request):
    from abr_iod_amd import ops
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import ImageList
    math = request.param
    os.environ["ABR_CONV_MATH"] = math
    try:
        cfg_s, cfg_t, ms, mt, sd_s, sd_t = E.build("cuda")
    finally:
        os.environ.pop("ABR_CONV_MATH", None)   # read at model construction only
    want = {"bf16x6": ops.MATH_BF16X6, "f16x3": ops.MATH_F16X3, "f32": ops.MATH_F32}[math]
    assert all(m.math == want for m in mt.modules() if hasattr(m, "math"))
    cpu_images = E.make_images()
    images = ImageList(cpu_images.cuda(), [tuple(s) for s in E.IMAGE_SIZES])
    gts, gt_labels = E.gt_arrays()
    targets = []
    for (h, w), b, l in zip(E.IMAGE_SIZES, gts, gt_labels):
        t = BoxList(torch.from_numpy(b).cuda(), (w, h), mode="xyxy")
        t.add_field("labels", torch.from_numpy(l).cuda())
        targets.append(t)
    return dict(math=math, cfg=cfg_t, ms=ms, mt=mt, sd_s=sd_s, sd_t=sd_t, images=images, cpu_images=cpu_images, targets=targets, gts=gts,
                gt_labels=gt_labels)


def _gpu_step(S):
    """the trainer's sequence (train_incremental.py:82-128) -> what the comparison needs, everything read back"""
    from abr_iod_amd.distillation.distillation import calculate_attentive_roi_feature_distillation, calculate_roi_distillation_losses
    ms, mt, images, targets, cfg = S["ms"], S["mt"], S["images"], S["targets"], S["cfg"]
    mt.train()
    mt.flat.zero_grad()
    torch.manual_seed(7)      # the samplers' draws and the 64 soften picks: the same in every run, so the measured bounds describe THIS case
    random.seed(7)
    with torch.no_grad():
        soften_result, _, soften_proposal, _, _, _, _, raf_s = ms.generate_soften_proposal(images)
    loss_dict, feats, _, anchors, rpn_out, props, _, _ = mt(images, targets)
    target_result, _, raf_t = mt.forward(images, targets, features=feats, proposals=soften_proposal)
    l_id = calculate_roi_distillation_losses(soften_result, target_result, dist=cfg.DIST.TYPE)
    l_ard = calculate_attentive_roi_feature_distillation(raf_s, raf_t, gamma=cfg.DIST.GAMMA)
    total = sum(loss_dict.values()) + cfg.DIST.ALPHA * l_id + cfg.DIST.BETA * l_ard
    total.backward()
    torch.cuda.synchronize()
    losses = {k: float(v) for k, v in loss_dict.items()}
    losses["id"], losses["ard"] = float(l_id), float(l_ard)
    ev, evb = mt.rpn.loss_evaluator, mt.roi_heads.box.loss_evaluator
    det = evb._proposals
    n_cand = [len(p) for p in evb.last_input_proposals]      # the post-NMS + GT lists the sampler drew from
    det_rois = np.concatenate([np.concatenate([np.full((len(p), 1), i, np.float32), N(p.bbox)], 1) for i, p in enumerate(det)])
    soft_rois = np.concatenate([np.concatenate([np.full((len(p), 1), i, np.float32), N(p.bbox)], 1) for i, p in enumerate(soften_proposal)])
    fe = mt.roi_heads.box.feature_extractor
    return dict(losses=losses, total=float(total), feats=[N(f) for f in feats], objs=[N(o) for o in rpn_out[0]], regs=[N(r) for r in rpn_out[1]],
                anchors=[[(N(a.bbox), N(a.get_field("visibility")).astype(bool)) for a in per] for per in anchors],
                rpn_labels=np.stack([N(l) for l in ev.last_targets[0]]), rpn_targets=np.stack([N(t) for t in ev.last_targets[1]]),
                pos_idx=N(ev.last_sampled[0]), samp_idx=N(ev.last_sampled[1]), det_rois=det_rois,
                det_labels=np.concatenate([N(p.get_field("labels")) for p in det]).astype(np.int64),
                det_reg_targets=np.concatenate([N(p.get_field("regression_targets")) for p in det]), soft_rois=soft_rois,
                det_levels=N(fe.pooler.map_levels(torch.from_numpy(det_rois).cuda())), soft_levels=N(fe.pooler.map_levels(torch.from_numpy(soft_rois).cuda())),
                n_soft=[len(p) for p in soften_proposal], n_cand=n_cand, picks=ms.last_soften_indices)


def _gpu_grads(mt, ref_grads):
    """{reference key: the GPU's gradient in the reference's layout}: OHWI -> OIHW for conv weights, fc6 through fc6_from_ohwi"""
    from abr_iod_amd.modeling.backbone.resnet import Conv2d
    convs = {id(m.weight): m for m in mt.modules() if isinstance(m, Conv2d)}
    out = {}
    for name, p in mt.named_parameters():
        if not p.requires_grad:
            assert not D.is_trainable(name), name + " is frozen on the GPU"
            continue
        assert D.is_trainable(name), name + " trains on the GPU"
        g, r = p.grad.detach(), ref_grads[name]
        if name.endswith("feature_extractor.fc6.weight"):
            g = torch.from_numpy(HR.fc6_from_ohwi(N(g).reshape(g.shape[0], -1), convs[id(p)].channels))
        elif id(p) in convs:
            g = g[..., : convs[id(p)].in_channels].permute(0, 3, 1, 2)
        elif g.dim() == 1 and g.numel() > r.numel():      # (a bias computed wider than it is stores only its real entries)
            g = g[: r.numel()]
        out[name] = g.cpu().double().reshape(r.shape)
    return out


def _compare(S, gpu, tag):
    """the float64 model on the model's CURRENT weights and the GPU's draws: exact checks, value checks, every gradient -> report rows"""
    mt = S["mt"]
    sd_t = E.cpu_sd(mt)
    cfg = S["cfg"]
    # ---------------- exact: anchor labels, box-head labels, RoI levels
    ref_tgt, n = [], None
    for i in range(2):
        boxes = np.concatenate([a for a, _ in gpu["anchors"][i]])
        vis = np.concatenate([v for _, v in gpu["anchors"][i]])
        want_boxes = E.anchors_np(E.IMAGE_SIZES[i])
        assert np.array_equal(boxes, want_boxes[1]) and np.array_equal(vis, want_boxes[2])
        t = LR.prepare_targets(boxes, vis, S["gts"][i])
        assert np.array_equal(gpu["rpn_labels"][i], t["labels"]), "anchor labels of image %d" % i
        assert (np.abs(gpu["rpn_targets"][i] - t["targets"]) <= t["target_bound"] + 1e-6)[t["labels"] == 1].all()
        ref_tgt.append(t)
        n = len(boxes)
        sel = gpu["det_rois"][:, 0] == i
        # an image with fewer candidates than BATCH_SIZE_PER_IMAGE ends in padding rows (label -1, skipped by the loss kernels): thresholds
        # 0.5 / 0.5 leave no candidate unlabelled, so every candidate is drawn and -1 marks padding only
        R = cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE
        drawn = min(R, gpu["n_cand"][i])
        got_lab = gpu["det_labels"][sel]
        assert len(got_lab) == R and (got_lab[:drawn] >= 0).all() and (got_lab[drawn:] == -1).all(), (i, drawn, got_lab.tolist())
        lab, tgt, _ = E.box_targets(S["gts"][i], S["gt_labels"][i], gpu["det_rois"][sel, 1:])
        lab[drawn:] = -1
        bad = np.nonzero(lab != got_lab)[0]
        assert len(bad) == 0, "box-head labels of image %d: rows %s gpu %s oracle %s boxes %s" % (
            i, bad.tolist(), got_lab[bad].tolist(), lab[bad].tolist(), gpu["det_rois"][sel][bad].tolist())
        np.testing.assert_allclose(gpu["det_reg_targets"][sel][lab > 0], tgt[lab > 0], rtol=1e-5, atol=1e-6)
    assert np.array_equal(gpu["det_levels"], P.levels(gpu["det_rois"])) and np.array_equal(gpu["soft_levels"], P.levels(gpu["soft_rois"]))
    pos, samp = gpu["pos_idx"][gpu["pos_idx"] >= 0], gpu["samp_idx"][gpu["samp_idx"] >= 0]
    lab_flat = gpu["rpn_labels"].reshape(-1)
    assert (lab_flat[pos] == 1).all() and (lab_flat[samp] >= 0).all() and len(np.unique(samp)) == len(samp)
    assert gpu["det_rois"].shape[0] == 2 * cfg.MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE and gpu["n_soft"] == [64, 64]
    assert all(len(set(p)) == 64 and 0 <= min(p) and max(p) < 128 for p in gpu["picks"])      # 64 distinct picks among the source's top 128
    live = gpu["det_labels"] >= 0      # the float64 model gets the drawn rows only
    print("candidates", gpu["n_cand"], "drawn rows", int(live.sum()), "per level", np.bincount(gpu["det_levels"][live], minlength=4).tolist())
    assert (np.bincount(gpu["det_levels"][live], minlength=4) > 0).all(), "a pooled level without a RoI"
    # ---------------- the float64 model
    ref = D.DetectorFPNRef(sd_t)
    src = D.DetectorFPNRef(S["sd_s"], trainable=False)
    out = D.step(ref, S["cpu_images"], np.stack([t["labels"] for t in ref_tgt]), np.stack([t["targets"] for t in ref_tgt]), pos, samp,
                 gpu["det_rois"][live], gpu["det_labels"][live], gpu["det_reg_targets"][live], dist_type=cfg.DIST.TYPE, n_old=15, source=src,
                 soft_rois=gpu["soft_rois"], alpha=cfg.DIST.ALPHA, beta=cfg.DIST.BETA, gamma=cfg.DIST.GAMMA)
    for l in range(5):
        _near(gpu["feats"][l], out["ps"][l].detach().numpy(), "P%d" % (l + 2))
        _near(gpu["objs"][l], out["objs"][l].detach().numpy(), "RPN logits, level %d" % l)
        _near(gpu["regs"][l], out["regs"][l].detach().numpy(), "RPN deltas, level %d" % l)
    print("GPU    ", gpu["losses"], gpu["total"])
    print("float64", out["losses"], out["total"])
    assert set(gpu["losses"]) == set(out["losses"]) and len(out["losses"]) == 6
    for k, v in out["losses"].items():
        assert _close(gpu["losses"][k], v), f"{k}: gpu {gpu['losses'][k]} vs float64 {v}"
    assert _close(gpu["total"], out["total"]), (gpu["total"], out["total"])
    # ---------------- gradients of every trainable tensor
    rgrads = ref.grads()
    ggrads = _gpu_grads(mt, rgrads)
    assert sorted(ggrads) == sorted(rgrads) == sorted(D.trainable_keys(E.shapes_json()["shapes"]))
    assert len(ggrads) == N_TRAINABLE == 72
    report = []
    for name, r in rgrads.items():
        g = ggrads[name]
        rel = float((g - r).abs().max()) / max(float(r.abs().max()), 1e-300)
        rel_l2 = float((g - r).norm()) / max(float(r.norm()), 1e-300)
        report.append((name, rel, rel_l2))
        print("PARITY %-7s %-6s %-62s max-rel %.2e  l2-rel %.2e" % (S["math"], tag, name, rel, rel_l2))
    print("PARITY-WORST %s %s max-rel %.3e l2-rel %.3e" % (S["math"], tag, max(r[1] for r in report), max(r[2] for r in report)))
    for name, rel, rel_l2 in report:
        assert rel <= E.GRAD_MAX_REL and rel_l2 <= E.GRAD_REL_L2, f"grad {name}: max-rel {rel}, l2-rel {rel_l2}"
    return report


def test_fpn_train_step_losses_and_grads_vs_float64(S):
    sd_now = E.cpu_sd(S["mt"])
    assert all(torch.equal(sd_now[k], v) for k, v in S["sd_t"].items()), "the loaded weights do not round-trip"
    _compare(S, _gpu_step(S), "step1")


def test_fpn_reference_draws_reproduce_reference_losses(S, gold):
    """the reference's own run (tests/golden/e2e_fpn_tiny.npz): its draws injected, its proposals, labels, losses and logits reproduced"""
    g = gold("e2e_fpn_tiny")
    assert int(g["image_seed"]) == E.IMAGE_SEED and int(g["enrich_seed"]) == E.ENRICH_SEED and int(g["straddle"]) == E.STRADDLE
    mt = S["mt"]
    sd_now = E.cpu_sd(mt)
    assert all(torch.equal(sd_now[k], v) for k, v in S["sd_t"].items()), "this test needs the fixture's weights: it runs before the step test"
    n = E.anchors_np(E.IMAGE_SIZES[0])[3][-1]
    pos = torch.from_numpy(np.concatenate([i * n + g[f"rpn_pos{i}"].astype(np.int64) for i in range(2)])).cuda()
    neg = torch.from_numpy(np.concatenate([i * n + g[f"rpn_neg{i}"].astype(np.int64) for i in range(2)])).cuda()
    ev, evb = mt.rpn.loss_evaluator, mt.roi_heads.box.loss_evaluator
    ev.inject_sampled = (pos, torch.cat([pos, neg]))
    evb.inject_sampled_inds = [torch.from_numpy(g[f"head_sel{i}"].astype(np.int64)).cuda() for i in range(2)]
    mt.train()
    try:
        with torch.no_grad():
            loss_dict, feats, _, _, rpn_out, props, _, soft_res = mt(S["images"], S["targets"])
            torch.cuda.synchronize()
    finally:
        ev.inject_sampled = None
        evb.inject_sampled_inds = None
    for l in range(5):
        err = np.abs(N(E.spot(feats[l], l)) - g[f"p{l + 2}_spot"]).max()
        assert err <= 1e-4 * float(g[f"p{l + 2}_absmax"]), ("P%d" % (l + 2), err)
        st = max(1, 8 >> l)
        err = np.abs(N(rpn_out[0][l][:, :, ::st, ::st]) - g[f"rpn_obj{l}_spot"]).max()
        assert err <= 1e-4 * float(g[f"rpn_obj{l}_absmax"]), ("RPN logits %d" % l, err)
    pre = evb.last_input_proposals
    for i in range(2):
        got, want = N(pre[i].bbox), g[f"props{i}"]
        print("image", i, "proposals", got.shape, want.shape)
        assert got.shape == want.shape
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-3)
        assert np.array_equal(N(props[i].get_field("labels")), g[f"det_labels{i}"])
        np.testing.assert_allclose(N(props[i].get_field("regression_targets")), g[f"det_reg_targets{i}"], rtol=1e-4, atol=1e-5)
    _near(N(soft_res[0]), g["det_logits"], "class logits")
    _near(N(soft_res[1]).reshape(g["det_boxreg"].shape), g["det_boxreg"], "box regression")
    for k in ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg"):
        print(k, float(loss_dict[k]), float(g[k]))
        assert _close(float(loss_dict[k]), float(g[k])), (k, float(loss_dict[k]), float(g[k]))


# ------------------------------------------------------------------------------------------------------------------ eval
def _iou64(a, b):
    area = lambda t: (t[:, 2] - t[:, 0] + 1) * (t[:, 3] - t[:, 1] + 1)     # noqa: E731
    lt, rb = np.maximum(a[:, None, :2], b[None, :, :2]), np.minimum(a[:, None, 2:], b[None, :, 2:])
    wh = np.clip(rb - lt + 1, 0, None)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area(a)[:, None] + area(b)[None, :] - inter)


def _filter64(prob, boxes, score_thresh, nms_thresh, max_det):
    """filter_results (box_head/inference.py:106-151) for one image in float64 -> (list of (label, score, box, unsure)), `unsure`: some decision
    behind this class's detections lies within 1e-5 of the score threshold or within 1e-6 of the NMS threshold"""
    dets = []
    for j in range(1, prob.shape[1]):
        s, b = prob[:, j], boxes[:, j]
        unsure = bool((np.abs(s - score_thresh) < 1e-5).any())
        idx = np.nonzero(s > score_thresh)[0]
        idx = idx[np.argsort(-s[idx], kind="stable")]
        iou = _iou64(b[idx], b[idx]) if len(idx) else np.zeros((0, 0))
        alive = np.ones(len(idx), bool)
        for a in range(len(idx)):
            if not alive[a]:
                continue
            later = np.arange(len(idx)) > a
            unsure |= bool((np.abs(iou[a] - nms_thresh) < 1e-6)[later & alive].any())
            alive &= ~(later & (iou[a] >= nms_thresh))
        dets += [(j, float(s[k]), b[k], unsure) for k in idx[alive]]
    if len(dets) > max_det > 0:
        cut = sorted(d[1] for d in dets)[len(dets) - max_det]
        near = any(abs(d[1] - cut) < 1e-5 and d[1] != cut for d in dets)
        dets = [(d[0], d[1], d[2], d[3] or near) for d in dets if d[1] >= cut]
    return dets


def test_fpn_eval_detections_vs_float64(S):
    from abr_iod_amd.structures.image_list import to_image_list
    mt, cfg = S["mt"], S["cfg"]
    mt.eval()
    try:
        with torch.no_grad():
            images = to_image_list(S["images"])
            feats, _ = mt.backbone(images.tensors)
            (proposals, _), _, _ = mt.rpn(images, feats)
            _, result, _ = mt.roi_heads.box(feats, proposals)
            whole = mt(S["images"])[0]
            torch.cuda.synchronize()
    finally:
        mt.train()
    for a, b in zip(result, whole):      # the pieces called here are the detector's eval path
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("scores"), b.get_field("scores"))
    rois = np.concatenate([np.concatenate([np.full((len(p), 1), i, np.float32), N(p.bbox)], 1) for i, p in enumerate(proposals)])
    ref = D.DetectorFPNRef(E.cpu_sd(mt), trainable=False)
    with torch.no_grad():
        _, logits, boxreg, _ = ref.box_head(ref.features(S["cpu_images"]), rois)
    heads = cfg.MODEL.ROI_HEADS
    # (softmax_decode_f64 takes float32 inputs and evaluates in float64: rounding the float64 logits once costs 6e-8 relative, far under the margins)
    dec = softmax_decode_f64(logits.numpy().astype(np.float32), boxreg.numpy().astype(np.float32), rois, np.array(E.IMAGE_SIZES))
    total = unsure = 0
    for i, det in enumerate(result):
        sel = rois[:, 0] == i
        want = _filter64(dec.prob[sel], dec.boxes[sel], heads.SCORE_THRESH, heads.NMS, heads.DETECTIONS_PER_IMG)
        total += len(want)
        unsure += sum(d[3] for d in want)
        gl, gs, gb = N(det.get_field("labels")), N(det.get_field("scores")), N(det.bbox)
        print("image", i, "detections", len(gl), "float64", len(want), "unsure", sum(d[3] for d in want))
        assert len(want) > 20, "too few detections for the comparison to mean anything"
        for j in sorted({d[0] for d in want} | set(gl.tolist())):
            w = sorted([d for d in want if d[0] == j], key=lambda d: -d[1])
            if any(d[3] for d in w):
                continue
            k = np.nonzero(gl == j)[0]
            assert len(k) == len(w), f"image {i}, class {j}: {len(k)} detections, float64 has {len(w)}"
            free = np.ones(len(k), bool)      # one-to-one: scores closer than 1e-4 to each other may come in either order
            for d in w:
                ok = free & (np.abs(gs[k] - d[1]) <= 1e-4) & (np.abs(gb[k] - d[2][None]).max(1) <= 1e-3)
                assert ok.any(), f"image {i}, class {j}: no detection with score {d[1]} +- 1e-4 and box {d[2]} +- 1e-3 among {gs[k][free]} {gb[k][free]}"
                free[np.nonzero(ok)[0][0]] = False
    print("excluded", unsure, "of", total)
    assert unsure < 0.02 * total, (unsure, total)


# ------------------------------------------------------------------------------------------------------------------ after a step
# (last: it changes the weights)
def test_fpn_step_then_forward_follows_the_weights(S):
    """one FusedSGD step large enough to matter (2 % of the weights' norm), then forward / backward again: everything derived from the weights
    (dgrad copies, the library's cached planes) must have followed, or the comparison with the float64 model on the NEW weights fails"""
    from abr_iod_amd.solver.build import make_optimizer
    mt = S["mt"]
    opt = make_optimizer(S["cfg"], mt)
    _gpu_step(S)                                     # gradients of the current weights (and every derived copy built)
    n = mt.flat.n_trainable
    before = mt.flat.params[:n].clone()
    lr = 0.02 * float(before.norm()) / float(mt.flat.grads.norm())
    for grp in opt.param_groups:
        grp["lr"] = lr
    opt.step()
    torch.cuda.synchronize()
    moved = float((mt.flat.params[:n] - before).norm() / before.norm())
    print("relative step", moved)
    assert 1e-2 <= moved <= 5e-2, moved
    _compare(S, _gpu_step(S), "step2")
    mt.flat.zero_grad()

#!/usr/bin/env python3
"""FPN keypoint head golden FROM THE REFERENCE (run by hand where the reference tree exists; see ref_harness.py): the reference's own
KeypointRCNNFeatureExtractor (modeling/roi_heads/keypoint_head/roi_keypoint_feature_extractors.py:11-43) built with FOUR pooler scales,
KeypointRCNNPredictor and KeypointRCNNLossComputation called directly on the CPU over the maps, the sampled set and the ground truth of
tests/keypoint_fpn_ref.py's scene: pooler 6 x 6, sampling ratio 2; CONV_LAYERS (16, 16); K = 5 and 17.  The extractor's weights AND biases
are drawn here, once for both K (the reference's init leaves every bias zero, which would hide a dropped bias).

tests/golden/keypoint_head_fpn.npz: w_/b_ of conv_fcn1, conv_fcn2; kept_rows (the rows of the sampled set the reference's subsample keeps),
levels (its LevelMapper's level of each), pooled [n,16,6,6] (its Pooler's output) and features [n,16,6,6] (the conv stack's); per K:
w<K>_/b<K>_kps_score_lowres, heat<K> / valid<K> [n,K], logits<K> (the first LOGIT_ROWS[K] RoIs, for the file's size), loss<K>, gw<K>_/gb<K>_
of the three layers.  The reference's ROIAlign backward is not implemented on the CPU: the pooler's output is a leaf and the maps' gradients
are the float64 model's business.
tests/golden/keypoint_fpn_state_dict_shapes.json: {"overrides": [...], "shapes": {key: shape}} of the reference's
build_detection_model(cfg).state_dict() for the tiny R-50-FPN + keypoint configuration.  The files hold data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))      # (the float64 model reads the oracle package)
import ref_harness as rh  # noqa: E402
import keypoint_fpn_ref as KR  # noqa: E402
from make_golden_box_head_fpn import DETECTOR  # noqa: E402

LOGIT_ROWS = {5: 2, 17: 1}


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.loss import make_roi_keypoint_loss_evaluator, project_keypoints_to_heatmap
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.roi_keypoint_feature_extractors import KeypointRCNNFeatureExtractor
    from maskrcnn_benchmark.modeling.roi_heads.keypoint_head.roi_keypoint_predictors import KeypointRCNNPredictor
    from maskrcnn_benchmark.structures.bounding_box import BoxList
    from maskrcnn_benchmark.structures.keypoint import PersonKeypoints

    gen = torch.Generator().manual_seed(KR.GOLDEN_SEED)

    def draw(lay, fan):
        with torch.no_grad():
            lay.weight.copy_(torch.randn(lay.weight.shape, generator=gen) * (2.0 / fan) ** 0.5)
            lay.bias.copy_((torch.rand(lay.bias.shape, generator=gen) * 2 - 1) * 0.3)

    out = dict(seed=np.int64(KR.GOLDEN_SEED))
    fe = None
    for K in KR.KS:
        sc = KR.scene(K)
        KR.check_scene(sc)
        cfg = rh.default_cfg(overrides=["MODEL.DEVICE", "cpu"] + KR.head_cfg_list(K))
        if fe is None:
            fe = KeypointRCNNFeatureExtractor(cfg, KR.C)
            assert fe.blocks == list(KR.BLOCKS) and len(fe.pooler.poolers) == 4
            for n in fe.blocks:
                draw(getattr(fe, n), 9 * getattr(fe, n).weight.shape[0])
        pred = KeypointRCNNPredictor(cfg, fe.out_channels)
        draw(pred.kps_score_lowres, 16 * KR.LAYERS[-1])
        ev = make_roi_keypoint_loss_evaluator(cfg)
        img_h, img_w = sc["image"]
        proposals, targets = [], []
        for b in range(KR.B):
            proposals.append(BoxList(torch.from_numpy(sc["rois"][sc["rois"][:, 0] == b, 1:].copy()), (img_w, img_h), mode="xyxy"))
            t = BoxList(torch.from_numpy(sc["gt_boxes"][b].copy()), (img_w, img_h), mode="xyxy")
            t.add_field("labels", torch.arange(1, len(sc["gt_boxes"][b]) + 1))
            t.add_field("keypoints", PersonKeypoints(torch.from_numpy(sc["keypoints"][b].copy()), (img_w, img_h)))
            targets.append(t)
        labels, _ = ev.prepare_targets(proposals, targets)
        matched = torch.cat([ev.match_targets_to_proposals(p, t).get_field("matched_idxs") for p, t in zip(proposals, targets)])
        assert np.array_equal(matched.numpy() >= 0, sc["labels"] > 0), "the reference's matcher sees another positive set"
        assert np.array_equal(np.nonzero(torch.cat(labels).numpy() > 0)[0], sc["sel"]["pos_rows"][: sc["sel"]["n_pos"]])
        kept = ev.subsample(proposals, targets)
        sel = sc["sel"]
        n = sel["n_pos"]
        rows = sel["pos_rows"][:n]
        assert [len(p) for p in kept] == [n, 0] and np.array_equal(torch.cat([p.bbox for p in kept]).numpy(), sc["rois"][rows, 1:]), \
            "the reference keeps other rows than tests/keypoint_ref.py's selection"
        lv = fe.pooler.map_levels(kept).numpy()
        assert np.array_equal(lv, sc["lv"][rows]), "the reference's LevelMapper disagrees with tests/pooler_ref.py"
        heat, valid = zip(*[project_keypoints_to_heatmap(p.get_field("keypoints"), p, KR.M) for p in kept if len(p)])
        heat, valid = torch.cat(heat).numpy(), torch.cat(valid).numpy()
        assert np.array_equal(heat * (valid > 0), sel["targets"][:n] * sel["valid"][:n]) and np.array_equal(valid > 0, sel["valid"][:n] > 0)

        xs = [torch.from_numpy(np.ascontiguousarray(f.transpose(0, 3, 1, 2))) for f in sc["feats"]]
        kept_leaf = {}

        def leaf(_module, _inputs, output):      # the pooler's result as a leaf: the reference's ROIAlign has no CPU backward
            kept_leaf["pooled"] = output.detach().requires_grad_(True)
            return kept_leaf["pooled"]

        hook = fe.pooler.register_forward_hook(leaf)
        fe.zero_grad()
        x = fe(xs, kept)
        hook.remove()
        logits = pred(x)
        loss = ev(kept, logits)
        loss.backward()
        if "pooled" not in out:
            out.update(kept_rows=rows.astype(np.int64), levels=lv.astype(np.int32), pooled=kept_leaf["pooled"].detach().numpy(), features=x.detach().numpy())
            for name in fe.blocks:
                out["w_" + name], out["b_" + name] = getattr(fe, name).weight.detach().numpy(), getattr(fe, name).bias.detach().numpy()
        else:
            assert np.array_equal(out["kept_rows"], rows) and np.array_equal(out["features"], x.detach().numpy())
        out["heat%d" % K], out["valid%d" % K] = heat.astype(np.int64), valid.astype(np.uint8)
        out["logits%d" % K], out["loss%d" % K] = logits.detach().numpy()[: LOGIT_ROWS[K]], np.float64(loss.double().item())
        dc = pred.kps_score_lowres
        out["w%d_kps_score_lowres" % K], out["b%d_kps_score_lowres" % K] = dc.weight.detach().numpy(), dc.bias.detach().numpy()
        out["gw%d_kps_score_lowres" % K], out["gb%d_kps_score_lowres" % K] = dc.weight.grad.numpy().copy(), dc.bias.grad.numpy().copy()
        for name in fe.blocks:
            out["gw%d_%s" % (K, name)], out["gb%d_%s" % (K, name)] = getattr(fe, name).weight.grad.numpy().copy(), getattr(fe, name).bias.grad.numpy().copy()
        print("K", K, "kept", n, "levels", lv.tolist(), "loss", float(out["loss%d" % K]), "valid", int((valid > 0).sum()))
    path = os.path.join(HERE, "keypoint_head_fpn.npz")
    np.savez_compressed(path, **out)
    size, cap = os.path.getsize(path), os.path.getsize(os.path.join(HERE, "mask_head_fpn.npz"))
    print("bytes", size, "of", cap)
    assert size <= cap

    det = [v for v in DETECTOR] + KR.KEYPOINT_CFG
    model = build_detection_model(rh.default_cfg(overrides=det))
    with open(os.path.join(HERE, "keypoint_fpn_state_dict_shapes.json"), "w") as f:
        shapes = [(k, list(v.shape)) for k, v in model.state_dict().items()]      # one key per line
        f.write('{"overrides": %s,\n "shapes": {\n' % json.dumps([list(v) if isinstance(v, tuple) else v for v in det]))
        for i, (k, shape) in enumerate(shapes):
            f.write("  %s: %s%s\n" % (json.dumps(k), json.dumps(shape), "," if i < len(shapes) - 1 else ""))
        f.write(" }}\n")


if __name__ == "__main__":
    main()

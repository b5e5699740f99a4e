"""CPU: tests/keypoint_ref.py (the yardstick of the GPU keypoint tests) and abr_iod_amd.structures.keypoint against what the reference's own
code recorded in tests/golden/keypoint_head.npz (make_golden_keypoint.py)."""
import os

import numpy as np
import pytest
import torch

import keypoint_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def G():
    return np.load(os.path.join(GOLDEN, "keypoint_head.npz"))


def _scene(G, K):
    counts = G["gt_counts"]
    off = np.concatenate([[0], np.cumsum(counts)])
    gt = [G["gt"][off[i]:off[i + 1]] for i in range(len(counts))]
    kps = [G["kp%d" % K][off[i]:off[i + 1]] for i in range(len(counts))]
    rois = G["rois"]
    order = np.concatenate([np.nonzero(rois[:, 0] == i)[0] for i in range(len(counts))])     # the reference's labels are in per-image order
    labels = np.zeros(len(rois), np.int64)
    labels[order] = G["labels%d" % K]
    return gt, kps, rois, labels, order


@pytest.mark.parametrize("K", [5, 17])
def test_targets_match_the_reference(G, K):
    gt, kps, rois, ref_labels, order = _scene(G, K)
    # the head's input: the box head's positives = matched at FG_IOU_THRESHOLD (the reference marks them > 0, or -1 when nothing is visible)
    labels_in = (ref_labels != 0).astype(np.int64)
    assert (ref_labels == -1).any() and (ref_labels == 0).any() and (ref_labels > 0).any()
    kept_boxes = G["kept_boxes%d" % K]
    for M in (8, 24, 56):
        # per-image order, as the reference concatenates its kept proposals
        got = R.select_targets(rois[order], labels_in[order], gt, kps, M, len(rois))
        n = got["n_pos"]
        assert n == len(kept_boxes) == int((ref_labels > 0).sum())
        assert np.array_equal(rois[order][got["pos_rows"][:n], 1:], kept_boxes)
        assert np.array_equal(got["targets"][:n], G["heat%d_M%d" % (K, M)]), M
        assert np.array_equal(got["valid"][:n], G["valid%d_M%d" % (K, M)]), M
        assert np.all(got["pos_rows"][n:] == -1) and not got["valid"][n:].any()
    counts = G["kept_counts%d" % K]
    assert counts[1] == 0, "the scene's second image must lose every positive"


@pytest.mark.parametrize("K", [5, 17])
def test_fold_upsample_and_loss_match_the_reference(G, K):
    feats = torch.from_numpy(G["features%d" % K]).double()
    w = torch.from_numpy(G["param%d.predictor.kps_score_lowres.weight" % K]).double()          # [C, K, 4, 4]
    b = torch.from_numpy(G["param%d.predictor.kps_score_lowres.bias" % K]).double()
    Kp, C = R.kp_pad(K), w.shape[0]
    wt = torch.zeros(4, 4, Kp, C, dtype=torch.float64)
    wt[:, :, :K] = w.permute(2, 3, 1, 0)
    assert torch.equal(R.gemm_columns_to_weight(wt.reshape(16 * Kp, C), K), w)
    y = feats.permute(0, 2, 3, 1) @ wt.reshape(16 * Kp, C).t()
    low = R.fold(y, b)
    logits = R.upsample2x(low[:, :K]).numpy()
    ref = G["logits%d" % K]
    assert np.abs(logits[:len(ref)] - ref).max() <= 64 * np.finfo(np.float32).eps * np.abs(ref).max()
    tgt, valid = torch.from_numpy(G["heat%d_M24" % K]), torch.from_numpy(G["valid%d_M24" % K]).to(torch.uint8)
    loss, grad, _ = R.loss_and_grad(low, K, tgt, valid)
    assert abs(loss - float(G["loss%d" % K])) <= 1e-5 * abs(float(G["loss%d" % K]))
    # the deconvolution's weight gradient through the restated loss gradient (the bias gradient is no check: softmax - onehot sums to zero
    # over a plane, and the recorded fp32 values are rounding noise around it)
    wq = w.clone().requires_grad_(True)
    out = torch.nn.functional.conv_transpose2d(feats, wq, b, stride=2, padding=1)
    assert (out.detach() - low[:, :K]).abs().max().item() <= 1e-12
    (gw,) = torch.autograd.grad(out, wq, grad_outputs=grad[:, :K])
    ref_gw = G["grad%d.predictor.kps_score_lowres.weight" % K]
    assert np.abs(gw.numpy() - ref_gw).max() <= 1e-4 * np.abs(ref_gw).max()
    assert np.abs(grad[:, :K].sum((2, 3)).numpy()).max() <= 1e-12 and np.abs(G["grad%d.predictor.kps_score_lowres.bias" % K]).max() <= 1e-6


def test_structures_keypoint_matches_the_reference(G):
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import Keypoints, PersonKeypoints
    assert PersonKeypoints.FLIP_INDS.tolist() == G["flip_inds"].tolist()
    assert np.array_equal(np.array(PersonKeypoints.CONNECTIONS), G["connections"])
    assert len(PersonKeypoints.NAMES) == 17 and len(PersonKeypoints.FLIP_MAP) == 8
    kp = PersonKeypoints(torch.from_numpy(G["api_in"]), (320, 256))
    assert np.array_equal(kp.resize((200, 300)).keypoints.numpy(), G["api_resize"])
    assert np.array_equal(kp.transpose(0).keypoints.numpy(), G["api_flip"])
    assert np.array_equal(kp[torch.tensor([2, 0])].keypoints.numpy(), G["api_index"])
    with pytest.raises(NotImplementedError):
        kp.transpose(1)
    kp.add_field("logits", torch.arange(3.0))
    assert kp[[1]].get_field("logits").tolist() == [1.0] and kp.to("cpu").get_field("logits").tolist() == [0.0, 1.0, 2.0]
    assert tuple(Keypoints(torch.zeros(0, 51), (4, 4)).keypoints.shape) == (0, 51)       # (the reference leaves an empty tensor as given)
    # BoxList carries the field as it carries "masks"
    b = BoxList(torch.tensor([[1., 2, 30, 40], [5, 6, 70, 80], [9, 9, 20, 20]]), (320, 256))
    b.add_field("keypoints", kp)
    assert np.array_equal(b.resize((200, 300)).get_field("keypoints").keypoints.numpy(), G["api_resize"])
    assert np.array_equal(b.transpose(0).get_field("keypoints").keypoints.numpy(), G["api_flip"])
    assert np.array_equal(b[torch.tensor([2, 0])].get_field("keypoints").keypoints.numpy(), G["api_index"])
    assert b.to("cpu").get_field("keypoints").size == (320, 256)


def test_decode_restatement_properties():
    """cv2 is not installed: heatmaps_to_keypoints is pinned by what its definition implies"""
    rng = np.random.default_rng(0)
    m = rng.standard_normal((7, 9))
    assert np.array_equal(R.resize_map(m, 9, 7), m)                                       # 1:1 is the identity
    for src, dst in [(8, 8), (8, 13), (8, 3), (56, 200), (5, 1)]:
        w = R.cubic_matrix(src, dst)
        assert np.abs(w.sum(1) - 1).max() <= 1e-12 and np.abs(w).sum(1).max() < 2         # rows sum to 1; the magnitudes stay below 2
    assert np.allclose(R.cubic_weights(np.array([0.5])), [[-0.09375, 0.59375, 0.59375, -0.09375]])
    assert R.grid_sides([10.2, 20.1, 10.7, 20.4])[2:] == (1, 1) and R.grid_sides([3.3, 4.4, 40.9, 29.1])[2:] == (38, 25)
    x, y = R.xy_at([3.3, 4.4, 40.9, 29.1], 38 + 2, 38, 25)
    assert abs(float(x) - (3.3 + 2.5 * 37.6 / 38)) < 1e-4 and abs(float(y) - (4.4 + 1.5 * 24.7 / 25)) < 1e-4

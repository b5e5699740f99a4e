"""GPU: the keypoint head (abr_iod_amd/modeling/roi_heads/keypoint_head) against a float64 restatement on the host, and inside the model.

The head test builds ROIKeypointHead alone at small sizes (8 input channels, CONV_LAYERS (16, 16), pooler 6 -> 24 x 24 heat maps, K = 5 and
17, 20 sampled RoIs over 3 images) and compares the heat-map logits, loss_kp and the gradient of every parameter with torch in float64:
the pooled features come from the kernel under test's own ROIAlign (pinned elsewhere: tests/test_gpu_roi_align.py), everything behind them
is conv2d / conv_transpose2d / interpolate / cross_entropy.  Bounds as tests/test_gpu_mask_head.py uses for the mask head: 64 * eps * max |ref|
on the logits, 1e-4 on the loss; the gradients of the parameters, of the pooled features and of the backbone features within 1e-4 of the
largest reference entry of their tensor (fp32 sums of a few thousand terms; the backbone features' reference is the existing ROIAlign
backward, pinned by tests/test_gpu_roi_align.py, applied to the float64 gradient of the pooled features).  The selection is compared
index-exactly with tests/keypoint_ref.py.  The training-step tests are in tests/test_gpu_keypoint_step.py."""
import os

import numpy as np
import pytest
import torch

import keypoint_ref as R

pytestmark = pytest.mark.gpu

EPS = float(np.finfo(np.float32).eps)


def _head_cfg(K, extra=()):
    from abr_iod_amd.config import cfg as base
    cfg = base.clone()
    cfg.merge_from_list(["MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False,
                         "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 6, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 24,
                         "MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS", (16, 16), "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", K,
                         "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", (0.0625,), "MODEL.ROI_BOX_HEAD.POOLER_SCALES", (0.0625,),
                         "MODEL.ROI_HEADS.BATCH_SIZE_PER_IMAGE", 16, "MODEL.ROI_HEADS.POSITIVE_FRACTION", 0.5] + list(extra))
    return cfg


def _scene(K, seed=0):
    """3 images of 320 x 256, 2-3 instances each with keypoints (some invisible, some outside); 20 sampled RoIs with labels"""
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    from abr_iod_amd.engine.synthetic import _box_keypoints
    g = torch.Generator().manual_seed(seed)
    W, H = 320, 256
    gts = [torch.tensor([[20., 30, 140, 200], [160, 40, 300, 180]]), torch.tensor([[10., 10, 100, 120], [120, 60, 310, 250], [40, 150, 110, 240]]),
           torch.tensor([[60., 20, 260, 230], [5, 5, 50, 60]])]
    targets, proposals = [], []
    for i, gt in enumerate(gts):
        kp = _box_keypoints(gt, K)
        kp[0, 0, :2] += 500.0                       # one labelled point far outside its box
        if i == 1:
            kp[2, :, 2] = 0                         # an instance with nothing visible: its positives are dropped
        t = BoxList(gt.cuda(), (W, H), mode="xyxy")
        t.add_field("labels", torch.arange(1, len(gt) + 1).cuda())
        t.add_field("keypoints", PersonKeypoints(kp.cuda(), (W, H)))
        targets.append(t)
        n = (7, 7, 6)[i]
        pick = torch.randint(0, len(gt), (n,), generator=g)
        boxes = gt[pick] + 6 * torch.randn(n, 4, generator=g)
        labels = torch.where(torch.rand(n, generator=g) < 0.75, pick + 1, torch.zeros(n, dtype=torch.int64))
        p = BoxList(boxes.cuda(), (W, H), mode="xyxy")
        p.add_field("labels", labels.cuda())
        proposals.append(p)
    feat = torch.randn(3, 8, H // 16, W // 16, generator=g).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    return feat, proposals, targets


@pytest.mark.parametrize("K", [5, 17])
def test_head_vs_float64(K):
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    torch.manual_seed(K)
    head = build_roi_keypoint_head(_head_cfg(K), 8).cuda()
    with torch.no_grad():
        for n, p in head.named_parameters():
            if n.endswith("bias"):
                p.normal_(0.0, 0.1)
        head.predictor.kps_score_lowres.bias[K:] = 0
    head.train()
    feat, proposals, targets = _scene(K)
    feat.requires_grad_(True)
    x, _, losses = head([feat], proposals, targets)
    loss = losses["loss_kp"]
    (2.0 * loss).backward()
    torch.cuda.synchronize()
    sel = head.last_selection
    # the selection, index-exact
    rois = torch.cat([torch.cat((torch.full((len(p), 1), float(i)), p.bbox.cpu()), 1) for i, p in enumerate(proposals)]).numpy()
    labels = torch.cat([p.get_field("labels") for p in proposals]).cpu().numpy()
    want = R.select_targets(rois, labels, [t.bbox.cpu().numpy() for t in targets], [t.get_field("keypoints").keypoints.cpu().numpy() for t in targets],
                            24, sel["pos_rows"].numel())
    for key in ("pos_rows", "inv", "targets", "valid"):
        assert np.array_equal(sel[key].cpu().numpy(), want[key]), key
    assert sel["n_pos"].item() == want["n_pos"] > 3 and sel["n_valid"].item() == want["n_valid"] > 0
    assert want["n_pos"] < sel["pos_rows"].numel(), "the scene must leave padding rows"
    # float64 behind the pooled features
    ext, pred = head.feature_extractor, head.predictor
    pooled = ops.roi_align_forward(feat.detach().permute(0, 2, 3, 1).contiguous(), sel["rois"], ext.spatial_scale, 6, 6, ext.sampling_ratio)
    h0 = pooled.permute(0, 3, 1, 2).cpu().double().requires_grad_(True)
    h = h0
    params = {}
    for c, name in zip(ext.convs(), ext.blocks):
        params[name + ".weight"] = c.oihw().cpu().double().requires_grad_(True)
        params[name + ".bias"] = c.bias.detach().cpu().double().requires_grad_(True)
        h = torch.relu(torch.nn.functional.conv2d(h, params[name + ".weight"], params[name + ".bias"], padding=1))
    dc = pred.kps_score_lowres
    params["kps.weight"] = dc.oihw().cpu().double().requires_grad_(True)
    params["kps.bias"] = dc.bias.detach()[:K].cpu().double().requires_grad_(True)
    assert tuple(params["kps.weight"].shape) == (16, K, 4, 4)
    low = torch.nn.functional.conv_transpose2d(h, params["kps.weight"], params["kps.bias"], stride=2, padding=1)
    z = R.upsample2x(low)
    got_z = head.last_kp_logits
    assert tuple(got_z.shape) == tuple(z.shape) == (sel["pos_rows"].numel(), K, 24, 24)
    live = torch.as_tensor(want["pos_rows"] >= 0)
    zerr = (got_z.cpu().double() - z.detach()).abs()[live].max().item()
    zmax = z.detach().abs()[live].max().item()
    print("logits: max err", zerr, "bound", 64 * EPS * zmax)
    assert zerr <= 64 * EPS * zmax
    v = torch.as_tensor(want["valid"]).reshape(-1).bool()
    ref_loss = torch.nn.functional.cross_entropy(z.reshape(-1, 24 * 24)[v], torch.as_tensor(want["targets"]).reshape(-1)[v])
    (2.0 * ref_loss).backward()
    print("loss", loss.item(), "float64", ref_loss.item())
    assert abs(loss.item() - ref_loss.item()) <= 1e-4 * max(1.0, abs(ref_loss.item()))
    got = {}
    for c, name in zip(ext.convs(), ext.blocks):
        got[name + ".weight"], got[name + ".bias"] = c.ref_layout(c.weight.grad), c.bias.grad
    got["kps.weight"], got["kps.bias"] = dc.ref_layout(dc.weight.grad), dc.bias.grad[:K]
    assert torch.all(dc.bias.grad[K:] == 0) and torch.all(dc.weight.grad.view(4, 4, dc.kp, 16)[:, :, K:] == 0), "padding rows take no gradient"
    for name, p in params.items():
        ref_g = p.grad
        err = (got[name].cpu().double() - ref_g).abs().max().item()
        print("grad", name, "max err", err, "of", ref_g.abs().max().item())
        if name == "kps.bias":
            # softmax - onehot sums to zero over a plane, so this gradient is zero: what is left is the rounding of sums whose magnitudes
            # add up to at most 2 * (the backward's factor 2) = 4 over all valid rows
            assert ref_g.abs().max().item() <= 1e-12 and err <= 16 * EPS * 4, name
            continue
        assert ref_g.abs().max().item() > 0 and err <= 1e-4 * ref_g.abs().max().item(), name
    # the backbone features' gradient = ROIAlign's backward (the existing kernel) of d loss / d pooled: the reference is that kernel applied to
    # the float64 gradient of the pooled features, which checks conv_fcn1's input-gradient GEMM, the predictor's, and the hand-over's layout
    gp64 = h0.grad                                                     # [P,C,6,6]
    live_rows = torch.as_tensor(want["pos_rows"] >= 0)
    assert gp64[live_rows].abs().max().item() > 0 and torch.all(gp64[~live_rows] == 0), "padding rows carry no gradient"
    B_, C_, H_, W_ = feat.shape
    ref_gfeat = ops.roi_align_backward(gp64.float().permute(0, 2, 3, 1).contiguous().cuda(), sel["rois"], ext.spatial_scale, 6, 6, ext.sampling_ratio,
                                       B_, H_, W_, C_).permute(0, 3, 1, 2)
    gfeat = feat.grad
    assert gfeat is not None and tuple(gfeat.shape) == tuple(feat.shape) and torch.isfinite(gfeat).all()
    gerr, gmax = (gfeat - ref_gfeat).abs().max().item(), ref_gfeat.abs().max().item()
    print("grad backbone features: max err", gerr, "of", gmax)
    assert gmax > 0 and gerr <= 1e-4 * gmax
    # a second pass reproduces the loss bit for bit
    for p in head.parameters():
        p.grad = None
    loss2 = head([feat.detach()], proposals, targets)[2]["loss_kp"]
    assert torch.equal(loss2, loss)


def test_eval_fields_for_zero_one_and_several_detections():
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    K = 17
    head = build_roi_keypoint_head(_head_cfg(K), 8).cuda().eval()
    feat, _, _ = _scene(K)
    feat = feat[:2]
    some = torch.tensor([[10., 20, 100, 140], [50, 60, 51.5, 60.2], [-5, -8, 330, 270]]).cuda()
    for counts in [(0, 0), (1, 0), (0, 1), (3, 2)]:
        dets = []
        for n in counts:
            b = BoxList(some[:n].clone(), (320, 256), mode="xyxy")
            b.add_field("scores", torch.ones(n).cuda())
            dets.append(b)
        with torch.no_grad():
            x, out, losses = head([feat], dets)
        assert losses == {} and len(out) == 2
        for n, r in zip(counts, out):
            kp = r.get_field("keypoints")
            assert isinstance(kp, PersonKeypoints) and tuple(kp.keypoints.shape) == (n, K, 3) and tuple(kp.get_field("logits").shape) == (n, K)
            assert r.has_field("scores") and len(r) == n
            if n:
                assert torch.all(kp.keypoints[..., 2] == 1) and torch.isfinite(kp.keypoints).all()
                b = r.bbox
                w, h = (b[:, 2] - b[:, 0]).clamp(min=1)[:, None], (b[:, 3] - b[:, 1]).clamp(min=1)[:, None]
                assert torch.all(kp.keypoints[..., 0] >= b[:, 0:1]) and torch.all(kp.keypoints[..., 0] <= b[:, 0:1] + w)
                assert torch.all(kp.keypoints[..., 1] >= b[:, 1:2]) and torch.all(kp.keypoints[..., 1] <= b[:, 1:2] + h)


# ------------------------------------------------------------------------------------------------ the reference's recorded head
@pytest.mark.parametrize("K", [5, 17])
def test_head_vs_reference_fixture(K):
    """tests/golden/keypoint_head.npz (the reference's KeypointRCNNFeatureExtractor conv stack, KeypointRCNNPredictor and loss on recorded
    pooled features): logits within 64 * eps * max |ref|, loss_kp within 1e-4, every parameter's gradient within 1e-4 of the tensor's largest
    reference entry (fp32 arithmetic on both sides).  The fixture holds no gradient of the pooled features: that one is compared with float64
    autograd through the same stack (conv2d / conv_transpose2d / interpolate / cross_entropy on the recorded parameters), at the same bound"""
    from abr_iod_amd.modeling.roi_heads.keypoint_head.keypoint_head import build_roi_keypoint_head
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keypoint_head.npz"))
    head = build_roi_keypoint_head(_head_cfg(K), 8).cuda().train()
    ext, pred = head.feature_extractor, head.predictor
    dc = pred.kps_score_lowres
    with torch.no_grad():
        for name in ext.blocks:
            getattr(ext, name).load_oihw(torch.from_numpy(G["param%d.%s.weight" % (K, name)]).cuda())
            getattr(ext, name).bias.copy_(torch.from_numpy(G["param%d.%s.bias" % (K, name)]).cuda())
        dc.load_oihw(torch.from_numpy(G["param%d.predictor.kps_score_lowres.weight" % K]).cuda())
        dc.bias.zero_()
        dc.bias[:K].copy_(torch.from_numpy(G["param%d.predictor.kps_score_lowres.bias" % K]).cuda())
    pooled = torch.from_numpy(G["pooled%d" % K]).cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    P = pooled.shape[0]
    valid = torch.from_numpy(G["valid%d_M24" % K]).to(torch.uint8).cuda()
    sel = dict(targets=torch.from_numpy(G["heat%d_M24" % K]).cuda(), valid=valid, n_valid=valid.sum().to(torch.int32).reshape(1))
    x = ext([pooled], None)
    feats = G["features%d" % K]
    assert np.abs(x.detach().cpu().numpy() - feats).max() <= 64 * EPS * np.abs(feats).max()
    loss = pred.loss(x, sel)
    loss.backward()
    torch.cuda.synchronize()
    ref = G["logits%d" % K]
    got = head.last_kp_logits.cpu().numpy()
    assert got.shape == (P, K, 24, 24)
    print("logits: max err", np.abs(got[:len(ref)] - ref).max(), "bound", 64 * EPS * np.abs(ref).max())
    assert np.abs(got[:len(ref)] - ref).max() <= 64 * EPS * np.abs(ref).max()
    print("loss", loss.item(), "reference", float(G["loss%d" % K]))
    assert abs(loss.item() - float(G["loss%d" % K])) <= 1e-4 * max(1.0, abs(float(G["loss%d" % K])))
    grads = {name + ".weight": getattr(ext, name).ref_layout(getattr(ext, name).weight.grad) for name in ext.blocks}
    grads.update({name + ".bias": getattr(ext, name).bias.grad for name in ext.blocks})
    grads["predictor.kps_score_lowres.weight"] = dc.ref_layout(dc.weight.grad)
    for name, g in grads.items():
        want = G["grad%d.%s" % (K, name)]
        err = np.abs(g.cpu().numpy() - want).max()
        print("grad", name, "max err", err, "of", np.abs(want).max())
        assert err <= 1e-4 * np.abs(want).max(), name
    # the deconvolution's bias gradient is a sum of (softmax - onehot) over whole planes: zero up to rounding, on both sides
    assert dc.bias.grad.abs().max().item() <= 1e-6 and np.abs(G["grad%d.predictor.kps_score_lowres.bias" % K]).max() <= 1e-6
    h0 = torch.from_numpy(G["pooled%d" % K]).double().requires_grad_(True)
    h = h0
    for name in ext.blocks:
        h = torch.relu(torch.nn.functional.conv2d(h, torch.from_numpy(G["param%d.%s.weight" % (K, name)]).double(),
                                                  torch.from_numpy(G["param%d.%s.bias" % (K, name)]).double(), padding=1))
    low = torch.nn.functional.conv_transpose2d(h, torch.from_numpy(G["param%d.predictor.kps_score_lowres.weight" % K]).double(),
                                               torch.from_numpy(G["param%d.predictor.kps_score_lowres.bias" % K]).double(), stride=2, padding=1)
    v = torch.from_numpy(G["valid%d_M24" % K]).reshape(-1).bool()
    ref_loss = torch.nn.functional.cross_entropy(R.upsample2x(low).reshape(-1, 24 * 24)[v], torch.from_numpy(G["heat%d_M24" % K]).reshape(-1)[v])
    assert abs(ref_loss.item() - float(G["loss%d" % K])) <= 1e-5 * abs(float(G["loss%d" % K]))      # the restated stack is the recorded one
    ref_loss.backward()
    assert pooled.grad is not None and tuple(pooled.grad.shape) == tuple(h0.shape)
    perr, pmax = (pooled.grad.cpu().double() - h0.grad).abs().max().item(), h0.grad.abs().max().item()
    print("grad pooled features: max err", perr, "of", pmax)
    assert pmax > 0 and perr <= 1e-4 * pmax

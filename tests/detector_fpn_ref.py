"""TEST INFRASTRUCTURE ONLY -- torch-CPU float64 restatement of the R-50-FPN detector (body with layer4, FPN neck with LastLevelMaxPool, the
shared RPN head and the multi-level RPN loss, the four-level pooler, FPN2MLP head + FPNPredictor and the box-head / ID / ARD losses) over a
reference-layout state dict.  Autograd on it supplies the gradients the whole-detector tests compare the HIP path with
(tests/test_gpu_e2e_fpn.py); tests/test_detector_fpn_ref.py pins it to the reference's own forward (tests/golden/e2e_fpn_tiny.npz).

Built from what exists: oracle.torch_ref.bottleneck / frozen_bn (body), F.conv2d + F.interpolate (neck, modeling/backbone/fpn.py:51-79),
tests/rpn_fpn_loss_ref.py's order, BCE, smooth L1 and denominator restated in torch (`rpn_loss`), tests/pooler_ref.py's float64 forward and its
transpose wrapped as one autograd Function (`pool`), oracle.torch_ref's box_head_loss / roi_distillation_loss / ard_loss.

`mutate` names one deliberate composition bug (tests/test_detector_fpn_ref.py::test_fixture_sees_composition_bugs): the fixture has to move some
parameter gradient by far more than the GPU test's bound under each of them.
    drop_p6_grad      P6's gradient does not return into P5
    drop_pool_level2  the pooler's gradient does not reach P4
    swap_rpn_levels   levels 1 and 2 change places in the RPN concatenation (predictions only: labels and draws stay)
    detach_topdown    the top-down add carries no gradient down
"""
import numpy as np
import torch
import torch.nn.functional as F

import pooler_ref as P
import rpn_fpn_loss_ref as LR
from oracle import torch_ref as R

BLOCKS = (("layer1", 3), ("layer2", 4), ("layer3", 6), ("layer4", 3))
FROZEN_PREFIXES = ("backbone.body.stem", "backbone.body.layer1")
MUTATIONS = ("drop_p6_grad", "drop_pool_level2", "swap_rpn_levels", "detach_topdown")
RES, SAMPLING = 7, 2


def is_trainable(key):
    """every key outside the stem and layer1 that is no FrozenBN tensor and no anchor buffer (FREEZE_CONV_BODY_AT 2)"""
    if key.startswith(FROZEN_PREFIXES) or "anchor_generator" in key:
        return False
    mod = key.split(".")[-2]
    return not (mod.startswith("bn") or key.split(".")[-3:-1] == ["downsample", "1"])


def trainable_keys(keys):
    return [k for k in keys if is_trainable(k)]


class _Pool(torch.autograd.Function):
    """pooler_ref.want_forward and its float64 transpose want_backward; maps logical NCHW, result logical [K,C,res,res]"""

    @staticmethod
    def forward(ctx, rois, lv, res, sr, *maps):
        ctx.meta = (rois, lv, res, sr, [tuple(m.shape) for m in maps])
        feats = [m.detach().permute(0, 2, 3, 1).numpy() for m in maps]
        want, _ = P.want_forward(feats, rois, lv, res, res, sr)
        return torch.from_numpy(np.ascontiguousarray(want.transpose(0, 3, 1, 2)))

    @staticmethod
    def backward(ctx, g):
        rois, lv, res, sr, shapes = ctx.meta
        nhwc = [(b, h, w, c) for b, c, h, w in shapes]
        out = P.want_backward(g.permute(0, 2, 3, 1).contiguous().numpy(), rois, lv, nhwc, res, res, sr)
        return (None, None, None, None) + tuple(torch.from_numpy(np.ascontiguousarray(w.transpose(0, 3, 1, 2))) for w, _ in out)


def pool(maps, rois, res=RES, sr=SAMPLING):
    """maps: P2..P5 (logical NCHW float64), rois [K,5] float32 numpy -> (pooled [K,C,res,res], levels)"""
    rois = np.ascontiguousarray(rois, np.float32)
    lv = P.levels(rois)
    assert (lv >= 0).all(), "a RoI without a level"
    return _Pool.apply(rois, lv, res, sr, *maps), lv


def neck(cs, params, mutate=None, first=1, top=True):
    """cs: C2..C5; params {"fpn_inner1": (w, b), ..} -> [P2..P6] (fpn.py:51-79; the maps are each exactly twice the next, as tests/fpn_ref.py::up2).
    first: the block number of cs[0] (RetinaNet's pyramid starts at C3: 2); top=False leaves LastLevelMaxPool's P6 out (tests/detector_retinanet_ref.py
    appends LastLevelP6P7's maps itself)"""
    n = len(cs)
    inner = lambda i, t: F.conv2d(t, *params["fpn_inner%d" % (i + first)])                # noqa: E731
    layer = lambda i, t: F.conv2d(t, *params["fpn_layer%d" % (i + first)], padding=1)     # noqa: E731
    last = inner(n - 1, cs[-1])
    ps = [layer(n - 1, last)]
    for i in range(n - 2, -1, -1):
        assert tuple(cs[i].shape[-2:]) == (2 * last.shape[-2], 2 * last.shape[-1]), "every map is exactly twice the next"
        up = F.interpolate(last.detach() if mutate == "detach_topdown" else last, scale_factor=2, mode="nearest")
        last = inner(i, cs[i]) + up
        ps.insert(0, layer(i, last))
    if not top:
        return ps
    top = ps[-1].detach() if mutate == "drop_p6_grad" else ps[-1]
    ps.append(top[:, :, ::2, ::2])      # F.max_pool2d(x, 1, 2, 0)
    return ps


def rpn_loss(objs, regs, labels, targets, pos_idx, samp_idx, mutate=None):
    """rpn_fpn_loss_ref.losses in torch: objs / regs lists of L [N,A,H,W] / [N,4A,H,W]; labels [N,n], targets [N,n,4] over the concatenation
    (level-major, location row-major, anchor of the cell: concat_predictions' order); pos_idx / samp_idx flat batch indices, < 0 padding.
    BCE with logits and smooth L1 (beta 1/9), both summed and divided by max(#sampled, 1)."""
    N, A = objs[0].shape[:2]
    order = list(range(len(objs)))
    if mutate == "swap_rpn_levels":
        order[1], order[2] = order[2], order[1]
    x = torch.cat([R.permute_and_flatten(objs[l], N, A, 1, *objs[l].shape[-2:]).reshape(N, -1) for l in order], 1).reshape(-1)
    reg = torch.cat([R.permute_and_flatten(regs[l], N, A, 4, *regs[l].shape[-2:]) for l in order], 1).reshape(-1, 4)
    lab = torch.as_tensor(np.asarray(labels, np.float64)).reshape(-1)
    tgt = torch.as_tensor(np.asarray(targets, np.float64)).reshape(-1, 4)
    assert lab.numel() == x.numel(), (lab.numel(), x.numel())
    pos = torch.as_tensor(np.asarray(pos_idx, np.int64)).reshape(-1)
    samp = torch.as_tensor(np.asarray(samp_idx, np.int64)).reshape(-1)
    pos, samp = pos[pos >= 0], samp[samp >= 0]
    den = float(max(samp.numel(), 1))
    xs, ys = x[samp], lab[samp]
    obj = (xs.clamp(min=0) - xs * ys + torch.log1p(torch.exp(-xs.abs()))).sum() / den
    d = (reg[pos] - tgt[pos]).abs()
    box = torch.where(d < LR.BETA, 0.5 * d * d / LR.BETA, d - 0.5 * LR.BETA).sum() / den
    return obj, box


class DetectorFPNRef(object):
    def __init__(self, sd, trainable=True):
        self.p = {}
        for k, v in sd.items():
            t = v.detach().cpu().double().clone()
            if trainable and is_trainable(k):
                t.requires_grad_(True)
            self.p[k] = t

    # ------------------------------------------------------------------------------------------------------------------ body + neck
    def _bn(self, prefix):
        return tuple(self.p[f"{prefix}.{n}"] for n in ("weight", "bias", "running_mean", "running_var"))

    def _block(self, x, prefix, stride):
        has_ds = f"{prefix}.downsample.0.weight" in self.p
        q = {"conv1.weight": self.p[f"{prefix}.conv1.weight"], "conv2.weight": self.p[f"{prefix}.conv2.weight"],
             "conv3.weight": self.p[f"{prefix}.conv3.weight"], "bn1": self._bn(f"{prefix}.bn1"), "bn2": self._bn(f"{prefix}.bn2"),
             "bn3": self._bn(f"{prefix}.bn3")}
        if has_ds:
            q["downsample.0.weight"] = self.p[f"{prefix}.downsample.0.weight"]
            q["ds_bn"] = self._bn(f"{prefix}.downsample.1")
        return R.bottleneck(x, q, stride, has_ds)

    def body(self, images):
        """-> [C2, C3, C4, C5]"""
        b = "backbone.body"
        x = F.relu(R.frozen_bn(F.conv2d(images.double(), self.p[f"{b}.stem.conv1.weight"][:, :3], stride=2, padding=3), *self._bn(f"{b}.stem.bn1")))
        x = F.max_pool2d(x, 3, 2, 1)
        out = []
        for name, n in BLOCKS:
            for i in range(n):
                x = self._block(x, f"{b}.{name}.{i}", (2 if name != "layer1" else 1) if i == 0 else 1)
            out.append(x)
        return out

    def neck(self, cs, mutate=None):
        params = {n: (self.p[f"backbone.fpn.{n}.weight"], self.p[f"backbone.fpn.{n}.bias"])
                  for i in range(1, len(cs) + 1) for n in ("fpn_inner%d" % i, "fpn_layer%d" % i)}
        return neck(cs, params, mutate)

    def features(self, images, mutate=None):
        """-> [P2..P6]"""
        return self.neck(self.body(images), mutate)

    # ------------------------------------------------------------------------------------------------------------------ RPN
    def rpn_head(self, ps):
        """the shared head on every level -> (objs, regs)"""
        h = "rpn.head"
        objs, regs = [], []
        for f in ps:
            t = F.relu(F.conv2d(f, self.p[f"{h}.conv.weight"], self.p[f"{h}.conv.bias"], padding=1))
            objs.append(F.conv2d(t, self.p[f"{h}.cls_logits.weight"], self.p[f"{h}.cls_logits.bias"]))
            regs.append(F.conv2d(t, self.p[f"{h}.bbox_pred.weight"], self.p[f"{h}.bbox_pred.bias"]))
        return objs, regs

    # ------------------------------------------------------------------------------------------------------------------ box head
    def box_head(self, ps, rois, mutate=None):
        """ps: P2..P6 (the pooler reads the first four), rois [K,5] -> (pooled [K,C,7,7], logits [K,nc], box regression [K,4nc], levels)"""
        maps = list(ps[:4])
        if mutate == "drop_pool_level2":
            maps[2] = maps[2].detach()
        pooled, lv = pool(maps, rois)
        fe, pr = "roi_heads.box.feature_extractor", "roi_heads.box.predictor"
        x = F.relu(F.linear(pooled.flatten(1), self.p[f"{fe}.fc6.weight"], self.p[f"{fe}.fc6.bias"]))
        x = F.relu(F.linear(x, self.p[f"{fe}.fc7.weight"], self.p[f"{fe}.fc7.bias"]))
        logits = F.linear(x, self.p[f"{pr}.cls_score.weight"], self.p[f"{pr}.cls_score.bias"])
        reg = F.linear(x, self.p[f"{pr}.bbox_pred.weight"], self.p[f"{pr}.bbox_pred.bias"])
        return pooled, logits, reg, lv

    def grads(self):
        return {k: v.grad for k, v in self.p.items() if v.requires_grad and v.grad is not None}


def step(model, images, rpn_labels, rpn_targets, pos_idx, samp_idx, det_rois, det_labels, det_reg_targets, dist_type="id", n_old=15,
         source=None, soft_rois=None, alpha=0.0, beta=0.0, gamma=1.0, mutate=None, backward=True):
    """One training step's forward (tools/train_incremental.py:82-116 over the FPN detector) and, with `backward`, autograd's gradient of the
    weighted total.  -> dict: ps (P2..P6), objs, regs, logits, boxreg, levels, losses {name: float}, total (float)."""
    ps = model.features(images, mutate)
    objs, regs = model.rpn_head(ps)
    lo, lb = rpn_loss(objs, regs, rpn_labels, rpn_targets, pos_idx, samp_idx, mutate)
    _, logits, boxreg, lv = model.box_head(ps, det_rois, mutate)
    labels = torch.as_tensor(np.asarray(det_labels, np.int64))
    assert (labels >= 0).all(), "a padding row among the sampled RoIs"
    lc, lbox = R.box_head_loss(logits, boxreg, labels, torch.as_tensor(np.asarray(det_reg_targets, np.float64)), dist_type, n_old)
    losses = dict(loss_classifier=lc, loss_box_reg=lbox, loss_objectness=lo, loss_rpn_box_reg=lb)
    total = lc + lbox + lo + lb
    out = dict(ps=ps, objs=objs, regs=regs, logits=logits, boxreg=boxreg, levels=lv)
    if source is not None:
        with torch.no_grad():
            pooled_s, zs, bs, _ = source.box_head(source.features(images), soft_rois)
        pooled_t, zt, bt, lv_s = model.box_head(ps, soft_rois, mutate)
        k_old, k_all = zs.shape[1], zt.shape[1]
        losses["id"] = R.roi_distillation_loss(zs, bs.view(-1, k_old, 4), zt, bt.view(-1, k_all, 4), dist_type)
        losses["ard"] = R.ard_loss(pooled_s, pooled_t, gamma)
        total = total + alpha * losses["id"] + beta * losses["ard"]
        out.update(soft_levels=lv_s, soft_logits=zt)
    if backward:
        total.backward()
    out["losses"] = {k: float(v.detach()) for k, v in losses.items()}
    out["total"] = float(total.detach())
    return out

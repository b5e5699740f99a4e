"""TEST INFRASTRUCTURE ONLY -- torch-CPU float64 restatement of the R-50-FPN-RETINANET detector's training step over a reference-layout state
dict: the body (C3..C5 of tests/detector_fpn_ref.py's), the three-level neck (detector_fpn_ref.neck without its max-pool), LastLevelP6P7 on C5 or
on P5, the shared head on five levels and the RetinaNet loss.  Autograd on it supplies the gradients the whole-detector test compares the HIP
path with (tests/test_gpu_e2e_retinanet.py); tests/test_detector_retinanet_ref.py pins it to the reference's own forward
(tests/golden/e2e_retinanet_tiny.npz) and its loss to tests/retinanet_loss_ref.py.

Built from what exists: retinanet_ref.p6p7_ref's and head_ref's arithmetic as torch graphs (`p6p7`, `head`: those two detach through numpy),
retinanet_loss_ref.losses restated in torch (`loss`: the focal loss through softplus, smooth-L1 with BETA, the denominators n_pos + N and
max(1, n_pos * NORM), ignored anchors and pad columns left out).

`mutate` names one deliberate composition bug (tests/test_detector_retinanet_ref.py::test_fixture_sees_composition_bugs): the fixture has to
move some parameter gradient by far more than the GPU test's bound under each of them.  None of them changes a forward value.
    drop_p7_grad               P7's gradient does not return into P6
    drop_top_grad              nothing returns from P6 into the top block's input (C5, or P5)
    p7_reads_p6_without_relu   P7's gradient passes P6's ReLU unmasked, as if p7 had read P6 itself
    detach_topdown             the top-down add carries no gradient down
    swap_head_levels           levels 1 and 2 change places in the concatenation of the predictions (labels and targets stay)
    head_grad_one_level_short  the head's parameter gradients leave out the coarsest level (its map still gets its gradient)
"""
import numpy as np
import torch
import torch.nn.functional as F

import detector_fpn_ref as D
import retinanet_loss_ref as RL

MUTATIONS = ("drop_p7_grad", "drop_top_grad", "p7_reads_p6_without_relu", "detach_topdown", "swap_head_levels", "head_grad_one_level_short")
TOWERS = (("cls_tower", "cls_logits"), ("bbox_tower", "bbox_pred"))


def is_trainable(key):
    """FREEZE_CONV_BODY_AT 2: everything but the stem, layer1, every FrozenBN tensor and the anchor buffers (detector_fpn_ref's rule; the
    names RetinaNet adds -- rpn.head.cls_tower.N, backbone.fpn.top_blocks.p6 -- fall under it unchanged)"""
    return D.is_trainable(key)


def trainable_keys(keys):
    return [k for k in keys if is_trainable(k)]


def softplus(x):
    """log(1 + e^x) without the threshold of F.softplus (which returns x itself above 20: 2e-9 off in float64)"""
    return torch.logaddexp(x, torch.zeros_like(x))


def p6p7(x, w6, b6, w7, b7, mutate=None):
    """retinanet_ref.p6p7_ref as a graph: x is C5, or P5 with use_P5 -> (P6, P7); fpn.py:82-99"""
    p6 = F.conv2d(x.detach() if mutate == "drop_top_grad" else x, w6, b6, stride=2, padding=1)
    src = p6.detach() if mutate == "drop_p7_grad" else p6
    r6 = F.relu(src)
    if mutate == "p7_reads_p6_without_relu":
        r6 = src + (r6 - src).detach()      # relu(P6)'s value with the identity's gradient
    return p6, F.conv2d(r6, w7, b7, stride=2, padding=1)


def head(ps, p, num_convs, prefix="rpn.head.", mutate=None, pre=None):
    """retinanet_ref.head_ref as a graph: the shared towers and output convs on every map -> (logits [N,A*C,H,W], deltas [N,4A,H,W]) per
    level.  pre: a list that receives every tower ReLU's input (the fixture keeps them away from zero)."""
    logits, deltas = [], []
    for l, x in enumerate(ps):
        q = p
        if mutate == "head_grad_one_level_short" and l == len(ps) - 1:
            q = {k: v.detach() for k, v in p.items()}
        outs = []
        for tower, last in TOWERS:
            t = x
            for n in range(num_convs):
                t = F.conv2d(t, q["%s%s.%d.weight" % (prefix, tower, 2 * n)], q["%s%s.%d.bias" % (prefix, tower, 2 * n)], padding=1)
                if pre is not None:
                    pre.append(t)
                t = F.relu(t)
            outs.append(F.conv2d(t, q[prefix + last + ".weight"], q[prefix + last + ".bias"], padding=1))
        logits.append(outs[0])
        deltas.append(outs[1])
    return logits, deltas


def loss(logits, deltas, labels, targets, mutate=None, gamma=RL.GAMMA, alpha=RL.ALPHA, beta=RL.BETA, norm=RL.NORM):
    """retinanet_loss_ref.losses in torch: logits / deltas lists of L [N,A*C,H,W] / [N,4A,H,W]; labels [N,n] (class, 0 background, -1
    ignored), targets [N,n,4] over the levels' concatenated anchors (level-major, location row-major, anchor of the cell)
    -> (focal loss / (n_pos + N), smooth-L1 over the positives / max(1, n_pos * norm), n_pos)"""
    N = logits[0].shape[0]
    A = deltas[0].shape[1] // 4
    C = logits[0].shape[1] // A
    order = list(range(len(logits)))
    if mutate == "swap_head_levels":
        order[1], order[2] = order[2], order[1]
    x = torch.cat([logits[l].permute(0, 2, 3, 1).reshape(N, -1, C) for l in order], 1)
    d = torch.cat([deltas[l].permute(0, 2, 3, 1).reshape(N, -1, 4) for l in order], 1)
    lab = torch.as_tensor(np.asarray(labels, np.int64))
    tgt = torch.as_tensor(np.asarray(targets, np.float64))
    assert tuple(lab.shape) == tuple(x.shape[:2]) and tuple(tgt.shape) == tuple(d.shape), (lab.shape, x.shape, tgt.shape, d.shape)
    n_pos = int((lab > 0).sum())
    positive = lab[:, :, None] == torch.arange(1, C + 1)[None, None, :]
    live = (lab >= 0)[:, :, None].expand_as(x)
    p, q = torch.sigmoid(x), torch.sigmoid(-x)
    v = torch.where(positive, alpha * q ** gamma * softplus(-x), (1 - alpha) * p ** gamma * softplus(x))      # -log p = softplus(-x)
    cls = v[live].sum() / float(n_pos + N)
    pos = lab > 0
    e = (d[pos] - tgt[pos]).abs()
    reg = torch.where(e < beta, 0.5 * e * e / beta, e - 0.5 * beta).sum() / float(max(1.0, n_pos * norm))
    return cls, reg, n_pos


class DetectorRetinaNetRef(D.DetectorFPNRef):
    """the parameters as float64 leaves (the trainable ones with requires_grad), DetectorFPNRef's body"""

    def __init__(self, sd, trainable=True):
        self.p = {}
        for k, v in sd.items():
            t = v.detach().cpu().double().clone()
            if trainable and is_trainable(k):
                t.requires_grad_(True)
            self.p[k] = t
        self.num_convs = sum(k.startswith("rpn.head.cls_tower.") and k.endswith(".weight") for k in self.p)
        w6 = self.p["backbone.fpn.top_blocks.p6.weight"]
        self.use_p5 = w6.shape[1] == w6.shape[0]      # LastLevelP6P7.use_P5: in_channels == out_channels

    def features(self, images, mutate=None, keep=None):
        """-> [P3..P7]; keep: a dict that receives the body's maps"""
        cs = self.body(images)[1:]      # C3..C5: the first level is skipped, there is no fpn_inner1 / fpn_layer1
        if keep is not None:
            keep["cs"] = cs
        params = {n: (self.p[f"backbone.fpn.{n}.weight"], self.p[f"backbone.fpn.{n}.bias"]) for i in (2, 3, 4) for n in ("fpn_inner%d" % i, "fpn_layer%d" % i)}
        assert "backbone.fpn.fpn_inner1.weight" not in self.p
        ps = D.neck(cs, params, mutate, first=2, top=False)
        t = "backbone.fpn.top_blocks."
        p6, p7 = p6p7(ps[-1] if self.use_p5 else cs[-1], self.p[t + "p6.weight"], self.p[t + "p6.bias"], self.p[t + "p7.weight"], self.p[t + "p7.bias"],
                      mutate)
        return ps + [p6, p7]


def step(model, images, labels, targets, use_p5, mutate=None, backward=True):
    """One training step's forward and, with `backward`, autograd's gradient of loss_retina_cls + loss_retina_reg.
    -> dict: ps (P3..P7), logits, deltas (per level, NCHW), pre (the tower ReLUs' inputs), losses {name: float}, n_pos, total (float)"""
    assert bool(use_p5) == model.use_p5, "the state dict's p6 reads %s" % ("P5" if model.use_p5 else "C5")
    ps = model.features(images, mutate)
    pre = []
    logits, deltas = head(ps, model.p, model.num_convs, mutate=mutate, pre=pre)
    lc, lr, n_pos = loss(logits, deltas, labels, targets, mutate)
    total = lc + lr
    if backward:
        total.backward()
    return dict(ps=ps, logits=logits, deltas=deltas, pre=pre, n_pos=n_pos, total=float(total.detach()),
                losses=dict(loss_retina_cls=float(lc.detach()), loss_retina_reg=float(lr.detach())))

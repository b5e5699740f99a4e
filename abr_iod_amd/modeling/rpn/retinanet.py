"""RetinaNet on the HIP library: head (forward and backward), anchors, loss, post-processor, module.

Mirrors
    make_anchor_generator_retinanet   maskrcnn_benchmark/modeling/rpn/anchor_generator.py:141-161
    RetinaNetHead                     modeling/rpn/retinanet/retinanet.py:13-85
    RetinaNetPostProcessor            modeling/rpn/retinanet/inference.py:14-194
    RetinaNetModule / build_retinanet modeling/rpn/retinanet/retinanet.py:88-152
    RetinaNetLossComputation, generate_retinanet_labels, make_retinanet_loss_evaluator
                                      modeling/rpn/retinanet/loss.py (over rpn/loss.py:66-102)

MI355X-first differences (results identical):
  * the head runs on NHWC maps: the towers through conv_stack_forward, the output convs with their bias in the epilogue.  An NHWC output
    [N,H,W,A*C] already IS the reference's permute_and_flatten order (location-major, then anchor, then class), so no permute kernels exist;
  * the post-processor is ONE library call for the whole batch (ops.retina_detect: 1 memset + 4 launches whatever N, L and the class count
    are) and ONE read-back of the per-image counts, where the reference loops over images, levels and classes on the host.

  * the loss reads the NHWC outputs where they lie (no permute + cat of ten tensors): ops.retina_targets labels the concatenated anchors of
    the whole batch in two launches, ops.retina_loss sums the focal loss over every (anchor, class) and the smooth-L1 over the positives in
    one, and its backward writes the gradient of every level into ONE allocation per output, which the head's backward reads in place;
  * the head in training is ONE autograd node for both towers and both output convs over all levels (RetinaNetHead.forward_train): the
    weight and bias gradients of the five levels accumulate in the flat gradient buffer.

Training needs targets: one BoxList with a `labels` field per image.  A call without them raises MissingTargets (a ValueError and, as while
the loss was missing, a NotImplementedError).  An image whose BoxList is empty is all background (the reference crashes there).
"""
import math

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import ops
from ...layers import SigmoidFocalLoss
from ...layers._layout import as_nhwc, from_nhwc
from ...structures.bounding_box import BoxList
from ..backbone.resnet import Conv2d, _grad_buf
from ..box_coder import BoxCoder
from ..matcher import Matcher
from ..roi_heads.conv_stack import conv_stack_backward, conv_stack_forward
from .rpn import AnchorGenerator, MissingTargets


def require_targets(what, targets, n_images=None):
    """Training RetinaNet needs one ground-truth BoxList carrying `labels` per image.  Anything else is a bad value for the caller
    (MissingTargets: a ValueError) -- and, as while the loss was missing, a NotImplementedError for callers that caught that.  Checked before
    the backbone or the library is touched."""
    def usable(t):
        return isinstance(t, BoxList) and t.has_field("labels")
    ok = isinstance(targets, (list, tuple)) and len(targets) > 0 and all(usable(t) for t in targets) \
        and (n_images is None or len(targets) == n_images)
    if ok:
        return
    if targets is None:
        shown = "None"
    elif isinstance(targets, (list, tuple)):
        shown = "[{}]".format(", ".join("None" if t is None else ("BoxList without 'labels'" if isinstance(t, BoxList) else type(t).__name__)
                                        for t in targets))
    else:
        shown = type(targets).__name__
    raise MissingTargets("{} in training mode got targets={}{}: the RetinaNet loss is not built without one ground-truth BoxList (with 'labels') "
                         "per image; eval() detects".format(what, shown, "" if n_images is None else " for {} images".format(n_images)))


def retinanet_anchor_sizes(cfg):
    """anchor_generator.py:149-155: per level the SCALES_PER_OCTAVE sizes size * OCTAVE ** (i / SCALES_PER_OCTAVE), in double precision"""
    r = cfg.MODEL.RETINANET
    return tuple(tuple(r.OCTAVE ** (i / float(r.SCALES_PER_OCTAVE)) * size for i in range(r.SCALES_PER_OCTAVE)) for size in r.ANCHOR_SIZES)


def make_anchor_generator_retinanet(cfg):
    r = cfg.MODEL.RETINANET
    assert len(r.ANCHOR_STRIDES) == len(r.ANCHOR_SIZES), "Only support FPN now"
    return AnchorGenerator(retinanet_anchor_sizes(cfg), r.ASPECT_RATIOS, r.ANCHOR_STRIDES, r.STRADDLE_THRESH)


class RetinaNetHead(nn.Module):
    """retinanet.py:13-85.  cls_tower / bbox_tower: NUM_CONVS x (3x3 conv + ReLU) as nn.Sequential, so the convs sit in the even slots and the
    state-dict keys are the reference's (cls_tower.0, cls_tower.2, ...); cls_logits (A * C outputs, C = NUM_CLASSES - 1) and bbox_pred (4A) are
    3x3 convs.  Where A * C is no multiple of 4 the cls_logits conv is computed with zero rows up to the next one (`ld_cls`); the checkpoint
    boundary stores the real rows."""

    def __init__(self, cfg, in_channels):
        super().__init__()
        r = cfg.MODEL.RETINANET
        self.num_classes = r.NUM_CLASSES - 1
        self.num_anchors = len(r.ASPECT_RATIOS) * r.SCALES_PER_OCTAVE
        if in_channels % 4:
            raise NotImplementedError("RetinaNetHead: {} input channels, need a multiple of 4".format(in_channels))
        n_cls = self.num_anchors * self.num_classes
        self.ld_cls, self.ld_reg = (n_cls + 3) // 4 * 4, self.num_anchors * 4
        for name in ("cls_tower", "bbox_tower"):
            layers = []
            for _ in range(r.NUM_CONVS):
                layers += [Conv2d(in_channels, in_channels, 3, stride=1, padding=1), nn.ReLU()]   # (the ReLU rides in the conv's epilogue)
            self.add_module(name, nn.Sequential(*layers))
        self.cls_logits = Conv2d(in_channels, n_cls, 3, stride=1, padding=1, cout_pad=self.ld_cls if self.ld_cls != n_cls else None)
        self.bbox_pred = Conv2d(in_channels, self.ld_reg, 3, stride=1, padding=1)
        for conv in self._tower("cls_tower") + self._tower("bbox_tower") + [self.cls_logits, self.bbox_pred]:
            with torch.no_grad():
                nn.init.normal_(conv.weight[: conv.out_channels], std=0.01)
        prior_prob = r.PRIOR_PROB   # retinanet_bias_init
        with torch.no_grad():
            self.cls_logits.bias[:n_cls].fill_(-math.log((1 - prior_prob) / prior_prob))
        self.math = ops.MATH_F32   # see backbone.resnet.set_conv_math

    def _tower(self, name):
        return [m for m in getattr(self, name) if isinstance(m, Conv2d)]

    def _out(self, x, conv):
        return ops.conv_forward(x, conv.weight, 1, 1, bias=conv.bias, math=self.math, w_version=conv.version())

    def prep_entries(self):
        """FusedSGD's batched weight preparation (see Bottleneck.prep_entries)"""
        convs = self._tower("cls_tower") + self._tower("bbox_tower") + [self.cls_logits, self.bbox_pred]
        return [(c, None, 1, 1, self.math) for c in convs if c.weight.requires_grad and c.weight.is_cuda]

    def forward_train(self, features):
        """The training entry: list of L maps, logical [N,C,H_l,W_l] -> (list of L cls NHWC [N,H_l,W_l,ld_cls], list of L reg NHWC
        [N,H_l,W_l,4A]) out of ONE autograd node (_HeadTrainFn).  Its backward adds every level's weight and bias gradients into the flat
        gradient buffer and hands each map the sum of the two towers' input gradients; the pad rows of cls_logits get exactly zero."""
        features = list(features)
        outs = _HeadTrainFn.apply(self, len(features), *features, *self.parameters())
        return list(outs[:len(features)]), list(outs[len(features):])

    def forward_nhwc(self, x):
        """x logical [N,C,H,W] -> (cls [N,H,W,ld_cls], reg [N,H,W,4A]) NHWC: column a * C + c the logit of (anchor a, class c + 1), columns
        4a .. 4a+3 anchor a's deltas; the columns of cls past A * C are padding"""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("RetinaNetHead.forward / forward_nhwc: the backward is not built on the reference's per-level signature; "
                                      "training goes through forward_train (one node over all levels), everything else under torch.no_grad()")
        xh = as_nhwc(x)
        cls = self._out(conv_stack_forward(self._tower("cls_tower"), xh, self.math), self.cls_logits)
        reg = self._out(conv_stack_forward(self._tower("bbox_tower"), xh, self.math), self.bbox_pred)
        return cls, reg

    def forward(self, x):
        """reference signature: list of maps -> (list of logical [N,A*C,H,W], list of logical [N,4A,H,W])"""
        n_cls = self.num_anchors * self.num_classes
        logits, bbox_reg = [], []
        for feature in x:
            cls, reg = self.forward_nhwc(feature)
            logits.append(from_nhwc(cls)[:, :n_cls])
            bbox_reg.append(from_nhwc(reg))
        return logits, bbox_reg


class _HeadTrainFn(Function):
    """(head, L, *maps logical [N,C,H_l,W_l], *parameters) -> L cls outputs then L reg outputs, NHWC.  Forward: per level the two towers through
    conv_stack_forward(keep=True) and the two output convs with their bias in the epilogue.  Backward, per level: the output convs' weight, bias
    and input gradients, then conv_stack_backward for each tower; the towers' two input gradients are added into the map's gradient."""

    @staticmethod
    def forward(ctx, head, nL, *args):
        math, saved = head.math, []
        cls_out, reg_out = [], []
        for f in args[:nL]:
            xh = as_nhwc(f)
            level = []
            for tower, last, out in ((head._tower("cls_tower"), head.cls_logits, cls_out), (head._tower("bbox_tower"), head.bbox_pred, reg_out)):
                acts, vs = conv_stack_forward(tower, xh, math, keep=True)
                v = ops.wino_v_alloc(acts[-1], last.weight, 1, 1, math) if last.weight.requires_grad else None
                out.append(ops.conv_forward(acts[-1], last.weight, 1, 1, bias=last.bias, math=math, wino_v=v, w_version=last.version()))
                level.append((acts, vs, v))
            saved.append(level)
        ctx.head, ctx.nL, ctx.saved = head, nL, saved
        return tuple(cls_out) + tuple(reg_out)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        head, nL, saved = ctx.head, ctx.nL, ctx.saved
        ctx.saved = None
        math = head.math
        gmaps = []
        for l in range(nL):
            need_dx = ctx.needs_input_grad[2 + l]
            gx = None
            for k, (tower, last) in enumerate(((head._tower("cls_tower"), head.cls_logits), (head._tower("bbox_tower"), head.bbox_pred))):
                g = grads[k * nL + l]
                if g is None:       # this output took no part in the loss
                    continue
                g = g if g.is_contiguous() else g.contiguous()
                acts, vs, v = saved[l][k]
                if last.weight.requires_grad:
                    ops.conv_wgrad_async(acts[-1], g, _grad_buf(last.weight), 1, 1, math=math, wino_v=v)
                    ops.bias_grad(g, _grad_buf(last.bias))
                below = any(c.weight.requires_grad for c in tower)
                if not (below or need_dx):
                    continue
                gt = ops.conv_forward(g, last.dgrad_weight(), 1, 1, math=math, w_version=last.version())
                gp = conv_stack_backward(tower, acts, vs, gt, math, need_dx)
                if gp is not None:
                    gx = gp if gx is None else ops.add_(gx, gp)
            gmaps.append(from_nhwc(gx) if gx is not None else None)
            saved[l] = None
        return (None, None) + tuple(gmaps) + (None,) * (len(ctx.needs_input_grad) - 2 - nL)


# ------------------------------------------------------------------------------------------------ loss
class _RetinaLossFn(Function):
    """(evaluator numbers, L, labels, reg_targets, n_pos, *cls NHWC, *reg NHWC) -> (loss_retina_cls, loss_retina_reg): ops.retina_loss reads the
    head's outputs where they lie; backward returns the views of the two gradient allocations of ops.retina_loss_backward (every element written
    by one launch: the derivative is recomputed from the logits)."""

    @staticmethod
    def forward(ctx, nums, nL, labels, reg_targets, n_pos, *outs):
        cls, reg = list(outs[:nL]), list(outs[nL:])
        losses = ops.retina_loss(cls, reg, *nums[:2], labels, reg_targets, n_pos, *nums[2:])
        ctx.nums, ctx.nL, ctx.saved = nums, nL, (cls, reg, labels, reg_targets, n_pos)
        return losses[0], losses[1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g_cls, g_reg):
        cls, reg, labels, reg_targets, n_pos = ctx.saved
        ctx.saved = None
        zero = None
        if g_cls is None or g_reg is None:
            zero = torch.zeros((1,), dtype=torch.float32, device=cls[0].device)
        d_cls, d_reg = ops.retina_loss_backward(cls, reg, *ctx.nums[:2], labels, reg_targets, n_pos, *ctx.nums[2:],
                                                zero if g_cls is None else g_cls.reshape(1), zero if g_reg is None else g_reg.reshape(1))
        need = ctx.needs_input_grad[5:]
        return (None,) * 5 + tuple(g if n else None for g, n in zip(d_cls + d_reg, need))


def generate_retinanet_labels(matched_targets):
    """loss.py:87-89: an anchor's label is its matched ground truth's class (the library's abr::head_label applies the same rule on the device)"""
    return matched_targets.get_field("labels")


class RetinaNetLossComputation(object):
    """loss.py:19-84 over rpn/loss.py:66-102: copied_fields = ['labels'], discard_cases = ['between_thresholds'] (no visibility discard), the
    Matcher with low-quality matches over the levels' concatenated anchors; sigmoid focal loss over every anchor with a label >= 0 and every
    class / (#positives + N), smooth-L1(beta) over the positives / max(1, #positives * regress_norm).  `last_targets` keeps what was drawn
    (per image: labels int32 [n], regression targets [n,4]) and `last_n_pos` the device count of positives, as the RPN's evaluator does."""

    def __init__(self, proposal_matcher, box_coder, generate_labels_func, sigmoid_focal_loss, bbox_reg_beta=0.11, regress_norm=1.0):
        self.proposal_matcher, self.box_coder = proposal_matcher, box_coder
        self.generate_labels_func = generate_labels_func
        self.box_cls_loss_func = sigmoid_focal_loss      # read for its gamma and alpha: the sum runs where the logits lie (csrc/focal.h's element)
        self.bbox_reg_beta, self.regress_norm = bbox_reg_beta, regress_norm
        self.copied_fields = ["labels"]
        self.discard_cases = ["between_thresholds"]
        self.last_targets = self.last_n_pos = None

    def prepare_targets(self, anchors, targets):
        """anchors: per image the list of L BoxLists AnchorGenerator returns (one grid for the batch) -> labels int32 [N,n], regression targets
        [N,n,4], n_pos [1] int32, all on the device"""
        first = anchors[0]
        first = list(first) if isinstance(first, (list, tuple)) else [first]
        pyr = getattr(first[0], "_pyramid", None)
        boxes = pyr[0] if pyr is not None and len(first) > 1 else (first[0].bbox if len(first) == 1 else torch.cat([b.bbox for b in first]))
        m = self.proposal_matcher
        return ops.retina_targets(boxes, [t.bbox for t in targets], [t.get_field("labels") for t in targets], m.high_threshold, m.low_threshold,
                                  self.box_coder.weights)

    def call_nhwc(self, anchors, cls, reg, targets, num_anchors, num_classes):
        """cls / reg: lists of L NHWC head outputs [N,H_l,W_l,ld]; num_classes: foreground classes -> (loss_retina_cls, loss_retina_reg)"""
        require_targets("RetinaNetLossComputation", targets, cls[0].shape[0])
        labels, reg_targets, n_pos = self.prepare_targets(anchors, targets)
        self.last_targets, self.last_n_pos = (list(labels.unbind(0)), list(reg_targets.unbind(0))), n_pos
        gamma, alpha = self.box_cls_loss_func.gamma, self.box_cls_loss_func.alpha
        nums = (int(num_anchors), int(num_classes), float(gamma), float(alpha), float(self.bbox_reg_beta), float(self.regress_norm))
        return _RetinaLossFn.apply(nums, len(cls), labels, reg_targets, n_pos, *cls, *reg)

    def __call__(self, anchors, box_cls, box_regression, targets):
        """the reference's signature: lists of L logical [N,A*C,H,W] / [N,4A,H,W].  The logits are copied into rows of a multiple of 4 columns
        where A * C is none (the module itself hands the head's NHWC outputs to call_nhwc: no copy)."""
        A = box_regression[0].shape[1] // 4
        C = box_cls[0].shape[1] // A
        cls = []
        for c in box_cls:
            c = as_nhwc(c)
            cls.append(nn.functional.pad(c, (0, -c.shape[-1] % 4)).contiguous())
        return self.call_nhwc(anchors, cls, [as_nhwc(r).contiguous() for r in box_regression], targets, A, C)


def make_retinanet_loss_evaluator(cfg, box_coder):
    r = cfg.MODEL.RETINANET
    matcher = Matcher(r.FG_IOU_THRESHOLD, r.BG_IOU_THRESHOLD, allow_low_quality_matches=True)
    return RetinaNetLossComputation(matcher, box_coder, generate_retinanet_labels, SigmoidFocalLoss(r.LOSS_GAMMA, r.LOSS_ALPHA), bbox_reg_beta=r.BBOX_REG_BETA,
                                    regress_norm=r.BBOX_REG_WEIGHT)


class RetinaNetPostProcessor(nn.Module):
    """inference.py:14-194 for the whole batch on the device (ops.retina_detect).  Where the reference leaves an order open the library fixes
    it: equal scores inside a level go by ascending flat index loc * A * C + a * C + c (topk(sorted=False)), equal scores inside a class by
    ascending candidate position level * pre_nms_top_n + rank."""

    def __init__(self, pre_nms_thresh, pre_nms_top_n, nms_thresh, fpn_post_nms_top_n, min_size, num_classes, box_coder=None):
        super().__init__()
        self.pre_nms_thresh, self.pre_nms_top_n, self.nms_thresh = pre_nms_thresh, pre_nms_top_n, nms_thresh
        self.fpn_post_nms_top_n, self.min_size, self.num_classes = fpn_post_nms_top_n, min_size, num_classes
        self.box_coder = box_coder if box_coder is not None else BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
        self._hw_cache = {}

    def launch(self, anchors, cls, reg, num_anchors):
        """cls / reg: lists of L NHWC head outputs [N,H_l,W_l,ld]; anchors: list (per image) of L BoxLists -> the device-side result, nothing
        read back"""
        nL = len(cls)
        if nL < 2:
            raise NotImplementedError("RetinaNetPostProcessor on one feature level: the reference skips select_over_all_levels there (no class-wise "
                                      "NMS); the RetinaNet bodies give five levels")
        limit = min(ops.rpn_pyramid_max_k(), ops.retina_max_candidates() // nL)
        if self.pre_nms_top_n > limit:
            raise ValueError("MODEL.RETINANET.PRE_NMS_TOP_N = {} on {} levels: at most {} candidates are ranked per level ({} per image)"
                             .format(self.pre_nms_top_n, nL, limit, ops.retina_max_candidates()))
        N = cls[0].shape[0]
        for l in range(nL):
            assert all(a[l].bbox.data_ptr() == anchors[0][l].bbox.data_ptr() for a in anchors), \
                "per-image anchor grids of one batch share (H,W): they differ only in the visibility field"
        hw = tuple((a[0].size[1], a[0].size[0]) for a in anchors)
        key = (hw, cls[0].device)
        img_hw = self._hw_cache.get(key)
        if img_hw is None:
            if len(self._hw_cache) > 64:
                self._hw_cache.clear()
            img_hw = self._hw_cache[key] = ops.h2d([list(v) for v in hw], torch.int32, cls[0].device)
        boxes, scores, labels, n_out = ops.retina_detect(
            [c.reshape(N, c.shape[1] * c.shape[2], c.shape[3]) for c in cls], [r.reshape(N, r.shape[1] * r.shape[2], r.shape[3]) for r in reg],
            [anchors[0][l].bbox for l in range(nL)], num_anchors, self.num_classes - 1, img_hw, self.pre_nms_thresh, self.pre_nms_top_n,
            self.nms_thresh, self.fpn_post_nms_top_n, self.box_coder.weights, self.min_size)
        return dict(boxes=boxes, scores=scores, labels=labels, n_out=n_out, sizes=[a[0].size for a in anchors])

    def collect(self, pending):
        """Host half: the one read-back (the per-image counts), then one BoxList per image with `scores` and `labels`"""
        nk = pending["n_out"].tolist()
        result = []
        for i, size in enumerate(pending["sizes"]):
            b = BoxList(pending["boxes"][i, : nk[i]], size, mode="xyxy")
            b.add_field("scores", pending["scores"][i, : nk[i]])
            b.add_field("labels", pending["labels"][i, : nk[i]])
            result.append(b)
        return result

    def forward_nhwc(self, anchors, cls, reg, num_anchors):
        return self.collect(self.launch(anchors, cls, reg, num_anchors))

    def forward(self, anchors, box_cls, box_regression, targets=None):
        """reference signature: lists of L logical [N,A*C,H,W] / [N,4A,H,W]"""
        A = box_regression[0].shape[1] // 4
        return self.forward_nhwc(anchors, [as_nhwc(c).contiguous() for c in box_cls], [as_nhwc(r).contiguous() for r in box_regression], A)


def make_retinanet_postprocessor(config, rpn_box_coder, is_train):
    r = config.MODEL.RETINANET
    return RetinaNetPostProcessor(pre_nms_thresh=r.INFERENCE_TH, pre_nms_top_n=r.PRE_NMS_TOP_N, nms_thresh=r.NMS_TH,
                                  fpn_post_nms_top_n=config.TEST.DETECTIONS_PER_IMG, min_size=0, num_classes=r.NUM_CLASSES,
                                  box_coder=rpn_box_coder)


class RetinaNetModule(nn.Module):
    """retinanet.py:88-152, with the RPN's return convention so that the detector calls it like RPNModule."""

    def __init__(self, cfg, in_channels):
        super().__init__()
        self.cfg = cfg.clone()
        self.anchor_generator = make_anchor_generator_retinanet(cfg)
        self.head = RetinaNetHead(cfg, in_channels)
        box_coder = BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
        self.box_selector_test = make_retinanet_postprocessor(cfg, box_coder, is_train=False)
        self.loss_evaluator = make_retinanet_loss_evaluator(cfg, box_coder)

    def forward(self, images, features, targets=None, rpn_output_source=None, defer_proposals=False):
        """eval -> ((boxes, {}), anchors, (box_cls, box_regression)): one BoxList of detections per image, the levels' anchors, and the head's
        outputs under the reference's names and shapes (views of the NHWC results).
        training (retinanet.py:120-135) -> ((anchors, {"loss_retina_cls", "loss_retina_reg"}), anchors, (box_cls, box_regression))"""
        if self.training:
            require_targets("RetinaNetModule", targets)
        if defer_proposals:
            raise NotImplementedError("RetinaNetModule: deferred proposals belong to the distillation pass, which is not built on RetinaNet")
        head = self.head
        n_cls = head.num_anchors * head.num_classes
        if self.training:
            cls, reg = head.forward_train(features)
            with torch.no_grad():
                anchors = self.anchor_generator(images, features)
            loss_cls, loss_reg = self.loss_evaluator.call_nhwc(anchors, cls, reg, targets, head.num_anchors, head.num_classes)
            losses = {"loss_retina_cls": loss_cls, "loss_retina_reg": loss_reg}
            return (anchors, losses), anchors, ([from_nhwc(c)[:, :n_cls] for c in cls], [from_nhwc(r) for r in reg])
        with torch.no_grad():
            outs = [head.forward_nhwc(f) for f in features]
            cls, reg = [o[0] for o in outs], [o[1] for o in outs]
            anchors = self.anchor_generator(images, features)
            boxes = self.box_selector_test.forward_nhwc(anchors, cls, reg, head.num_anchors)
        return (boxes, {}), anchors, ([from_nhwc(c)[:, :n_cls] for c in cls], [from_nhwc(r) for r in reg])


def build_retinanet(cfg, in_channels):
    return RetinaNetModule(cfg, in_channels)

"""RetinaNet on the HIP library: the inference half (head forward, anchors, post-processor, module).

Mirrors
    make_anchor_generator_retinanet   maskrcnn_benchmark/modeling/rpn/anchor_generator.py:141-161
    RetinaNetHead                     modeling/rpn/retinanet/retinanet.py:13-85
    RetinaNetPostProcessor            modeling/rpn/retinanet/inference.py:14-194
    RetinaNetModule / build_retinanet modeling/rpn/retinanet/retinanet.py:88-152

MI355X-first differences (results identical):
  * the head runs on NHWC maps: the towers through conv_stack_forward, the output convs with their bias in the epilogue.  An NHWC output
    [N,H,W,A*C] already IS the reference's permute_and_flatten order (location-major, then anchor, then class), so no permute kernels exist;
  * the post-processor is ONE library call for the whole batch (ops.retina_detect: 1 memset + 4 launches whatever N, L and the class count
    are) and ONE read-back of the per-image counts, where the reference loops over images, levels and classes on the host.

The loss (rpn/retinanet/loss.py) and the head's backward are not built: the module raises in training mode.
"""
import math

import torch
from torch import nn

from ... import ops
from ...layers._layout import as_nhwc, from_nhwc
from ...structures.bounding_box import BoxList
from ..backbone.resnet import Conv2d
from ..box_coder import BoxCoder
from ..roi_heads.conv_stack import conv_stack_forward
from .rpn import AnchorGenerator


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

    def forward_nhwc(self, x):
        """x logical [N,C,H,W] -> (cls [N,H,W,ld_cls], reg [N,H,W,4A]) NHWC: column a * C + c the logit of (anchor a, class c + 1), columns
        4a .. 4a+3 anchor a's deltas; the columns of cls past A * C are padding"""
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            raise NotImplementedError("RetinaNetHead: the head's backward is not built (the RetinaNet loss is not built either); call it "
                                      "under torch.no_grad()")
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
    """retinanet.py:88-152 in eval, with the RPN's return convention so that the detector calls it like RPNModule."""

    def __init__(self, cfg, in_channels):
        super().__init__()
        self.cfg = cfg.clone()
        self.anchor_generator = make_anchor_generator_retinanet(cfg)
        self.head = RetinaNetHead(cfg, in_channels)
        box_coder = BoxCoder(weights=(10.0, 10.0, 5.0, 5.0))
        self.box_selector_test = make_retinanet_postprocessor(cfg, box_coder, is_train=False)

    def forward(self, images, features, targets=None, rpn_output_source=None, defer_proposals=False):
        """-> ((boxes, {}), anchors, (box_cls, box_regression)): one BoxList of detections per image, the levels' anchors, and the head's outputs
        under the reference's names and shapes (views of the NHWC results)"""
        if self.training:
            raise NotImplementedError("RetinaNetModule in training mode: the RetinaNet loss is not built (rpn/retinanet/loss.py, the focal "
                                      "kernels' caller) and neither is the head's backward; eval() detects")
        if defer_proposals:
            raise NotImplementedError("RetinaNetModule: deferred proposals belong to the distillation pass, which is not built on RetinaNet")
        head = self.head
        n_cls = head.num_anchors * head.num_classes
        with torch.no_grad():
            outs = [head.forward_nhwc(f) for f in features]
            cls, reg = [o[0] for o in outs], [o[1] for o in outs]
            anchors = self.anchor_generator(images, features)
            boxes = self.box_selector_test.forward_nhwc(anchors, cls, reg, head.num_anchors)
        return (boxes, {}), anchors, ([from_nhwc(c)[:, :n_cls] for c in cls], [from_nhwc(r) for r in reg])


def build_retinanet(cfg, in_channels):
    return RetinaNetModule(cfg, in_channels)

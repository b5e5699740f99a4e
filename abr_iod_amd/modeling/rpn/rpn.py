"""Region Proposal Network on the HIP library.

Mirrors, for the single-level C4 case every configs/voc YAML uses and over a feature pyramid (anchors, proposal selection, and the loss over the
levels' concatenated anchors, so RPNModule trains on an FPN body):
    AnchorGenerator          maskrcnn_benchmark/modeling/rpn/anchor_generator.py:34-123, 215-284
    RPNHead                  modeling/rpn/rpn.py:70-121  (conv3x3+ReLU, cls_logits 1x1, bbox_pred 1x1)
    RPNPostProcessor         modeling/rpn/inference.py:14-147
    RPNLossComputation       modeling/rpn/loss.py:21-148
    RPNModule / build_rpn    modeling/rpn/rpn.py:124-230

MI355X-first differences (results identical):
  * cls_logits and bbox_pred are ONE 1x1 conv with 15+60(+1 pad)=76 output channels over the shared 3x3 feature: the
    1024-channel tensor `t` is read once.  The NHWC output [N,H,W,76] already IS the reference's
    permute_and_flatten order (location-major, anchor-minor; rpn/utils.py:10-14), so no permute kernels exist.
  * proposals for all images are decoded / clipped / NMS-ed in batched launches; the greedy NMS sweep stays on device.
  * anchors are cached per (H, W, image size) instead of being rebuilt with numpy every step.
  * IoU + Matcher + labels + BoxCoder.encode for 35 910 anchors is one kernel per image.
  * over L > 1 levels the loss never concatenates predictions: the levels' anchors are ONE cached tensor (AnchorGenerator.pyramid), matching and
    sampling run over it as over a single level, and abr_rpn_pyramid_loss reads each sampled anchor out of its level's fused output by address
    (one launch); the backward is one memset of the levels' gradients (one allocation) plus one scatter of the sampled entries.
"""
import math

import numpy as np
import os

import torch
from torch import nn
from torch.autograd import Function

from ... import ops
from ...layers._layout import as_nhwc, from_nhwc
from ...structures.bounding_box import BoxList
from ...structures.image_list import ImageList
from ..backbone.resnet import Conv2d, _grad_buf
from ..balanced_positive_negative_sampler import BalancedPositiveNegativeSampler
from ..box_coder import BoxCoder
from ..matcher import Matcher


# ------------------------------------------------------------------------------------------------ anchors
def generate_anchors(stride=16, sizes=(32, 64, 128, 256, 512), aspect_ratios=(0.5, 1, 2)):
    """Cell anchors (anchor_generator.py:215-284): float64, numpy round (half-to-even) on the ratio enumeration."""
    base = float(stride)
    xc = yc = 0.5 * (base - 1)
    area = base * base
    out = []
    for r in aspect_ratios:
        ws = np.round(np.sqrt(area / r))
        hs = np.round(ws * r)
        x1, y1, x2, y2 = xc - 0.5 * (ws - 1), yc - 0.5 * (hs - 1), xc + 0.5 * (ws - 1), yc + 0.5 * (hs - 1)
        w0, h0 = x2 - x1 + 1, y2 - y1 + 1
        cx, cy = x1 + 0.5 * (w0 - 1), y1 + 0.5 * (h0 - 1)
        for s in sizes:
            sc = float(s) / stride
            w, h = w0 * sc, h0 * sc
            out.append([cx - 0.5 * (w - 1), cy - 0.5 * (h - 1), cx + 0.5 * (w - 1), cy + 0.5 * (h - 1)])
    return torch.tensor(np.array(out, dtype=np.float64)).float()


PROPOSALS_SIDE_STREAM = os.environ.get("ABR_PROPOSAL_STREAM", "1") != "0"


class LazyProposals(object):
    """The training selector's output before anything has been read back: the decoded score-sorted boxes, the NMS keep lists and
    their device-resident counts (RPNPostProcessor.launch).  The box head consumes it as is (ROIBoxHead.forward ->
    ops.roi_head_targets: GT append, matching, sampling and the RoI table in three launches, no host round trip).  Any other use --
    indexing, iteration, len() -- materialises the reference's list of per-image BoxLists (RPNPostProcessor.collect: one read-back
    of the counts), so it can stand wherever that list is expected."""

    def __init__(self, selector, pending, targets):
        self.selector, self.pending, self.targets = selector, pending, targets
        self._list = None

    def raw(self):
        """(props [N,k,4], scores [N,k], keep [N,post] int32, n_keep [N] int32, image sizes) visible to the current stream"""
        p = self.selector.join(self.pending)
        return p["props"], p["scores"], p["keep"], p["n_keep"], p["sizes"]

    def materialize(self):
        if self._list is None:
            self._list = self.selector.collect(self.pending, self.targets)
        return self._list

    def __len__(self):
        return len(self.pending["sizes"])

    def __iter__(self):
        return iter(self.materialize())

    def __getitem__(self, i):
        return self.materialize()[i]


class LazyPyramidProposals(LazyProposals):
    """LazyProposals for the pyramid selector's pending state (RPNPostProcessor.launch_pyramid): the proposals already are a dense table --
    rois [N,cap,4], objectness [N,cap], n_out [N] -- so the box head's training path feeds it to ops.roi_head_targets_table; any other use
    materialises through `collect`, as the single-level object does."""
    is_table = True

    def raw(self):
        """(rois [N,cap,4], objectness [N,cap], n_out [N] int32, image sizes) visible to the current stream"""
        p = self.selector.join(self.pending)
        return p["rois"], p["objectness"], p["n_out"], p["sizes"]


class AnchorGenerator(nn.Module):
    def __init__(self, sizes=(128, 256, 512), aspect_ratios=(0.5, 1.0, 2.0), anchor_strides=(8, 16, 32), straddle_thresh=0):
        super().__init__()
        if len(anchor_strides) == 1:
            cells = [generate_anchors(anchor_strides[0], sizes, aspect_ratios)]
        else:                                 # a feature pyramid: one cell-anchor set per level (anchor_generator.py:49-71)
            if len(anchor_strides) != len(sizes):
                raise RuntimeError("FPN should have #anchor_strides == #sizes")
            cells = [generate_anchors(st, s if isinstance(s, (tuple, list)) else (s,), aspect_ratios) for st, s in zip(anchor_strides, sizes)]
        self.strides = anchor_strides
        self.straddle_thresh = straddle_thresh
        self.register_buffer("cell_anchors", cells[0])
        for l, c in enumerate(cells[1:], 1):  # (level 0 keeps the single-level name)
            self.register_buffer("cell_anchors_%d" % l, c)
        self._cache = {}

    def level_cell_anchors(self, level):
        return self.cell_anchors if level == 0 else getattr(self, "cell_anchors_%d" % level)

    def num_anchors_per_location(self):
        return [self.level_cell_anchors(l).shape[0] for l in range(len(self.strides))]

    def grid(self, H, W, image_hw, level=0):
        """([H*W*A,4] anchors, [H*W*A] uint8 visibility) of one level for one image size; cached on device."""
        cell = self.level_cell_anchors(level)
        lv = (level,) if level else ()
        key = (H, W, int(image_hw[0]), int(image_hw[1]), cell.device) + lv
        hit = self._cache.get(key)
        if hit is None:
            a, vis = ops.grid_anchors(cell, H, W, self.strides[level], int(image_hw[0]), int(image_hw[1]), self.straddle_thresh)
            # the boxes depend on (H, W) only, the visibility also on the image size: share ONE box tensor per grid
            a = self._cache.setdefault((H, W, cell.device) + lv, a)
            hit = self._cache[key] = (a, vis, vis.bool())   # uint8 for the kernels, bool for the reference-typed BoxList field: made once
        return hit

    def pyramid(self, grids, image_hw):
        """The anchors of all levels as ONE tensor, in the reference's cat_boxlist order (level-major, then location row-major, then the anchor of
        the cell): ([n,4] anchors, [n] uint8 visibility for this image size, the L+1 level offsets).  Built once per (grids, image size, device)
        from the levels' grid() results; the box tensor is shared by every image size (only the visibility differs)."""
        grids = tuple((int(h), int(w)) for h, w in grids)
        assert len(grids) == len(self.strides), "one grid per anchor stride"
        dev = self.cell_anchors.device
        key = ("pyramid", grids, int(image_hw[0]), int(image_hw[1]), dev)
        hit = self._cache.get(key)
        if hit is None:
            per = [self.grid(H, W, image_hw, l) for l, (H, W) in enumerate(grids)]
            boxes = self._cache.get(("pyramid", grids, dev))
            if boxes is None:
                boxes = self._cache[("pyramid", grids, dev)] = torch.cat([p[0] for p in per])
            offs = [0]
            for p in per:
                offs.append(offs[-1] + p[0].shape[0])
            hit = self._cache[key] = (boxes, torch.cat([p[1] for p in per]), tuple(offs))
        return hit

    def forward(self, image_list, feature_maps):
        assert len(feature_maps) == len(self.strides), "one feature map per anchor stride"
        grids = [f.shape[-2:] for f in feature_maps]
        anchors = []
        for (ih, iw) in image_list.image_sizes:
            per_level = []
            for l, (H, W) in enumerate(grids):
                a, vis, vis_bool = self.grid(H, W, (ih, iw), l)
                bl = BoxList(a, (iw, ih), mode="xyxy")
                bl.add_field("visibility", vis_bool)
                bl._visibility_u8 = vis                   # the same mask as the kernels read it (no per-step dtype round trip)
                per_level.append(bl)
            if len(grids) > 1:
                per_level[0]._pyramid = self.pyramid(grids, (ih, iw))   # the loss matches over the concatenation (no per-step torch.cat)
            anchors.append(per_level)
        return anchors


def make_anchor_generator(cfg):
    sizes, strides = cfg.MODEL.RPN.ANCHOR_SIZES, cfg.MODEL.RPN.ANCHOR_STRIDE
    if cfg.MODEL.RPN.USE_FPN:
        assert len(strides) == len(sizes), "FPN should have len(ANCHOR_STRIDE) == len(ANCHOR_SIZES)"
    else:
        assert len(strides) == 1, "Non-FPN should have a single ANCHOR_STRIDE"
    return AnchorGenerator(sizes, cfg.MODEL.RPN.ASPECT_RATIOS, strides, cfg.MODEL.RPN.STRADDLE_THRESH)


# ------------------------------------------------------------------------------------------------ head
class _RPNHeadFn(Function):
    """t = relu(conv3x3(x)+b) ; y = conv1x1_fused(t)+b  as one autograd node with a hand-scheduled backward."""

    @staticmethod
    def forward(ctx, x, head, *params):
        xh = as_nhwc(x)
        v = ops.wino_v_alloc(xh, head.conv.weight, 1, 1, head.math) if head.conv.weight.requires_grad else None
        t = ops.conv_forward(xh, head.conv.weight, 1, 1, bias=head.conv.bias, relu=True, math=head.math, wino_v=v, w_version=head.conv.version())
        y = ops.conv_forward(t, head.fused_weight, 1, 0, bias=head.fused_bias, math=head.math, w_version=head.fused_version())
        ctx.head, ctx.saved = head, (xh, t, v)
        ctx.need_dx = x.requires_grad
        return from_nhwc(y)

    @staticmethod
    def backward(ctx, gy):
        head = ctx.head
        xh, t, v = ctx.saved
        g = as_nhwc(gy)
        if not g.is_contiguous():
            g = g.contiguous()
        ops.conv_wgrad_async(t, g, head.fused_weight_grad, 1, 0, math=head.math)
        ops.bias_grad(g, head.fused_bias_grad)
        gt = ops.conv_forward(g, head.fused_dgrad_weight(), 1, 0, mask=t, math=head.math)   # (reduction width 76: exact fp32 either way)
        ops.conv_wgrad_async(xh, gt, _grad_buf(head.conv.weight), 1, 1, math=head.math, wino_v=v)
        ops.bias_grad(gt, _grad_buf(head.conv.bias))
        gx = from_nhwc(ops.conv_forward(gt, head.conv.dgrad_weight(), 1, 1, math=head.math, w_version=head.conv.version())) if ctx.need_dx else None
        ctx.saved = None
        return (gx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class RPNHead(nn.Module):
    """rpn.py:70-121.  `cls_logits` / `bbox_pred` keep their reference names and shapes; their storage is two
    row-slices of one fused [76,1,1,C] buffer (rows 0..14, 15..74, row 75 = zero pad so that Cout % 4 == 0)."""

    def __init__(self, cfg, in_channels, num_anchors):
        super().__init__()
        self.num_anchors = num_anchors
        self.math = ops.MATH_F32   # see backbone.resnet.set_conv_math
        self.conv = Conv2d(in_channels, in_channels, 3, stride=1, padding=1)
        self.cls_logits = Conv2d(in_channels, num_anchors, 1)
        self.bbox_pred = Conv2d(in_channels, num_anchors * 4, 1)
        for l in (self.conv, self.cls_logits, self.bbox_pred):  # rpn.py:87-89
            nn.init.normal_(l.weight, std=0.01)
            nn.init.constant_(l.bias, 0)
        if cfg.MODEL.RPN.CONV_FREEZE:
            for p in self.conv.parameters():
                p.requires_grad = False
        if cfg.MODEL.RPN.CLS_FREEZE:
            for p in self.cls_logits.parameters():
                p.requires_grad = False
        if cfg.MODEL.RPN.BBS_FREEZE:
            for p in self.bbox_pred.parameters():
                p.requires_grad = False
        self.n_out = num_anchors * 5
        self.n_out_pad = (self.n_out + 3) // 4 * 4
        self._fuse()

    def _fuse(self):
        """(re)build the fused storage and re-point the two reference-named parameters into it"""
        A, C_, dev = self.num_anchors, self.conv.in_channels, self.cls_logits.weight.device
        fw = torch.zeros(self.n_out_pad, 1, 1, C_, device=dev)
        fb = torch.zeros(self.n_out_pad, device=dev)
        with torch.no_grad():
            fw[:A].copy_(self.cls_logits.weight)
            fw[A:5 * A].copy_(self.bbox_pred.weight)
            fb[:A].copy_(self.cls_logits.bias)
            fb[A:5 * A].copy_(self.bbox_pred.bias)
        self._set_fused(fw, fb, torch.zeros_like(fw), torch.zeros_like(fb))

    def _set_fused(self, fw, fb, gw, gb):
        A = self.num_anchors
        self.fused_weight, self.fused_bias = fw, fb
        self.fused_weight_grad, self.fused_bias_grad = gw, gb
        for mod, lo, hi in ((self.cls_logits, 0, A), (self.bbox_pred, A, 5 * A)):
            mod.weight.data, mod.bias.data = fw[lo:hi], fb[lo:hi]
            mod.weight.grad, mod.bias.grad = gw[lo:hi], gb[lo:hi]
        self._wt, self._wt_version = None, -1

    def rehome(self, which, view, grad_view):
        """called by flatten_parameters: adopt flat-buffer storage for the fused weight / bias"""
        if which == "weight":
            shp = self.fused_weight.shape
            self._set_fused(view.view(shp), self.fused_bias, grad_view.view(shp), self.fused_bias_grad)
        else:
            self._set_fused(self.fused_weight, view, self.fused_weight_grad, grad_view)

    def _apply(self, fn, *a, **k):
        out = super()._apply(fn, *a, **k)
        self._fuse()
        return out

    def flat_groups(self):
        """tensors that must stay contiguous when the model's parameters are re-homed into one flat buffer"""
        return [("weight", [self.cls_logits.weight, self.bbox_pred.weight], self.n_out_pad - self.n_out),
                ("bias", [self.cls_logits.bias, self.bbox_pred.bias], self.n_out_pad - self.n_out)]

    def prep_entries(self):
        """the 3x3 head conv goes with FusedSGD's batched preparation (see Bottleneck.prep_entries); prepare_rest() does the fused 1x1 heads"""
        return [(self.conv, None, 1, 1, self.math)] if (self.conv.weight.requires_grad and self.conv.weight.is_cuda) else []

    def prepare_rest(self):
        if self.fused_weight.is_cuda and self.fused_weight_grad is not None and (self.cls_logits.weight.requires_grad or self.bbox_pred.weight.requires_grad):
            self.fused_dgrad_weight()
            ops.conv_prepare_weights(self.fused_weight, 1, 0, self.math, self.fused_version())

    def fused_version(self):
        """abr_conv_desc::w_version of the fused cls | bbox weight (Conv2d.version's rule: it moves with optimiser steps iff an optimiser
        owns one of its two halves)"""
        from ..backbone.resnet import _PARAM_VERSION, _STATIC_VERSION
        opt = self.cls_logits._optimised or self.bbox_pred._optimised
        return 2 * _PARAM_VERSION[0] + 1 if opt else 2 * _STATIC_VERSION[0] + 2

    def fused_dgrad_weight(self):
        from ..backbone.resnet import _PARAM_VERSION
        ops.prep_wait()
        if self._wt is None or self._wt_version != _PARAM_VERSION[0]:
            self._wt = ops.conv_dgrad_weights(self.fused_weight, None, out=self._wt)
            self._wt_version = _PARAM_VERSION[0]
        return self._wt

    def forward_fused(self, x):
        """x logical [N,C,H,W] -> logical [N,76,H,W] whose NHWC memory is [N,H,W,(15 obj | 60 reg | pad)]"""
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _RPNHeadFn.apply(x, self, *params)
        xh = as_nhwc(x)
        t = ops.conv_forward(xh, self.conv.weight, 1, 1, bias=self.conv.bias, relu=True, math=self.math, w_version=self.conv.version())
        return from_nhwc(ops.conv_forward(t, self.fused_weight, 1, 0, bias=self.fused_bias, math=self.math, w_version=self.fused_version()))

    def forward(self, x):
        logits, bbox_reg = [], []
        for feature in x:
            y = self.forward_fused(feature)
            logits.append(y[:, : self.num_anchors])
            bbox_reg.append(y[:, self.num_anchors: 5 * self.num_anchors])
        return logits, bbox_reg


# ------------------------------------------------------------------------------------------------ proposals
class RPNPostProcessor(nn.Module):
    """inference.py:14-147: sigmoid -> top-k (sorted) -> decode -> clip -> remove small -> NMS -> first post_nms (+GT in training)."""

    def __init__(self, pre_nms_top_n, post_nms_top_n, nms_thresh, min_size, box_coder=None, fpn_post_nms_top_n=None,
                 fpn_post_nms_per_batch=True):
        super().__init__()
        self._hw_cache = {}
        self.pre_nms_top_n, self.post_nms_top_n = pre_nms_top_n, post_nms_top_n
        self.nms_thresh, self.min_size = nms_thresh, min_size
        self.box_coder = box_coder if box_coder is not None else BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.fpn_post_nms_top_n = post_nms_top_n if fpn_post_nms_top_n is None else fpn_post_nms_top_n
        self.fpn_post_nms_per_batch = fpn_post_nms_per_batch

    def add_gt_proposals(self, proposals, targets):
        out = []
        for p, t in zip(proposals, targets):
            gt = BoxList(t.bbox, t.size, t.mode)
            gt.add_field("objectness", torch.ones(len(gt), device=t.bbox.device))
            b = BoxList(torch.cat((p.bbox, gt.bbox), 0), p.size, p.mode)
            b.add_field("objectness", torch.cat((p.get_field("objectness"), gt.get_field("objectness")), 0))
            out.append(b)
        return out

    def launch(self, anchors, fused, num_anchors):
        """Device half of forward_fused: top-k -> decode -> clip -> NMS, all enqueued on the CURRENT stream, nothing read back.
        Returns the pending state for `collect`.  A list of several levels' outputs, or MIN_SIZE > 0, goes through `launch_pyramid`."""
        if isinstance(fused, (list, tuple)):
            if len(fused) > 1 or self.min_size > 0:
                return self.launch_pyramid(anchors, fused, num_anchors)
            fused = fused[0]
        elif self.min_size > 0:
            return self.launch_pyramid(anchors, [fused], num_anchors)
        y = as_nhwc(fused)
        N, H, W, Cf = y.shape
        A = num_anchors
        n_anchor = H * W * A
        yf = y.reshape(N, H * W, Cf)
        k = min(self.pre_nms_top_n, n_anchor)
        if k <= 15360:   # one fused kernel per batch: sigmoid + radix select + in-LDS bitonic sort (inference.py:87-96)
            scores, topk_idx = ops.topk_sigmoid(yf, A, k)
        else:            # beyond the in-LDS sort capacity (no voc config gets here: PRE_NMS_TOP_N is 12000 / 6000)
            scores, topk_idx = yf[:, :, :A].reshape(N, n_anchor).sigmoid().topk(k, dim=1, sorted=True)
        same = all(a[0].bbox.data_ptr() == anchors[0][0].bbox.data_ptr() for a in anchors)
        img_hw = self._img_hw(anchors, y.device)
        assert same, "per-image anchor grids of one batch share (H,W): they differ only in the visibility field"
        props = ops.rpn_decode_clip(yf, A, anchors[0][0].bbox, topk_idx, img_hw, self.box_coder.weights, A=A)  # :101-112
        counts = torch.full((N,), k, dtype=torch.int32, device=y.device)   # (MIN_SIZE == 0 here: remove_small_boxes drops nothing)
        keep, n_keep = ops.nms_sorted_batched(props, counts, self.nms_thresh, self.post_nms_top_n)     # :113-116
        return dict(props=props, scores=scores, keep=keep, n_keep=n_keep, sizes=[a[0].size for a in anchors], fused=yf)

    def _img_hw(self, anchors, device):
        """[N,2] int32 (h, w) on the device; image sizes repeat from step to step, so the copy is kept"""
        hw_key = (tuple((a[0].size[1], a[0].size[0]) for a in anchors), device)
        img_hw = self._hw_cache.get(hw_key)
        if img_hw is None:
            if len(self._hw_cache) > 64:
                self._hw_cache.clear()
            img_hw = self._hw_cache[hw_key] = ops.h2d([list(v) for v in hw_key[0]], torch.int32, device)
        return img_hw

    def launch_pyramid(self, anchors, fused, num_anchors):
        """`launch` for L levels (inference.py:120-176) and for MIN_SIZE > 0: every (image, level) segment goes through ranking, decode + clip +
        remove_small_boxes, NMS and the cross-level selection together, on the CURRENT stream, nothing read back (ops.rpn_pyramid_*).
        fused: list of L logical [N,5A(+pad),H_l,W_l]; anchors: list (per image) of L BoxLists."""
        ys = [as_nhwc(f) for f in fused]
        nL, N, dev = len(ys), ys[0].shape[0], ys[0].device
        yfs = [y.reshape(N, y.shape[1] * y.shape[2], y.shape[3]) for y in ys]
        As = [num_anchors] * nL if isinstance(num_anchors, int) else list(num_anchors)
        for l in range(nL):
            assert all(a[l].bbox.data_ptr() == anchors[0][l].bbox.data_ptr() for a in anchors), \
                "per-image anchor grids of one batch share (H,W): they differ only in the visibility field"
        grids = [anchors[0][l].bbox for l in range(nL)]
        img_hw = self._img_hw(anchors, dev)
        ks = ops.rpn_pyramid_ks(yfs, As, self.pre_nms_top_n)
        if max(ks) <= ops.rpn_pyramid_max_k():
            scores, topk_idx = ops.rpn_pyramid_topk(yfs, As, self.pre_nms_top_n)                       # :87-96, all levels at once
        else:   # beyond the pyramid ranking's in-LDS sort: the single-level operator, level by level, into the same tables
            scores = torch.zeros((N, nL, max(ks)), dtype=torch.float32, device=dev)
            topk_idx = torch.zeros((N, nL, max(ks)), dtype=torch.int64, device=dev)
            for l, (yf, A, k) in enumerate(zip(yfs, As, ks)):
                if k <= 15360 and yf.shape[1] * A <= 196608:
                    s_l, i_l = ops.topk_sigmoid(yf, A, k)
                else:
                    s_l, i_l = yf[:, :, :A].reshape(N, -1).sigmoid().topk(k, dim=1, sorted=True)
                scores[:, l, :k], topk_idx[:, l, :k] = s_l, i_l
        props, scores, counts = ops.rpn_pyramid_decode(yfs, As, grids, topk_idx, scores, img_hw, self.pre_nms_top_n, self.box_coder.weights,
                                                       self.min_size)                                  # :96-112 + remove_small_boxes
        keep, n_keep = ops.nms_sorted_batched(props, counts, self.nms_thresh, self.post_nms_top_n)     # :113-116, N*L segments
        # one level: no cross-level cut (:139-140), the selection below then only gathers the kept rows
        fpn_post = self.fpn_post_nms_top_n if nL > 1 else self.post_nms_top_n
        rois, out_scores, src, n_out = ops.rpn_pyramid_select(props, scores, keep, n_keep, N, fpn_post,
                                                              self.training and self.fpn_post_nms_per_batch and nL > 1)   # :149-176
        return dict(rois=rois, objectness=out_scores, src=src, n_out=n_out, sizes=[a[0].size for a in anchors], fused=yfs)

    def collect(self, pending, targets=None):
        """Host half: read the per-image keep counts (the only host sync of the proposal path; the reference syncs inside every
        nms call) and cut the BoxLists."""
        counts = "n_out" if "n_out" in pending else "n_keep"     # (the pyramid path's pending state, or the single-level one)
        side = pending.get("stream")
        if side is not None:
            # read the counts ON THE SIDE STREAM: the copy then waits for the selection only, not for whatever the caller has queued
            # on the main stream in the meantime (a main-stream read-back would stall the host behind all of it)
            with torch.cuda.stream(side):
                nk = pending[counts].tolist()
            self.join(pending)
        else:
            nk = pending[counts].tolist()
        result = []
        if counts == "n_out":
            for i, size in enumerate(pending["sizes"]):
                b = BoxList(pending["rois"][i, : nk[i]], size, mode="xyxy")
                b.add_field("objectness", pending["objectness"][i, : nk[i]])
                result.append(b)
        else:
            props, scores, keep = pending["props"], pending["scores"], pending["keep"]
            for i, size in enumerate(pending["sizes"]):
                ki = keep[i, : nk[i]].long()
                b = BoxList(props[i].index_select(0, ki), size, mode="xyxy")
                b.add_field("objectness", scores[i].index_select(0, ki))
                result.append(b)
        if self.training and targets is not None:
            result = self.add_gt_proposals(result, targets)                               # :144-145
        return result

    def launch_on_side_stream(self, anchors, fused, num_anchors, tag="proposals"):
        """`launch` on a side stream: the selection is a chain of latency-bound kernels (a 1024-thread top-k and a one-workgroup-per-
        image NMS sweep, ~0.9 ms with a handful of CUs busy) that has no consumer until `collect`, so it runs NEXT to whatever the
        caller enqueues on the current stream meanwhile (the RPN loss; for the frozen source model, the target's whole backbone)."""
        maps = list(fused) if isinstance(fused, (list, tuple)) else [fused]
        cur = torch.cuda.current_stream()
        side = ops.side_stream((maps[0].device.index, tag))
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            pending = self.launch(anchors, fused, num_anchors)
        for f in maps:
            f.record_stream(side)
        pending["stream"] = side
        return pending

    def join(self, pending):
        """Make the current stream (and the caching allocator) see the side stream's results."""
        side = pending.pop("stream", None)
        if side is not None:
            cur = torch.cuda.current_stream()
            cur.wait_stream(side)
            for k in ("props", "scores", "keep", "n_keep", "rois", "objectness", "src", "n_out"):
                if k in pending:
                    pending[k].record_stream(cur)
        return pending

    def forward_fused(self, anchors, fused, num_anchors, targets=None):
        """fused: logical [N,5A(+pad),H,W] head output, or the list of L of them.  anchors: list (per image) of the levels' BoxLists as
        AnchorGenerator returns."""
        return self.collect(self.launch(anchors, fused, num_anchors), targets)

    def forward(self, anchors, objectness, box_regression, targets=None):
        """reference signature (lists of L logical [N,A,H,W] / [N,4A,H,W]); re-fuses the two tensors of every level (compat path)."""
        assert len(objectness) == len(box_regression) and all(len(a) == len(objectness) for a in anchors), "one entry per feature level"
        fused = [torch.cat((o, b), 1) for o, b in zip(objectness, box_regression)]
        return self.forward_fused(anchors, fused if len(fused) > 1 else fused[0], objectness[0].shape[1], targets)


def make_rpn_postprocessor(config, rpn_box_coder, is_train):
    pre = config.MODEL.RPN.PRE_NMS_TOP_N_TRAIN if is_train else config.MODEL.RPN.PRE_NMS_TOP_N_TEST
    post = config.MODEL.RPN.POST_NMS_TOP_N_TRAIN if is_train else config.MODEL.RPN.POST_NMS_TOP_N_TEST
    fpn_post = config.MODEL.RPN.FPN_POST_NMS_TOP_N_TRAIN if is_train else config.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST
    return RPNPostProcessor(pre, post, config.MODEL.RPN.NMS_THRESH, config.MODEL.RPN.MIN_SIZE, rpn_box_coder, fpn_post,
                            config.MODEL.RPN.FPN_POST_NMS_PER_BATCH)


# ------------------------------------------------------------------------------------------------ loss
class _RPNLossFn(Function):
    """BCE-with-logits over the sampled anchors + smooth-L1(beta=1/9) over the sampled positives / #sampled
    (rpn/loss.py:136,145-146), reading objectness and deltas straight out of the fused NHWC head output."""

    @staticmethod
    def forward(ctx, fused, A, labels, reg_targets, pos_idx, samp_idx, denom=None, prepared=None):
        y = as_nhwc(fused)
        N, H, W, Cf = y.shape
        y2 = y.reshape(N * H * W, Cf)
        # index lists may be fixed-size and -1 padded (fused sampler): negative entries stay negative below and are skipped
        # by the kernels; `denom` is then the device-resident number of sampled anchors
        n_samp = samp_idx.numel()
        # anchor j of the flattened batch lives in row j // A; objectness at column j % A, deltas at A + 4*(j % A)
        if prepared is not None:   # (obj_flat_idx, pos rows, pos columns) straight from ops.rpn_loss_indices
            obj_flat_idx, prow, pcol = prepared
        else:
            row = torch.div(samp_idx, A, rounding_mode="floor")
            obj_flat_idx = row * Cf + (samp_idx - row * A)
            prow = torch.div(pos_idx, A, rounding_mode="floor")
            pcol = A + 4 * (pos_idx - prow * A)
        want = fused.requires_grad
        lo, g_obj = ops.bce_logits_gather(y2, labels, obj_flat_idx, want_grad=want, yidx=samp_idx, denom_dev=denom)
        lb, g_reg = ops.smooth_l1_rows(y2, reg_targets, prow, pcol, 1.0 / 9,
                                       scale=1.0 if denom is not None else 1.0 / max(n_samp, 1), want_grad=want, trows=pos_idx,
                                       denom_dev=denom)
        ctx.shape = (N, H, W, Cf)
        ctx.save_for_backward(g_obj, g_reg)
        return lo[0], lb[0]

    @staticmethod
    def backward(ctx, g_lo, g_lb):
        g_obj, g_reg = ctx.saved_tensors
        ops.scale_(g_obj, 1.0, g_lo.contiguous())
        ops.scale_(g_reg, 1.0, g_lb.contiguous())
        ops.add_(g_obj, g_reg)  # disjoint columns of the same [N*H*W, Cf] buffer
        return from_nhwc(g_obj.view(ctx.shape)), None, None, None, None, None, None, None


class _RPNPyramidLossFn(Function):
    """The same two losses over L levels (rpn/loss.py:104-148): ops.rpn_pyramid_loss reads every sampled anchor out of its level's fused NHWC
    output; backward returns the L views of one gradient allocation (ops.rpn_pyramid_loss_backward)."""

    @staticmethod
    def forward(ctx, A, labels, reg_targets, pos, neg, counts, *fused):
        ys = [as_nhwc(f) for f in fused]
        want = any(f.requires_grad for f in fused)
        losses, rec = ops.rpn_pyramid_loss(ys, A, labels, reg_targets, pos, neg, counts, want_grad=want)
        ctx.meta = ([tuple(y.shape) for y in ys], A, pos.shape[1], neg.shape[1], ys[0].device)
        ctx.rec = rec
        return losses[0], losses[1]

    @staticmethod
    def backward(ctx, g_lo, g_lb):
        shapes, A, max_pos, batch, dev = ctx.meta
        grads = ops.rpn_pyramid_loss_backward(shapes, A, ctx.rec, max_pos, batch, g_lo, g_lb, dev)
        return (None,) * 6 + tuple(from_nhwc(g) if need else None for g, need in zip(grads, ctx.needs_input_grad[6:]))


def _padded_from_flat(pos_idx, samp_idx, N, n):
    """injected batch-flat index lists of any length (entries < 0 ignored) -> the sampler's padded form: pos [N,max_pos], neg [N,batch] (per image
    ascending, -1 padded) and counts [N,2] int32; the negatives are the sampled entries that are no positives"""
    pos_idx, samp_idx = pos_idx.reshape(-1), samp_idx.reshape(-1)
    pos_idx, samp_idx = pos_idx[pos_idx >= 0], samp_idx[samp_idx >= 0]
    neg_idx = samp_idx[~torch.isin(samp_idx, pos_idx)]

    def pad(idx):
        idx = idx.sort().values
        img = torch.div(idx, n, rounding_mode="floor")
        cnt = torch.bincount(img, minlength=N)
        out = torch.full((N, max(int(cnt.max()) if idx.numel() else 0, 1)), -1, dtype=torch.int64, device=idx.device)
        out[img, torch.arange(idx.numel(), device=idx.device) - (cnt.cumsum(0) - cnt)[img]] = idx
        return out, cnt

    (pos, n_pos), (neg, n_neg) = pad(pos_idx), pad(neg_idx)
    return pos, neg, torch.stack([n_pos, n_neg], 1).to(torch.int32)


class RPNLossComputation(object):
    def __init__(self, proposal_matcher, fg_bg_sampler, box_coder, generate_labels_func=None):
        self.proposal_matcher, self.fg_bg_sampler, self.box_coder = proposal_matcher, fg_bg_sampler, box_coder
        self.discard_cases = ["not_visibility", "between_thresholds"]

    def prepare_targets(self, anchors, targets):
        """rpn/loss.py:66-102 per image -> labels fp32 {1,0,-1}, regression targets, matched idxs"""
        labels, regression_targets, matched = [], [], []
        for a, t in zip(anchors, targets):
            vis = getattr(a, "_visibility_u8", None)
            if vis is None:
                vis = a.get_field("visibility")
                vis = vis.to(torch.uint8) if vis.dtype != torch.uint8 else vis
            m, lab, tgt = self.proposal_matcher.match_boxes(t.bbox, a.bbox, None, vis, self.box_coder.weights, rpn_labels=True)
            labels.append(lab)
            regression_targets.append(tgt)
            matched.append(m)
        return labels, regression_targets, matched

    def sample(self, labels):
        """One fused sampler launch for the whole batch, nothing leaves the device.  Returns batch-flattened index lists of
        FIXED length (-1 padded): positives [N*128], all sampled (positives then negatives) [N*128 + N*256], and the device
        scalar #sampled that normalises both losses (rpn/loss.py:119-123,136,146)."""
        lab2d = torch.stack(labels)
        n = lab2d.shape[1]
        pos, neg, counts = self.fg_bg_sampler.sample_padded(lab2d, index_offset_per_image=n)
        pos = pos.reshape(-1)
        return pos, torch.cat([pos, neg.reshape(-1)]), counts.sum().to(torch.float32).reshape(1)

    def __call__(self, anchors, objectness, box_regression, targets, rpn_output_source=None, fused=None, sampled=None):
        """Returns (objectness_loss, box_loss).  `rpn_output_source` is accepted and ignored as in the reference (:129-143).
        `sampled=(pos_idx, samp_idx)` injects the sampler's choice (parity tests).  A list of L > 1 fused outputs (`fused=[...]`), or the
        reference's lists of L objectness and L regression tensors, goes through `call_pyramid`; one level stays on the route below."""
        if sampled is None:
            sampled = getattr(self, "inject_sampled", None)  # parity tests pin the sampler's draw here
        if isinstance(fused, (list, tuple)) or (fused is None and len(objectness) > 1):
            if fused is None:   # the reference's signature: re-fuse the two tensors of every level (compat path), pad columns zero
                assert len(objectness) == len(box_regression), "one entry per feature level"
                A = objectness[0].shape[1]
                fused = [torch.cat((o, b) + ((o.new_zeros((o.shape[0], -5 * A % 4) + tuple(o.shape[2:])),) if 5 * A % 4 else ()), 1)
                         for o, b in zip(objectness, box_regression)]
            if len(fused) > 1:
                return self.call_pyramid(anchors, list(fused), targets, sampled)
            fused = fused[0]
        anchors = [a[0] if isinstance(a, (list, tuple)) else a for a in anchors]
        if fused is None:
            fused = torch.cat((objectness[0], box_regression[0]), 1)
            A = objectness[0].shape[1]
        else:
            A = anchors[0].bbox.shape[0] // (fused.shape[-1] * fused.shape[-2])
        shared = fused.is_cuda and all(a.bbox.data_ptr() == anchors[0].bbox.data_ptr() and getattr(a, "_visibility_u8", None) is not None for a in anchors)
        if shared:
            # the batch's targets in two launches (one anchor grid for all images), the sampler in one, the loss bookkeeping in one
            lab2d, tgt3d, _keep = ops.rpn_targets_batched(anchors[0].bbox, [a._visibility_u8 for a in anchors], [t.bbox for t in targets],
                                                          self.proposal_matcher.high_threshold, self.proposal_matcher.low_threshold,
                                                          self.box_coder.weights)
            labels, regression_targets = list(lab2d.unbind(0)), list(tgt3d.unbind(0))      # views (introspection, API)
            lab_flat, tgt_flat = lab2d.view(-1), tgt3d.view(-1, 4)
        else:
            labels, regression_targets, _ = self.prepare_targets(anchors, targets)
            lab2d = None
            lab_flat, tgt_flat = torch.cat(labels), torch.cat(regression_targets)
        denom = prepared = None
        if sampled is not None:
            pos_idx, samp_idx = sampled
        elif lab2d is not None:
            n = lab2d.shape[1]
            pos, neg, counts = self.fg_bg_sampler.sample_padded(lab2d, index_offset_per_image=n)
            samp_idx, obj_flat, prow, pcol, denom = ops.rpn_loss_indices(pos, neg, counts, A, fused.shape[1])
            pos_idx = pos.reshape(-1)
            prepared = (obj_flat, prow, pcol)
        else:
            pos_idx, samp_idx, denom = self.sample(labels)
        self.last_sampled, self.last_targets = (pos_idx, samp_idx), (labels, regression_targets)  # introspection for parity tests
        return _RPNLossFn.apply(fused, A, lab_flat, tgt_flat, pos_idx, samp_idx, denom, prepared)


    def call_pyramid(self, anchors, fused, targets, sampled=None):
        """__call__ for L > 1 fused head outputs (logical [N,Cf,H_l,W_l]); anchors: per image the list of L BoxLists AnchorGenerator returns.
        Matching (IoU, Matcher with low-quality matches, labels, encode) runs over the levels' CONCATENATED anchors, so a ground truth's
        low-quality match is its best anchor over all levels (rpn/loss.py:104-118 after cat_boxlist); the sampler draws per image over the same
        concatenation; the loss reads the sampled anchors by address."""
        nL = len(fused)
        assert all(len(a) == nL for a in anchors), "one anchor BoxList per feature level and image"
        A = anchors[0][0].bbox.shape[0] // (fused[0].shape[-1] * fused[0].shape[-2])
        boxes, vis = None, []
        for a in anchors:
            pyr = getattr(a[0], "_pyramid", None)
            if pyr is None:       # anchors that did not come from AnchorGenerator.forward: concatenate here
                v = [getattr(b, "_visibility_u8", None) for b in a]
                v = [b.get_field("visibility").to(torch.uint8) if x is None else x for b, x in zip(a, v)]
                pyr = (torch.cat([b.bbox for b in a]), torch.cat(v))
            if boxes is None:
                boxes = pyr[0]
            assert pyr[0].shape == boxes.shape, "the images of one batch share the levels' grids: they differ only in the visibility field"
            vis.append(pyr[1])
        lab2d, tgt3d, _keep = ops.rpn_targets_batched(boxes, vis, [t.bbox for t in targets], self.proposal_matcher.high_threshold,
                                                      self.proposal_matcher.low_threshold, self.box_coder.weights)
        N, n = lab2d.shape
        if sampled is not None:
            pos, neg, counts = _padded_from_flat(sampled[0], sampled[1], N, n)
        else:
            pos, neg, counts = self.fg_bg_sampler.sample_padded(lab2d, index_offset_per_image=n)
        pos_flat = pos.reshape(-1)
        self.last_sampled = (pos_flat, torch.cat([pos_flat, neg.reshape(-1)]))   # (-1 padded, as the single-level route's)
        self.last_targets = (list(lab2d.unbind(0)), list(tgt3d.unbind(0)))
        return _RPNPyramidLossFn.apply(A, lab2d, tgt3d, pos, neg, counts, *fused)


def make_rpn_loss_evaluator(cfg, box_coder):
    matcher = Matcher(cfg.MODEL.RPN.FG_IOU_THRESHOLD, cfg.MODEL.RPN.BG_IOU_THRESHOLD, allow_low_quality_matches=True)
    sampler = BalancedPositiveNegativeSampler(cfg.MODEL.RPN.BATCH_SIZE_PER_IMAGE, cfg.MODEL.RPN.POSITIVE_FRACTION)
    return RPNLossComputation(matcher, sampler, box_coder)


# ------------------------------------------------------------------------------------------------ module
class MissingTargets(ValueError, NotImplementedError):
    """RPNModule.train() over a feature pyramid was called with targets=None: a bad value for the caller.  While the multi-level RPN loss was
    missing, exactly this call raised NotImplementedError; callers that caught it keep working (coco_eval.MissingObjectness is the precedent)."""


class RPNModule(nn.Module):
    def __init__(self, cfg, in_channels):
        super().__init__()
        self.cfg = cfg.clone()
        self.anchor_generator = make_anchor_generator(cfg)
        per_level = self.anchor_generator.num_anchors_per_location()
        if len(set(per_level)) != 1:   # rpn.py:150-152: ONE head is shared by the levels of a pyramid
            raise ValueError("the RPN head is shared by all feature levels, so every level needs the same number of anchors per location; "
                             "ANCHOR_SIZES / ASPECT_RATIOS give %s" % (per_level,))
        self.head = RPNHead(cfg, in_channels, per_level[0])
        rpn_box_coder = BoxCoder(weights=(1.0, 1.0, 1.0, 1.0))
        self.box_selector_train = make_rpn_postprocessor(cfg, rpn_box_coder, is_train=True)
        self.box_selector_test = make_rpn_postprocessor(cfg, rpn_box_coder, is_train=False)
        self.loss_evaluator = make_rpn_loss_evaluator(cfg, rpn_box_coder)

    def forward(self, images, features, targets=None, rpn_output_source=None, defer_proposals=False):
        """-> ((boxes, losses), anchors, rpn_output) exactly as rpn.py:161-183."""
        if self.training:
            if len(features) > 1 and targets is None:
                raise MissingTargets("training the RPN on %d feature levels: the multi-level RPN loss (rpn/loss.py over the concatenated "
                                     "levels) needs targets, got targets=None; eval() selects proposals over a pyramid" % len(features))
            return self.forward_finish(self.forward_begin(images, features, targets, rpn_output_source))
        A = self.head.num_anchors
        if len(features) > 1:   # a feature pyramid: the shared head per level, the multi-level selector (rpn.py:161-183, inference.py:120-176)
            fused = [self.head.forward_fused(f) for f in features]
            rpn_output = ([f[:, :A] for f in fused], [f[:, A:5 * A] for f in fused])
        else:
            fused = self.head.forward_fused(features[0])
            rpn_output = ([fused[:, :A]], [fused[:, A:5 * A]])
        anchors = self.anchor_generator(images, features)
        self.box_selector_test.eval()
        if defer_proposals:   # the caller collects later (GeneralizedRCNN.soften_begin / soften_finish)
            pending = self.box_selector_test.launch_on_side_stream(anchors, fused, A, tag="source-proposals")
            return (pending, {}), anchors, rpn_output
        boxes = self.box_selector_test.forward_fused(anchors, fused, A)
        return (boxes, {}), anchors, rpn_output

    def forward_begin(self, images, features, targets, rpn_output_source=None):
        """Training forward up to (not including) the read-back of the proposal counts: head conv, anchors, the proposal selection
        launched on a side stream, the loss on the current stream.  One feature map or a pyramid (rpn.py:161-183): the shared head runs per
        level, and over L > 1 maps its weight and bias gradients accumulate over the L backward nodes (conv_wgrad and bias_grad add into the
        fused gradient buffers)."""
        A = self.head.num_anchors
        fused = [self.head.forward_fused(f) for f in features]
        anchors = self.anchor_generator(images, features)
        rpn_output = ([f[:, :A] for f in fused], [f[:, A:5 * A] for f in fused])
        # one level: the selector and the loss get the tensor, not a one-element list, and take their single-level routes
        head_out = fused if len(fused) > 1 else fused[0]
        with torch.no_grad():
            self.box_selector_train.train()
            detached = [f.detach() for f in fused] if len(fused) > 1 else fused[0].detach()
            if PROPOSALS_SIDE_STREAM and fused[0].is_cuda:   # selection runs next to the loss kernels below
                pending = self.box_selector_train.launch_on_side_stream(anchors, detached, A)
            else:
                pending = self.box_selector_train.launch(anchors, detached, A)
        loss_objectness, loss_rpn_box_reg = self.loss_evaluator(anchors, None, None, targets, rpn_output_source, fused=head_out)
        return dict(pending=pending, targets=targets, anchors=anchors, rpn_output=rpn_output,
                    losses={"loss_objectness": loss_objectness, "loss_rpn_box_reg": loss_rpn_box_reg})

    def forward_finish(self, state):
        with torch.no_grad():
            # training: hand the box head the selector's RAW device output (LazyProposals) instead of per-image BoxLists cut on the host
            pending = state["pending"]
            if "props" in pending and pending["props"].is_cuda and state["targets"] is not None:
                boxes = LazyProposals(self.box_selector_train, pending, state["targets"])
            elif "n_out" in pending and pending["rois"].is_cuda and state["targets"] is not None:    # the pyramid selector's table
                boxes = LazyPyramidProposals(self.box_selector_train, pending, state["targets"])
            else:
                boxes = self.box_selector_train.collect(state["pending"], state["targets"])
        return (boxes, state["losses"]), state["anchors"], state["rpn_output"]


def build_rpn(cfg, in_channels):
    """rpn.py:224-230: RetinaNet takes the RPN's place in the detector"""
    if cfg.MODEL.RETINANET_ON:
        from .retinanet import build_retinanet
        return build_retinanet(cfg, in_channels)
    return RPNModule(cfg, in_channels)

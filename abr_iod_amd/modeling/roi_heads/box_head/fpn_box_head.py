"""The FPN box head on the HIP library.

Mirrors:
    FPN2MLPFeatureExtractor   maskrcnn_benchmark/modeling/roi_heads/box_head/roi_box_feature_extractors.py:59-101
    FPNPredictor              modeling/roi_heads/box_head/roi_box_predictors.py:36-132
    make_fc                   modeling/make_layers.py:80-92 (kaiming_uniform_(a=1), bias 0)

Departure at the seam, on purpose: the reference's FPN2MLPFeatureExtractor.forward returns ONE value while its ROIBoxHead.forward unpacks two
(`x, roi_align_features = self.feature_extractor(...)`, box_head.py:37,52,74), so the reference cannot run this head as written.  Here the
extractor returns (x [K,D], pooled logical [K,C,res,res]), which is what ROIBoxHead and the distillation losses expect.

MI355X-first differences (results identical):
  * the pooled tensor is NHWC in memory ([K,res,res,C]); fc6's weight is stored with its columns in that (h,w,c) order -- the bytes of an OHWI
    [D,res,res,C] conv weight, held as the 1x1 conv's [D,1,1,res*res*C] like DeformConv2d holds its taps -- so neither the activations nor the
    weight are transposed per step.  The checkpoint boundary sees the reference's [D, C*res*res] in (c,h,w) order.
  * fc6, fc7 and the fused predictor are the conv library's 1x1 contraction over [K,1,1,*] rows: the ReLUs ride in the forward epilogues, the
    ReLU masks of the backward pass in the epilogue of the contraction that PRODUCES the gradient (mask=), weight gradients run on the side
    stream (conv_wgrad_async) straight into the flat gradient buffer.
  * cls_score and bbox_pred are ONE GEMM with padded columns, as FastRCNNPredictor's.
  * the multi-level Pooler tags its output with the largest of the levels' amax words (ops.amax_bound_levels), so fc6 under f16x3 does not
    reduce the [K,res,res,C] tensor first.
"""
import torch
from torch import nn
from torch.autograd import Function

from .... import ops
from ....layers._layout import as_nhwc, from_nhwc
from ...backbone import resnet
from ...backbone.resnet import Conv2d, _grad_buf
from ...poolers import make_pooler
from .box_head import FastRCNNPredictor


def _rows(t):
    """[K, ...] contiguous -> the [K,1,1,n] view the 1x1 contraction reads (the same elements: an amax tag stays valid)"""
    return ops.amax_carry(t.view(t.shape[0], 1, 1, -1), t)


class _FC(Conv2d):
    """nn.Linear stand-in over the flattened NHWC rows of a [K,res,res,C] tensor: weight [out,1,1,res*res*C], columns in (h,w,c) order;
    the reference layout is [out, C*res*res] with columns in (c,h,w) order (x.view(K, -1) of an NCHW tensor)."""
    whole_only = True     # (checkpoint.load_reference_state_dict: always through load_oihw, never a partial row copy in memory layout)

    def __init__(self, channels, res, out_features):
        super().__init__(channels * res * res, out_features, 1, bias=True)
        self.channels, self.res = channels, res
        self.kaiming_uniform_(a=1)          # make_fc; fan_in = channels * res * res, bias 0

    def load_oihw(self, w):
        D, C_, r = self.out_channels, self.channels, self.res
        with torch.no_grad():
            self.weight.copy_(w.reshape(D, C_, r, r).permute(0, 2, 3, 1).reshape(self.weight.shape))
        self._wt_version = -1

    def ref_layout(self, t):
        D, C_, r = self.out_channels, self.channels, self.res
        return t.view(D, r, r, C_).permute(0, 3, 1, 2).reshape(D, C_ * r * r)


class _MLPFn(Function):
    """x = relu(fc7(relu(fc6(flatten(pooled))))) as one autograd node with a hand-scheduled backward: (pooled logical [K,C,res,res],
    extractor, *parameters) -> [K,D]"""

    @staticmethod
    def forward(ctx, pooled, ext, *params):
        xh = as_nhwc(pooled)
        flat = _rows(xh)
        h6, h7 = ext._mlp(flat)
        ctx.ext, ctx.saved, ctx.xshape = ext, (flat, h6, h7), tuple(xh.shape)
        out = ops.amax_carry(h7.view(h7.shape[0], -1), h7)
        return out

    @staticmethod
    def backward(ctx, gout):
        ext = ctx.ext
        flat, h6, h7 = ctx.saved
        ctx.saved = None
        fc6, fc7, m = ext.fc6, ext.fc7, ext.math
        need_dx = bool(ctx.needs_input_grad[0])
        train6, train7 = fc6.weight.requires_grad, fc7.weight.requires_grad
        if not (need_dx or train6 or train7):
            return (None,) * len(ctx.needs_input_grad)
        # fc7's ReLU mask: applied already when the producer of gout (the predictor's input gradient) carried it in its epilogue -- the token
        # is bound to that very storage and version (see box_head._PredictorFn.backward); any other gradient is masked here
        masked = getattr(gout, "_abr_relu_masked", None) == (gout.data_ptr(), gout._version)
        g = gout if gout.is_contiguous() else gout.contiguous()
        g = _rows(g) if masked else ops.relu_backward(_rows(g), h7)
        if train7:
            ops.conv_wgrad_async(h6, g, _grad_buf(fc7.weight), 1, 0, math=m)
            ops.bias_grad(g, _grad_buf(fc7.bias))
        gx = None
        if need_dx or train6:
            g6 = ops.conv_forward(g, fc7.dgrad_weight(), 1, 0, mask=h6, math=m, w_version=fc7.version())     # (fc6's ReLU mask rides here)
            if train6:
                ops.conv_wgrad_async(flat, g6, _grad_buf(fc6.weight), 1, 0, math=m)
                ops.bias_grad(g6, _grad_buf(fc6.bias))
            if need_dx:
                gx = from_nhwc(ops.conv_forward(g6, fc6.dgrad_weight(), 1, 0, math=m, w_version=fc6.version()).view(ctx.xshape))
        return (gx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class FPN2MLPFeatureExtractor(nn.Module):
    """roi_box_feature_extractors.py:59-101.  forward -> (x [K,D], pooled logical [K,C,res,res])."""

    def __init__(self, cfg, in_channels):
        super().__init__()
        head = cfg.MODEL.ROI_BOX_HEAD
        if head.USE_GN:
            raise NotImplementedError("MODEL.ROI_BOX_HEAD.USE_GN True: the GroupNorm fully connected layers (make_fc(use_gn=True)) are not built")
        res, D = head.POOLER_RESOLUTION, head.MLP_HEAD_DIM
        if in_channels % 4 or D % 4:
            raise NotImplementedError("FPN2MLPFeatureExtractor: {} input channels, MODEL.ROI_BOX_HEAD.MLP_HEAD_DIM {}: the contractions move 4 "
                                      "channels per lane, both must be multiples of 4".format(in_channels, D))
        self.pooler = make_pooler(cfg, "ROI_BOX_HEAD")
        self.n_levels = len(head.POOLER_SCALES)
        self.fc6 = _FC(in_channels, res, D)
        self.fc7 = _FC(D, 1, D)
        self.out_channels = D
        self.resolution = res
        self.in_channels = in_channels
        self.math = ops.MATH_F32   # the contractions' arithmetic (resnet.set_conv_math)
        if cfg.MODEL.ROI_HEADS.FC_FREEZE:   # :79-91
            for p in list(self.fc6.parameters()) + list(self.fc7.parameters()):
                p.requires_grad = False

    joint_supported = True    # every bin is read: no bin_step trick, nothing to refuse

    def prep_entries(self):
        """FusedSGD's batched weight preparation (see Bottleneck.prep_entries): the dgrad copies and what the library derives from the weights"""
        return [(c, None, 1, 0, self.math) for c in (self.fc6, self.fc7) if c.weight.requires_grad and c.weight.is_cuda]

    def _mlp(self, flat):
        """flat [K,1,1,res*res*C] -> (h6, h7), each [K,1,1,D] and already through its ReLU"""
        h6 = ops.conv_forward(flat, self.fc6.weight, 1, 0, bias=self.fc6.bias, relu=True, math=self.math, w_version=self.fc6.version())
        h7 = ops.conv_forward(h6, self.fc7.weight, 1, 0, bias=self.fc7.bias, relu=True, math=self.math, w_version=self.fc7.version())
        return h6, h7

    def _pool(self, x, rois):
        """the box pooler sees the first len(POOLER_SCALES) maps (the RPN's coarsest, P6, is not pooled: the reference's zip drops it)"""
        x = list(x)
        if len(x) < self.n_levels:
            raise RuntimeError("FPN2MLPFeatureExtractor: {} feature maps for {} MODEL.ROI_BOX_HEAD.POOLER_SCALES".format(len(x), self.n_levels))
        return self.pooler(x[: self.n_levels], rois)

    def _head(self, pooled):
        K = pooled.shape[0]
        if K == 0:
            return pooled.new_zeros((0, self.out_channels))
        params = list(self.parameters())
        if torch.is_grad_enabled() and (pooled.requires_grad or any(p.requires_grad for p in params)):
            x = _MLPFn.apply(pooled, self, *params)
        else:
            h7 = self._mlp(_rows(as_nhwc(pooled)))[1]
            x = ops.amax_carry(h7.view(K, -1), h7)
        x._abr_relu_output = True     # (the predictor's backward may fold fc7's ReLU mask into its input gradient's epilogue)
        return x

    def _table(self, boxes):
        return boxes if torch.is_tensor(boxes) else self.pooler.convert_to_roi_format(boxes)

    def forward(self, x, proposals, need_roi_features=True):
        """x: the pyramid's maps, logical [B,C,H_l,W_l]; proposals: list of BoxLists or a ready [K,5] RoI table.  need_roi_features is
        accepted for the C4 extractor's signature: every bin is pooled either way."""
        rois = self._table(proposals)
        if rois.shape[0] == 0:
            r = self.resolution
            return rois.new_zeros((0, self.out_channels)), rois.new_zeros((0, r, r, self.in_channels)).permute(0, 3, 1, 2)
        pooled = self._pool(x, rois)
        return self._head(pooled), pooled

    def forward_joint(self, x, det_proposals, soft_proposals, soft_early=None):
        """Detection RoIs and the source model's distillation RoIs from ONE concatenated RoI table: one pooler launch, one MLP pass.
        -> (x [Kd+Ks,D], detection pooled [Kd,C,res,res], distillation pooled [Ks,C,res,res])"""
        det, soft = self._table(det_proposals), self._table(soft_proposals)
        Kd = det.shape[0]
        pooled = self._pool(x, torch.cat((det, soft.to(det.dtype)), 0))
        return self._head(pooled), pooled[:Kd], pooled[Kd:]


class _FPNPredictorFn(Function):
    """the fused cls | bbox GEMM over [K,D] rows: (x, predictor, *parameters) -> [K, n_out_pad]"""

    @staticmethod
    def forward(ctx, x, pred, *params):
        xr = _rows(x if x.is_contiguous() else x.contiguous())
        K_ = xr.shape[0]
        y = ops.conv_forward(xr, pred.fused_weight, 1, 0, bias=pred.fused_bias).view(K_, -1)
        ctx.pred, ctx.saved = pred, xr
        ctx.relu_of = xr if getattr(x, "_abr_relu_output", False) and x.is_contiguous() else None
        return y

    @staticmethod
    def backward(ctx, gy):
        pred, xr = ctx.pred, ctx.saved
        ctx.saved = None
        K_ = xr.shape[0]
        g = gy.contiguous().view(K_, 1, 1, -1)
        pred._weight_grads(xr, g)
        gx = None
        if ctx.needs_input_grad[0]:
            gp = ops.conv_forward(g, pred.fused_dgrad_weight(), 1, 0, mask=ctx.relu_of, emit_amax=True)     # (amax word for fc7's f16x3 backward)
            gx = ops.amax_carry(gp.view(K_, -1), gp)
            if ctx.relu_of is not None:
                gx._abr_relu_masked = (gx.data_ptr(), gx._version)    # the token of box_head._PredictorFn.backward: see _MLPFn.backward
        ctx.relu_of = None
        return (gx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class FPNPredictor(FastRCNNPredictor):
    """roi_box_predictors.py:36-132 without the offset layers: FastRCNNPredictor's fused storage, flat-buffer hooks and init (std 0.01 /
    0.001), no average pool, CLS_FREEZE / BBS_FREEZE honoured.  Accepts [K,D] or [K,D,1,1]."""

    def __init__(self, config, in_channels):
        heads = config.MODEL.ROI_HEADS
        for key in ("CLS_OFFSET", "BBS_OFFSET"):
            if heads[key]:
                raise NotImplementedError("MODEL.ROI_HEADS.{} True: the predictor's offset layers are not built (the reference's BBS_OFFSET "
                                          "broadcasts for exactly one new class only)".format(key))
        if in_channels % 4:
            raise NotImplementedError("FPNPredictor: {} input features, need a multiple of 4".format(in_channels))
        super().__init__(config, in_channels)
        if heads.CLS_FREEZE:     # :82-90
            for p in self.cls_score.parameters():
                p.requires_grad = False
        if heads.BBS_FREEZE:
            for p in self.bbox_pred.parameters():
                p.requires_grad = False
        self._set_fused(self._fw2d, self.fused_bias, self._gw2d, self.fused_bias_grad)

    def _trains(self):
        return self.cls_score.weight.requires_grad, self.bbox_pred.weight.requires_grad

    def _set_fused(self, fw, fb, gw, gb):
        super()._set_fused(fw, fb, gw, gb)
        for mod in (self.cls_score, self.bbox_pred):     # a frozen layer has no gradient (its rows of the fused gradient buffer stay zero)
            if not mod.weight.requires_grad:
                mod.weight.grad = mod.bias.grad = None
        self._snap = None
        self._keep_frozen_rows()      # new storage (construction, a device move, the flat buffers): the frozen half's copy is taken now

    # --- a frozen half inside the fused storage.  The two layers share one flat segment (flat_groups: the GEMM needs them adjacent), which the
    # fused optimiser updates as a whole: the frozen rows' gradient is zero, but weight decay would still shrink them.  So the frozen rows
    # are kept as a copy -- taken when the storage is set and again by the first forward pass after weights were loaded or set
    # (resnet._STATIC_VERSION; a step cannot come before that pass) -- and written back after every optimiser step: by prepare_derived on the
    # weight-preparation stream, behind the SGD kernel and ahead of the dgrad copy derived from the fused weight, or, without that stream, by
    # the next forward pass.  Every forward pass of a half-frozen predictor waits for the preparation (ops.prep_wait) before it reads the
    # fused weight, whether or not it is the call that restores.
    def _half_frozen(self):
        cls_t, bbs_t = self._trains()
        return cls_t != bbs_t and self.fused_weight.is_cuda

    def _keep_frozen_rows(self):
        if not self._half_frozen():
            return
        K, R4 = self.num_classes, self.num_bbox_reg_classes * 4
        lo, hi = (0, K) if not self._trains()[0] else (K, K + R4)
        pv, sv = resnet._PARAM_VERSION[0], resnet._STATIC_VERSION[0]
        snap = self._snap
        if snap is None or snap["static"] != sv:
            self._snap = dict(static=sv, param=pv, w=self._fw2d[lo:hi].clone(), b=self.fused_bias[lo:hi].clone())
        elif snap["param"] != pv:
            with torch.no_grad():
                self._fw2d[lo:hi].copy_(snap["w"])
                self.fused_bias[lo:hi].copy_(snap["b"])
            snap["param"] = pv

    def prepare_derived(self):
        """FusedSGD.step, right after the update: a frozen half restored, the fused dgrad copy rebuilt"""
        self._keep_frozen_rows()
        if self.fused_weight.is_cuda and any(self._trains()):
            self.fused_dgrad_weight()

    def _weight_grads(self, xr, g):
        """weight and bias gradients of the trainable layers only (a frozen layer launches nothing); g [K,1,1,n_out_pad] contiguous"""
        cls_t, bbs_t = self._trains()
        if cls_t and bbs_t:
            ops.conv_wgrad_async(xr, g, self.fused_weight_grad, 1, 0)
            ops.bias_grad(g, self.fused_bias_grad)
            return
        if not (cls_t or bbs_t):
            return
        K, R4 = self.num_classes, self.num_bbox_reg_classes * 4
        g2 = g.view(g.shape[0], -1)
        if bbs_t:
            lo, n = K, R4
            part = g2[:, lo:lo + n].contiguous()
        else:
            # the weight gradient kernel writes multiples of 4 rows: the columns past the K class logits are ZERO here, so the first rows of the
            # frozen bbox_pred gradient receive + 0.0 (rows [K, n) exist: n <= n_out_pad)
            lo, n = 0, (K + 3) // 4 * 4
            part = torch.zeros((g2.shape[0], n), dtype=g2.dtype, device=g2.device)
            part[:, :K].copy_(g2[:, :K])
        part = part.view(part.shape[0], 1, 1, n)
        ops.conv_wgrad_async(xr, part, self.fused_weight_grad[lo:lo + n], 1, 0)
        ops.bias_grad(part, self.fused_bias_grad[lo:lo + n])

    def forward_fused(self, x):
        if x.dim() == 4:
            if x.shape[2] != 1 or x.shape[3] != 1:
                raise ValueError("FPNPredictor: expected [K,D] or [K,D,1,1], got {}".format(tuple(x.shape)))
            flat = x.reshape(x.shape[0], x.shape[1])
            if getattr(x, "_abr_relu_output", False):
                flat._abr_relu_output = True
            x = ops.amax_carry(flat, x)
        if x.shape[0] == 0:
            return x.new_zeros((0, self.n_out_pad))
        if self._half_frozen():
            ops.prep_wait()           # the restore of the frozen rows may have run on the weight-preparation stream: read behind it
            self._keep_frozen_rows()
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _FPNPredictorFn.apply(x, self, *params)
        xr = _rows(x if x.is_contiguous() else x.contiguous())
        return ops.conv_forward(xr, self.fused_weight, 1, 0, bias=self.fused_bias).view(xr.shape[0], -1)

"""RoI mask head on the HIP library (MODEL.MASK_ON; the C4 variant: the reference's defaults, config/defaults.py:258-274).

Mirrors:
    ROIMaskHead                 maskrcnn_benchmark/modeling/roi_heads/mask_head/mask_head.py:13-89
    MaskRCNNC4Predictor         mask_head/roi_mask_predictors.py:10-32
    MaskRCNNLossComputation     mask_head/loss.py:11-141
    MaskPostProcessor / Masker  mask_head/inference.py:12-209

MI355X-first differences (results identical):
  * the positives of the box head's sampled set are compacted ON THE DEVICE into a fixed-size, -1 padded list (at most POSITIVE_FRACTION *
    BATCH_SIZE_PER_IMAGE rows per image): no nonzero(), no read-back; padding rows carry zeros through the predictor and the loss skips them.
  * the mask targets of the whole batch are ONE launch (the reference crops and resizes per RoI on the host, loss.py:31), for bitmask
    targets (ops.mask_targets) and for polygon targets (PolygonList fields, ops.poly_mask_targets) alike.
  * ConvTranspose2d(2, 2, 0) is a GEMM with 4 * C_mid output columns on the conv planner plus one depth-to-space + bias + ReLU pass.
"""
import torch
from torch import nn
from torch.autograd import Function

from .... import ops
from ....layers._layout import as_nhwc, from_nhwc
from ....structures.bounding_box import BoxList
from ....structures.polygon import PolygonList
from ...backbone.resnet import Conv2d, _grad_buf


FPN_LEVEL_SCALES = (0.25, 0.125, 0.0625, 0.03125)      # P2..P5: the maps a RoI pooler may read (P6 is the RPN's alone)


def check_mask_head_cfg(cfg):
    """C4 body: NotImplementedError naming the key for everything but the shared C4 head; ValueError when RESOLUTION does not fit the box head's
    pooler.  FPN body: the unshared MaskRCNNFPNFeatureExtractor + MaskRCNNC4Predictor; every refusal names its key and value."""
    from ...backbone.resnet import FPN_BODIES
    m, b = cfg.MODEL.ROI_MASK_HEAD, cfg.MODEL.ROI_BOX_HEAD
    body = cfg.MODEL.BACKBONE.CONV_BODY

    def unsupported(key, value, why):
        raise NotImplementedError("MODEL.ROI_MASK_HEAD.{} = {!r}: {}".format(key, value, why))

    if body in FPN_BODIES:
        if m.FEATURE_EXTRACTOR != "MaskRCNNFPNFeatureExtractor":
            raise NotImplementedError("MODEL.MASK_ON True on MODEL.BACKBONE.CONV_BODY {!r} with MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR = {!r}: an FPN "
                                      "body runs the mask head on its own pyramid pooler; set MODEL.ROI_MASK_HEAD.FEATURE_EXTRACTOR to "
                                      "'MaskRCNNFPNFeatureExtractor' (and SHARE_BOX_FEATURE_EXTRACTOR to False)".format(body, m.FEATURE_EXTRACTOR))
        if m.PREDICTOR != "MaskRCNNC4Predictor":
            unsupported("PREDICTOR", m.PREDICTOR, "this build runs MaskRCNNC4Predictor only (upstream's FPN configurations name it too)")
        if m.SHARE_BOX_FEATURE_EXTRACTOR:
            unsupported("SHARE_BOX_FEATURE_EXTRACTOR", m.SHARE_BOX_FEATURE_EXTRACTOR,
                        "the FPN box extractor ends in the MLP head's [N, MLP_HEAD_DIM] rows, which no mask predictor can read; set it to False")
        if m.USE_GN:
            unsupported("USE_GN", m.USE_GN, "the GroupNorm mask convs are not built")
        if m.DILATION != 1:
            unsupported("DILATION", m.DILATION, "dilated mask convs are not built")
        layers = tuple(m.CONV_LAYERS)
        if not layers or any(c <= 0 or c % 4 for c in layers):
            unsupported("CONV_LAYERS", layers, "channel counts must be positive multiples of 4")
        scales = tuple(m.POOLER_SCALES)
        if not scales or scales != FPN_LEVEL_SCALES[:len(scales)]:
            unsupported("POOLER_SCALES", scales, "the mask pooler reads the leading maps of the pyramid, at most the four of P2..P5: a prefix of {!r}"
                        .format(FPN_LEVEL_SCALES))
        if m.RESOLUTION != 2 * m.POOLER_RESOLUTION:
            raise ValueError("MODEL.ROI_MASK_HEAD.RESOLUTION = {} but the predictor's output is {} x {} for MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION = {} "
                             "(the conv stack keeps the pooled size, the deconvolution doubles it): set RESOLUTION to {}".format(
                                 m.RESOLUTION, 2 * m.POOLER_RESOLUTION, 2 * m.POOLER_RESOLUTION, m.POOLER_RESOLUTION, 2 * m.POOLER_RESOLUTION))
        return
    if m.FEATURE_EXTRACTOR != "ResNet50Conv5ROIFeatureExtractor":
        unsupported("FEATURE_EXTRACTOR", m.FEATURE_EXTRACTOR, "a C4 body runs the C4 mask head (ResNet50Conv5ROIFeatureExtractor) only, no FPN extractor "
                    "(MaskRCNNFPNFeatureExtractor pools a pyramid: MODEL.BACKBONE.CONV_BODY {!r} has none)".format(body))
    if m.PREDICTOR != "MaskRCNNC4Predictor":
        unsupported("PREDICTOR", m.PREDICTOR, "this build runs MaskRCNNC4Predictor only")
    if m.USE_GN:
        unsupported("USE_GN", m.USE_GN, "GroupNorm mask heads belong to the FPN extractor")
    if m.DILATION != 1:
        unsupported("DILATION", m.DILATION, "dilated mask convs belong to the FPN extractor")
    if not m.SHARE_BOX_FEATURE_EXTRACTOR:
        unsupported("SHARE_BOX_FEATURE_EXTRACTOR", m.SHARE_BOX_FEATURE_EXTRACTOR, "the mask head reads the box head's layer4 output; a second layer4 is not built")
    for key in ("POOLER_RESOLUTION", "POOLER_SAMPLING_RATIO", "POOLER_SCALES"):
        mv, bv = m[key], b[key]
        same = tuple(mv) == tuple(bv) if isinstance(mv, (tuple, list)) else mv == bv
        if not same:
            unsupported(key, mv, "the shared feature extractor pools with MODEL.ROI_BOX_HEAD.{} = {!r}".format(key, bv))
    side = (b.POOLER_RESOLUTION - 1) // 2 + 1      # layer4's stride-2 first block over the pooled map
    if 2 * side != m.RESOLUTION:
        raise ValueError("MODEL.ROI_MASK_HEAD.RESOLUTION = {} but the C4 predictor's output is {} x {} for MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION = {} "
                         "(layer4 gives {} x {}, the deconvolution doubles it): set RESOLUTION to {}".format(
                             m.RESOLUTION, 2 * side, 2 * side, b.POOLER_RESOLUTION, side, side, 2 * side))


class ConvTranspose2x2(Conv2d):
    """nn.ConvTranspose2d(Cin, Cmid, 2, 2, 0) as the 1x1 conv (GEMM) whose 4 * Cmid output columns are (dy, dx, co): the weight is held as that
    conv's OHWI [4 Cmid, 1, 1, Cin], the bias as the reference's [Cmid]; the checkpoint boundary sees [Cin, Cmid, 2, 2]."""
    whole_only = True    # (rows of the stored tensor are not rows of this layout: utils/checkpoint.py never copies a leading part)

    def __init__(self, in_channels, out_channels):
        super().__init__(in_channels, 4 * out_channels, 1, bias=False)
        self.out_channels = out_channels
        self.bias = nn.Parameter(torch.zeros(out_channels))

    def load_oihw(self, w):
        with torch.no_grad():
            self.weight.copy_(w.permute(2, 3, 1, 0).reshape(self.weight.shape))
        self._wt_version = -1

    def ref_layout(self, t):
        return t.view(2, 2, self.out_channels, self.in_channels).permute(3, 2, 0, 1)


class _PredictorFn(Function):
    """logits = conv1x1(relu(deconv2x2(x))) as one autograd node; the weight gradients go straight into the flat gradient buffer"""

    @staticmethod
    def forward(ctx, x, pred, *params):
        xh = as_nhwc(x)
        t, z = pred._run(xh)
        ctx.pred, ctx.saved, ctx.need_dx = pred, (xh, t), x.requires_grad
        return from_nhwc(z)

    @staticmethod
    def backward(ctx, gz):
        pred = ctx.pred
        xh, t = ctx.saved
        c5, cl, math = pred.conv5_mask, pred.mask_fcn_logits, pred.math
        g = as_nhwc(gz)
        if not g.is_contiguous():
            g = g.contiguous()
        if cl.weight.requires_grad:
            ops.conv_wgrad_async(t, g, _grad_buf(cl.weight), 1, 0, math=math)
            ops.bias_grad(g, _grad_buf(cl.bias))
        gt = ops.conv_forward(g, cl.dgrad_weight(), 1, 0, math=math)
        gy = ops.mask_d2s_bias_relu_backward(gt, t)
        if c5.weight.requires_grad:
            ops.bias_grad(gy.view(-1, c5.out_channels), _grad_buf(c5.bias))
            ops.conv_wgrad_async(xh, gy, _grad_buf(c5.weight), 1, 0, math=math)
        gx = from_nhwc(ops.conv_forward(gy, c5.dgrad_weight(), 1, 0, math=math, w_version=c5.version())) if ctx.need_dx else None
        ctx.saved = None
        return (gx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class MaskRCNNC4Predictor(nn.Module):
    def __init__(self, cfg, in_channels):
        super().__init__()
        num_classes = cfg.MODEL.ROI_BOX_HEAD.NUM_CLASSES
        dim_reduced = cfg.MODEL.ROI_MASK_HEAD.CONV_LAYERS[-1]
        if dim_reduced % 4 or in_channels % 4:
            raise NotImplementedError("MODEL.ROI_MASK_HEAD.CONV_LAYERS[-1] = {}: channel counts must be multiples of 4".format(dim_reduced))
        self.num_classes = num_classes
        self.math = ops.MATH_F32     # see backbone.resnet.set_conv_math
        self.conv5_mask = ConvTranspose2x2(in_channels, dim_reduced)
        self.mask_fcn_logits = Conv2d(dim_reduced, num_classes, 1, cout_pad=(num_classes + 3) // 4 * 4)
        with torch.no_grad():    # roi_mask_predictors.py:24-29: biases 0, weights kaiming_normal_(mode="fan_out", nonlinearity="relu")
            self.conv5_mask.weight.normal_(0.0, (2.0 / (4 * in_channels)) ** 0.5)
            self.mask_fcn_logits.weight.zero_()
            self.mask_fcn_logits.weight[:num_classes].normal_(0.0, (2.0 / num_classes) ** 0.5)

    def prep_entries(self):
        """FusedSGD's batched weight preparation (see Bottleneck.prep_entries)"""
        return [(c, None, 1, 0, self.math) for c in (self.conv5_mask, self.mask_fcn_logits) if c.weight.requires_grad and c.weight.is_cuda]

    def _run(self, xh):
        c5, cl = self.conv5_mask, self.mask_fcn_logits
        y = ops.conv_forward(xh, c5.weight, 1, 0, math=self.math, w_version=c5.version())
        t = ops.mask_d2s_bias_relu(y, c5.bias)
        z = ops.conv_forward(t, cl.weight, 1, 0, bias=cl.bias, math=self.math, w_version=cl.version())
        return t, z

    def forward_padded(self, x):
        """x logical [P,C_head,h,w] -> logical [P,K_pad,2h,2w]: the logits with the class axis padded to a multiple of 4 (NHWC memory; the
        padding channels are zero-weight outputs no consumer reads)"""
        if x.shape[0] == 0:
            return x.new_zeros((0, 2 * x.shape[2], 2 * x.shape[3], self.mask_fcn_logits.weight.shape[0])).permute(0, 3, 1, 2)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            return _PredictorFn.apply(x, self, *params)
        return from_nhwc(self._run(as_nhwc(x))[1])

    def forward(self, x):
        """-> mask logits, logical [P,num_classes,2h,2w]"""
        return self.forward_padded(x)[:, :self.num_classes]


class _GatherRowsFn(Function):
    """rows pos_rows of the head output (zeros for the -1 padding); backward writes every row of the gradient once through the inverse map"""

    @staticmethod
    def forward(ctx, x, pos_rows, inv):
        xh = as_nhwc(x)
        out = ops.mask_gather_rows(xh, pos_rows)
        ops.amax_carry_bound(out, xh)      # a subset of x's values (and zeros): x's amax word bounds it (f16x3 scales)
        ctx.save_for_backward(inv)
        return from_nhwc(out)

    @staticmethod
    def backward(ctx, g):
        (inv,) = ctx.saved_tensors
        gh = as_nhwc(g)
        return from_nhwc(ops.mask_gather_rows(gh if gh.is_contiguous() else gh.contiguous(), inv)), None, None


class _MaskLossFn(Function):
    @staticmethod
    def forward(ctx, logits, num_classes, labels, targets, n_pos):
        zh = as_nhwc(logits)
        want = logits.requires_grad
        loss, grad = ops.mask_loss(zh, num_classes, labels, targets, n_pos=n_pos, want_grad=want)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        grad = grad.clone()
        ops.scale_(grad, 1.0, g.contiguous())
        return from_nhwc(grad), None, None, None, None


class MaskRCNNLossComputation(object):
    def __init__(self, discretization_size, max_pos_per_image):
        self.discretization_size, self.max_pos_per_image = discretization_size, max_pos_per_image

    def select(self, proposals, targets, fused=None):
        """the positives of the box head's sampled proposals (labels > 0, loss.py:86 / mask_head.py:27-33) and their targets, on the device:
        -> dict(pos_rows, pos_labels, inv, n_pos, mask_targets [P_max,M,M], rois: the sampled set's [R,5] table pos_rows indexes)"""
        if fused is not None:      # ops.roi_head_targets' output: the batch's RoI table and labels are single tensors already
            labels, rois = fused["labels"], fused["rois"]
        else:
            labels = torch.cat([p.get_field("labels") for p in proposals])
            dev = labels.device
            rois = torch.cat([torch.cat((torch.full((len(p), 1), float(i), device=dev), p.convert("xyxy").bbox), 1) for i, p in enumerate(proposals)])
        p_max = max(1, min(labels.numel(), self.max_pos_per_image * len(proposals)))
        pos_rows, pos_labels, inv, n_pos = ops.mask_compact_pos(labels, p_max)
        segs = []
        for p, t in zip(proposals, targets):
            seg = t.get_field("masks")
            if tuple(seg.size) != tuple(p.size):
                raise AssertionError("{}, {}".format(seg, p))     # loss.py:27
            segs.append(seg)
        gt_boxes = [t.convert("xyxy").bbox for t in targets]
        n_poly = sum(isinstance(seg, PolygonList) for seg in segs)
        if n_poly:       # polygon targets: cropped, scaled and rasterised per RoI on the device (the reference: pycocotools on the host)
            if n_poly != len(segs):
                raise TypeError("the \"masks\" fields of a batch must be all PolygonList or all SegmentationMask, got {}: convert the polygon "
                                "lists with .convert(\"mask\")".format([type(seg).__name__ for seg in segs]))
            mt = ops.poly_mask_targets(segs, gt_boxes, rois, pos_rows, self.discretization_size)
        else:
            mt = ops.mask_targets([seg.masks for seg in segs], gt_boxes, rois, pos_rows, self.discretization_size)
        return dict(pos_rows=pos_rows, pos_labels=pos_labels, inv=inv, n_pos=n_pos, mask_targets=mt, rois=rois)

    def __call__(self, sel, padded_logits, num_classes):
        """padded_logits: MaskRCNNC4Predictor.forward_padded's"""
        return _MaskLossFn.apply(padded_logits, num_classes, sel["pos_labels"], sel["mask_targets"], sel["n_pos"])


class MaskPostProcessor(nn.Module):
    """inference.py:12-61 (+ Masker, :162-199, when POSTPROCESS_MASKS)"""

    def __init__(self, paste=False, threshold=0.5):
        super().__init__()
        self.paste, self.threshold = paste, threshold

    def forward(self, x, boxes, num_classes):
        """x: the predictor's padded logits, logical [D,K_pad,M,M]"""
        labels = torch.cat([b.get_field("labels") for b in boxes]) if boxes else x.new_zeros((0,), dtype=torch.int64)
        D = x.shape[0]
        prob = ops.mask_select_sigmoid(as_nhwc(x), num_classes, labels) if D else x.new_zeros((0, 1) + tuple(x.shape[2:]))
        results, off = [], 0
        for b in boxes:
            n = len(b)
            m = prob[off:off + n]
            off += n
            if self.paste:
                im_w, im_h = b.size
                m = ops.mask_paste(m, b.convert("xyxy").bbox, im_h, im_w, self.threshold) if n else m.new_empty((0, 1) + tuple(m.shape[2:]))
            r = BoxList(b.bbox, b.size, mode="xyxy")
            for f in b.fields():
                r.add_field(f, b.get_field(f))
            r.add_field("mask", m)
            results.append(r)
        return results


class ROIMaskHead(nn.Module):
    """Two modes.  SHARED (the C4 bodies): the extractor is the box head's, training reads the box head's layer4 rows.  UNSHARED (the FPN bodies,
    SHARE_BOX_FEATURE_EXTRACTOR False): its own MaskRCNNFPNFeatureExtractor (fpn_mask_head.py) on the pyramid, registered here."""

    def __init__(self, cfg, in_channels, box_feature_extractor):
        super().__init__()
        check_mask_head_cfg(cfg)
        self.unshared = not cfg.MODEL.ROI_MASK_HEAD.SHARE_BOX_FEATURE_EXTRACTOR
        if self.unshared:
            from .fpn_mask_head import MaskRCNNFPNFeatureExtractor
            self.add_module("feature_extractor", MaskRCNNFPNFeatureExtractor(cfg, in_channels))
        else:
            # the SHARED extractor is the box head's module; it is not registered a second time (one set of parameters in the flat buffers);
            # reference_state_dict emits the reference's duplicate roi_heads.mask.feature_extractor.* keys
            self.__dict__["_feature_extractor"] = box_feature_extractor
        self.predictor = MaskRCNNC4Predictor(cfg, self.feature_extractor.out_channels)
        self.post_processor = MaskPostProcessor(cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS, cfg.MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS_THRESHOLD)
        rh = cfg.MODEL.ROI_HEADS
        self.loss_evaluator = MaskRCNNLossComputation(cfg.MODEL.ROI_MASK_HEAD.RESOLUTION, int(rh.BATCH_SIZE_PER_IMAGE * rh.POSITIVE_FRACTION))

    @property
    def feature_extractor(self):
        own = self._modules.get("feature_extractor")
        return own if own is not None else self._feature_extractor

    def forward(self, features, proposals, targets=None, fused=None):
        """training: `features` = the box head's layer4 output for `proposals` (its sampled set, with "labels") -- unshared: the backbone's
        maps -> (x, proposals, {loss_mask});
        eval: `features` = the backbone's, `proposals` = the detections -> (x, detections with "mask", {})  (mask_head.py:46-79)"""
        K = self.predictor.num_classes
        if self.training:
            with torch.no_grad():
                sel = self.loss_evaluator.select(proposals, targets, fused=fused)
            if self.unshared:     # the positives are pooled as rows of the sampled set's table: nothing is gathered, nothing read back
                x = self.feature_extractor(features, sel["rois"], rows=sel["pos_rows"])
            else:
                x = _GatherRowsFn.apply(features, sel["pos_rows"], sel["inv"])
            padded = self.predictor.forward_padded(x)
            self.last_selection, self.last_mask_logits = sel, padded[:, :K]       # (introspection for parity tests)
            return x, proposals, dict(loss_mask=self.loss_evaluator(sel, padded, K))
        if sum(len(p) for p in proposals) == 0:
            side = self.loss_evaluator.discretization_size
            empty = features[0].new_zeros((0, side, side, 4)).permute(0, 3, 1, 2)
            return None, self.post_processor(empty, proposals, K), {}
        if self.unshared:
            x = self.feature_extractor(features, proposals)
        else:
            x, _ = self.feature_extractor(features, proposals, need_roi_features=False)
        return x, self.post_processor(self.predictor.forward_padded(x), proposals, K), {}

    def calculate_soften_label(self, features, proposals=None):
        """mask_head.py:81-86: the predictor on the given head features.  Unshared: `features` = the backbone's maps and the logits are
        predictor(extractor(features, proposals)) on the proposals the box soften labels use -- this project's definition (the reference
        feeds the MLP head's [N,1024] output to the deconvolution and fails there); an empty set gives an empty tensor."""
        if self.unshared:
            return self.predictor(self.feature_extractor(features, proposals))
        return self.predictor(features)


def build_roi_mask_head(cfg, in_channels, box_feature_extractor):
    return ROIMaskHead(cfg, in_channels, box_feature_extractor)

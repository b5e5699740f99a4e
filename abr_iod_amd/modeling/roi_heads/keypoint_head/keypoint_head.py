"""RoI keypoint head on the HIP library (MODEL.KEYPOINT_ON on the C4 and the FPN bodies, SHARE_BOX_FEATURE_EXTRACTOR False).

Mirrors:
    ROIKeypointHead                  maskrcnn_benchmark/modeling/roi_heads/keypoint_head/keypoint_head.py
    KeypointRCNNFeatureExtractor     keypoint_head/roi_keypoint_feature_extractors.py:11-43
    KeypointRCNNPredictor            keypoint_head/roi_keypoint_predictors.py:8-33
    KeypointRCNNLossComputation      keypoint_head/loss.py:54-169
    KeypointPostProcessor            keypoint_head/inference.py:5-125

MI355X-first differences:
  * the head's sampler can never cut (its input is the box head's sampled set, at most POSITIVE_FRACTION * BATCH_SIZE_PER_IMAGE positives per
    image at the same thresholds), so the selection is deterministic: the box-head positives, in row order, whose matched instance has a visible
    keypoint inside its box.  It and the heat-map targets are ONE launch for the batch (ops.kp_select_targets), nothing read back; the list is
    fixed-size and -1 padded, padding rows pool a degenerate RoI, carry valid = 0 and so add no loss and exactly zero gradients.  The two
    randperm draws per image the reference spends in its sampler are not reproduced.
  * ConvTranspose2d(C, K, 4, 2, 1) is a GEMM with 16 * Kp output columns on the conv planner plus a fold pass into PLANAR maps [P,Kp,2h,2w].
  * training never materialises the upsampled logits: ops.kp_loss upsamples on the fly and returns the gradient of the low-resolution maps.
  * heatmaps_to_keypoints runs on the device (ops.kp_decode), for any number of images (the reference asserts one).

On an FPN body (upstream's only published keypoint setting: four POOLER_SCALES, pooler 14, sampling ratio 2, RESOLUTION 56) the extractor is
its pyramid form, roi_heads/pyramid_extractor.py's pooler + conv stack node, the one the FPN mask head runs.  Training pools
rows = pos_rows of the table the sampled set already is on the device (the fused sampler's, or the concatenated BoxLists'): no gathered RoI
table is built.  A padding row is ZERO features in and relu(bias) features out (the C4 form pools a degenerate RoI instead); it never reads
the table, has valid = 0, and so adds no loss and exactly zero gradient to weights, biases and maps.  Eval pools the detections of all
images through the same extractor, without rows.
"""
import torch
from torch import nn
from torch.autograd import Function

from .... import ops
from ....layers._layout import as_nhwc, from_nhwc
from ....structures.bounding_box import BoxList
from ....structures.keypoint import PersonKeypoints
from ...backbone.resnet import Conv2d, _grad_buf
from ..box_head.box_head import convert_to_roi_format
from ..conv_stack import conv_stack_backward, conv_stack_forward
from ..pyramid_extractor import PyramidConvExtractor, make_conv3x3_stack


def _on_pyramid(cfg):
    from ...backbone.resnet import FPN_BODIES
    return cfg.MODEL.BACKBONE.CONV_BODY in FPN_BODIES


def check_keypoint_head_cfg(cfg, body_scale=None):
    """C4 body: NotImplementedError naming the key for everything but the keypoint head with its own extractor on the body's one scale.
    FPN body: the same extractor and predictor on its own pyramid pooler, POOLER_SCALES a leading run of P2..P5's; every refusal names its key
    and value.  Both: ValueError when RESOLUTION is not four times the pooler's"""
    k = cfg.MODEL.ROI_KEYPOINT_HEAD
    body, pyramid = cfg.MODEL.BACKBONE.CONV_BODY, _on_pyramid(cfg)

    def unsupported(key, value, why):
        raise NotImplementedError("MODEL.ROI_KEYPOINT_HEAD.{} = {!r}: {}".format(key, value, why))

    if k.FEATURE_EXTRACTOR != "KeypointRCNNFeatureExtractor":
        unsupported("FEATURE_EXTRACTOR", k.FEATURE_EXTRACTOR, "this build runs KeypointRCNNFeatureExtractor only")
    if k.PREDICTOR != "KeypointRCNNPredictor":
        unsupported("PREDICTOR", k.PREDICTOR, "this build runs KeypointRCNNPredictor only")
    if pyramid:
        from ..mask_head.mask_head import FPN_LEVEL_SCALES
        scales = tuple(k.POOLER_SCALES)
        if k.SHARE_BOX_FEATURE_EXTRACTOR:
            raise NotImplementedError("MODEL.KEYPOINT_ON True on MODEL.BACKBONE.CONV_BODY {!r} with MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR = "
                                      "{!r}: the FPN box extractor ends in the MLP head's [N, MLP_HEAD_DIM] rows, which no keypoint predictor can read; "
                                      "an FPN body runs the keypoint head on its own pyramid pooler: set SHARE_BOX_FEATURE_EXTRACTOR to False and "
                                      "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES to the body's {!r} (upstream's keypoint configs do)".format(
                                          body, k.SHARE_BOX_FEATURE_EXTRACTOR, FPN_LEVEL_SCALES))
        if not scales or scales != FPN_LEVEL_SCALES[:len(scales)]:
            raise NotImplementedError("MODEL.KEYPOINT_ON True on MODEL.BACKBONE.CONV_BODY {!r} with MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES = {!r}: the "
                                      "keypoint pooler reads the leading maps of the pyramid, at most the four of P2..P5: set POOLER_SCALES to a "
                                      "prefix of {!r}".format(body, scales, FPN_LEVEL_SCALES))
    elif k.SHARE_BOX_FEATURE_EXTRACTOR:
        unsupported("SHARE_BOX_FEATURE_EXTRACTOR", k.SHARE_BOX_FEATURE_EXTRACTOR,
                    "on a C4 body the box extractor's output is layer4's [N,2048,7,7], which the reference then pools as if it were a feature-map "
                    "list, for a predictor built for CONV_LAYERS[-1] channels: it cannot run; set it to False (upstream's keypoint configs do)")
    scales = tuple(k.POOLER_SCALES)
    want = tuple(cfg.MODEL.ROI_BOX_HEAD.POOLER_SCALES) if body_scale is None else (body_scale,)
    if not pyramid and (len(scales) != 1 or scales != want):
        unsupported("POOLER_SCALES", scales, "one pooler scale, the C4 body's {!r}, is run (no FPN level mapping)".format(want))
    layers = tuple(k.CONV_LAYERS)
    if not layers or any(c <= 0 or c % 4 for c in layers):
        unsupported("CONV_LAYERS", layers, "channel counts must be positive multiples of 4")
    if k.NUM_CLASSES < 1:
        unsupported("NUM_CLASSES", k.NUM_CLASSES, "at least one keypoint")
    if k.RESOLUTION != 4 * k.POOLER_RESOLUTION:
        raise ValueError("MODEL.ROI_KEYPOINT_HEAD.RESOLUTION = {} but the predictor's heat maps are {} x {} for POOLER_RESOLUTION = {} (the "
                         "deconvolution and the bilinear upsampling double it each): set RESOLUTION to {}".format(
                             k.RESOLUTION, 4 * k.POOLER_RESOLUTION, 4 * k.POOLER_RESOLUTION, k.POOLER_RESOLUTION, 4 * k.POOLER_RESOLUTION))
    if (4 * k.POOLER_RESOLUTION) ** 2 > 4096:
        unsupported("POOLER_RESOLUTION", k.POOLER_RESOLUTION, "the decode stages one heat map of at most 4096 values (64 x 64, a pooler of 16) in LDS; "
                    "the loss's low-resolution plane alone would fit up to 32")


# ------------------------------------------------------------------------------------------------ feature extractor
class _ExtractorFn(Function):
    """ROIAlign + n x relu(conv3x3 + bias) as one autograd node; the weight gradients go straight into the flat gradient buffer"""

    @staticmethod
    def forward(ctx, feat, ext, rois, *params):
        fh = as_nhwc(feat)
        acts, vs = ext._run(fh, rois, keep=True)
        ctx.ext, ctx.saved, ctx.rois, ctx.feat_shape = ext, (acts, vs), rois, tuple(fh.shape)
        ctx.need_dx = feat.requires_grad
        return from_nhwc(acts[-1])

    @staticmethod
    def backward(ctx, g):
        ext = ctx.ext
        acts, vs = ctx.saved
        gp = conv_stack_backward(ext.convs(), acts, vs, as_nhwc(g), ext.math, ctx.need_dx)
        gx = None
        if gp is not None:
            if ctx.rois is None:
                gx = from_nhwc(gp)
            else:
                B, H, W, C_ = ctx.feat_shape
                r = ext.resolution
                gx = from_nhwc(ops.roi_align_backward(gp, ctx.rois, ext.spatial_scale, r, r, ext.sampling_ratio, B, H, W, C_))
        ctx.saved = None
        return (gx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class KeypointRCNNFeatureExtractor(PyramidConvExtractor):
    """roi_keypoint_feature_extractors.py:11-43: one class, one set of names (conv_fcn1..n) on both kinds of body, as upstream, so a reference
    checkpoint loads key for key.  On an FPN body (`pyramid`) it IS roi_heads/pyramid_extractor.py's node over its own multi-scale pooler:
    forward(maps, proposals or a [K,5] table, rows=None).  On a C4 body it is the single-scale form below: forward([feature map], rois)."""

    def __init__(self, cfg, in_channels):
        k = cfg.MODEL.ROI_KEYPOINT_HEAD
        if in_channels % 4:
            raise NotImplementedError("the keypoint head's input has {} channels: channel counts must be multiples of 4".format(in_channels))
        if _on_pyramid(cfg):
            super().__init__(cfg, in_channels, "ROI_KEYPOINT_HEAD", "conv_fcn")
            self.pyramid = True
            return
        nn.Module.__init__(self)
        self.pyramid = False
        self.resolution, self.spatial_scale, self.sampling_ratio = k.POOLER_RESOLUTION, tuple(k.POOLER_SCALES)[0], k.POOLER_SAMPLING_RATIO
        self.math = ops.MATH_F32     # see backbone.resnet.set_conv_math
        # kaiming_normal_(mode="fan_out", nonlinearity="relu"), bias 0 (roi_keypoint_feature_extractors.py:31-32)
        self.blocks, self.out_channels = make_conv3x3_stack(self, in_channels, k.CONV_LAYERS, "conv_fcn")

    def _run(self, fh, rois, keep=False):
        """fh NHWC features, rois [P,5] (None: fh is the pooled tensor already) -> the activations [pooled, conv_fcn1's, ...] (keep) or just
        the last one"""
        r, x = self.resolution, fh
        if rois is not None:
            x = ops.roi_align_forward(fh, rois, self.spatial_scale, r, r, self.sampling_ratio)
            ops.amax_carry_bound(x, fh)      # pooled values are averages of bilinear samples: bounded by the feature map's amax (f16x3 scales)
        return conv_stack_forward(self.convs(), x, self.math, keep)

    def forward(self, features, rois, rows=None):
        """C4 form -- features: the backbone's list (one level); rois [P,5] (image index, xyxy) -> logical [P,C,r,r].  rois None: features[0]
        is the pooled tensor [P,C,r,r] itself (the conv stack alone, for parity tests).
        Pyramid form -- PyramidConvExtractor.forward(maps, proposals or a [K,5] table, rows)"""
        if self.pyramid:
            return super().forward(features, rois, rows)
        if rows is not None:
            raise RuntimeError("KeypointRCNNFeatureExtractor: rows index a RoI table for the pyramid pooler; the single-scale form takes the RoIs themselves")
        feat = features[0]
        if rois is not None and rois.shape[0] == 0:
            return feat.new_zeros((0, self.resolution, self.resolution, self.out_channels)).permute(0, 3, 1, 2)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (feat.requires_grad or any(p.requires_grad for p in params)):
            return _ExtractorFn.apply(feat, self, rois, *params)
        return from_nhwc(self._run(as_nhwc(feat), rois))


# ------------------------------------------------------------------------------------------------ predictor
class ConvTranspose4x4(Conv2d):
    """nn.ConvTranspose2d(Cin, K, 4, stride 2, padding 1) as the 1x1 conv (GEMM) whose 16 * Kp output columns are (ky, kx, k), Kp = K rounded
    up to a multiple of 4 (zero rows), followed by ops.kp_deconv_fold: the weight is held as that conv's OHWI [16 Kp, 1, 1, Cin], the bias
    as [Kp]; the checkpoint boundary sees [Cin, K, 4, 4] and [K]."""
    whole_only = True    # (rows of the stored tensor are not rows of this layout: utils/checkpoint.py never copies a leading part)

    def __init__(self, in_channels, num_keypoints):
        kp = ops.kp_pad(num_keypoints)
        super().__init__(in_channels, 16 * kp, 1, bias=False)
        self.kp, self.num_keypoints = kp, num_keypoints
        self.out_channels = num_keypoints     # (the checkpoint boundary stores bias[:out_channels])
        self.bias = nn.Parameter(torch.zeros(self.kp))

    def load_oihw(self, w):
        with torch.no_grad():
            self.weight.zero_()
            self.weight.view(4, 4, self.kp, self.in_channels)[:, :, :self.num_keypoints].copy_(w.permute(2, 3, 1, 0))
        self._wt_version = -1

    def ref_layout(self, t):
        return t.view(4, 4, self.kp, self.in_channels)[:, :, :self.num_keypoints].permute(3, 2, 0, 1)


class _TrainFn(Function):
    """loss_kp = cross-entropy(upsample2x(deconv4x4(x))) as one autograd node: GEMM, fold, and the fused upsampling + loss + gradient; the
    weight and bias gradients go straight into the flat gradient buffer"""

    @staticmethod
    def forward(ctx, x, pred, sel, *params):
        xh = as_nhwc(x)
        low = pred._lowres(xh)
        want = x.requires_grad or any(p.requires_grad for p in params)
        loss, grad, rows = ops.kp_loss(low, pred.num_keypoints, sel["targets"], sel["valid"], sel["n_valid"], want_grad=want)
        pred.last_lowres = low
        ctx.pred, ctx.saved, ctx.need_dx = pred, (xh, grad, rows), x.requires_grad
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        pred, c, math = ctx.pred, ctx.pred.kps_score_lowres, ctx.pred.math
        xh, grad, rows = ctx.saved
        g = g.contiguous()
        grad, rows = ops.scale_(grad, 1.0, g), ops.scale_(rows, 1.0, g)      # (this node's own buffers: scaled in place)
        gy = ops.kp_deconv_unfold(grad, pred.num_keypoints)
        if c.weight.requires_grad:
            ops.bias_grad(rows, _grad_buf(c.bias))
            ops.conv_wgrad_async(xh, gy, _grad_buf(c.weight), 1, 0, math=math)
        gx = from_nhwc(ops.conv_forward(gy, c.dgrad_weight(), 1, 0, math=math, w_version=c.version())) if ctx.need_dx else None
        ctx.saved = None
        return (gx, None, None) + (None,) * (len(ctx.needs_input_grad) - 3)


class KeypointRCNNPredictor(nn.Module):
    def __init__(self, cfg, in_channels):
        super().__init__()
        if in_channels % 4:
            raise NotImplementedError("MODEL.ROI_KEYPOINT_HEAD.CONV_LAYERS[-1] = {}: channel counts must be multiples of 4".format(in_channels))
        self.num_keypoints = cfg.MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES
        self.math = ops.MATH_F32     # see backbone.resnet.set_conv_math
        self.kps_score_lowres = ConvTranspose4x4(in_channels, self.num_keypoints)
        self.up_scale = 2
        self.last_lowres = None
        with torch.no_grad():        # roi_keypoint_predictors.py:22-25: kaiming_normal_(mode="fan_out") of a [Cin, K, 4, 4] weight, bias 0
            w = torch.zeros(in_channels, self.num_keypoints, 4, 4).normal_(0.0, (2.0 / (16 * in_channels)) ** 0.5)
            self.kps_score_lowres.load_oihw(w)

    def prep_entries(self):
        c = self.kps_score_lowres
        return [(c, None, 1, 0, self.math)] if c.weight.requires_grad and c.weight.is_cuda else []

    def _lowres(self, xh):
        """NHWC head features [P,h,w,C] -> planar low-resolution maps [P,Kp,2h,2w]"""
        c = self.kps_score_lowres
        if xh.shape[0] == 0:
            return xh.new_zeros((0, c.kp, 2 * xh.shape[1], 2 * xh.shape[2]))
        y = ops.conv_forward(xh, c.weight, 1, 0, math=self.math, w_version=c.version())
        return ops.kp_deconv_fold(y, c.bias[:self.num_keypoints])

    def forward(self, x):
        """-> the heat-map logits [P,K,4h,4w] (eval and introspection; training goes through loss())"""
        return ops.kp_upsample2x(self._lowres(as_nhwc(x)), self.num_keypoints)

    def loss(self, x, sel):
        return _TrainFn.apply(x, self, sel, *self.parameters())


# ------------------------------------------------------------------------------------------------ loss / post-processing
class KeypointRCNNLossComputation(object):
    def __init__(self, discretization_size, max_pos_per_image):
        self.discretization_size, self.max_pos_per_image = discretization_size, max_pos_per_image

    def select(self, proposals, targets, fused=None, gather=True):
        """the box head's sampled positives whose matched instance has a visible keypoint inside its box (loss.py:79-143) and their heat-map
        targets (loss.py:145-157), on the device: ops.kp_select_targets' dict + table [R,5], the sampled set's RoI table pos_rows indexes, and,
        with `gather` (the single-scale pooler), rois [P_max,5], the kept rows' RoIs"""
        if fused is not None:      # ops.roi_head_targets' output: the batch's RoI table and labels are single tensors already
            labels, rois = fused["labels"], fused["rois"]
        else:
            labels = torch.cat([p.get_field("labels") for p in proposals])
            dev = labels.device
            rois = torch.cat([torch.cat((torch.full((len(p), 1), float(i), device=dev), p.convert("xyxy").bbox), 1) for i, p in enumerate(proposals)])
        kps = []
        for p, t in zip(proposals, targets):
            kp = t.get_field("keypoints")
            if tuple(kp.size) != tuple(p.size):
                raise AssertionError("{}, {}".format(kp, p))
            kps.append(kp.keypoints)
        p_max = max(1, min(labels.numel(), self.max_pos_per_image * len(proposals)))
        sel = ops.kp_select_targets(rois, labels, [t.convert("xyxy").bbox for t in targets], kps, self.discretization_size, p_max)
        sel["table"] = rois
        if gather:
            wide = torch.zeros((rois.shape[0], 8), dtype=rois.dtype, device=rois.device)      # (row gather moves 16-byte pieces)
            wide[:, :5] = rois
            sel["rois"] = ops.mask_gather_rows(wide, sel["pos_rows"])[:, :5].contiguous()
        return sel


class KeypointPostProcessor(nn.Module):
    """inference.py:5-32 with the Keypointer (heatmaps_to_keypoints) on the device, for any number of images"""

    def forward(self, x, boxes):
        """x: the heat-map logits [D,K,M,M]; boxes: the detections per image -> BoxLists with a "keypoints" field (PersonKeypoints [n,K,3]
        carrying "logits" [n,K])"""
        D, K = x.shape[0], x.shape[1]
        if D:
            xy, logits = ops.kp_decode(x, torch.cat([b.convert("xyxy").bbox for b in boxes]))
        else:
            xy, logits = x.new_zeros((0, K, 3)), x.new_zeros((0, K))
        results, off = [], 0
        for b in boxes:
            n = len(b)
            r = BoxList(b.bbox, b.size, mode="xyxy")
            for f in b.fields():
                r.add_field(f, b.get_field(f))
            kp = PersonKeypoints(xy[off:off + n], b.size)
            kp.add_field("logits", logits[off:off + n])
            r.add_field("keypoints", kp)
            results.append(r)
            off += n
        return results


class ROIKeypointHead(nn.Module):
    def __init__(self, cfg, in_channels):
        super().__init__()
        check_keypoint_head_cfg(cfg)
        self.feature_extractor = KeypointRCNNFeatureExtractor(cfg, in_channels)
        self.predictor = KeypointRCNNPredictor(cfg, self.feature_extractor.out_channels)
        self.post_processor = KeypointPostProcessor()
        rh = cfg.MODEL.ROI_HEADS
        self.loss_evaluator = KeypointRCNNLossComputation(cfg.MODEL.ROI_KEYPOINT_HEAD.RESOLUTION, int(rh.BATCH_SIZE_PER_IMAGE * rh.POSITIVE_FRACTION))
        self.last_selection = None

    @property
    def last_kp_logits(self):
        """the last training pass's heat-map logits [P_max,K,M,M], upsampled on demand (introspection for parity tests: training itself never
        forms them)"""
        low = self.predictor.last_lowres
        return None if low is None else ops.kp_upsample2x(low, self.predictor.num_keypoints)

    def forward(self, features, proposals, targets=None, fused=None):
        """training: `features` = the backbone's, `proposals` = the box head's sampled set (with "labels") -> (x, proposals, {loss_kp});
        eval: `proposals` = the detections -> (x, detections with "keypoints", {})  (keypoint_head.py:20-49)"""
        pyramid = self.feature_extractor.pyramid
        if self.training:
            with torch.no_grad():
                sel = self.loss_evaluator.select(proposals, targets, fused=fused, gather=not pyramid)
            if pyramid:      # the kept positives are pooled as rows of the sampled set's table: nothing is gathered, nothing read back
                x = self.feature_extractor(features, sel["table"], rows=sel["pos_rows"])
            else:
                x = self.feature_extractor(features, sel["rois"])
            self.last_selection = sel
            return x, proposals, dict(loss_kp=self.predictor.loss(x, sel))
        K, side = self.predictor.num_keypoints, self.loss_evaluator.discretization_size
        if sum(len(p) for p in proposals) == 0:
            return None, self.post_processor(features[0].new_zeros((0, K, side, side)), proposals), {}
        if pyramid:
            x = self.feature_extractor(features, proposals)
            return x, self.post_processor(self.predictor(x), proposals), {}
        x = self.feature_extractor(features, convert_to_roi_format([p.convert("xyxy") for p in proposals]))
        return x, self.post_processor(self.predictor(x), proposals), {}


def build_roi_keypoint_head(cfg, in_channels):
    return ROIKeypointHead(cfg, in_channels)

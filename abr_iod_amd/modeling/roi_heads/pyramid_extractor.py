"""Pyramid pooler + n x relu(conv3x3 + bias) as ONE autograd node: the feature extractor the FPN mask head (MaskRCNNFPNFeatureExtractor,
mask_head/fpn_mask_head.py) and the FPN keypoint head (the pyramid form of KeypointRCNNFeatureExtractor, keypoint_head/keypoint_head.py)
share.  The two differ in the config section they read and in the names of their convs (mask_fcn1..n, conv_fcn1..n): nothing else.

The pooler is the one-launch pyramid ROIAlign (modeling/poolers.py), the stack the loop of roi_heads/conv_stack.py; the node's backward ends in
the indexed pyramid backward, which hands every level's map its gradient.  With `rows` only those rows of the RoI table are pooled
(ops.roi_align_pyramid_forward(rows=)): an entry < 0 is padding -- zero features in, relu(bias) features out; it never reads the table and
sends no gradient to any map."""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from ... import ops
from ...layers._layout import as_nhwc, from_nhwc
from ..backbone.resnet import Conv2d
from ..poolers import make_pooler
from .conv_stack import conv_stack_backward, conv_stack_forward


class _PyramidExtractorFn(Function):
    """(extractor, rois [K,5], rows int64 [P] or None, n_maps, *maps logical [B,C,H_l,W_l], *parameters) -> logical [P or K, width, r, r]"""

    @staticmethod
    def forward(ctx, ext, rois, rows, n_maps, *args):
        xs = [as_nhwc(f) for f in args[:n_maps]]
        acts, vs = conv_stack_forward(ext.convs(), ext._pool(xs, rois, rows), ext.math, keep=True)
        ctx.ext, ctx.saved, ctx.table, ctx.n_maps = ext, (acts, vs), (rois, rows), n_maps
        ctx.shapes = [tuple(x.shape) for x in xs]
        return from_nhwc(acts[-1])

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        ext = ctx.ext
        acts, vs = ctx.saved
        ctx.saved = None
        need_dx = any(ctx.needs_input_grad[4:4 + ctx.n_maps])
        gp = conv_stack_backward(ext.convs(), acts, vs, as_nhwc(g), ext.math, need_dx)
        gmaps = (None,) * ctx.n_maps
        if gp is not None:
            rois, rows = ctx.table
            (ph, pw), scales, sr, rule = ext.pooler.geometry()
            gmaps = tuple(from_nhwc(t) for t in ops.roi_align_pyramid_backward(gp, rois, scales, ph, pw, sr, ctx.shapes, *rule, rows=rows))
        return (None, None, None, None) + gmaps + (None,) * (len(ctx.needs_input_grad) - 4 - ctx.n_maps)


def make_conv3x3_stack(module, in_channels, layers, prefix):
    """registers prefix1..n = Conv2d 3x3 (pad 1) on `module`, initialised as the reference's make_conv3x3 (modeling/make_layers.py:47-77:
    kaiming_normal_(mode="fan_out", nonlinearity="relu"), bias 0) -> (the names, the last width)"""
    blocks, c = [], in_channels
    for i, width in enumerate(layers, 1):
        name = "{}{}".format(prefix, i)
        conv = Conv2d(c, width, 3, stride=1, padding=1)
        with torch.no_grad():
            conv.weight.normal_(0.0, (2.0 / (9 * width)) ** 0.5)
        module.add_module(name, conv)
        blocks.append(name)
        c = width
    return blocks, c


class PyramidConvExtractor(nn.Module):
    """section: the MODEL.<section> node holding POOLER_RESOLUTION / POOLER_SCALES / POOLER_SAMPLING_RATIO / CONV_LAYERS; prefix: the convs'
    name.  forward -> logical [P,CONV_LAYERS[-1],r,r]"""

    def __init__(self, cfg, in_channels, section, prefix):
        super().__init__()
        m = cfg.MODEL[section]
        if in_channels % 4:
            raise NotImplementedError("{}: {} input channels, need a multiple of 4".format(type(self).__name__, in_channels))
        self.section = section
        self.pooler = make_pooler(cfg, section)
        self.n_levels = len(m.POOLER_SCALES)
        self.resolution, self.in_channels = m.POOLER_RESOLUTION, in_channels
        self.math = ops.MATH_F32     # see backbone.resnet.set_conv_math
        self.blocks, self.out_channels = make_conv3x3_stack(self, in_channels, m.CONV_LAYERS, prefix)

    def convs(self):
        return [getattr(self, n) for n in self.blocks]

    def prep_entries(self):
        """FusedSGD's batched weight preparation (see Bottleneck.prep_entries)"""
        return [(c, None, 1, 1, self.math) for c in self.convs() if c.weight.requires_grad and c.weight.is_cuda]

    def _pool(self, xs, rois, rows):
        """NHWC maps -> NHWC [P or K, r, r, C], tagged with the levels' amax bound (a subset of the table's rows and zeros keep it)"""
        (ph, pw), scales, sr, rule = self.pooler.geometry()
        out = ops.roi_align_pyramid_forward(xs, rois, scales, ph, pw, sr, *rule, rows=rows)
        return ops.amax_bound_levels(out, xs)

    def forward(self, x, proposals, rows=None):
        """x: the pyramid's maps, logical [B,C,H_l,W_l] -- the first len(POOLER_SCALES) are pooled (P6 is the RPN's alone: the reference's
        zip drops it); proposals: list of BoxLists or a ready [K,5] RoI table; rows: int64 [P] device list of rows of that table (entries < 0
        are padding: zero features in, relu(bias) features out, no gradient to the maps)"""
        x = list(x)
        if len(x) < self.n_levels:
            raise RuntimeError("{}: {} feature maps for {} MODEL.{}.POOLER_SCALES".format(type(self).__name__, len(x), self.n_levels, self.section))
        x = x[: self.n_levels]
        rois = proposals if torch.is_tensor(proposals) else self.pooler.convert_to_roi_format(proposals)
        n = rois.shape[0] if rows is None else rows.shape[0]
        r = self.resolution
        if n == 0:
            return rois.new_zeros((0, r, r, self.out_channels)).permute(0, 3, 1, 2)
        params = list(self.parameters())
        if torch.is_grad_enabled() and (any(f.requires_grad for f in x) or any(p.requires_grad for p in params)):
            return _PyramidExtractorFn.apply(self, rois, rows, len(x), *x, *params)
        return from_nhwc(conv_stack_forward(self.convs(), self._pool([as_nhwc(f) for f in x], rois, rows), self.math))

"""The feature pyramid network neck on the HIP library (mirror of maskrcnn_benchmark/modeling/backbone/fpn.py).

    FPN (:7-74)                the reference's class called on a list of maps C2..C5: per level a 1x1 lateral conv `fpn_inner{i}` and a 3x3
                               output conv `fpn_layer{i}`, the top-down pathway between them, `top_blocks` on the coarsest result
    LastLevelMaxPool (:77-79)  P6 = F.max_pool2d(P5, 1, 2, 0)
The conv block is conv_with_kaiming_uniform(use_gn=False, use_relu=False) (make_layers.py:92-122): a conv with bias, kaiming_uniform_(a=1)
weight and zero bias.  Module and parameter NAMES are the reference's (state-dict keys match; the weights are OHWI, converted at the checkpoint
boundary like every resnet.Conv2d).  LastLevelP6P7 (RetinaNet), GroupNorm and ReLU inside the block are not built.

Execution model: the whole neck is ONE autograd node (_FPNFn, in the manner of resnet._StageFn).  Forward: L lateral convs, ONE top-down launch
(ops.fpn_topdown_forward: bit-equal to the level-by-level lateral + F.interpolate), L output convs, one subsample launch.  Backward is
hand-scheduled: per level the 3x3's bias gradient, weight gradient (side stream) and input gradient; ONE top-down backward launch written over
those input gradients; per level the 1x1's bias gradient, weight gradient and input gradient.  Parameter gradients are accumulated straight
into p.grad (views of the flat gradient buffer).  A level whose output received no gradient costs nothing.
"""
import torch
from torch import nn
from torch.autograd import Function

from ... import ops
from ...layers._layout import as_nhwc, from_nhwc
from .resnet import Conv2d, _grad_buf


class LastLevelMaxPool(nn.Module):
    """fpn.py:77-79: a stride-2 subsample of the coarsest result (a 1x1 max-pool window holds one pixel)"""

    def forward(self, x):
        return [from_nhwc(ops.fpn_subsample2(as_nhwc(x)))]


class _FPNFn(Function):
    """FPN.forward as one autograd node: (fpn, n maps, *maps, *parameters) -> the results, finest first, plus the top block's"""

    @staticmethod
    def forward(ctx, fpn, n, *args):
        ctx.set_materialize_grads(False)
        xs = [as_nhwc(x) for x in args[:n]]
        laterals, inners, results = fpn._run(xs)
        ctx.fpn, ctx.xs, ctx.inners = fpn, xs, inners
        ctx.n_args = len(args)
        return tuple(from_nhwc(r) for r in results)

    @staticmethod
    def backward(ctx, *gouts):
        fpn, xs, inners = ctx.fpn, ctx.xs, ctx.inners
        ctx.xs = ctx.inners = None
        L = len(xs)
        m = fpn.math
        gP = [as_nhwc(g) if g is not None else None for g in gouts[:L]]
        if fpn.has_top and len(gouts) > L and gouts[L] is not None:   # P6 = P5's even pixels: its gradient joins P5's
            gP[L - 1] = ops.fpn_subsample2_backward(as_nhwc(gouts[L]), inners[L - 1].shape, gP[L - 1])
        # the 3x3 output convs: gradient of inner_l as far as P_l alone reaches it
        g_inner = [None] * L
        need_lat = [fpn._inner(l).weight.requires_grad or ctx.needs_input_grad[2 + l] for l in range(L)]
        for l in range(L):
            g = gP[l]
            if g is None:
                continue
            conv = fpn._layer(l)
            if conv.weight.requires_grad:
                ops.bias_grad(g, _grad_buf(conv.bias))
            # inner_l reaches lateral l and, through the top-down adds, every coarser one
            need_dx = any(need_lat[l:])
            if conv.weight.requires_grad:
                g_inner[l] = ops.conv_backward(inners[l], g, _grad_buf(conv.weight), conv.dgrad_weight(None) if need_dx else None, 1, 1, math=m,
                                               w_version=conv.version(), dgrad=need_dx)
            elif need_dx:
                g_inner[l] = ops.conv_forward(g, conv.dgrad_weight(None), 1, 1, math=m, w_version=conv.version())
        gx = [None] * L
        lo = next((l for l in range(L) if g_inner[l] is not None), None)
        if lo is not None:
            # the top-down pathway's adjoint from the finest level that has a gradient, in one launch, over the dgrad results
            d_lat = [None] * lo + ops.fpn_topdown_backward(g_inner[lo:], inplace=True)
            for l in range(lo, L):
                if not need_lat[l]:
                    continue
                conv, g = fpn._inner(l), d_lat[l]
                need_dx = bool(ctx.needs_input_grad[2 + l])
                if conv.weight.requires_grad:
                    ops.bias_grad(g, _grad_buf(conv.bias))
                    gx[l] = ops.conv_backward(xs[l], g, _grad_buf(conv.weight), conv.dgrad_weight(None) if need_dx else None, 1, 0, math=m,
                                              w_version=conv.version(), dgrad=need_dx)
                elif need_dx:
                    gx[l] = ops.conv_forward(g, conv.dgrad_weight(None), 1, 0, math=m, w_version=conv.version())
        return (None, None) + tuple(from_nhwc(g) if g is not None else None for g in gx) + (None,) * (ctx.n_args - L)


class FPN(nn.Module):
    """Adds an FPN on top of a list of feature maps, in increasing depth order and consecutive (fpn.py:7-74).  in_channels_list: the channels
    of every map fed (an entry 0 is skipped: no blocks for that level, as in the reference); out_channels: of the FPN representation;
    top_blocks: None or LastLevelMaxPool, applied to the coarsest result and appended."""

    def __init__(self, in_channels_list, out_channels, top_blocks=None):
        super().__init__()
        if top_blocks is not None and not isinstance(top_blocks, LastLevelMaxPool):
            raise NotImplementedError("FPN top_blocks {}: only LastLevelMaxPool is built (no LastLevelP6P7 / RetinaNet)".format(type(top_blocks).__name__))
        if out_channels % 4:
            raise NotImplementedError("FPN out_channels = {}: the top-down kernels move 4 channels per lane".format(out_channels))
        self.inner_blocks, self.layer_blocks = [], []
        for idx, in_channels in enumerate(in_channels_list, 1):
            inner_block, layer_block = "fpn_inner{}".format(idx), "fpn_layer{}".format(idx)
            if in_channels == 0:
                continue
            inner = Conv2d(in_channels, out_channels, 1, stride=1, padding=0, bias=True)
            layer = Conv2d(out_channels, out_channels, 3, stride=1, padding=1, bias=True)
            for conv in (inner, layer):   # conv_with_kaiming_uniform: kaiming_uniform_(a=1), bias 0
                conv.kaiming_uniform_(a=1)
            self.add_module(inner_block, inner)
            self.add_module(layer_block, layer)
            self.inner_blocks.append(inner_block)
            self.layer_blocks.append(layer_block)
        self.top_blocks = top_blocks
        self.has_top = top_blocks is not None
        self.math = ops.MATH_F32   # the convs' contraction arithmetic (resnet.set_conv_math)

    def _inner(self, l):
        return getattr(self, self.inner_blocks[l])

    def _layer(self, l):
        return getattr(self, self.layer_blocks[l])

    def _convs(self):
        return [getattr(self, n) for pair in zip(self.inner_blocks, self.layer_blocks) for n in pair]

    def _param_list(self):
        """the neck's parameters in module order (kept: the parameter OBJECTS never change, see resnet._stage_params)"""
        cached = self.__dict__.get("_params_cache")
        convs = self._convs()
        if cached is None or not all(c.weight is w for c, w in cached[1]):
            cached = self.__dict__["_params_cache"] = ([p for c in convs for p in (c.weight, c.bias)], [(c, c.weight) for c in convs])
        return cached[0]

    def _trains(self):
        return any(p.requires_grad for p in self._param_list())

    def prep_entries(self):
        """(conv, scale, stride, pad, math) of the trainable convs: FusedSGD.step rebuilds their dgrad copies and what the library derives
        from the weights right after the update (resnet.Bottleneck.prep_entries)"""
        return [(c, None, c.stride, c.padding, self.math) for c in self._convs() if c.weight.requires_grad and c.weight.is_cuda]

    def _conv(self, x, conv):
        return ops.conv_forward(x, conv.weight, conv.stride, conv.padding, bias=conv.bias, math=self.math, w_version=conv.version())

    def _run(self, xs):
        """xs: NHWC maps -> (laterals, inners, results incl. the top block's), NHWC"""
        laterals = [self._conv(x, self._inner(l)) for l, x in enumerate(xs)]
        inners = ops.fpn_topdown_forward(laterals)
        results = [self._conv(t, self._layer(l)) for l, t in enumerate(inners)]
        if self.has_top:
            results.append(ops.fpn_subsample2(results[-1]))
        return laterals, inners, results

    def forward(self, x):
        """x: list of logical [B,C_l,H_l,W_l] maps, one per built level, each exactly twice the next -> tuple of results, highest resolution first"""
        x = list(x)
        if len(x) < len(self.inner_blocks):
            raise ValueError("FPN: {} feature maps for {} levels".format(len(x), len(self.inner_blocks)))
        x = x[len(x) - len(self.inner_blocks):]   # (a skipped level's map is passed and not read: the reference zips from the coarsest end)
        if torch.is_grad_enabled() and (self._trains() or any(t.requires_grad for t in x)):
            return _FPNFn.apply(self, len(x), *x, *self._param_list())
        return tuple(from_nhwc(r) for r in self._run([as_nhwc(t) for t in x])[2])

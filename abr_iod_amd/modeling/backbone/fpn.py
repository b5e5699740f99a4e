"""The feature pyramid network neck on the HIP library (mirror of maskrcnn_benchmark/modeling/backbone/fpn.py).

    FPN (:7-74)                the reference's class called on a list of maps C2..C5: per level a 1x1 lateral conv `fpn_inner{i}` and a 3x3
                               output conv `fpn_layer{i}`, the top-down pathway between them, `top_blocks` on the coarsest result
    LastLevelMaxPool (:77-79)  P6 = F.max_pool2d(P5, 1, 2, 0)
    LastLevelP6P7 (:82-99)     RetinaNet's top block: P6 = p6(C5, or P5 when the channel counts agree), P7 = p7(relu(P6)), 3x3 stride-2 convs
The conv block is conv_with_kaiming_uniform(use_gn=False, use_relu=False) (make_layers.py:92-122): a conv with bias, kaiming_uniform_(a=1)
weight and zero bias.  Module and parameter NAMES are the reference's (state-dict keys match; the weights are OHWI, converted at the checkpoint
boundary like every resnet.Conv2d).  GroupNorm and ReLU inside the block are not built.

Execution model: the whole neck is ONE autograd node (_FPNFn, in the manner of resnet._StageFn).  Forward: L lateral convs, ONE top-down launch
(ops.fpn_topdown_forward: bit-equal to the level-by-level lateral + F.interpolate), L output convs, one subsample launch.  Backward is
hand-scheduled: per level the 3x3's bias gradient, weight gradient (side stream) and input gradient; ONE top-down backward launch written over
those input gradients; per level the 1x1's bias gradient, weight gradient and input gradient.  Parameter gradients are accumulated straight
into p.grad (views of the flat gradient buffer).  A level whose output received no gradient costs nothing; neither does P6 or P7.
With LastLevelP6P7 the node also carries the gradients of P7 and P6 back through p7, the ReLU mask and p6, into C5's gradient or into P5's.
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


class LastLevelP6P7(nn.Module):
    """fpn.py:82-99: P6 and P7 of RetinaNet.  p6 reads C5, or P5 when in_channels == out_channels (`use_P5`); p7 reads relu(P6), which is
    not an output.  Both are 3x3, stride 2, pad 1 convs with bias, kaiming_uniform_(a=1) weights and zero bias."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        if in_channels % 4 or out_channels % 4:
            raise NotImplementedError("LastLevelP6P7: {} -> {} channels, need multiples of 4".format(in_channels, out_channels))
        self.p6 = Conv2d(in_channels, out_channels, 3, stride=2, padding=1)
        self.p7 = Conv2d(out_channels, out_channels, 3, stride=2, padding=1)
        for conv in (self.p6, self.p7):
            conv.kaiming_uniform_(a=1)
        self.use_P5 = in_channels == out_channels
        self.math = ops.MATH_F32   # the convs' contraction arithmetic (resnet.set_conv_math; inside an FPN the neck's own)

    def run(self, x, math):
        """x NHWC (C5 or P5) -> (P6, relu(P6), P7), NHWC"""
        p6 = ops.conv_forward(x, self.p6.weight, 2, 1, bias=self.p6.bias, math=math, w_version=self.p6.version())
        r6 = ops.relu_backward(p6, p6)   # P6 * (P6 > 0): the ReLU as its own tensor, P6 itself stays an output
        p7 = ops.conv_forward(r6, self.p7.weight, 2, 1, bias=self.p7.bias, math=math, w_version=self.p7.version())
        return p6, r6, p7

    def forward(self, c5, p5):
        p6, _, p7 = self.run(as_nhwc(p5 if self.use_P5 else c5), self.math)
        return [from_nhwc(p6), from_nhwc(p7)]


def _stride2_backward(conv, x, g, need_dx, math):
    """a 3x3 stride-2 pad-1 conv's bias, weight and (need_dx) input gradient from its output gradient g; x: its NHWC input.  The input gradient
    is the stride-1 pad-1 conv of g spread over the even pixels of a zero map of x's size with the flipped weight: out(o) reads x(2o - 1 + r),
    so x(i) collects w(r) g((i + 1 - r) / 2) where that is a pixel."""
    dx = None
    if conv.weight.requires_grad:
        ops.bias_grad(g, _grad_buf(conv.bias))
        ops.conv_backward(x, g, _grad_buf(conv.weight), None, 2, 1, math=math, w_version=conv.version(), dgrad=False)
    if need_dx:
        spread = ops.fpn_subsample2_backward(g, x.shape[:3] + (g.shape[3],))
        dx = ops.conv_forward(spread, conv.dgrad_weight(None), 1, 1, math=math, w_version=conv.version())
    return dx


class _FPNFn(Function):
    """FPN.forward as one autograd node: (fpn, n maps, *maps, *parameters) -> the results, finest first, plus the top block's"""

    @staticmethod
    def forward(ctx, fpn, n, *args):
        ctx.set_materialize_grads(False)
        xs = [as_nhwc(x) for x in args[:n]]
        laterals, inners, results = fpn._run(xs, keep_top=True)
        ctx.fpn, ctx.xs, ctx.inners = fpn, xs, inners
        ctx.top = fpn.__dict__.pop("_top_saved", None)   # LastLevelP6P7: (its input, P6, relu(P6))
        ctx.n_args = len(args)
        return tuple(from_nhwc(r) for r in results)

    @staticmethod
    def backward(ctx, *gouts):
        fpn, xs, inners = ctx.fpn, ctx.xs, ctx.inners
        top_saved, ctx.top = ctx.top, None
        ctx.xs = ctx.inners = None
        L = len(xs)
        m = fpn.math
        gP = [as_nhwc(g) if g is not None else None for g in gouts[:L]]
        g_c5 = None          # LastLevelP6P7 on C5: what P6 and P7 send to the coarsest input map
        if fpn.p6p7:
            top, (tx, p6, r6) = fpn.top_blocks, top_saved
            g6 = as_nhwc(gouts[L]) if gouts[L] is not None else None
            g7 = as_nhwc(gouts[L + 1]) if gouts[L + 1] is not None else None
            need_lat = [fpn._inner(l).weight.requires_grad or ctx.needs_input_grad[2 + l] for l in range(L)]
            # the top block's input gradient is wanted where something below it can use it: C5 itself, or P5's conv and everything under it
            below = (any(need_lat) or fpn._layer(L - 1).weight.requires_grad) if top.use_P5 else bool(ctx.needs_input_grad[2 + L - 1])
            if g7 is not None:
                g_r6 = _stride2_backward(top.p7, r6, g7, top.p6.weight.requires_grad or below, m)
                if g_r6 is not None:   # through the ReLU mask, joining P6's own gradient
                    g_r6 = ops.relu_backward(g_r6, p6, inplace=True)
                    g6 = g_r6 if g6 is None else ops.add_(g_r6, g6 if g6.is_contiguous() else g6.contiguous())
            if g6 is not None:
                g_top = _stride2_backward(top.p6, tx, g6, below, m)
                if g_top is not None:
                    if top.use_P5:
                        gP[L - 1] = g_top if gP[L - 1] is None else ops.add_(g_top, gP[L - 1] if gP[L - 1].is_contiguous() else gP[L - 1].contiguous())
                    else:
                        g_c5 = g_top
        elif fpn.has_top and len(gouts) > L and gouts[L] is not None:   # P6 = P5's even pixels: its gradient joins P5's
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
        if g_c5 is not None:
            gx[L - 1] = g_c5 if gx[L - 1] is None else ops.add_(g_c5, gx[L - 1])
        return (None, None) + tuple(from_nhwc(g) if g is not None else None for g in gx) + (None,) * (ctx.n_args - L)


class FPN(nn.Module):
    """Adds an FPN on top of a list of feature maps, in increasing depth order and consecutive (fpn.py:7-74).  in_channels_list: the channels
    of every map fed (an entry 0 is skipped: no blocks for that level, as in the reference); out_channels: of the FPN representation;
    top_blocks: None, LastLevelMaxPool (applied to the coarsest result) or LastLevelP6P7 (to the coarsest input map or result); appended."""

    def __init__(self, in_channels_list, out_channels, top_blocks=None):
        super().__init__()
        if top_blocks is not None and not isinstance(top_blocks, (LastLevelMaxPool, LastLevelP6P7)):
            raise NotImplementedError("FPN top_blocks {}: only LastLevelMaxPool and LastLevelP6P7 are built".format(type(top_blocks).__name__))
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
        self.p6p7 = isinstance(top_blocks, LastLevelP6P7)
        self.math = ops.MATH_F32   # the convs' contraction arithmetic (resnet.set_conv_math)

    def _inner(self, l):
        return getattr(self, self.inner_blocks[l])

    def _layer(self, l):
        return getattr(self, self.layer_blocks[l])

    def _convs(self):
        top = [self.top_blocks.p6, self.top_blocks.p7] if self.p6p7 else []
        return [getattr(self, n) for pair in zip(self.inner_blocks, self.layer_blocks) for n in pair] + top

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

    def _run(self, xs, keep_top=False):
        """xs: NHWC maps -> (laterals, inners, results incl. the top block's), NHWC; keep_top: LastLevelP6P7's (input, P6, relu(P6)) are left
        in _top_saved for the autograd node"""
        laterals = [self._conv(x, self._inner(l)) for l, x in enumerate(xs)]
        inners = ops.fpn_topdown_forward(laterals)
        results = [self._conv(t, self._layer(l)) for l, t in enumerate(inners)]
        if self.p6p7:
            tx = results[-1] if self.top_blocks.use_P5 else xs[-1]
            p6, r6, p7 = self.top_blocks.run(tx, self.math)
            if keep_top:
                self.__dict__["_top_saved"] = (tx, p6, r6)
            results += [p6, p7]
        elif self.has_top:
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

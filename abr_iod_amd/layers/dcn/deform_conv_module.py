"""Mirror of maskrcnn_benchmark/layers/dcn/deform_conv_module.py: DeformConv, ModulatedDeformConv, ModulatedDeformConvPack with the
reference's parameter names, OIHW shapes, reset_parameters bounds and __repr__.

A weight is a Parameter of the reference's logical shape [Cout, Cin/groups, kh, kw] over channels-last memory (the OHWI bytes the kernels
read, like an activation's logical NCHW over NHWC): state_dict() and load_state_dict() see OIHW, the kernels a view."""
import math

import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from ... import ops
from ..._lib import require_cuda
from .._layout import as_nhwc, from_nhwc
from .deform_conv_func import deform_conv, modulated_deform_conv


def _oihw_parameter(cout, cin, kh, kw):
    return nn.Parameter(torch.zeros(cout, kh, kw, cin).permute(0, 3, 1, 2))


def _uniform_by_fan_in(module):
    """reset_parameters of deform_conv_module.py:49-54 / :112-119: U(-1/sqrt(n), 1/sqrt(n)), n = in_channels * kh * kw"""
    n = module.in_channels
    for k in module.kernel_size:
        n *= k
    stdv = 1. / math.sqrt(n)
    module.weight.data.uniform_(-stdv, stdv)


def _repr(module):
    return "".join([
        "{}(".format(module.__class__.__name__),
        "in_channels={}, ".format(module.in_channels),
        "out_channels={}, ".format(module.out_channels),
        "kernel_size={}, ".format(module.kernel_size),
        "stride={}, ".format(module.stride),
        "dilation={}, ".format(module.dilation),
        "padding={}, ".format(module.padding),
        "groups={}, ".format(module.groups),
        "deformable_groups={}, ".format(module.deformable_groups),
        "bias={})".format(module.with_bias),
    ])


class DeformConv(nn.Module):
    """deform_conv_module.py:10-73"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=False):
        assert not bias
        super(DeformConv, self).__init__()
        self.with_bias = bias
        assert in_channels % groups == 0, 'in_channels {} cannot be divisible by groups {}'.format(in_channels, groups)
        assert out_channels % groups == 0, 'out_channels {} cannot be divisible by groups {}'.format(out_channels, groups)
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = _pair(stride)
        self.padding = _pair(padding)
        self.dilation = _pair(dilation)
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.weight = _oihw_parameter(out_channels, in_channels // self.groups, *self.kernel_size)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_by_fan_in(self)

    def forward(self, input, offset):
        return deform_conv(input, offset, self.weight, self.stride, self.padding, self.dilation, self.groups, self.deformable_groups)

    def __repr__(self):
        return _repr(self)


class ModulatedDeformConv(nn.Module):
    """deform_conv_module.py:76-138 (stride, padding and dilation are kept as given, as there)"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=True):
        super(ModulatedDeformConv, self).__init__()
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.kernel_size = _pair(kernel_size)
        self.stride = stride
        self.padding = padding
        self.dilation = dilation
        self.groups = groups
        self.deformable_groups = deformable_groups
        self.with_bias = bias
        self.weight = _oihw_parameter(out_channels, in_channels // groups, *self.kernel_size)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        _uniform_by_fan_in(self)
        if self.bias is not None:
            self.bias.data.zero_()

    def forward(self, input, offset, mask):
        return modulated_deform_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)

    def __repr__(self):
        return _repr(self)


class _Conv2dFunction(Function):
    """A plain convolution with bias through the library's conv entry points, for the offset convs that feed the deformable ones: forward
    ops.conv_forward; weight gradient ops.conv_wgrad; bias gradient ops.bias_grad; input gradient the stride-1 convolution of the output
    gradient -- spread over a zeroed [B, H + kh - 1, W + kw - 1] map at the conv's stride, which is both its zero insertion and its
    padding -- with the flipped weights.  An output width that is no multiple of 4 is padded with zero rows (27 -> 28)."""

    @staticmethod
    def forward(ctx, input, weight, bias, stride, padding):
        require_cuda(input, weight, bias)
        x, w = as_nhwc(input.detach()), as_nhwc(weight.detach())
        cout, kh, kw, cin = w.shape
        if padding > min(kh, kw) - 1:
            raise NotImplementedError("Conv2d: padding {} exceeds kernel - 1 = {}".format(padding, min(kh, kw) - 1))
        cop = (cout + 3) // 4 * 4
        b = None if bias is None else bias.detach()
        if cop != cout:
            wp = w.new_zeros((cop, kh, kw, cin))
            wp[:cout].copy_(w)
            w = wp
            if b is not None:
                bp = b.new_zeros((cop,))
                bp[:cout].copy_(b)
                b = bp
        ctx.math = ops.default_conv_math()
        y = ops.conv_forward(x, w, stride, padding, bias=b, math=ctx.math)
        ctx.save_for_backward(x, w)
        ctx.cout, ctx.stride, ctx.padding, ctx.with_bias = cout, stride, padding, bias is not None
        return from_nhwc(y if cop == cout else y[..., :cout].contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, w = ctx.saved_tensors
        cop, kh, kw, cin = w.shape
        cout, s, p = ctx.cout, ctx.stride, ctx.padding
        gy = as_nhwc(grad_output)
        B, Ho, Wo, _ = gy.shape
        if cop != cout:
            g = gy.new_zeros((B, Ho, Wo, cop))
            g[..., :cout].copy_(gy)
            gy = g
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            H, W = x.shape[1], x.shape[2]
            spread = gy.new_zeros((B, H + kh - 1, W + kw - 1, cop))
            t, l = kh - 1 - p, kw - 1 - p
            spread[:, t:t + (Ho - 1) * s + 1:s, l:l + (Wo - 1) * s + 1:s].copy_(gy)
            dx = from_nhwc(ops.conv_forward(spread, ops.conv_dgrad_weights(w), 1, 0, math=ctx.math))
        if ctx.needs_input_grad[1]:
            dw = ops.conv_wgrad(x, gy, torch.zeros_like(w), s, p, math=ctx.math)
            dw = from_nhwc(dw[:cout])
        if ctx.with_bias and ctx.needs_input_grad[2]:
            db = ops.bias_grad(gy, gy.new_zeros((cop,)))[:cout]
        return dx, dw, db, None, None


class Conv2d(nn.Module):
    """nn.Conv2d's parameters and state_dict (weight [Cout, Cin, kh, kw], bias [Cout]) for a convolution that runs in the library: the
    conv_offset_mask of ModulatedDeformConvPack, or the offset conv in front of a DeformConv.  One stride and one padding for both axes."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, bias=True):
        super().__init__()
        self.in_channels, self.out_channels, self.kernel_size = in_channels, out_channels, _pair(kernel_size)
        self.stride, self.padding = stride, padding
        if in_channels % 4:
            raise NotImplementedError("Conv2d: in_channels = {} is not a multiple of 4".format(in_channels))
        self.weight = _oihw_parameter(out_channels, in_channels, *self.kernel_size)
        self.bias = nn.Parameter(torch.zeros(out_channels)) if bias else None
        with torch.no_grad():   # nn.Conv2d.reset_parameters
            nn.init.kaiming_uniform_(self.weight, a=math.sqrt(5))
            if bias:
                bound = 1. / math.sqrt(in_channels * self.kernel_size[0] * self.kernel_size[1])
                self.bias.uniform_(-bound, bound)

    def forward(self, input):
        return _Conv2dFunction.apply(input, self.weight, self.bias, self.stride, self.padding)

    def extra_repr(self):
        return "{}, {}, kernel_size={}, stride={}, padding={}".format(self.in_channels, self.out_channels, self.kernel_size, _pair(self.stride),
                                                                      _pair(self.padding))


class ModulatedDeformConvPack(ModulatedDeformConv):
    """deform_conv_module.py:140-177"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, bias=True):
        super(ModulatedDeformConvPack, self).__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups,
                                                      deformable_groups, bias)
        if groups != 1:
            # its offset conv takes in_channels // groups channels (deform_conv_module.py:156-157) and is then fed all in_channels of them
            raise NotImplementedError("ModulatedDeformConvPack: groups = {}: conv_offset_mask takes in_channels // groups = {} channels but is "
                                      "fed the input's {}, so the reference's layer only runs with groups == 1"
                                      .format(groups, in_channels // groups, in_channels))
        self.conv_offset_mask = Conv2d(self.in_channels // self.groups, self.deformable_groups * 3 * self.kernel_size[0] * self.kernel_size[1],
                                       kernel_size=self.kernel_size, stride=self.stride, padding=self.padding, bias=True)
        self.init_offset()

    def init_offset(self):
        self.conv_offset_mask.weight.data.zero_()
        self.conv_offset_mask.bias.data.zero_()

    def forward(self, input):
        out = self.conv_offset_mask(input)
        o1, o2, mask = torch.chunk(out, 3, dim=1)
        offset = torch.cat((o1, o2), dim=1)
        mask = torch.sigmoid(mask)
        return modulated_deform_conv(input, offset, mask, self.weight, self.bias, self.stride, self.padding, self.dilation, self.groups,
                                     self.deformable_groups)

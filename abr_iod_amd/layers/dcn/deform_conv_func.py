"""Mirror of maskrcnn_benchmark/layers/dcn/deform_conv_func.py: deform_conv and modulated_deform_conv as autograd functions over the
library's general deformable conv (ops.deform_conv_forward / ops.deform_conv_backward: columns, one 1x1 contraction per group in the
library's default arithmetic, the col2im + coord kernel).

Tensors have the reference's logical shapes -- input [B,C,H,W], offset [B,dg*2*K,Ho,Wo], mask [B,dg*K,Ho,Wo], weight [Cout,C/groups,kh,kw]
-- and are read through as_nhwc: channels-last memory is a view, plain NCHW memory is converted once.  Results and gradients come back as
logical-NCHW views of channels-last memory."""
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from ... import ops
from ..._lib import require_cuda
from .._layout import as_nhwc, from_nhwc


def _geometry(weight, stride, padding, dilation):
    return (weight.size(2), weight.size(3)), _pair(stride), _pair(padding), _pair(dilation)


class DeformConvFunction(Function):
    """deform_conv_func.py:9-147"""

    @staticmethod
    def forward(ctx, input, offset, weight, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1, im2col_step=64):
        if input is not None and input.dim() != 4:
            raise ValueError("Expected 4D tensor as input, got {}D tensor instead.".format(input.dim()))
        ctx.geom = _geometry(weight, stride, padding, dilation)
        ctx.groups, ctx.deformable_groups = groups, deformable_groups
        DeformConvFunction._output_size(input, weight, ctx.geom[2], ctx.geom[3], ctx.geom[1])
        # the columns are built for the whole batch at once: im2col_step changes no result, its assertion stays (deform_conv_func.py:46-48)
        cur_im2col_step = min(im2col_step, input.shape[0])
        assert (input.shape[0] % cur_im2col_step) == 0, 'im2col step must divide batchsize'
        require_cuda(input, offset, weight)
        x, off, w = as_nhwc(input.detach()), as_nhwc(offset.detach()), as_nhwc(weight.detach())
        y, cols = ops.deform_conv_forward(x, off, None, w, None, *ctx.geom, groups=groups, dg=deformable_groups)
        ctx.save_for_backward(x, off, w, cols)
        return from_nhwc(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, off, w, cols = ctx.saved_tensors
        need_input = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        dx, d_off, _, dw, _ = ops.deform_conv_backward(as_nhwc(grad_output), x, off, None, w, cols, *ctx.geom, groups=ctx.groups,
                                                       dg=ctx.deformable_groups, need_input=need_input, need_weight=ctx.needs_input_grad[2])
        return ((from_nhwc(dx) if need_input else None), (from_nhwc(d_off) if need_input else None),
                (from_nhwc(dw) if dw is not None else None), None, None, None, None, None, None)

    @staticmethod
    def _output_size(input, weight, padding, dilation, stride):
        """deform_conv_func.py:134-147"""
        channels = weight.size(0)
        output_size = (input.size(0), channels)
        for d in range(input.dim() - 2):
            in_size = input.size(d + 2)
            pad = padding[d]
            kernel = dilation[d] * (weight.size(d + 2) - 1) + 1
            stride_ = stride[d]
            output_size += ((in_size + (2 * pad) - kernel) // stride_ + 1, )
        if not all(map(lambda s: s > 0, output_size)):
            raise ValueError("convolution input is too small (output would be {})".format('x'.join(map(str, output_size))))
        return output_size


class ModulatedDeformConvFunction(Function):
    """deform_conv_func.py:150-258.  The mask is used as given (ModulatedDeformConvPack applies the sigmoid)."""

    @staticmethod
    def forward(ctx, input, offset, mask, weight, bias=None, stride=1, padding=0, dilation=1, groups=1, deformable_groups=1):
        ctx.geom = _geometry(weight, stride, padding, dilation)
        ctx.groups, ctx.deformable_groups = groups, deformable_groups
        ctx.with_bias = bias is not None
        require_cuda(input, offset, mask, weight, bias)
        x, off, m, w = as_nhwc(input.detach()), as_nhwc(offset.detach()), as_nhwc(mask.detach()), as_nhwc(weight.detach())
        b = bias.detach().contiguous() if ctx.with_bias else None
        y, cols = ops.deform_conv_forward(x, off, m, w, b, *ctx.geom, groups=groups, dg=deformable_groups)
        ctx.save_for_backward(x, off, m, w, cols)
        return from_nhwc(y)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        x, off, m, w, cols = ctx.saved_tensors
        need_input = any(ctx.needs_input_grad[:3])
        dx, d_off, d_m, dw, db = ops.deform_conv_backward(as_nhwc(grad_output), x, off, m, w, cols, *ctx.geom, groups=ctx.groups,
                                                          dg=ctx.deformable_groups, need_input=need_input,
                                                          need_weight=ctx.needs_input_grad[3], need_bias=ctx.with_bias and ctx.needs_input_grad[4])
        return ((from_nhwc(dx) if need_input else None), (from_nhwc(d_off) if need_input else None),
                (from_nhwc(d_m) if need_input else None), (from_nhwc(dw) if dw is not None else None), db, None, None, None, None, None)

    @staticmethod
    def _infer_shape(ctx, input, weight):
        """deform_conv_func.py:249-258, for pair-valued ctx.geom"""
        return (input.size(0), weight.size(0)) + ops.deform_out_size(input.size(2), input.size(3), *ctx.geom)


deform_conv = DeformConvFunction.apply
modulated_deform_conv = ModulatedDeformConvFunction.apply

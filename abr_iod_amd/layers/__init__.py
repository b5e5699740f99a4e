"""Mirror of maskrcnn_benchmark/layers/__init__.py:4-20: same public names (ROIAlign, roi_align, ROIPool, roi_pool, nms, smooth_l1_loss,
SigmoidFocalLoss, FrozenBatchNorm2d, deform_roi_pooling, DeformRoIPooling, DeformRoIPoolingPack, ModulatedDeformRoIPoolingPack, and from
layers/dcn: deform_conv, modulated_deform_conv, DeformConv, ModulatedDeformConv, ModulatedDeformConvPack), backed by the HIP library."""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable
from torch.nn.modules.utils import _pair

from .. import _C, ops
from .._lib import require_cuda
from ._layout import as_nhwc, from_nhwc
from .dcn import DeformConv, ModulatedDeformConv, ModulatedDeformConvPack, deform_conv, modulated_deform_conv  # noqa: F401  (layers/__init__.py:6-7)

nms = _C.nms  # layers/nms.py:8 (amp.float_function is a no-op at O0)


# ------------------------------------------------------------------------------------------- ROIAlign
class _ROIAlign(Function):
    """layers/roi_align.py:12-48.  input: logical [B,C,H,W]; output: logical [K,C,ph,pw] (channels-last memory)."""

    @staticmethod
    def forward(ctx, input, roi, output_size, spatial_scale, sampling_ratio, bin_step=1):
        require_cuda(input, roi)
        ctx.save_for_backward(roi)
        ctx.output_size = _pair(output_size)
        ctx.spatial_scale, ctx.sampling_ratio, ctx.bin_step = spatial_scale, sampling_ratio, bin_step
        ctx.input_shape = input.size()
        xin = as_nhwc(input)
        out = ops.roi_align_forward(xin, roi, spatial_scale, ctx.output_size[0], ctx.output_size[1],
                                    sampling_ratio, bin_step)
        ops.amax_carry_bound(out, xin)   # pooled values are averages of bilinear samples: bounded by the feature map's amax (f16x3 scales)
        return from_nhwc(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        (rois,) = ctx.saved_tensors
        bs, ch, h, w = ctx.input_shape
        g = ops.roi_align_backward(as_nhwc(grad_output), rois, ctx.spatial_scale, ctx.output_size[0], ctx.output_size[1],
                                   ctx.sampling_ratio, bs, h, w, ch, ctx.bin_step)
        return from_nhwc(g), None, None, None, None, None


roi_align = _ROIAlign.apply


class ROIAlign(nn.Module):
    """layers/roi_align.py:51-70"""

    def __init__(self, output_size, spatial_scale, sampling_ratio):
        super().__init__()
        self.output_size, self.spatial_scale, self.sampling_ratio = output_size, spatial_scale, sampling_ratio

    def forward(self, input, rois, bin_step=1):
        return roi_align(input, rois, self.output_size, self.spatial_scale, self.sampling_ratio, bin_step)

    def __repr__(self):
        return "{}(output_size={}, spatial_scale={}, sampling_ratio={})".format(
            self.__class__.__name__, self.output_size, self.spatial_scale, self.sampling_ratio)


# ------------------------------------------------------------------------------------------- ROIPool
class _ROIPool(Function):
    """layers/roi_pool.py:12-44.  input: logical [B,C,H,W]; output: logical [K,C,ph,pw] (channels-last memory)."""

    @staticmethod
    def forward(ctx, input, roi, output_size, spatial_scale):
        require_cuda(input, roi)
        ctx.output_size = _pair(output_size)
        ctx.spatial_scale = spatial_scale
        ctx.input_shape = input.size()
        xin = as_nhwc(input)
        out, argmax = ops.roi_pool_forward(xin, roi, spatial_scale, ctx.output_size[0], ctx.output_size[1])
        ops.amax_carry_bound(out, xin)   # every pooled value is one of the map's own (or 0 for an empty bin): bounded by the map's amax
        ctx.save_for_backward(roi, argmax)
        return from_nhwc(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        rois, argmax = ctx.saved_tensors
        bs, ch, h, w = ctx.input_shape
        g = ops.roi_pool_backward(as_nhwc(grad_output), rois, argmax, bs, h, w)
        return from_nhwc(g), None, None, None


roi_pool = _ROIPool.apply


class ROIPool(nn.Module):
    """layers/roi_pool.py:50-65"""

    def __init__(self, output_size, spatial_scale):
        super().__init__()
        self.output_size, self.spatial_scale = output_size, spatial_scale

    def forward(self, input, rois):
        return roi_pool(input, rois, self.output_size, self.spatial_scale)

    def __repr__(self):
        return "{}(output_size={}, spatial_scale={})".format(self.__class__.__name__, self.output_size, self.spatial_scale)


# ------------------------------------------------------------------------------------------- deformable PS-RoI pooling
class _DeformRoIPooling(Function):
    """layers/dcn/deform_pool_func.py:8-92, plus one optional operand: mask_logits [K, P, P] (the output is multiplied by their sigmoid inside
    the kernel, which is ModulatedDeformRoIPoolingPack's `* mask`).  data: logical [B,C,H,W]; offset: [K, 2 num_classes, part, part] (unused
    under no_trans); output: logical [K, out_channels, P, P] (channels-last memory)."""

    @staticmethod
    def forward(ctx, data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4,
                trans_std=.0, mask_logits=None):
        assert 0.0 <= trans_std <= 1.0
        require_cuda(data, rois)
        part_size = out_size if part_size is None else part_size
        ctx.args = (spatial_scale, out_channels, group_size, out_size, part_size, sample_per_part, trans_std)
        ctx.no_trans = no_trans
        xin = as_nhwc(data)
        trans = None if no_trans else offset.detach().contiguous()
        logits = None if mask_logits is None else mask_logits.detach().contiguous()
        out, count = ops.deform_psroi_forward(xin, rois, trans, *ctx.args, mask_logits=logits)
        # an average of bilinear samples (weights sum to at most 1), times a sigmoid <= 1: bounded by the map's amax
        ops.amax_carry_bound(out, xin)
        ctx.save_for_backward(xin, rois, trans, logits, count)
        ctx.offset_shape = tuple(offset.shape)
        return from_nhwc(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        xin, rois, trans, logits, count = ctx.saved_tensors
        gfeat, gtrans, glogits = ops.deform_psroi_backward(as_nhwc(grad_output), xin, rois, trans, count, *ctx.args, mask_logits=logits)
        if gtrans is None:
            gtrans = xin.new_zeros(ctx.offset_shape)   # deform_pool_func.py:73 (the empty tensor under no_trans)
        else:
            gtrans = gtrans.view(ctx.offset_shape)
        return (from_nhwc(gfeat), None, gtrans) + (None,) * 8 + (glogits,)


def deform_roi_pooling(data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4,
                       trans_std=.0, mask_logits=None):
    """layers/dcn/deform_pool_func.py:95; mask_logits [K, P, P]: see _DeformRoIPooling"""
    if mask_logits is not None and tuple(mask_logits.shape) != (rois.shape[0], out_size, out_size):
        raise RuntimeError(f"deform_roi_pooling: mask_logits {tuple(mask_logits.shape)} is not {(rois.shape[0], out_size, out_size)}")
    return _DeformRoIPooling.apply(data, rois, offset, spatial_scale, out_size, out_channels, no_trans, group_size, part_size, sample_per_part,
                                   trans_std, mask_logits)


class _PadLinear(nn.Module):
    """nn.Linear's parameters -- weight [out, in], bias [out], its default initialisation -- as views of buffers whose output width is padded
    to a multiple of 4: the contraction kernels take channel counts that are multiples of 4, on the output side too (the input gradient
    contracts over it).  The padding rows stay zero.  Gradients accumulate in buffers of the same shape, of which .grad are views
    (modeling/roi_heads/box_head/box_head.py, FastRCNNPredictor, keeps its two layers the same way)."""

    def __init__(self, in_features, out_features, zero=False):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.out_pad = (out_features + 3) // 4 * 4
        w, b = torch.zeros(self.out_pad, in_features), torch.zeros(self.out_pad)
        if not zero:   # nn.Linear.reset_parameters
            nn.init.kaiming_uniform_(w[:out_features], a=5 ** 0.5)
            bound = in_features ** -0.5
            nn.init.uniform_(b[:out_features], -bound, bound)
        self.weight, self.bias = nn.Parameter(w[:out_features]), nn.Parameter(b[:out_features])
        self._w, self._b, self._gw, self._gb = w, b, None, None

    def home(self):
        """(padded weight [out_pad,1,1,in], padded bias): the parameters moved (to a device, by a load that replaced them) -> back into fresh buffers"""
        n, p = self.out_features, self.weight
        if p.data_ptr() != self._w.data_ptr() or self.bias.data_ptr() != self._b.data_ptr() or self._w.device != p.device:
            w, b = torch.zeros(self.out_pad, self.in_features, device=p.device), torch.zeros(self.out_pad, device=p.device)
            with torch.no_grad():
                w[:n].copy_(p)
                b[:n].copy_(self.bias)
            self._w, self._b, self._gw, self._gb = w, b, None, None
            p.data, self.bias.data = w[:n], b[:n]
        return self._w.view(self.out_pad, 1, 1, self.in_features), self._b

    def grad_home(self):
        """(padded weight gradient [out_pad,1,1,in], padded bias gradient) that .grad are views of; what .grad already holds is kept"""
        n = self.out_features
        for name, p, shape in (("_gw", self.weight, (self.out_pad, self.in_features)), ("_gb", self.bias, (self.out_pad,))):
            buf = getattr(self, name)
            if buf is None or buf.device != p.device or p.grad is None or p.grad.data_ptr() != buf.data_ptr():
                buf = torch.zeros(shape, device=p.device)
                if p.grad is not None:
                    buf[:n].copy_(p.grad)
                setattr(self, name, buf)
                p.grad = buf[:n]
        return self._gw.view(self.out_pad, 1, 1, self.in_features), self._gb

    def extra_repr(self):
        return "in_features={}, out_features={}, bias=True".format(self.in_features, self.out_features)


class _FCStack(nn.Module):
    """nn.Sequential(Linear, ReLU, Linear, ReLU, ..., Linear) of the reference with its state-dict keys: the linear layers sit at the even
    indices '0', '2', ...; the last one is zero-initialised (deform_pool_module.py:63-64,125-126)"""

    def __init__(self, widths):
        super().__init__()
        self.n = len(widths) - 1
        for i in range(self.n):
            self.add_module(str(2 * i), _PadLinear(widths[i], widths[i + 1], zero=i == self.n - 1))

    def __getitem__(self, i):
        """index over the reference Sequential's 2 n - 1 slots, negative ones from the end; the odd slots are its ReLUs, which hold nothing"""
        slots = 2 * self.n - 1
        j = i + slots if i < 0 else i
        if not 0 <= j < slots:
            raise IndexError(f"index {i} is out of range for {slots} slots")
        if j % 2:
            raise IndexError(f"slot {i} is the reference's ReLU: the linear layers sit at the even slots 0 .. {slots - 1}")
        return getattr(self, str(j))

    def layers(self):
        return [getattr(self, str(2 * i)) for i in range(self.n)]

    def forward(self, x):
        """x: logical [K, C, P, P] -> [K, out] of the flattened (c, ph, pw) features, as x.view(n, -1) gives the reference's stack"""
        return _FCStackFn.apply(x, self, *self.parameters())


class _FCStackFn(Function):
    """The FC stack as 1x1 contractions over [K, 1, 1, width] (the model is box_head._PredictorFn): bias and ReLU in the contraction's epilogue;
    backward: weight gradients on the side stream into the parameters' gradient buffers, bias gradients, input gradients through the
    transposed weights.  The parameters are arguments so that autograd runs this node for them; their gradients are WRITTEN (accumulated into
    the buffers `.grad` are views of, as _PredictorFn does), not returned: `loss.backward()` fills `.grad` as usual, `torch.autograd.grad`
    with respect to a parameter of the stack gets None, and a parameter with requires_grad=False still has its `.grad` written."""

    @staticmethod
    def forward(ctx, x, stack, *params):
        K = x.shape[0]
        xh = as_nhwc(x)                                            # [K, P, P, C]
        a = ops.nhwc_to_nchw(xh).view(K, 1, 1, -1)                 # (c, ph, pw) order: the columns of the reference's first weight
        acts, lins = [a], stack.layers()
        for i, lin in enumerate(lins):
            w, b = lin.home()
            a = ops.conv_forward(a, w, 1, 0, bias=b, relu=i < len(lins) - 1)
            acts.append(a)
        ctx.stack, ctx.acts, ctx.xshape, ctx.need_dx = stack, acts[:-1], tuple(xh.shape), x.requires_grad
        last = lins[-1]
        y = a.view(K, last.out_pad)
        return y if last.out_pad == last.out_features else y[:, :last.out_features].contiguous()

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        lins, acts = ctx.stack.layers(), ctx.acts
        K, last = gy.shape[0], lins[-1]
        if last.out_pad != last.out_features:
            g = gy.new_zeros((K, last.out_pad))
            g[:, :last.out_features].copy_(gy)
        else:
            g = gy.contiguous()
        g = g.view(K, 1, 1, -1)
        gx = None
        for i in range(len(lins) - 1, -1, -1):
            lin = lins[i]
            w, _ = lin.home()
            gw, gb = lin.grad_home()
            ops.conv_wgrad_async(acts[i], g, gw, 1, 0)
            ops.bias_grad(g, gb)
            if i > 0 or ctx.need_dx:
                gx = ops.conv_forward(g, ops.conv_dgrad_weights(w), 1, 0)
            if i > 0:
                g = ops.relu_backward(gx, acts[i])                 # acts[i] is layer i-1's ReLU output
        if ctx.need_dx:
            Kx, P, Q, Ch = ctx.xshape
            gx = from_nhwc(ops.nchw_to_nhwc(gx.view(Kx, Ch, P, Q)))
        else:
            gx = None
        ctx.acts = None
        return (gx, None) + (None,) * (len(ctx.needs_input_grad) - 2)


class DeformRoIPooling(nn.Module):
    """layers/dcn/deform_pool_module.py:6-33"""

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0):
        super().__init__()
        self.spatial_scale, self.out_size, self.out_channels, self.no_trans = spatial_scale, out_size, out_channels, no_trans
        self.group_size = group_size
        self.part_size = out_size if part_size is None else part_size
        self.sample_per_part, self.trans_std = sample_per_part, trans_std

    def _pool(self, data, rois, offset, no_trans, mask_logits=None):
        return deform_roi_pooling(data, rois, offset, self.spatial_scale, self.out_size, self.out_channels, no_trans, self.group_size,
                                  self.part_size, self.sample_per_part, self.trans_std, mask_logits)

    def forward(self, data, rois, offset):
        if self.no_trans:
            offset = data.new_empty(0)
        return self._pool(data, rois, offset, self.no_trans)

    def _check_fc(self, deform_fc_channels):
        # the FC stacks run as contractions over channel vectors of 16 bytes: P * P * out_channels and deform_fc_channels are their widths
        if self.out_channels % 4 != 0:
            raise NotImplementedError(f"{type(self).__name__}: out_channels = {self.out_channels} is not a multiple of 4")
        if deform_fc_channels % 4 != 0:
            raise NotImplementedError(f"{type(self).__name__}: deform_fc_channels = {deform_fc_channels} is not a multiple of 4")


class DeformRoIPoolingPack(DeformRoIPooling):
    """layers/dcn/deform_pool_module.py:36-86: a first pass without offsets, an FC stack that turns it into offsets, the pass with them"""

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0,
                 deform_fc_channels=1024):
        super().__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            self._check_fc(deform_fc_channels)
            n_in = self.out_size * self.out_size * self.out_channels
            self.offset_fc = _FCStack([n_in, deform_fc_channels, deform_fc_channels, self.out_size * self.out_size * 2])

    def forward(self, data, rois):
        assert data.size(1) == self.out_channels
        n = rois.shape[0]
        if self.no_trans or n == 0:   # (no RoI: nothing for the FC stacks to contract, and the pooled tensor is empty either way)
            return self._pool(data, rois, data.new_empty(0), True)
        x = self._pool(data, rois, data.new_empty(0), True)
        offset = self.offset_fc(x).view(n, 2, self.out_size, self.out_size)
        return self._pool(data, rois, offset, False)


class ModulatedDeformRoIPoolingPack(DeformRoIPooling):
    """layers/dcn/deform_pool_module.py:89-150.  mask_fc ends in the reference's nn.Sigmoid (index 3, no parameters); here the sigmoid and
    the product with the pooled values happen inside the pooling kernel, which takes the stack's logits."""

    def __init__(self, spatial_scale, out_size, out_channels, no_trans, group_size=1, part_size=None, sample_per_part=4, trans_std=.0,
                 deform_fc_channels=1024):
        super().__init__(spatial_scale, out_size, out_channels, no_trans, group_size, part_size, sample_per_part, trans_std)
        self.deform_fc_channels = deform_fc_channels
        if not no_trans:
            self._check_fc(deform_fc_channels)
            n_in = self.out_size * self.out_size * self.out_channels
            self.offset_fc = _FCStack([n_in, deform_fc_channels, deform_fc_channels, self.out_size * self.out_size * 2])
            self.mask_fc = _FCStack([n_in, deform_fc_channels, self.out_size * self.out_size])

    def forward(self, data, rois):
        assert data.size(1) == self.out_channels
        n = rois.shape[0]
        if self.no_trans or n == 0:   # (no RoI: nothing for the FC stacks to contract, and the pooled tensor is empty either way)
            return self._pool(data, rois, data.new_empty(0), True)
        x = self._pool(data, rois, data.new_empty(0), True)
        offset = self.offset_fc(x).view(n, 2, self.out_size, self.out_size)
        logits = self.mask_fc(x).view(n, self.out_size, self.out_size)
        return self._pool(data, rois, offset, False, logits)


# ------------------------------------------------------------------------------------------- smooth L1
class _SmoothL1(Function):
    @staticmethod
    def forward(ctx, input, target, beta, size_average):
        scale = 1.0 / max(input.numel(), 1) if size_average else 1.0
        loss, grad = ops.smooth_l1(input, target, beta, scale=scale, want_grad=input.requires_grad)
        ctx.save_for_backward(grad)
        return loss[0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        (grad,) = ctx.saved_tensors
        return ops.scale_(grad, 1.0, g.contiguous()), None, None, None


def smooth_l1_loss(input, target, beta=1.0 / 9, size_average=True):
    """layers/smooth_l1_loss.py:6-17"""
    if input.numel() == 0:
        return input.sum() * 0.0
    return _SmoothL1.apply(input, target.detach(), beta, size_average)


# ------------------------------------------------------------------------------------------- focal loss
class _SigmoidFocalLoss(Function):
    """layers/sigmoid_focal_loss.py:9-35"""

    @staticmethod
    def forward(ctx, logits, targets, gamma, alpha):
        ctx.save_for_backward(logits, targets)
        ctx.num_classes, ctx.gamma, ctx.alpha = logits.shape[1], gamma, alpha
        return _C.sigmoid_focalloss_forward(logits, targets, ctx.num_classes, gamma, alpha)

    @staticmethod
    @once_differentiable
    def backward(ctx, d_loss):
        logits, targets = ctx.saved_tensors
        d = _C.sigmoid_focalloss_backward(logits, targets, d_loss.contiguous(), ctx.num_classes, ctx.gamma, ctx.alpha)
        return d, None, None, None, None


sigmoid_focal_loss_cuda = _SigmoidFocalLoss.apply


class SigmoidFocalLoss(nn.Module):
    """layers/sigmoid_focal_loss.py:55-76 (returns the SUM)."""

    def __init__(self, gamma, alpha):
        super().__init__()
        self.gamma, self.alpha = gamma, alpha

    def forward(self, logits, targets):
        return sigmoid_focal_loss_cuda(logits, targets, self.gamma, self.alpha).sum()

    def __repr__(self):
        return "{}(gamma={}, alpha={})".format(self.__class__.__name__, self.gamma, self.alpha)


# ------------------------------------------------------------------------------------------- FrozenBN
class FrozenBatchNorm2d(nn.Module):
    """layers/batch_norm.py:6-31: fixed statistics and affine, NO epsilon.  On the hot path it never runs as its
    own kernel: `scale_bias()` feeds the conv kernel's epilogue (y = acc*scale + bias)."""

    def __init__(self, n):
        super().__init__()
        self.register_buffer("weight", torch.ones(n))
        self.register_buffer("bias", torch.zeros(n))
        self.register_buffer("running_mean", torch.zeros(n))
        self.register_buffer("running_var", torch.ones(n))
        self._fused = None

    def scale_bias(self):
        if self._fused is None or self._fused[0].device != self.weight.device:
            scale = self.weight * self.running_var.rsqrt()      # batch_norm.py:27
            bias = self.bias - self.running_mean * scale        # :28
            self._fused = (scale.contiguous(), bias.contiguous())
        return self._fused

    def invalidate(self):
        self._fused = None

    def _load_from_state_dict(self, *a, **k):
        super()._load_from_state_dict(*a, **k)
        self._fused = None

    def forward(self, x):
        scale, bias = self.scale_bias()
        eye = torch.eye(scale.numel(), device=x.device).view(scale.numel(), 1, 1, scale.numel())
        return from_nhwc(ops.conv_forward(as_nhwc(x), eye, scale=scale, bias=bias))

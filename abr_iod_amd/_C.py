"""Drop-in replacement for the reference's pybind11 module `maskrcnn_benchmark._C`
(maskrcnn_benchmark/csrc/vision.cpp:10-16) on the hot path: same callable names, argument order,
tensor layouts (NCHW fp32), return types and error behaviour — backed by libabr_iod_hip.so.

    nms(dets[n,4], scores[n], threshold) -> int64[k]                     csrc/nms.h:10-27
    roi_align_forward(input, rois, spatial_scale, ph, pw, sampling_ratio) csrc/ROIAlign.h:11-25
    roi_align_backward(grad, rois, spatial_scale, ph, pw, B, C, H, W, sr) csrc/ROIAlign.h:27-45
    sigmoid_focalloss_forward(logits, targets, num_classes, gamma, alpha) csrc/SigmoidFocalLoss.h:10-23
    sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha)   :25-41
    roi_pool_forward(input, rois, spatial_scale, ph, pw) -> (output, argmax int32)  csrc/ROIPool.h:10-24
    roi_pool_backward(grad, input, rois, argmax, spatial_scale, ph, pw, B, C, H, W)      :26-47
    deform_psroi_pooling_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim, group_size, pooled_size,
                                 part_size, sample_per_part, trans_std)             csrc/deform_pool.h:11-40   (writes out, top_count)
    deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad, no_trans, ...)  :43-70
                                                                          (adds into input_grad, writes trans_grad)
    deform_conv_forward(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
                        deformable_group, im2col_step)                              csrc/deform_conv.h:11-42   (writes output)
    deform_conv_backward_input(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, ...)       :45-77
                                                                          (writes gradInput, gradOffset)
    deform_conv_backward_parameters(input, offset, gradOutput, gradWeight, columns, ones, kW, ..., scale, im2col_step)   :80-112
                                                                          (adds scale * gradient into gradWeight)
    modulated_deform_conv_forward(input, weight, bias, ones, offset, mask, output, columns, kernel_h, kernel_w, stride_h, stride_w,
                                  pad_h, pad_w, dilation_h, dilation_w, group, deformable_group, with_bias)      :115-149  (writes output)
    modulated_deform_conv_backward(input, weight, bias, ones, offset, mask, columns, grad_input, grad_weight, grad_bias, grad_offset,
                                   grad_mask, grad_output, kernel_h, ...)            :152-191
                                                      (adds into grad_weight, grad_bias; writes grad_input, grad_offset, grad_mask)

The RoI poolers take float32 and float64 like the reference's dispatch, the deformable pooling pair and the deformable convolutions
float32 only; anything else raises RuntimeError naming the dtype.  The deformable convolutions run the general kernels of csrc/deform.hip
(abr_deform_im2col_general, abr_deform_col2im_coord_general) around the library's 1x1 contraction; their scratch arguments (columns, ones)
are accepted and ignored, and the shape checks of deform_conv_cuda.cu raise with its wording.  The body's DCN keeps its specialised kernels.

The reference's multi-level Pooler (modeling/poolers.py) is Python over roi_align_forward / roi_align_backward above and works through this
module level by level; abr_iod_amd.modeling.poolers.Pooler pools several scales in one launch each way instead (ops.roi_align_pyramid_*).

CPU tensors raise RuntimeError (the reference raises "Not compiled with GPU support" the other way round):
this library is MI355X-only by design; the CPU restatement lives in oracle/ and is test infrastructure.
"""
import torch

from . import _lib as L
from . import ops

# NMS comparison rule.  The reference is inconsistent: CPU suppresses at IoU >= thr (nms_cpu.cpp:60),
# CUDA at IoU > thr (nms.cu:60).  The CPU path is the parity oracle, so '>=' is the default here.
NMS_STRICT_GT = False


def nms(dets, scores, threshold, strict_gt=None):
    L.require_cuda(dets, scores)
    if dets.numel() == 0:  # nms.h:15-16
        return torch.empty((0,), dtype=torch.int64, device=dets.device)
    if dets.dtype != torch.float32 or scores.dtype != torch.float32:
        raise RuntimeError("nms: dets and scores must be float32 (nms.cu:71 is float-only)")
    strict = NMS_STRICT_GT if strict_gt is None else strict_gt
    n = dets.shape[0]
    if n <= int(L.lib().abr_sort_scores_max_n()):
        # the whole call inside the library (round 5): score ranking on the proposal ranking's own kernels, gather, mask + sweep, and the
        # survivors' original indices compacted in ascending order -- no ATen sort on either side of the suppression
        d, s = dets.contiguous(), scores.contiguous()
        nbytes = int(L.lib().abr_nms_unsorted_workspace_bytes(n))
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dets.device)
        keep_out = torch.empty((n,), dtype=torch.int64, device=dets.device)
        n_keep = torch.empty((1,), dtype=torch.int32, device=dets.device)
        L.check(L.lib().abr_nms(L.ptr(d), L.ptr(s), n, float(threshold), int(strict), L.ptr(keep_out), L.ptr(n_keep), L.ptr(ws), nbytes, L.stream()), "nms")
        return keep_out[: int(n_keep.item())]   # the reference blocks here too (nms.cu:100 cudaMemcpy D2H)
    # more boxes than the in-LDS merge of the score sort takes (15360; the reference's call sites stay at or below 12000): ATen's sort
    order = torch.sort(scores, dim=0, descending=True, stable=True)[1]
    boxes = dets.index_select(0, order).contiguous()
    counts = torch.tensor([n], dtype=torch.int32, device=dets.device)
    keep = torch.empty((1, n), dtype=torch.int32, device=dets.device)
    n_keep = torch.empty((1,), dtype=torch.int32, device=dets.device)
    ws_bytes = L.lib().abr_nms_workspace_bytes(1, n)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dets.device)
    L.check(L.lib().abr_nms_sorted_batched(L.ptr(boxes), L.ptr(counts), 1, n, float(threshold), int(strict), n,
                                           L.ptr(keep), L.ptr(n_keep), L.ptr(ws), ws_bytes, L.stream()), "nms")
    k = int(n_keep.item())  # the reference blocks here too (nms.cu:100 cudaMemcpy D2H)
    # nms.cu:127-130 / nms_cpu.cpp:66: ascending ORIGINAL indices of the survivors
    return order.index_select(0, keep[0, :k].long()).sort()[0]


def roi_align_forward(input, rois, spatial_scale, pooled_height, pooled_width, sampling_ratio):
    """float32 or float64 (AT_DISPATCH_FLOATING_TYPES, ROIAlign_cuda.cu:283)"""
    L.require_cuda(input, rois)
    x = L.fpc(input)
    r = L.fpc(rois, like=x)
    B, Ch, H, W = x.shape
    K = r.shape[0]
    out = torch.empty((K, Ch, pooled_height, pooled_width), dtype=x.dtype, device=x.device)
    if out.numel() == 0:
        return out
    if x.dtype == torch.float64:
        L.check(L.lib().abr_roi_align_forward_f64(L.ptr(x), L.ptr(r), K, B, Ch, H, W, float(spatial_scale), pooled_height, pooled_width,
                                                  sampling_ratio, L.ptr(out), L.stream()), "roi_align_forward (float64)")
        return out
    L.check(L.lib().abr_roi_align_forward(L.ptr(x), L.ptr(r), K, B, Ch, H, W, float(spatial_scale), pooled_height,
                                          pooled_width, sampling_ratio, 1, L.NCHW, L.ptr(out), L.stream()),
            "roi_align_forward")
    return out


def roi_align_backward(grad, rois, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width,
                       sampling_ratio):
    L.require_cuda(grad, rois)
    g = L.fpc(grad)
    r = L.fpc(rois, like=g)
    K = r.shape[0]
    out = torch.empty((batch_size, channels, height, width), dtype=g.dtype, device=g.device)
    if g.dtype == torch.float64:   # ROIAlign_cuda.cu:329
        L.check(L.lib().abr_roi_align_backward_f64(L.ptr(g), L.ptr(r), K, batch_size, channels, height, width, float(spatial_scale), pooled_height,
                                                   pooled_width, sampling_ratio, L.ptr(out), L.stream()), "roi_align_backward (float64)")
        return out
    L.check(L.lib().abr_roi_align_backward(L.ptr(g), L.ptr(r), K, batch_size, channels, height, width,
                                           float(spatial_scale), pooled_height, pooled_width, sampling_ratio, 1, L.NCHW,
                                           0, L.ptr(out), L.stream()), "roi_align_backward")
    return out


def sigmoid_focalloss_forward(logits, targets, num_classes, gamma, alpha):
    L.require_cuda(logits, targets)
    if logits.dim() != 2:
        raise RuntimeError("logits should be NxClass")  # SigmoidFocalLoss_cuda.cu:112
    x = L.fpc(logits)
    t = targets.to(torch.int32).contiguous()
    out = torch.empty_like(x)
    if x.dtype == torch.float64:   # SigmoidFocalLoss_cuda.cu:128
        L.check(L.lib().abr_sigmoid_focal_forward_f64(L.ptr(x), L.ptr(t), x.shape[0], num_classes, float(gamma), float(alpha), L.ptr(out), L.stream()),
                "sigmoid_focalloss_forward (float64)")
        return out
    L.check(L.lib().abr_sigmoid_focal_forward(L.ptr(x), L.ptr(t), x.shape[0], num_classes, float(gamma), float(alpha),
                                              L.ptr(out), L.stream()), "sigmoid_focalloss_forward")
    return out


def sigmoid_focalloss_backward(logits, targets, d_losses, num_classes, gamma, alpha):
    L.require_cuda(logits, targets, d_losses)
    x = L.fpc(logits)
    d = L.fpc(d_losses, like=x)
    t = targets.to(torch.int32).contiguous()
    out = torch.empty_like(x)
    if x.dtype == torch.float64:   # SigmoidFocalLoss_cuda.cu:172
        L.check(L.lib().abr_sigmoid_focal_backward_f64(L.ptr(x), L.ptr(t), L.ptr(d), x.shape[0], num_classes, float(gamma), float(alpha), L.ptr(out),
                                                       L.stream()), "sigmoid_focalloss_backward (float64)")
        return out
    L.check(L.lib().abr_sigmoid_focal_backward(L.ptr(x), L.ptr(t), L.ptr(d), x.shape[0], num_classes, float(gamma),
                                               float(alpha), L.ptr(out), L.stream()), "sigmoid_focalloss_backward")
    return out


def _f32_only(name, *tensors):
    for t in tensors:
        if t.dtype != torch.float32:
            raise RuntimeError(f"{name}: float32 only, got {t.dtype}")   # (the reference also dispatches double and half; this library does not)


def roi_pool_forward(input, rois, spatial_scale, pooled_height, pooled_width):
    """-> (output, argmax int32), both [K, C, ph, pw]; float32 or float64 (AT_DISPATCH_FLOATING_TYPES, ROIPool_cuda.cu:134)"""
    L.require_cuda(input, rois)
    x = L.fpc(input)
    r = L.fpc(rois, like=x)
    B, Ch, H, W = x.shape
    K = r.shape[0]
    out = torch.empty((K, Ch, pooled_height, pooled_width), dtype=x.dtype, device=x.device)
    argmax = torch.zeros((K, Ch, pooled_height, pooled_width), dtype=torch.int32, device=x.device)   # at::zeros, ROIPool_cuda.cu:125
    if out.numel() == 0:
        return out, argmax
    if x.dtype == torch.float64:
        L.check(L.lib().abr_roi_pool_forward_f64(L.ptr(x), L.ptr(r), K, B, Ch, H, W, float(spatial_scale), pooled_height, pooled_width, L.ptr(out),
                                                 L.ptr(argmax), L.stream()), "roi_pool_forward (float64)")
        return out, argmax
    L.check(L.lib().abr_roi_pool_forward(L.ptr(x), L.ptr(r), K, B, Ch, H, W, float(spatial_scale), pooled_height, pooled_width, L.NCHW, L.ptr(out),
                                         L.ptr(argmax), L.stream()), "roi_pool_forward")
    return out, argmax


def roi_pool_backward(grad, input, rois, argmax, spatial_scale, pooled_height, pooled_width, batch_size, channels, height, width):
    L.require_cuda(grad, rois, argmax)
    g = L.fpc(grad)
    r = L.fpc(rois, like=g)
    K = r.shape[0]
    if argmax.dtype != torch.int32 or tuple(argmax.shape) != tuple(g.shape):
        raise RuntimeError(f"roi_pool_backward: argmax must be int32 of grad's shape {tuple(g.shape)}, got {argmax.dtype} {tuple(argmax.shape)}")
    am = argmax.contiguous()
    out = torch.empty((batch_size, channels, height, width), dtype=g.dtype, device=g.device)
    if g.dtype == torch.float64:   # ROIPool_cuda.cu:177
        L.check(L.lib().abr_roi_pool_backward_f64(L.ptr(g), L.ptr(r), L.ptr(am), K, batch_size, channels, height, width, pooled_height, pooled_width,
                                                  L.ptr(out), L.stream()), "roi_pool_backward (float64)")
        return out
    L.check(L.lib().abr_roi_pool_backward(L.ptr(g), L.ptr(r), L.ptr(am), K, batch_size, channels, height, width, pooled_height, pooled_width, L.NCHW, 0,
                                          L.ptr(out), L.stream()), "roi_pool_backward")
    return out


def _psroi_args(name, input, bbox, trans, out, no_trans, output_dim, pooled_size, part_size):
    """the checks of deform_pool_cuda.cu:47-65: contiguous NCHW float32 tensors, the output's first dimension is the box count"""
    L.require_cuda(input, bbox, out)
    _f32_only(name, input, bbox, out)
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")   # deform_pool_cuda.cu:47
    K = bbox.shape[0]
    if K != out.shape[0]:
        raise RuntimeError(f"Output shape and bbox number wont match: ({out.shape[0]} vs {K}).")   # :63-65
    t = None
    ncls = 1
    if not no_trans:
        L.require_cuda(trans)
        _f32_only(name, trans)
        t = trans.contiguous()
        if t.dim() != 4 or t.shape[0] != K or t.shape[1] % 2 or tuple(t.shape[2:]) != (part_size, part_size):
            raise RuntimeError(f"{name}: trans {tuple(t.shape)} is not [{K}, 2 * num_classes, {part_size}, {part_size}]")
        ncls = t.shape[1] // 2
    if tuple(out.shape) != (K, output_dim, pooled_size, pooled_size) or not out.is_contiguous():
        raise RuntimeError(f"{name}: a contiguous [{K}, {output_dim}, {pooled_size}, {pooled_size}] tensor is expected, got {tuple(out.shape)}")
    return bbox.contiguous(), t, ncls


def deform_psroi_pooling_forward(input, bbox, trans, out, top_count, no_trans, spatial_scale, output_dim, group_size, pooled_size, part_size,
                                 sample_per_part, trans_std):
    """writes out and top_count [K, output_dim, P, P]; float32 only"""
    r, t, ncls = _psroi_args("deform_psroi_pooling_forward", input, bbox, trans, out, no_trans, output_dim, pooled_size, part_size)
    L.require_cuda(top_count)
    _f32_only("deform_psroi_pooling_forward", top_count)
    if tuple(top_count.shape) != tuple(out.shape) or not top_count.is_contiguous():
        raise RuntimeError(f"deform_psroi_pooling_forward: top_count {tuple(top_count.shape)} must be contiguous and shaped like out")
    B, Ch, H, W = input.shape
    L.check(L.lib().abr_deform_psroi_forward(L.ptr(input), L.ptr(r), L.ptr(t), None, r.shape[0], B, Ch, H, W, float(spatial_scale), output_dim,
                                             group_size, pooled_size, part_size, sample_per_part, float(trans_std), ncls, L.NCHW, L.ptr(out),
                                             L.ptr(top_count), L.stream()), "deform_psroi_pooling_forward")


def deform_psroi_pooling_backward(out_grad, input, bbox, trans, top_count, input_grad, trans_grad, no_trans, spatial_scale, output_dim, group_size,
                                  pooled_size, part_size, sample_per_part, trans_std):
    """ADDS into input_grad (atomics) and writes trans_grad; float32 only"""
    name = "deform_psroi_pooling_backward"
    r, t, ncls = _psroi_args(name, input, bbox, trans, out_grad, no_trans, output_dim, pooled_size, part_size)
    L.require_cuda(top_count, input_grad)
    _f32_only(name, top_count, input_grad)
    if tuple(top_count.shape) != tuple(out_grad.shape) or not top_count.is_contiguous():
        raise RuntimeError(f"{name}: top_count {tuple(top_count.shape)} must be contiguous and shaped like out_grad")
    if tuple(input_grad.shape) != tuple(input.shape) or not input_grad.is_contiguous():
        raise RuntimeError(f"{name}: input_grad {tuple(input_grad.shape)} must be contiguous and shaped like input")
    gt = None
    if t is not None:
        L.require_cuda(trans_grad)
        _f32_only(name, trans_grad)
        if tuple(trans_grad.shape) != tuple(t.shape) or not trans_grad.is_contiguous():
            raise RuntimeError(f"{name}: trans_grad {tuple(trans_grad.shape)} must be contiguous and shaped like trans")
        gt = trans_grad
    B, Ch, H, W = input.shape
    L.check(L.lib().abr_deform_psroi_backward(L.ptr(out_grad), L.ptr(input), L.ptr(r), L.ptr(t), None, L.ptr(top_count), r.shape[0], B, Ch, H, W,
                                              float(spatial_scale), output_dim, group_size, pooled_size, part_size, sample_per_part, float(trans_std),
                                              ncls, L.NCHW, L.ptr(input_grad), L.ptr(gt), None, L.stream()), name)


# ------------------------------------------------------------------------------------------- deformable convolutions (csrc/deform_conv.h)
def _deform_shape_check(input, offset, grad_output, weight, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group):
    """shape_check of deform_conv_cuda.cu:70-159, in its order and with its wording -> (outputHeight, outputWidth)"""
    if weight.dim() != 4:
        raise RuntimeError(f"4D weight tensor (nOutputPlane,nInputPlane,kH,kW) expected, but got: {weight.dim()}")
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")
    if not (kW > 0 and kH > 0):
        raise RuntimeError(f"kernel size should be greater than zero, but got kH: {kH} kW: {kW}")
    if not (weight.size(2) == kH and weight.size(3) == kW):
        raise RuntimeError("kernel size should be consistent with weight, "
                           f"but got kH: {kH} kW: {kW} weight.size(2): {weight.size(2)}, weight.size(3): {weight.size(3)}")
    if not (dW > 0 and dH > 0):
        raise RuntimeError(f"stride should be greater than zero, but got dH: {dH} dW: {dW}")
    if not (dilationW > 0 and dilationH > 0):
        raise RuntimeError(f"dilation should be greater than 0, but got dilationH: {dilationH} dilationW: {dilationW}")
    if input.dim() != 4:   # (the reference also takes an unbatched 3D input and adds the batch dimension; this library does not)
        raise RuntimeError(f"3D or 4D input tensor expected but got: {input.dim()}")
    nInputPlane = weight.size(1) * group
    inputHeight, inputWidth = input.size(2), input.size(3)
    nOutputPlane = weight.size(0)
    outputHeight = (inputHeight + 2 * padH - (dilationH * (kH - 1) + 1)) // dH + 1
    outputWidth = (inputWidth + 2 * padW - (dilationW * (kW - 1) + 1)) // dW + 1
    if nInputPlane % deformable_group != 0:
        raise RuntimeError("input channels must divide deformable group size")
    if outputWidth < 1 or outputHeight < 1:
        raise RuntimeError(f"Given input size: ({nInputPlane} x {inputHeight} x {inputWidth}). "
                           f"Calculated output size: ({nOutputPlane} x {outputHeight} x {outputWidth}). Output size is too small")
    if input.size(1) != nInputPlane:
        raise RuntimeError(f"invalid number of input planes, expected: {nInputPlane}, but got: {input.size(1)}")
    if not (inputHeight >= kH and inputWidth >= kW):
        raise RuntimeError("input image is smaller than kernel")
    if not (offset.size(2) == outputHeight and offset.size(3) == outputWidth):
        raise RuntimeError(f"invalid spatial size of offset, expected height: {outputHeight} width: {outputWidth}, but "
                           f"got height: {offset.size(2)} width: {offset.size(3)}")
    if offset.size(1) != deformable_group * 2 * kH * kW:
        raise RuntimeError("invalid number of channels of offset")
    if grad_output is not None:
        if grad_output.size(1) != nOutputPlane:
            raise RuntimeError(f"invalid number of gradOutput planes, expected: {nOutputPlane}, but got: {grad_output.size(1)}")
        if not (grad_output.size(2) == outputHeight and grad_output.size(3) == outputWidth):
            raise RuntimeError(f"invalid size of gradOutput, expected height: {outputHeight} width: {outputWidth} , but "
                               f"got height: {grad_output.size(2)} width: {grad_output.size(3)}")
    if offset.size(0) != input.size(0):
        raise RuntimeError("invalid batch size of offset")   # deform_conv_cuda.cu:203
    return outputHeight, outputWidth


def _deform_written(name, what, t, shape):
    """a tensor one of these entry points writes: float32, on the device, contiguous NCHW of the expected shape (the reference views it)"""
    L.require_cuda(t)
    _f32_only(name, t)
    if tuple(t.shape) != tuple(shape) or not t.is_contiguous():
        raise RuntimeError(f"{name}: {what} must be a contiguous {tuple(shape)} tensor, got {tuple(t.shape)}")


def _deform_nhwc(*tensors):
    return [None if t is None else ops.nchw_to_nhwc(t.contiguous()) for t in tensors]


def _deform_v1_args(name, input, offset, grad_output, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group,
                    im2col_step):
    present = [t for t in (input, offset, grad_output, weight) if t is not None]
    L.require_cuda(*present)
    _f32_only(name, *present)
    _deform_shape_check(input, offset, grad_output, weight, kH, kW, dH, dW, padH, padW, dilationH, dilationW, group, deformable_group)
    if input.size(0) % im2col_step != 0:
        raise RuntimeError(f"{name}: im2col_step {im2col_step} does not divide the batch size {input.size(0)}")
    return dict(kernel=(kH, kW), stride=(dH, dW), padding=(padH, padW), dilation=(dilationH, dilationW), groups=group, dg=deformable_group)


def deform_conv_forward(input, weight, offset, output, columns, ones, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
                        deformable_group, im2col_step):
    """writes output [B, Cout, Ho, Wo]; columns and ones (the reference's scratch) are accepted and ignored; float32 only"""
    name = "deform_conv_forward"
    g = _deform_v1_args(name, input, offset, None, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group, im2col_step)
    Ho, Wo = offset.size(2), offset.size(3)
    _deform_written(name, "output", output, (input.size(0), weight.size(0), Ho, Wo))
    x, off, w = _deform_nhwc(input, offset, weight)
    y, _ = ops.deform_conv_forward(x, off, None, w, None, **g)
    L.check(L.lib().abr_nhwc_to_nchw(L.ptr(y), y.shape[0], y.shape[3], Ho, Wo, L.ptr(output), L.stream()), name)
    return 1


def deform_conv_backward_input(input, offset, gradOutput, gradInput, gradOffset, weight, columns, kW, kH, dW, dH, padW, padH, dilationW,
                               dilationH, group, deformable_group, im2col_step):
    """writes gradInput (like input) and gradOffset (like offset); float32 only"""
    name = "deform_conv_backward_input"
    g = _deform_v1_args(name, input, offset, gradOutput, weight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group,
                        im2col_step)
    _deform_written(name, "gradInput", gradInput, input.shape)
    _deform_written(name, "gradOffset", gradOffset, offset.shape)
    x, off, gy, w = _deform_nhwc(input, offset, gradOutput, weight)
    cols = ops.deform_im2col_general(x, off, None, **g)
    dx, d_off, _, _, _ = ops.deform_conv_backward(gy, x, off, None, w, cols, need_input=True, need_weight=False, **g)
    B, Ch, H, W = input.shape
    L.check(L.lib().abr_nhwc_to_nchw(L.ptr(dx), B, Ch, H, W, L.ptr(gradInput), L.stream()), name)
    L.check(L.lib().abr_nhwc_to_nchw(L.ptr(d_off), B, offset.size(1), offset.size(2), offset.size(3), L.ptr(gradOffset), L.stream()), name)
    return 1


def _deform_add_weight_grad(name, grad_weight, dw, scale):
    """grad_weight [Cout, C/groups, kh, kw] += scale * dw (OHWI)"""
    g = ops.nhwc_to_nchw(dw)
    if scale != 1:
        ops.scale_(g, float(scale))
    ops.add_(grad_weight, g)


def deform_conv_backward_parameters(input, offset, gradOutput, gradWeight, columns, ones, kW, kH, dW, dH, padW, padH, dilationW, dilationH,
                                    group, deformable_group, scale, im2col_step):
    """ADDS scale times the weight gradient into gradWeight (like weight, which it stands for in the shape check); float32 only"""
    name = "deform_conv_backward_parameters"
    g = _deform_v1_args(name, input, offset, gradOutput, gradWeight, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group,
                        im2col_step)
    x, off, gy = _deform_nhwc(input, offset, gradOutput)
    cols = ops.deform_im2col_general(x, off, None, **g)
    w = gradWeight.new_zeros((gradWeight.size(0), kH, kW, gradWeight.size(1)))     # (the weight's values play no part in its gradient)
    _, _, _, dw, _ = ops.deform_conv_backward(gy, x, off, None, w, cols, need_input=False, need_weight=True, **g)
    _deform_add_weight_grad(name, gradWeight, dw, scale)
    return 1


def _deform_v2_args(name, input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                    deformable_group, with_bias, more=()):
    tensors = [input, weight, offset, mask] + ([bias] if with_bias else []) + list(more)
    L.require_cuda(*tensors)
    _f32_only(name, *tensors)
    if not input.is_contiguous():
        raise RuntimeError("input tensor has to be contiguous")    # deform_conv_cuda.cu:507
    if not weight.is_contiguous():
        raise RuntimeError("weight tensor has to be contiguous")   # :508
    if weight.size(2) != kernel_h or weight.size(3) != kernel_w:   # :520-522 (its own argument order)
        raise RuntimeError(f"Input shape and kernel shape wont match: ({weight.size(2)} x {kernel_w} vs {weight.size(2)} x {weight.size(3)}).")
    if input.size(1) != weight.size(1) * group:                    # :523-525
        raise RuntimeError(f"Input shape and kernel channels wont match: ({input.size(1)} vs {weight.size(1) * group}).")
    geom = dict(kernel=(kernel_h, kernel_w), stride=(stride_h, stride_w), padding=(pad_h, pad_w), dilation=(dilation_h, dilation_w))
    Ho, Wo = ops.deform_out_size(input.size(2), input.size(3), **geom)
    B, K = input.size(0), kernel_h * kernel_w
    if tuple(offset.shape) != (B, deformable_group * 2 * K, Ho, Wo):
        raise RuntimeError(f"{name}: offset {tuple(offset.shape)} is not {(B, deformable_group * 2 * K, Ho, Wo)}")
    if tuple(mask.shape) != (B, deformable_group * K, Ho, Wo):
        raise RuntimeError(f"{name}: mask {tuple(mask.shape)} is not {(B, deformable_group * K, Ho, Wo)}")
    if with_bias and tuple(bias.shape) != (weight.size(0),):
        raise RuntimeError(f"{name}: bias {tuple(bias.shape)} is not {(weight.size(0),)}")
    geom.update(groups=group, dg=deformable_group)
    return geom, (B, weight.size(0), Ho, Wo)


def modulated_deform_conv_forward(input, weight, bias, ones, offset, mask, output, columns, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w,
                                  dilation_h, dilation_w, group, deformable_group, with_bias):
    """writes output [B, Cout, Ho, Wo]; ones and columns are accepted and ignored, and so is bias unless with_bias; float32 only"""
    name = "modulated_deform_conv_forward"
    g, out_shape = _deform_v2_args(name, input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                   dilation_w, group, deformable_group, with_bias)
    _deform_written(name, "output", output, out_shape)
    x, off, m, w = _deform_nhwc(input, offset, mask, weight)
    y, _ = ops.deform_conv_forward(x, off, m, w, bias.contiguous() if with_bias else None, **g)
    L.check(L.lib().abr_nhwc_to_nchw(L.ptr(y), out_shape[0], out_shape[1], out_shape[2], out_shape[3], L.ptr(output), L.stream()), name)


def modulated_deform_conv_backward(input, weight, bias, ones, offset, mask, columns, grad_input, grad_weight, grad_bias, grad_offset, grad_mask,
                                   grad_output, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h, dilation_w, group,
                                   deformable_group, with_bias):
    """ADDS into grad_weight and (with_bias) grad_bias; writes grad_input, grad_offset and grad_mask; float32 only"""
    name = "modulated_deform_conv_backward"
    g, out_shape = _deform_v2_args(name, input, weight, bias, offset, mask, kernel_h, kernel_w, stride_h, stride_w, pad_h, pad_w, dilation_h,
                                   dilation_w, group, deformable_group, with_bias, more=(grad_output,))
    if tuple(grad_output.shape) != out_shape:
        raise RuntimeError(f"{name}: grad_output {tuple(grad_output.shape)} is not {out_shape}")
    for what, t, like in (("grad_input", grad_input, input), ("grad_weight", grad_weight, weight), ("grad_offset", grad_offset, offset),
                          ("grad_mask", grad_mask, mask)) + ((("grad_bias", grad_bias, bias),) if with_bias else ()):
        _deform_written(name, what, t, like.shape)
    x, off, m, w, gy = _deform_nhwc(input, offset, mask, weight, grad_output)
    cols = ops.deform_im2col_general(x, off, m, **g)
    dx, d_off, d_m, dw, db = ops.deform_conv_backward(gy, x, off, m, w, cols, need_input=True, need_weight=True, need_bias=bool(with_bias), **g)
    for src, dst in ((dx, grad_input), (d_off, grad_offset), (d_m, grad_mask)):
        L.check(L.lib().abr_nhwc_to_nchw(L.ptr(src), dst.size(0), dst.size(1), dst.size(2), dst.size(3), L.ptr(dst), L.stream()), name)
    _deform_add_weight_grad(name, grad_weight, dw, 1)
    if with_bias:
        ops.add_(grad_bias, db)

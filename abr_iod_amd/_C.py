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

The RoI poolers take float32 and float64 like the reference's dispatch, the deformable pair float32 only; anything else raises
RuntimeError naming the dtype.  deform_conv_* / modulated_deform_conv_* are not carried (the body's DCN runs specialised kernels).

CPU tensors raise RuntimeError (the reference raises "Not compiled with GPU support" the other way round):
this library is MI355X-only by design; the CPU restatement lives in oracle/ and is test infrastructure.
"""
import torch

from . import _lib as L

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

"""Functional host API over the C ABI in the library's NATIVE layout (NHWC activations, OHWI weights).

Thin: shape bookkeeping + output allocation (torch = device-memory plumbing) + one C-ABI call each.
The reference-shaped wrappers (autograd Functions, nn.Modules with the reference's names) live in
abr_iod_amd/layers and abr_iod_amd/modeling and are built from these.
"""
import ctypes as C
import os
import threading

import torch

from . import _lib as L

_f32 = torch.float32


def _empty(shape, like, dtype=_f32):
    return torch.empty(shape, dtype=dtype, device=like.device)


def _cached_workspace(cache, nbytes, device, floor):
    """a uint8 workspace of at least `nbytes` (`floor` when first made) that the op keeps between calls: one per (device, stream) -- calls on
    one stream are ordered, and the source and target models may run on different streams"""
    key = (device, L.stream())
    ws = cache.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = cache[key] = torch.empty((max(nbytes, floor),), dtype=torch.uint8, device=device)
    return ws


# ----------------------------------------------------------------------------------------------- ROIAlign
def roi_align_forward(feat, rois, spatial_scale, ph, pw, sampling_ratio, bin_step=1, out=None):
    """feat [B,H,W,C], rois [K,5] -> [K, ceil(ph/step), ceil(pw/step), C] (written into `out`, a contiguous tensor of that shape, when given)"""
    L.require_cuda(feat, rois)
    feat, rois = L.f32c(feat), L.f32c(rois)
    B, H, W, Ch = feat.shape
    K = rois.shape[0]
    pho, pwo = -(-ph // bin_step), -(-pw // bin_step)
    if out is None:
        out = _empty((K, pho, pwo, Ch), feat)
    else:
        assert tuple(out.shape) == (K, pho, pwo, Ch) and out.is_contiguous() and out.dtype == _f32
    L.check(L.lib().abr_roi_align_forward(L.ptr(feat), L.ptr(rois), K, B, Ch, H, W, float(spatial_scale), ph, pw,
                                          sampling_ratio, bin_step, L.NHWC, L.ptr(out), L.stream()), "roi_align_forward")
    return out


_roi_bwd_ws = {}


def roi_align_backward(grad, rois, spatial_scale, ph, pw, sampling_ratio, B, H, W, Ch, bin_step=1, out=None, method="gather"):
    """grad [K,pho,pwo,C] -> grad_feat [B,H,W,C]; accumulates into `out` when given.
    method 'gather' = atomic-free two-kernel form (default), 'scatter' = per-RoI atomics (abr_roi_align_backward)."""
    L.require_cuda(grad, rois)
    grad, rois = L.f32c(grad), L.f32c(rois)
    K = rois.shape[0]
    acc = out is not None
    if out is None:
        out = _empty((B, H, W, Ch), grad)
    if method == "gather" and Ch % 4 == 0 and -(-ph // bin_step) <= 8 and -(-pw // bin_step) <= 8:
        nbytes = L.lib().abr_roi_align_backward_ws_bytes(K, B, H, W, ph, pw, bin_step)
        ws = _cached_workspace(_roi_bwd_ws, nbytes, grad.device, 1 << 20)
        L.check(L.lib().abr_roi_align_backward_gather(L.ptr(grad), L.ptr(rois), K, B, Ch, H, W, float(spatial_scale), ph, pw,
                                                      sampling_ratio, bin_step, int(acc), L.ptr(out), L.ptr(ws), ws.numel(),
                                                      L.stream()), "roi_align_backward_gather")
        amax_drop(out)
        return out
    L.check(L.lib().abr_roi_align_backward(L.ptr(grad), L.ptr(rois), K, B, Ch, H, W, float(spatial_scale), ph, pw,
                                           sampling_ratio, bin_step, L.NHWC, int(acc), L.ptr(out), L.stream()),
            "roi_align_backward")
    amax_drop(out)
    return out


def roi_align_taps(rois, H, W, spatial_scale, ph, pw, sampling_ratio, max_s):
    rois = L.f32c(rois)
    K = rois.shape[0]
    idx = torch.empty((K, ph * pw, max_s, 4), dtype=torch.int32, device=rois.device)
    grid = torch.empty((K, 2), dtype=torch.int32, device=rois.device)
    L.check(L.lib().abr_roi_align_taps(L.ptr(rois), K, H, W, float(spatial_scale), ph, pw, sampling_ratio, max_s,
                                       L.ptr(idx), L.ptr(grid), L.stream()), "roi_align_taps")
    return idx, grid


# ----------------------------------------------------------------------------------------------- ROIAlign over a feature pyramid
MAX_PYRAMID_LEVELS = 8   # ABR_MAX_PYRAMID_LEVELS


def fpn_levels(rois, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
    """rois [K,5] -> int32 [K]: the pyramid level of every row (modeling/poolers.py:37-42 in fp32), -1 for a row without one (NaN or negative area)"""
    L.require_cuda(rois)
    rois = L.f32c(rois)
    K = rois.shape[0]
    levels = torch.empty((K,), dtype=torch.int32, device=rois.device)
    L.check(L.lib().abr_fpn_levels(L.ptr(rois), K, float(k_min), float(k_max), float(canonical_scale), float(canonical_level), float(eps),
                                   L.ptr(levels), L.stream()), "fpn_levels")
    return levels


def _pyramid_tables(what, tensors, shapes, scales):
    """the host arrays of the pyramid entry points: (pointers, H, W, scales) of `tensors`, a list of contiguous fp32 [B,H_l,W_l,C] device tensors"""
    n = len(shapes)
    if not 1 <= n <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"{what}: {n} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    if len(scales) != n:
        raise RuntimeError(f"{what}: {len(scales)} scales for {n} levels")
    return ((C.c_void_p * n)(*[t.data_ptr() for t in tensors]), (C.c_int * n)(*[s[1] for s in shapes]), (C.c_int * n)(*[s[2] for s in shapes]),
            (C.c_float * n)(*[float(s) for s in scales]))


def _pyramid_check(what, feats, name="feats"):
    """B, C, device and dtype agree across the levels -> (B, C)"""
    if not 1 <= len(feats) <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"{what}: {name} has {len(feats)} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    f0 = feats[0]
    for l, f in enumerate(feats):
        if not f.is_cuda:
            raise RuntimeError(f"{what}: {name}[{l}] is a CPU tensor; abr_iod_amd ops need device tensors")
        if f.dtype != _f32:
            raise RuntimeError(f"{what}: {name}[{l}] has dtype {f.dtype}, expected float32")
        if f.dim() != 4 or not f.is_contiguous():
            raise RuntimeError(f"{what}: {name}[{l}] must be a contiguous [B,H,W,C] tensor, got shape {tuple(f.shape)}")
        if f.device != f0.device:
            raise RuntimeError(f"{what}: device of {name}[{l}] is {f.device}, of {name}[0] {f0.device}")
        if f.shape[0] != f0.shape[0]:
            raise RuntimeError(f"{what}: B of {name}[{l}] is {f.shape[0]}, of {name}[0] {f0.shape[0]}")
        if f.shape[3] != f0.shape[3]:
            raise RuntimeError(f"{what}: C of {name}[{l}] is {f.shape[3]}, of {name}[0] {f0.shape[3]}")
    return f0.shape[0], f0.shape[3]


def _pyramid_rows(what, rows, rois):
    """the device row list of the indexed pyramid calls: int64 [P], contiguous, on the table's device"""
    if not torch.is_tensor(rows) or rows.dtype != torch.int64 or rows.dim() != 1:
        raise RuntimeError(f"{what}: rows must be a one-dimensional int64 tensor")
    if rows.device != rois.device:
        raise RuntimeError(f"{what}: rows is on {rows.device}, rois on {rois.device}")
    return rows.contiguous()


def roi_align_pyramid_forward(feats, rois, scales, ph, pw, sampling_ratio, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6,
                              out=None, want_levels=False, rows=None):
    """feats: list of contiguous [B,H_l,W_l,C], rois [K,5] -> [K,ph,pw,C] in ONE launch (written into `out` when given): every row pooled on
    the level fpn_levels gives it, all zero for a row without one.  want_levels: -> (out, int32 [K] levels).  The result carries no amax
    tag: its rows come from maps with different amax words (modeling.poolers.Pooler tags it with their maximum: amax_bound_levels).
    rows: int64 [P] on the device -> [P,ph,pw,C] (and [P] levels), out[p] = the bits row rows[p] of the table gets without `rows`; an entry
    < 0 or >= K is padding: all zero, level -1, its table row never read."""
    what = "roi_align_pyramid_forward"
    feats = list(feats)
    B, Ch = _pyramid_check(what, feats)
    L.require_cuda(rois)
    rois = L.f32c(rois)
    K = rois.shape[0]
    if rows is not None:
        rows = _pyramid_rows(what, rows, rois)
    N = K if rows is None else rows.shape[0]
    if out is None:
        out = _empty((N, ph, pw, Ch), rois)
    else:
        assert tuple(out.shape) == (N, ph, pw, Ch) and out.is_contiguous() and out.dtype == _f32
    levels = torch.empty((N,), dtype=torch.int32, device=rois.device) if want_levels else None
    fp, Hs, Ws, sc = _pyramid_tables(what, feats, [f.shape for f in feats], scales)
    rule = (float(k_min), float(k_max), float(canonical_scale), float(canonical_level), float(eps))
    if rows is None:
        rc = L.lib().abr_roi_align_pyramid_forward(fp, Hs, Ws, sc, len(feats), L.ptr(rois), K, B, Ch, ph, pw, sampling_ratio, *rule, L.ptr(out),
                                                   L.ptr(levels), L.stream())
    else:
        rc = L.lib().abr_roi_align_pyramid_rows_forward(fp, Hs, Ws, sc, len(feats), L.ptr(rois), K, L.ptr(rows), N, B, Ch, ph, pw, sampling_ratio,
                                                        *rule, L.ptr(out), L.ptr(levels), L.stream())
    L.check(rc, what)
    amax_drop(out)
    return (out, levels) if want_levels else out


def roi_align_pyramid_backward(grad, rois, scales, ph, pw, sampling_ratio, shapes, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6,
                               out=None, rows=None):
    """grad [K,ph,pw,C], shapes: the [B,H_l,W_l,C] of every level -> list of grad_feat [B,H_l,W_l,C]: one launch over the RoIs adds into
    float64 scratch with hardware atomics (their order varies from run to run), a second rounds every level's sums to fp32 once; every level is
    written whole, reached or not, unless the list `out` is given: then it accumulates.
    rows: int64 [P] on the device, grad [P,ph,pw,C]: grad[p] belongs to row rows[p] of the table; a padding entry (< 0 or >= K) adds nothing
    and its grad row is not read."""
    what = "roi_align_pyramid_backward"
    L.require_cuda(grad, rois)
    grad, rois = L.f32c(grad), L.f32c(rois)
    K = rois.shape[0]
    if rows is not None:
        rows = _pyramid_rows(what, rows, rois)
    N = K if rows is None else rows.shape[0]
    shapes = [tuple(int(v) for v in s) for s in shapes]
    acc = out is not None
    if out is None:
        out = [_empty(s, grad) for s in shapes]
    else:
        out = list(out)
        if [tuple(o.shape) for o in out] != shapes:
            raise RuntimeError(f"{what}: out has shapes {[tuple(o.shape) for o in out]}, expected {shapes}")
    B, Ch = _pyramid_check(what, out, "out")
    if tuple(grad.shape) != (N, ph, pw, Ch):
        raise RuntimeError(f"{what}: grad {tuple(grad.shape)} is not [{N}, {ph}, {pw}, {Ch}]")
    gp, Hs, Ws, sc = _pyramid_tables(what, out, shapes, scales)
    rule = (float(k_min), float(k_max), float(canonical_scale), float(canonical_level), float(eps))
    if rows is None:
        rc = L.lib().abr_roi_align_pyramid_backward(L.ptr(grad), L.ptr(rois), K, B, Ch, Hs, Ws, sc, len(out), ph, pw, sampling_ratio, *rule, int(acc),
                                                    gp, L.stream())
    else:
        rc = L.lib().abr_roi_align_pyramid_rows_backward(L.ptr(grad), L.ptr(rois), L.ptr(rows), N, K, B, Ch, Hs, Ws, sc, len(out), ph, pw,
                                                         sampling_ratio, *rule, int(acc), gp, L.stream())
    L.check(rc, what)
    for o in out:
        amax_drop(o)
    return out


# ----------------------------------------------------------------------------------------------- the FPN neck (csrc/fpn.hip)
def _fpn_levels_check(what, maps, name):
    """`maps`: the levels' contiguous fp32 [B,H_l,W_l,C] device tensors (None where the caller allows it) -> (B, C), C a multiple of 4"""
    B, Ch = _pyramid_check(what, [m for m in maps if m is not None], name)
    if Ch % 4:
        raise ValueError(f"{what}: C = {Ch} is not a multiple of 4")
    return B, Ch


def _fpn_shapes_check(what, shapes):
    """every level exactly twice the next coarser one, else ValueError before any launch (the reference's `lateral + upsampled` raises there too)"""
    for l in range(len(shapes) - 1):
        (_, h, w, _), (_, h1, w1, _) = shapes[l], shapes[l + 1]
        if h != 2 * h1 or w != 2 * w1:
            raise ValueError(f"{what}: level {l} is {h} x {w}, not twice level {l + 1}'s {h1} x {w1}")


def fpn_topdown_forward(laterals):
    """laterals: list of contiguous [B,H_l,W_l,C], finest first -> the list of inners, inner_l = lateral_l + nearest-upsampled inner_{l+1}, in ONE
    launch; the top inner IS the top lateral (the same tensor).  Bit-equal to the level-by-level lateral + F.interpolate(.., scale_factor=2)."""
    lats = list(laterals)
    B, Ch = _fpn_levels_check("fpn_topdown_forward", lats, "laterals")
    shapes = [tuple(t.shape) for t in lats]
    _fpn_shapes_check("fpn_topdown_forward", shapes)
    n = len(lats)
    inners = [torch.empty_like(t) for t in lats[:-1]] + [lats[-1]]
    if n > 1:
        L.check(L.lib().abr_fpn_topdown_forward((C.c_void_p * n)(*[t.data_ptr() for t in lats]), (C.c_void_p * n)(*[t.data_ptr() for t in inners]),
                                                (C.c_int * n)(*[s[1] for s in shapes]), (C.c_int * n)(*[s[2] for s in shapes]), n, B, Ch, L.stream()),
                "fpn_topdown_forward")
    return inners


def fpn_topdown_backward(grads, inplace=False):
    """grads: the gradients arriving at inner_0 .. inner_{L-1} (contiguous [B,H_l,W_l,C]; None past level 0 = none arrives) -> the list of
    lateral gradients T_l, T_0 = g_0, T_l = g_l + ((T_{l-1}(2y,2x) + T_{l-1}(2y,2x+1)) + (T_{l-1}(2y+1,2x) + T_{l-1}(2y+1,2x+1))), in ONE launch
    and this fixed order.  T_0 is g_0 itself; inplace: every T_l is written over g_l (a level without g_l still gets a new tensor)."""
    gs = list(grads)
    if not gs or gs[0] is None:
        raise ValueError("fpn_topdown_backward: the finest level's gradient is missing (start the list at the finest level that has one)")
    B, Ch = _fpn_levels_check("fpn_topdown_backward", gs, "grads")
    g0 = gs[0]
    shapes = [tuple(g0.shape)]
    for l in range(1, len(gs)):
        shapes.append(tuple(gs[l].shape) if gs[l] is not None else (B, shapes[-1][1] // 2, shapes[-1][2] // 2, Ch))
    _fpn_shapes_check("fpn_topdown_backward", shapes)
    n = len(gs)
    outs = [g0] + [g if (inplace and g is not None) else _empty(s, g0) for g, s in zip(gs[1:], shapes[1:])]
    if n > 1:
        L.check(L.lib().abr_fpn_topdown_backward((C.c_void_p * n)(*[L.ptr(g) for g in gs]), (C.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                                 (C.c_int * n)(*[s[1] for s in shapes]), (C.c_int * n)(*[s[2] for s in shapes]), n, B, Ch, L.stream()),
                "fpn_topdown_backward")
        for t in outs[1:]:
            amax_drop(t)
    return outs


def fpn_subsample2(x):
    """LastLevelMaxPool, F.max_pool2d(x, 1, 2, 0): x [B,H,W,C] -> [B,(H-1)//2+1,(W-1)//2+1,C], out(y,x) = x(2y,2x)"""
    L.require_cuda(x)
    x = L.f32c(x)
    B, H, W, Ch = x.shape
    out = _empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Ch), x)
    L.check(L.lib().abr_fpn_subsample2_forward(L.ptr(x), B, H, W, Ch, L.ptr(out), L.stream()), "fpn_subsample2_forward")
    return out


def fpn_subsample2_backward(g_out, shape, g_in=None, inplace=False):
    """g_out [B,Ho,Wo,C], shape = x's [B,H,W,C] -> g_x = g_in (None: zero) + g_out scattered to the even pixels, every element written once;
    inplace: g_x is written over g_in"""
    L.require_cuda(g_out, g_in)
    g_out = L.f32c(g_out)
    B, H, W, Ch = (int(v) for v in shape)
    if tuple(g_out.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Ch):
        raise ValueError(f"fpn_subsample2_backward: g_out {tuple(g_out.shape)} is not the subsampled shape of {(B, H, W, Ch)}")
    if g_in is not None:
        if tuple(g_in.shape) != (B, H, W, Ch):
            raise ValueError(f"fpn_subsample2_backward: g_in {tuple(g_in.shape)} is not {(B, H, W, Ch)}")
        g_in = L.f32c(g_in)
    g_x = g_in if (inplace and g_in is not None) else _empty((B, H, W, Ch), g_out)
    L.check(L.lib().abr_fpn_subsample2_backward(L.ptr(g_out), L.ptr(g_in), B, H, W, Ch, L.ptr(g_x), L.stream()), "fpn_subsample2_backward")
    amax_drop(g_x)
    return g_x


# ----------------------------------------------------------------------------------------------- ROIPool, deformable PS-RoI pooling
def roi_pool_forward(feat, rois, spatial_scale, ph, pw, out=None):
    """feat [B,H,W,C], rois [K,5] -> (out [K,ph,pw,C], argmax int32 [K,ph,pw,C]: flat pixel h*W+w of the bin's first maximum, -1 for none);
    the values are written into `out`, a contiguous tensor of that shape, when given"""
    L.require_cuda(feat, rois)
    feat, rois = L.f32c(feat), L.f32c(rois)
    B, H, W, Ch = feat.shape
    K = rois.shape[0]
    if out is None:
        out = _empty((K, ph, pw, Ch), feat)
    else:
        assert tuple(out.shape) == (K, ph, pw, Ch) and out.is_contiguous() and out.dtype == _f32
    argmax = _empty((K, ph, pw, Ch), feat, torch.int32)
    L.check(L.lib().abr_roi_pool_forward(L.ptr(feat), L.ptr(rois), K, B, Ch, H, W, float(spatial_scale), ph, pw, L.NHWC, L.ptr(out), L.ptr(argmax),
                                         L.stream()), "roi_pool_forward")
    return out, argmax


def roi_pool_backward(grad, rois, argmax, B, H, W, out=None):
    """grad, argmax [K,ph,pw,C] -> grad_feat [B,H,W,C] (fp32 atomics); accumulates into `out` when given"""
    L.require_cuda(grad, rois, argmax)
    grad, rois = L.f32c(grad), L.f32c(rois)
    K, ph, pw, Ch = grad.shape
    if argmax.dtype != torch.int32 or tuple(argmax.shape) != tuple(grad.shape) or not argmax.is_contiguous():
        raise RuntimeError(f"roi_pool_backward: argmax must be a contiguous int32 tensor of grad's shape {tuple(grad.shape)}")
    acc = out is not None
    if out is None:
        out = _empty((B, H, W, Ch), grad)
    else:
        assert tuple(out.shape) == (B, H, W, Ch) and out.is_contiguous() and out.dtype == _f32
    L.check(L.lib().abr_roi_pool_backward(L.ptr(grad), L.ptr(rois), L.ptr(argmax), K, B, Ch, H, W, ph, pw, L.NHWC, int(acc), L.ptr(out), L.stream()),
            "roi_pool_backward")
    amax_drop(out)
    return out


def _psroi_operands(rois, trans, mask_logits, K, P, part):
    """(trans, num_classes, mask_logits) as the library takes them: trans [K, 2 num_classes, part, part] or None, mask_logits [K, P, P] or None"""
    ncls = 1
    if trans is not None:
        trans = L.f32c(trans)
        if trans.dim() != 4 or trans.shape[0] != K or trans.shape[1] % 2 or tuple(trans.shape[2:]) != (part, part):
            raise RuntimeError(f"deform_psroi: trans {tuple(trans.shape)} is not [{K}, 2 * num_classes, {part}, {part}]")
        ncls = trans.shape[1] // 2
    if mask_logits is not None:
        mask_logits = L.f32c(mask_logits)
        if mask_logits.numel() != K * P * P:
            raise RuntimeError(f"deform_psroi: mask_logits {tuple(mask_logits.shape)} is not [{K}, {P}, {P}]")
    return trans, ncls, mask_logits


def deform_psroi_forward(feat, rois, trans, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part, trans_std,
                         mask_logits=None, out=None):
    """feat [B,H,W,C], rois [K,5], trans [K, 2 num_classes, part, part] or None (no_trans), mask_logits [K,P,P] or None
    -> (out [K,P,P,output_dim], top_count of the same shape); out is multiplied by sigmoid(mask_logits) of its bin when they are given.
    The values are written into `out`, a contiguous tensor of that shape, when given."""
    L.require_cuda(feat, rois, trans, mask_logits)
    feat, rois = L.f32c(feat), L.f32c(rois)
    B, H, W, Ch = feat.shape
    K, P = rois.shape[0], pooled_size
    trans, ncls, mask_logits = _psroi_operands(rois, trans, mask_logits, K, P, part_size)
    if out is None:
        out = _empty((K, P, P, output_dim), feat)
    else:
        assert tuple(out.shape) == (K, P, P, output_dim) and out.is_contiguous() and out.dtype == _f32
    count = _empty((K, P, P, output_dim), feat)
    L.check(L.lib().abr_deform_psroi_forward(L.ptr(feat), L.ptr(rois), L.ptr(trans), L.ptr(mask_logits), K, B, Ch, H, W, float(spatial_scale),
                                             output_dim, group_size, P, part_size, sample_per_part, float(trans_std), ncls, L.NHWC, L.ptr(out),
                                             L.ptr(count), L.stream()), "deform_psroi_forward")
    return out, count


def deform_psroi_backward(grad, feat, rois, trans, top_count, spatial_scale, output_dim, group_size, pooled_size, part_size, sample_per_part,
                          trans_std, mask_logits=None, out=None):
    """-> (grad_feat [B,H,W,C] by fp32 atomics, ADDED into `out` when given; grad_trans like trans or None; grad_mask_logits [K,P,P] or None).
    The last two are bit-reproducible."""
    L.require_cuda(grad, feat, rois, trans, top_count, mask_logits)
    grad, feat, rois, top_count = L.f32c(grad), L.f32c(feat), L.f32c(rois), L.f32c(top_count)
    B, H, W, Ch = feat.shape
    K, P = rois.shape[0], pooled_size
    if tuple(grad.shape) != (K, P, P, output_dim) or tuple(top_count.shape) != tuple(grad.shape):
        raise RuntimeError(f"deform_psroi_backward: grad {tuple(grad.shape)} / top_count {tuple(top_count.shape)} are not {(K, P, P, output_dim)}")
    trans, ncls, mask_logits = _psroi_operands(rois, trans, mask_logits, K, P, part_size)
    if out is None:
        out = torch.zeros_like(feat)
    else:
        assert tuple(out.shape) == (B, H, W, Ch) and out.is_contiguous() and out.dtype == _f32
    gtrans = torch.empty_like(trans) if trans is not None else None
    gmask = _empty((K, P, P), feat) if mask_logits is not None else None
    L.check(L.lib().abr_deform_psroi_backward(L.ptr(grad), L.ptr(feat), L.ptr(rois), L.ptr(trans), L.ptr(mask_logits), L.ptr(top_count), K, B, Ch, H, W,
                                              float(spatial_scale), output_dim, group_size, P, part_size, sample_per_part, float(trans_std), ncls,
                                              L.NHWC, L.ptr(out), L.ptr(gtrans), L.ptr(gmask), L.stream()), "deform_psroi_backward")
    amax_drop(out)
    return out, gtrans, gmask


# ----------------------------------------------------------------------------------------------- NMS
_nms_ws = {}


def nms_sorted_batched(boxes, counts, thr, max_keep, strict_gt=False):
    """boxes [N,n,4] sorted by descending score per image, counts [N] int32 -> keep [N,max_keep] int32, n_keep [N]"""
    L.require_cuda(boxes, counts)
    boxes = L.f32c(boxes)
    N, n = boxes.shape[0], boxes.shape[1]
    keep = torch.empty((N, max(max_keep, 1)), dtype=torch.int32, device=boxes.device)
    n_keep = torch.empty((N,), dtype=torch.int32, device=boxes.device)
    ws_bytes = L.lib().abr_nms_workspace_bytes(N, n)
    ws = _cached_workspace(_nms_ws, ws_bytes, boxes.device, 8)
    L.check(L.lib().abr_nms_sorted_batched(L.ptr(boxes), L.ptr(counts), N, n, float(thr), int(strict_gt), max_keep,
                                           L.ptr(keep), L.ptr(n_keep), L.ptr(ws), ws_bytes, L.stream()), "nms")
    return keep, n_keep


# ----------------------------------------------------------------------------------------------- losses
def _ard_dims(f, layout):
    """(N, Ch, HW) of a feature map [N,...,C] (NHWC) or [N,C,...] (NCHW)"""
    if layout == L.NHWC:
        return f.shape[0], f.shape[-1], f.shape[1:-1].numel()
    return f.shape[0], f.shape[1], f.shape[2:].numel()


def ard_forward(f_src, f_tgt, gamma, layout=L.NHWC):
    """f_* [N,HW,C] (NHWC) -> (loss[4] = total, afd, pad, -), coef [N,2,HW])"""
    L.require_cuda(f_src, f_tgt)
    f_src, f_tgt = L.f32c(f_src), L.f32c(f_tgt)
    N, Ch, HW = _ard_dims(f_src, layout)
    loss = _empty((4,), f_src)
    coef = _empty((max(N, 1), 2, HW), f_src)
    L.check(L.lib().abr_ard_forward(L.ptr(f_src), L.ptr(f_tgt), N, Ch, HW, float(gamma), layout, L.ptr(coef),
                                    L.ptr(loss), L.stream()), "ard_forward")
    return loss, coef


def ard_backward(f_src, f_tgt, coef, gamma, gscale=1.0, gscale_dev=None, layout=L.NHWC):
    f_src, f_tgt = L.f32c(f_src), L.f32c(f_tgt)
    N, Ch, HW = _ard_dims(f_src, layout)
    grad = torch.empty_like(f_tgt)
    L.check(L.lib().abr_ard_backward(L.ptr(f_src), L.ptr(f_tgt), L.ptr(coef), N, Ch, HW, float(gamma), layout,
                                     float(gscale), L.ptr(gscale_dev), L.ptr(grad), L.stream()), "ard_backward")
    return grad


def smooth_l1(x, t, beta, scale=1.0, gscale=1.0, want_grad=False):
    L.require_cuda(x, t)
    x, t = L.f32c(x), L.f32c(t)
    loss = _empty((4,), x)
    grad = torch.empty_like(x) if want_grad else None
    L.check(L.lib().abr_smooth_l1(L.ptr(x), L.ptr(t), x.numel(), float(beta), float(scale), L.ptr(loss), float(gscale),
                                  L.ptr(grad), L.stream()), "smooth_l1")
    return loss, grad


def smooth_l1_rows(x, t, rows, col0, beta, scale=1.0, gscale=1.0, want_grad=False, trows=None, denom_dev=None):
    """sum over i of smoothL1(x[rows[i], col0[i]:col0[i]+4] - t[trows[i] (default rows[i]), :4]) * scale"""
    L.require_cuda(x, t, rows)
    x, t = L.f32c(x), L.f32c(t)
    loss = _empty((4,), x)
    grad = torch.zeros_like(x) if want_grad else None
    L.check(L.lib().abr_smooth_l1_rows(L.ptr(x), x.shape[1], L.ptr(t), L.ptr(rows), L.ptr(col0), L.ptr(trows), rows.numel(), float(beta),
                                       float(scale), L.ptr(denom_dev), L.ptr(loss), float(gscale), L.ptr(grad), L.stream()), "smooth_l1_rows")
    return loss, grad


def _rows2d(t):
    """2-D fp32 tensor whose rows are contiguous (column slices of a fused buffer are fine) -> (tensor, row pitch)"""
    if t.dtype != _f32:
        raise RuntimeError(f"expected float32, got {t.dtype}")
    if t.dim() != 2 or t.stride(1) != 1:
        t = t.reshape(t.shape[0], -1).contiguous()
    return t, t.stride(0) if t.shape[0] > 1 else t.shape[1]


def softmax_ce(logits, labels, inclusive=False, n_old=0, gscale=1.0, want_grad=False, grad_out=None):
    """grad_out: optional [n,>=K]-pitched view to receive d_logits (e.g. a column slice of the fused grad buffer)"""
    L.require_cuda(logits, labels)
    logits, ldz = _rows2d(logits)
    labels = labels.contiguous()
    loss = _empty((4,), logits)
    grad = None
    if want_grad:
        grad = grad_out if grad_out is not None else torch.empty((logits.shape[0], logits.shape[1]), dtype=_f32, device=logits.device)
    ldg = grad.stride(0) if grad is not None and grad.shape[0] > 1 else logits.shape[1]
    L.check(L.lib().abr_softmax_ce(L.ptr(logits), ldz, L.ptr(labels), logits.shape[0], logits.shape[1], int(inclusive), n_old,
                                   L.ptr(loss), float(gscale), L.ptr(grad), ldg, L.stream()), "softmax_ce")
    return loss, grad


def roi_distill(z_s, b_s, z_t, b_t, dist_id=True, gscale=1.0, want_grad=False, d_zt=None, d_bt=None):
    """z_s [n,K_old], b_s [n,K_old,4], z_t [n,K_all], b_t [n,K_all,4]; any of them may be a column slice of a fused
    [n,ld] buffer (rows contiguous).  d_zt / d_bt: optional pre-made (possibly sliced) gradient destinations."""
    L.require_cuda(z_s, b_s, z_t, b_t)
    n, K_old, K_all = z_t.shape[0], z_s.shape[1], z_t.shape[1]
    z_s, l0 = _rows2d(z_s)
    b_s, l1 = _rows2d(b_s.reshape(n, K_old * 4) if b_s.dim() == 3 else b_s)
    z_t, l2 = _rows2d(z_t)
    b_t, l3 = _rows2d(b_t.reshape(n, K_all * 4) if b_t.dim() == 3 else b_t)
    loss = _empty((4,), z_t)
    if want_grad:
        d_zt = d_zt if d_zt is not None else torch.empty((n, K_all), dtype=_f32, device=z_t.device)
        d_bt = d_bt if d_bt is not None else torch.empty((n, K_all * 4), dtype=_f32, device=z_t.device)
    else:
        d_zt = d_bt = None
    l4 = d_zt.stride(0) if d_zt is not None and n > 1 else K_all
    l5 = d_bt.stride(0) if d_bt is not None and n > 1 else K_all * 4
    ld = (C.c_int32 * 6)(l0, l1, l2, l3, l4, l5)
    L.check(L.lib().abr_roi_distill(L.ptr(z_s), L.ptr(b_s), L.ptr(z_t), L.ptr(b_t), n, K_old, K_all, C.cast(ld, C.c_void_p),
                                    int(dist_id), L.ptr(loss), float(gscale), L.ptr(d_zt), L.ptr(d_bt), L.stream()), "roi_distill")
    return loss, d_zt, d_bt


def bce_logits_gather(x, y, idx, gscale=1.0, want_grad=False, yidx=None, denom_dev=None):
    L.require_cuda(x, y, idx)
    x, y = L.f32c(x), L.f32c(y)
    loss = _empty((4,), x)
    grad = torch.zeros_like(x) if want_grad else None
    L.check(L.lib().abr_bce_logits_gather(L.ptr(x), L.ptr(y), L.ptr(idx), L.ptr(yidx), idx.numel(), L.ptr(denom_dev), L.ptr(loss), float(gscale),
                                          L.ptr(grad), L.stream()), "bce_logits_gather")
    return loss, grad


# ----------------------------------------------------------------------------------------------- conv
MATH_F32, MATH_BF16, MATH_BF16X6, MATH_F16X3, MATH_F16 = 0, 1, 2, 3, 4   # abr_conv_desc::math (include/abr_iod_hip.h)
X6_FLAG_TINY, X6_FLAG_NONFINITE = 1, 2       # ABR_X6_FLAG_*
H3_FLAG_STALE = 8                            # ABR_H3_FLAG_STALE


CONV_MATH = {"f32": MATH_F32, "bf16x6": MATH_BF16X6, "f16x3": MATH_F16X3, "f16": MATH_F16}
DEFAULT_CONV_MATH = "f16x3"                  # the library's default arithmetic; ABR_CONV_MATH overrides it


def default_conv_math():
    """abr_conv_desc::math of ABR_CONV_MATH (f32, bf16x6 or f16x3; default DEFAULT_CONV_MATH): the arithmetic of a contraction outside a model,
    which has no GeneralizedRCNN.set_conv_math to choose it"""
    name = os.environ.get("ABR_CONV_MATH", DEFAULT_CONV_MATH)
    if name not in ("f32", "bf16x6", "f16x3"):
        raise ValueError("ABR_CONV_MATH must be f32, bf16x6 or f16x3, got {!r}".format(name))
    return CONV_MATH[name]


def uses_amax(math):
    """the arithmetic scales its operands by their amax words (f16x3, and f16 = its one-product rounded form)"""
    return math == MATH_F16X3 or math == MATH_F16

# ---- f16x3 (MATH_F16X3): amax words.  A tensor's amax word (include/abr_iod_hip.h, abr_conv_desc) rides on the torch.Tensor OBJECT the producing
# op returned, as `_abr_amax` = (word address, epoch, data_ptr, tensor version, allocation count): valid only while that object still names the
# same bytes (same storage address, no in-place write since) and the library's ring has not wrapped past it.  A consumer that finds no valid tag
# lets the library reduce the tensor itself (one extra pass over it: always correct).  ABR_H3_TAGS=0: never tag (every consumer reduces).
H3_TAGS = os.environ.get("ABR_H3_TAGS", "1") != "0"
_AMAX_RING = 65536
_amax_count = [0]
amax_reductions = [0, 0]   # (calls, bytes) of amax_compute: operands whose producer did not emit an amax word (bench.py reports them per step)


_AMAX_BLOCK = 512
_amax_block = {"it": iter(()), "base": 0}
_amax_lock = threading.Lock()


def amax_new():
    """a fresh amax word of the library's ring: (address, epoch).  Words come in blocks of _AMAX_BLOCK consecutive allocations
    (abr_h3_amax_alloc_block) handed out here: one library call per block instead of one per tensor (~200 per training step)."""
    try:
        c = next(_amax_block["it"])       # (atomic under the GIL: the forward pass and autograd's thread both allocate)
    except StopIteration:
        with _amax_lock:
            try:
                c = next(_amax_block["it"])
            except StopIteration:
                base, first = C.c_void_p(0), C.c_uint64(0)
                L.check(L.lib().abr_h3_amax_alloc_block(_AMAX_BLOCK, C.byref(base), C.byref(first)), "h3_amax_alloc_block")
                _amax_block["base"] = int(base.value)
                it = iter(range(int(first.value), int(first.value) + _AMAX_BLOCK))
                c = next(it)
                _amax_block["it"] = it
    _amax_count[0] += 1
    return _amax_block["base"] + (c % _AMAX_RING) * 8, (c + 1) & 0xFFFFFFFF


def amax_tag(t, word, epoch, stream=None):
    """remember that `word` (epoch) holds max |t| -- called by the op that just produced t with that word as its out_amax.  stream: the word
    was written by a reduction queued on that stream AFTER t was produced (amax_compute): only consumers on the same stream are ordered
    behind it; a producer's own word (stream=None) is as ordered as the tensor's bytes."""
    t._abr_amax = (word, epoch, t.data_ptr(), t._version, _amax_count[0], stream)
    return t


def amax_of(t):
    """(word, epoch) of t's amax if t still carries a valid tag, else (None, 0)"""
    tag = getattr(t, "_abr_amax", None)
    if (tag is not None and tag[2] == t.data_ptr() and tag[3] == t._version and _amax_count[0] - tag[4] < _AMAX_RING // 4
            and (tag[5] is None or tag[5] == L.stream())):
        return tag[0], tag[1]
    return None, 0


def amax_carry(dst, src):
    """dst is another view of exactly src's elements (permute / reshape of the whole tensor): it inherits the tag"""
    tag = getattr(src, "_abr_amax", None)
    if tag is not None and tag[2] == dst.data_ptr() and dst.numel() == src.numel():
        dst._abr_amax = (tag[0], tag[1], tag[2], dst._version, tag[4], tag[5])
    return dst


def amax_carry_bound(dst, src):
    """dst holds a subset / masked copy of src's values in fresh memory: src's amax is an upper bound of dst's"""
    w, e = amax_of(src)
    if w is not None:
        dst._abr_amax = (w, e, dst.data_ptr(), dst._version, src._abr_amax[4], src._abr_amax[5])
    return dst


def amax_drop(t):
    """t was written in place by a raw kernel: whatever tag it carried no longer describes it (nor does the "zero except the pixels of a
    strided scatter" mark: add_ fills the holes, and scale_ by inf / nan would too)"""
    if getattr(t, "_abr_amax", None) is not None:
        t._abr_amax = None
    if getattr(t, "_abr_scatter", None) is not None:
        t._abr_scatter = None
    return t


def amax_compute(t):
    """reduce max |t| into a fresh word on the current stream and tag t with it"""
    t = L.f32c(t)
    w, e = amax_new()
    st = L.stream()
    L.check(L.lib().abr_h3_amax(L.ptr(t), t.numel(), w, e, st), "h3_amax")
    amax_reductions[0] += 1
    amax_reductions[1] += t.numel() * 4
    return amax_tag(t, w, e, st)


def amax_bound_levels(dst, srcs):
    """dst holds, in fresh memory, values each bounded by one of the tensors `srcs` (the multi-level Pooler's output: a row is an average of
    bilinear samples of ONE level's map): tag it with a fresh word holding the largest of their amax words (abr_h3_amax_max, one tiny launch
    on the current stream) -- amax_carry_bound for more than one source.  If any source has no valid tag, dst stays untagged."""
    if not H3_TAGS or not 1 <= len(srcs) <= MAX_PYRAMID_LEVELS:
        return dst
    refs = [amax_of(s) for s in srcs]
    if any(w is None for w, _ in refs):
        return dst
    streams = {s._abr_amax[5] for s in srcs} - {None}
    st = L.stream()
    if streams - {st}:       # (a word reduced on another stream is not ordered before this launch)
        return dst
    n = len(refs)
    words = (C.c_void_p * n)(*[w for w, _ in refs])
    epochs = (C.c_uint32 * n)(*[e for _, e in refs])
    w, e = amax_new()
    L.check(L.lib().abr_h3_amax_max(C.cast(words, C.c_void_p), C.cast(epochs, C.c_void_p), n, w, e, st), "h3_amax_max")
    return amax_tag(dst, w, e, st if streams else None)


# ---- the conv amax-word protocol: every conv call path (conv_forward, conv_wgrad[_async], conv_backward, resnet._FwdPlan) decides its words here.
# Where the paths differ on purpose: conv_forward(emit_amax=True) emits under any arithmetic, conv_backward's dgrad only under those that read
# the words (it has no such argument); _FwdPlan gives the downsample branch's output no word (it lives in the table's temporaries, and nothing
# contracts over it), the per-conv path tags that tensor like any fresh result.
def amax_operand(t, reduce=True):
    """(word, epoch) of a contraction operand: its tag while valid -- also with H3_TAGS off; else, with H3_TAGS on and `reduce`, a reduction
    queued here, on the current stream, which must be the one that produced t (a side stream's wait is recorded AFTER this); else (None, 0):
    the library reduces t inside the call.  A contiguous copy the caller had to make is a new object without a tag, so it is reduced even
    where the original carried one."""
    w, e = amax_of(t)
    if w is None and reduce and H3_TAGS:
        w, e = amax_of(amax_compute(t))
    return w, e


def amax_wgrad_operands(x, gy, wino_v=None):
    """((word, epoch) of x, of gy) for a weight gradient over contiguous x, gy: x first, then gy.  With the forward pass's Winograd-domain V
    kept (wino_v) x is never reduced -- V carries its own word inside the library -- and x's tag, when valid, is still passed on.  The pair
    may be handed to another stream's launch (conv_wgrad(amax_refs=)) once that stream waits for this one."""
    return amax_operand(x, reduce=wino_v is None), amax_operand(gy)


def conv_out_emits(out, residual, sh, sw, emit_amax, math):
    """Before the launch: may the epilogue write the amax word of the conv's result?  out = None: a fresh result.  The epilogue sees only the
    pixels it writes, so its maximum is the tensor's when the result is fresh; when the conv adds into the very tensor it reads as residual;
    and, scattered with strides (sh, sw) -- rows land on every sh-th / sw-th pixel of a zeroed tensor, the dgrad of a stride-2 1x1 conv --
    only into the tensor a fresh pass of the SAME geometry zero-filled and nothing has written since (its _abr_scatter mark).  Any other
    caller's `out` holds pixels the epilogue never sees.  emit_amax None: under the arithmetics that read the words."""
    if emit_amax is None:
        emit_amax = uses_amax(math)
    if not (emit_amax and H3_TAGS):
        return False
    if out is None:
        return True
    if out is not residual:
        return False
    return (sh == 1 and sw == 1) or getattr(out, "_abr_scatter", None) == (out.data_ptr(), sh, sw)


def conv_out_done(out, fresh, word, epoch, sh=1, sw=1):
    """After the launch: tag the result with the word its epilogue wrote; a caller's `out` written without one loses whatever tag (and scatter
    mark) it carried -- a raw kernel moves neither data_ptr nor _version; a fresh strided result is marked "zero everywhere but the pixels
    this geometry writes"."""
    if word is not None:
        amax_tag(out, word, epoch)
    elif not fresh:
        amax_drop(out)
    if fresh and (sh != 1 or sw != 1):
        out._abr_scatter = (out.data_ptr(), sh, sw)
    return out


def _conv_result(d, scattered, device):
    """a conv's fresh result: zeros under a scatter (out_hw given: the kernel writes only some pixels), else uninitialised"""
    return (torch.zeros if scattered else torch.empty)((d.B, d.out_H, d.out_W, d.Cout), dtype=_f32, device=device)


def h3_range_stats(reset=True):
    """(operand elements more than 18 binades below their tensor's amax, operand elements inspected) by the f16x3 kernels since the last
    reset (abr_h3_range_stats).  Synchronises the current stream."""
    import ctypes
    v = (ctypes.c_uint64 * 2)(0, 0)
    L.check(L.lib().abr_h3_range_stats(ctypes.cast(v, ctypes.c_void_p), int(bool(reset)), L.stream()), "h3_range_stats")
    return int(v[0]), int(v[1])


def x6_range_flags(reset=True):
    """Range guard of the bf16x6 arithmetic (include/abr_iod_hip.h, abr_x6_range_flags): OR of X6_FLAG_* raised by any bf16x6 kernel
    since the last reset -- an operand left the domain in which the three-way bf16 split is exact (non-zero |x| < 2^-110, inf, nan).
    Synchronises the current stream."""
    import ctypes
    v = ctypes.c_uint32(0)
    L.check(L.lib().abr_x6_range_flags(ctypes.cast(ctypes.pointer(v), ctypes.c_void_p), int(bool(reset)), L.stream()), "x6_range_flags")
    return int(v.value)


class X6RangeWatch(object):
    """Non-blocking poll of the range guard for a training loop: `poll()` at the end of every step enqueues an asynchronous copy of the
    flag word into pinned host memory and returns the value of the PREVIOUS copy once its event has completed (no host stall)."""

    def __init__(self):
        self._host = torch.zeros(1, dtype=torch.int32).pin_memory()
        self._dev = None
        self._event = None

    def poll(self, reduce_over_ranks=False):
        """reduce_over_ranks (data-parallel training): the flag word is MAX-reduced over the process group ON THE DEVICE before it is
        copied out (4 bytes per step on the collective's stream, still no host stall), so every rank sees a trip at the same poll."""
        seen = 0
        if self._event is not None and reduce_over_ranks:
            # ranks must issue the SAME collective sequence and read the SAME poll: wait for the previous copy instead of skipping a round
            # (free in the training step: its one read-back during the forward pass already passed the previous step's end)
            self._event.synchronize()
        if self._event is not None and self._event.query():
            seen = int(self._host[0].item()) & 0xFFFFFFFF
            self._event = None
        if self._event is None:
            if reduce_over_ranks:
                import torch.distributed as dist
                if self._dev is None:
                    self._dev = torch.zeros(1, dtype=torch.int32, device="cuda")
                L.check(L.lib().abr_x6_range_flags_to_device(self._dev.data_ptr(), L.stream()), "x6_range_flags_to_device")
                dist.all_reduce(self._dev, op=dist.ReduceOp.MAX)   # TINY = 1, NONFINITE = 2, both = 3: MAX keeps "tripped" alive
                self._host.copy_(self._dev, non_blocking=True)
            else:
                L.check(L.lib().abr_x6_range_flags_async(self._host.data_ptr(), L.stream()), "x6_range_flags_async")
            self._event = torch.cuda.Event()
            self._event.record()
        return seen

    def reset(self):
        """clear the device word AND the copy in flight (its value predates the reset and would re-trip the next poll)"""
        x6_range_flags(reset=True)    # synchronises the stream: the pending copy has landed
        self._event = None
        self._host.zero_()

    def poll_h3_stats(self, reduce_over_ranks=False):
        """f16x3: enqueue an asynchronous read of (small operand elements, inspected operand elements) since the previous call (the device
        counters are reset by the read; SUM over the ranks first under data parallelism) and return the PREVIOUS read's pair, or None while
        none has landed.  No host stall."""
        seen = None
        ev = getattr(self, "_h3_event", None)
        if ev is not None and reduce_over_ranks:
            ev.synchronize()   # (every rank reads the same poll: see poll())
        if ev is not None and ev.query():
            seen = (int(self._h3_host[0].item()), int(self._h3_host[1].item()))
            self._h3_event = ev = None
        if ev is None:
            if getattr(self, "_h3_dev", None) is None:
                self._h3_dev = torch.zeros(2, dtype=torch.int64, device="cuda")
                self._h3_host = torch.zeros(2, dtype=torch.int64).pin_memory()
            L.check(L.lib().abr_h3_range_stats_to_device(self._h3_dev.data_ptr(), 1, L.stream()), "h3_range_stats_to_device")
            if reduce_over_ranks:
                import torch.distributed as dist
                dist.all_reduce(self._h3_dev, op=dist.ReduceOp.SUM)
            self._h3_host.copy_(self._h3_dev, non_blocking=True)
            self._h3_event = torch.cuda.Event()
            self._h3_event.record()
        return seen


_desc_templates = {}


def conv_desc(x_shape, w_shape, stride, pad, scale=None, bias=None, residual=None, mask=None, relu=False,
              out_hw=None, out_stride=(1, 1), math=MATH_F32):
    """abr_conv_desc of a conv.  The geometry part is built once per distinct (shapes, stride, pad, epilogue flags, math) and kept as a
    byte image: a call copies it and fills in the pointers (the field-by-field build costs 4.7 us, ~300 descriptors per training step)."""
    key = (x_shape, w_shape, stride, pad, relu, out_hw, out_stride, math)
    tmpl = _desc_templates.get(key)
    if tmpl is None:
        B, H, W, Cin = x_shape
        Cout, R, S, Cin2 = w_shape
        if Cin != Cin2:
            raise RuntimeError(f"conv: input has {Cin} channels, weight expects {Cin2}")
        Ho = (H + 2 * pad - R) // stride + 1
        Wo = (W + 2 * pad - S) // stride + 1
        d = L.ConvDesc()
        d.B, d.H, d.W, d.Cin, d.Cout, d.R, d.S = B, H, W, Cin, Cout, R, S
        d.stride, d.pad, d.Ho, d.Wo = stride, pad, Ho, Wo
        d.relu = int(relu)
        if out_hw is None:
            d.out_H, d.out_W, d.out_sh, d.out_sw = Ho, Wo, 1, 1
        else:
            d.out_H, d.out_W = out_hw
            d.out_sh, d.out_sw = out_stride
        d.math = int(math)
        if len(_desc_templates) > 8192:     # (ragged batches: every image size brings its own set)
            _desc_templates.clear()
        tmpl = _desc_templates[key] = bytes(d)
    d = L.ConvDesc.from_buffer_copy(tmpl)
    if scale is not None:
        d.scale = scale.data_ptr()
    if bias is not None:
        d.bias = bias.data_ptr()
    if residual is not None:
        d.residual = residual.data_ptr()
    if mask is not None:
        d.mask = mask.data_ptr()
    return d


def conv_route_info(x_shape, w_shape, stride, pad, scale=None, bias=None, residual=None, mask=None, relu=False,
                    out_hw=None, out_stride=(1, 1), math=MATH_F32):
    """What the library decided for conv_desc(the same arguments) (abr_conv_route_info; host only, no device call): (the arithmetic the forward
    pass runs in, forward takes Winograd, weight gradient takes Winograd, the weight gradient's arithmetic)."""
    d = conv_desc(tuple(x_shape), tuple(w_shape), stride, pad, scale, bias, residual, mask, relu, out_hw, out_stride, math)
    out = (C.c_int32 * 4)()
    L.check(L.lib().abr_conv_route_info(C.byref(d), out), "conv_route_info")
    return int(out[0]), bool(out[1]), bool(out[2]), int(out[3])


KEEP_WINO_V = os.environ.get("ABR_WINOGRAD_KEEP_V", "1") != "0"


def wino_v_alloc(x, w, stride, pad, math=MATH_F32):
    """Buffer for the Winograd-domain input V of conv(x, w) if both its forward pass and its weight gradient take the Winograd path
    (abr_conv_wino_v_floats), else None.  Passed to conv_forward(wino_v=) to be filled and to conv_wgrad(wino_v=) to be reused:
    the gradient then skips its own input transform (the same B^T d B over the same x)."""
    if not KEEP_WINO_V:
        return None
    d = conv_desc(x.shape, w.shape, stride, pad, math=math)
    n = int(L.lib().abr_conv_wino_v_floats(C.byref(d)))
    return torch.empty(n, dtype=_f32, device=x.device) if n > 0 else None


def conv_forward(x, w, stride=1, pad=0, scale=None, bias=None, residual=None, mask=None, relu=False,
                 out=None, out_hw=None, out_stride=(1, 1), math=MATH_F32, wino_v=None, w_planes=None, w_version=0, emit_amax=None):
    """x [B,H,W,Cin] NHWC, w [Cout,R,S,Cin] OHWI -> [B,Ho,Wo,Cout] (or scattered into `out` [B,out_H,out_W,Cout]).
    math=MATH_BF16: operands rounded to bf16 inside the kernel, bf16 MFMA, fp32 accumulate (fp32 tensors in and out).
    math=MATH_F16X3 / MATH_F16: x's amax word is taken from its tag when it has one (else the library reduces x first); emit_amax (default: under
    those) makes the kernel's epilogue write the output's amax word, and the result is tagged with it -- not when the conv accumulates
    into a caller's `out` that already holds other pixels (a scattered second pass), whose amax the epilogue cannot know."""
    L.require_cuda(x, w)
    xc, w = L.f32c(x), L.f32c(w)
    d = conv_desc(xc.shape, w.shape, stride, pad, scale, bias, residual, mask, relu, out_hw, out_stride, math)
    d.wino_v = L.ptr(wino_v)
    d.w_planes = L.ptr(w_planes)   # MATH_BF16X6: the caller's own pack_weights(w) planes (else the library packs (w, w_version) itself)
    d.w_version = int(w_version)   # non-zero: the library may keep data derived from (w, w_version): Winograd-domain weights, packed bf16x3 planes
    if uses_amax(math):
        d.x_amax, d.x_amax_epoch = amax_operand(xc)
    fresh = out is None
    ow, oe = amax_new() if conv_out_emits(out, residual, d.out_sh, d.out_sw, emit_amax, math) else (None, 0)
    d.out_amax, d.out_amax_epoch = ow, oe
    if fresh:
        out = _conv_result(d, out_hw is not None, x.device)
    L.check(L.lib().abr_conv_forward(C.byref(d), L.ptr(xc), L.ptr(w), L.ptr(out), L.stream()), "conv_forward")
    return conv_out_done(out, fresh, ow, oe, d.out_sh, d.out_sw)


# Main-stream timeline of the UN-PROFILED step (tools/step_marks.py): with ABR_STEP_MARKS=1 `mark(name)` records an event on the current stream at
# a handful of points of the step (a kernel trace slows the host enough to change what the device waits for; events do not).  Off: a no-op.
STEP_MARKS = os.environ.get("ABR_STEP_MARKS", "0") != "0"
_marks = []


def mark(name):
    if STEP_MARKS and torch.cuda.is_available():
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        _marks.append((name, ev))


def take_marks():
    """[(name, ms since the first mark)] of the marks recorded since the last call (synchronises)"""
    torch.cuda.synchronize()
    out = [(n, _marks[0][1].elapsed_time(e)) for n, e in _marks] if _marks else []
    del _marks[:]
    return out


def bottleneck_tail64_applies(o1, w2, w3, math):
    """the fused tail takes the 64-wide bottleneck of the frozen layer1 in the bf16x6 arithmetic (abr_conv_tail64_forward)"""
    return (math == MATH_BF16X6 and tuple(w2.shape) == (64, 3, 3, 64) and tuple(w3.shape) == (256, 1, 1, 64)
            and o1.shape[-1] == 64 and o1.numel() * 4 * 4 < 0x7FFFFFF0)


def bottleneck_tail64(o1, w2, w3, scale2, bias2, scale3, bias3, residual, w2_version, w3_version, out=None):
    """relu(bn3(conv1x1(relu(bn2(conv3x3(o1)))) + residual) in ONE launch (resnet.py:327-346 without a backward pass): o1 [B,H,W,64] NHWC,
    w2 [64,3,3,64], w3 [256,1,1,64] OHWI -> [B,H,W,256]; bit-identical to the two conv_forward calls it replaces."""
    L.require_cuda(o1, w2, w3)
    o1, w2, w3 = L.f32c(o1), L.f32c(w2), L.f32c(w3)
    d2 = conv_desc(o1.shape, w2.shape, 1, 1, scale2, bias2, None, None, True, math=MATH_BF16X6)
    B, H, W, _ = o1.shape
    d3 = conv_desc((B, H, W, 64), w3.shape, 1, 0, scale3, bias3, residual, None, True, math=MATH_BF16X6)
    d2.w_version, d3.w_version = int(w2_version), int(w3_version)
    if out is None:
        out = _empty((B, H, W, 256), o1)
    L.check(L.lib().abr_conv_tail64_forward(C.byref(d2), C.byref(d3), L.ptr(o1), L.ptr(w2), L.ptr(w3), L.ptr(out), L.stream()), "conv_tail64_forward")
    return out


def conv_prepare_weights(w, stride, pad, math, w_version):
    """Derive on the CURRENT stream what conv_forward(.., w, stride, pad, math=, w_version=) would derive from w (the Winograd-domain
    weights of a wide 3x3 conv) so that the call itself finds it cached; consumers on other streams are ordered behind it."""
    Cout, R, S, Cin = w.shape
    L.check(L.lib().abr_conv_prepare_weights(L.ptr(w), Cout, R, S, Cin, stride, pad, int(math), int(w_version), L.stream()), "conv_prepare_weights")


def conv_prepare_batch(entries):
    """entries: [(w [Cout,R,S,Cin], scale or None, wt or None, stride, pad, math, w_version)] -- what conv_prepare_weights(w, ...) derives,
    and for wt != None the dgrad copy wt = conv_dgrad_weights(w, scale) plus what conv_prepare_weights(wt, 1, R-1-pad, ...) derives from
    it, for ALL entries in three launches on the current stream (abr_conv_prepare_batch)."""
    if not entries:
        return
    arr = (L.PrepItem * len(entries))()
    keep = []
    for a, (w, scale, wt, stride, pad, math, ver) in zip(arr, entries):
        Cout, R, S, Cin = w.shape
        if scale is not None:
            scale = L.f32c(scale)
            keep.append(scale)
        a.w, a.scale, a.wt = L.ptr(w), L.ptr(scale), L.ptr(wt)
        a.Cout, a.R, a.S, a.Cin, a.stride, a.pad, a.math, a.w_version = Cout, R, S, Cin, int(stride), int(pad), int(math), int(ver)
    L.check(L.lib().abr_conv_prepare_batch(C.cast(arr, C.c_void_p), len(entries), L.stream()), "conv_prepare_batch")


class PreparedBatch(object):
    """conv_prepare_batch with its table built ONCE: the weights live in the model's flat storage, the dgrad copies and the folded FrozenBN
    scales in buffers their modules keep, so every pointer of an entry is fixed from step to step and only w_version moves.  `entries` as for
    conv_prepare_batch, with a CALLABLE in the version slot (read at every run).  `still_valid()` re-reads the pointers (a re-homed weight, a
    re-fused scale or another math mode means: rebuild)."""

    def __init__(self, entries):
        self.n = len(entries)
        self.arr = (L.PrepItem * max(self.n, 1))()
        self.keep, self.vers, self.sig_src = [], [], []
        for a, (w, scale, wt, stride, pad, math, ver) in zip(self.arr, entries):
            Cout, R, S, Cin = w.shape
            if scale is not None:
                scale = L.f32c(scale)
            self.keep.append((w, scale, wt))
            a.w, a.scale, a.wt = L.ptr(w), L.ptr(scale), L.ptr(wt)
            a.Cout, a.R, a.S, a.Cin, a.stride, a.pad, a.math = Cout, R, S, Cin, int(stride), int(pad), int(math)
            self.vers.append(ver)
        self.ptr = C.cast(self.arr, C.c_void_p)

    def run(self):
        if not self.n:
            return
        for a, ver in zip(self.arr, self.vers):
            a.w_version = int(ver())
        L.check(L.lib().abr_conv_prepare_batch(self.ptr, self.n, L.stream()), "conv_prepare_batch")


def conv_cache_clear():
    """Drop the library's per-weight derived data (Winograd-domain weights); call when parameter storage is released or rebuilt."""
    L.check(L.lib().abr_conv_cache_clear(), "conv_cache_clear")


def conv_cache_drop_range(base, nbytes):
    """Drop the derived data of the weights stored inside [base, base + nbytes) only (abr_conv_cache_drop_range)."""
    L.check(L.lib().abr_conv_cache_drop_range(int(base), int(nbytes)), "conv_cache_drop_range")


def conv_cache_bytes():
    return int(L.lib().abr_conv_cache_bytes())


def scratch_bytes():
    """Bytes of the library's own per-stream scratch and process-wide words (not the derived-weight cache)."""
    return int(L.lib().abr_scratch_bytes())


def conv_wgrad(x, gy, dw, stride=1, pad=0, scale=None, math=MATH_F32, wino_v=None, amax_refs=None, stream=None):
    """dw [Cout,R,S,Cin] += scale * gy^T im2col(x) (fp32 atomics; caller zeroes dw once per step).  MATH_F16X3 / MATH_F16: the amax words of x and
    gy come from their tags (else the library reduces the operand first); amax_refs = ((word, epoch) of x, of gy) taken by the caller on
    the stream that produced the operands (conv_wgrad_async)."""
    L.require_cuda(x, gy, dw)
    xc, gyc = L.f32c(x), L.f32c(gy)
    d = conv_desc(xc.shape, dw.shape, stride, pad, scale=scale, math=math)
    d.wino_v = L.ptr(wino_v)
    if uses_amax(math):   # (reduced here rather than inside the call so that a second consumer of the same tensor finds the tag)
        (d.x_amax, d.x_amax_epoch), (d.gy_amax, d.gy_amax_epoch) = amax_refs or amax_wgrad_operands(xc, gyc, wino_v)
    L.check(L.lib().abr_conv_wgrad(C.byref(d), L.ptr(xc), L.ptr(gyc), L.ptr(dw), L.stream() if stream is None else stream), "conv_wgrad")
    return dw


# Weight gradients do not feed anything else in backward (they accumulate atomically into the flat gradient buffer), so they
# run on a SIDE HIP stream next to the dgrad chain: their workgroups fill the tail rounds of the main stream's kernels (and
# vice versa) instead of each kernel draining the chip alone.  ABR_WGRAD_STREAM=0 keeps everything on one stream.
WGRAD_SIDE_STREAM = os.environ.get("ABR_WGRAD_STREAM", "1") != "0"
_side_streams = {}
_join_pending = [False]


def h2d(values, dtype, device):
    """Small host list -> device tensor WITHOUT stalling the host: a pageable-memory copy (`torch.tensor(..., device=)`) waits for
    everything queued on the stream (measured: ~3 ms per call inside the training step, six calls per step); staging through the
    caching pinned allocator makes it a true async copy."""
    t = torch.tensor(values, dtype=dtype)
    if torch.device(device).type != "cuda":
        return t.to(device)
    return t.pin_memory().to(device, non_blocking=True)


# Weight preparation off the critical stream (solver/build.py::FusedSGD.step): after the SGD kernel the data derived from the new weights
# (flipped dgrad copies, Winograd-domain weights) is rebuilt on its own stream, next to the following step's source-model forward; the
# first consumer on another stream waits for the event recorded behind it.
_prep = {"event": None, "waited": set()}


def prep_done(stream):
    ev = torch.cuda.Event()
    ev.record(stream)
    _prep["event"], _prep["waited"] = ev, set()


def prep_wait():
    """make the current stream see the last weight preparation (no-op once per stream and preparation)"""
    ev = _prep["event"]
    if ev is not None:
        raw = L.stream()      # (torch.cuda.current_stream() builds a Stream object: ~9 us, and every dgrad call comes through here)
        if raw not in _prep["waited"]:
            torch.cuda.current_stream().wait_event(ev)
            _prep["waited"].add(raw)


def side_stream(key):
    """key = device index (the wgrad stream) or (device index, tag)"""
    s = _side_streams.get(key)
    if s is None:
        s = _side_streams[key] = torch.cuda.Stream(device=key[0] if isinstance(key, tuple) else key)
    return s


def mark_overlap(on):
    """Tell the per-launch profiler (abr_prof_*) that main-stream launches now share the device with another stream."""
    L.lib().abr_prof_mark_overlap(1 if on else 0)


# Weight gradients go to this many side streams.  Two are worth 0.7 ms per step now that the small gradients are short (three: +0.5, four:
# +0.8 ms over two).  A weight's gradient always goes to the SAME stream (first-seen round-robin over the gradient buffers): a weight
# that is used twice in a step (layer4 serves the detection RoIs and the distillation RoIs) gets `dw +=` from two launches, and the
# Winograd inverse transform adds with a plain read-modify-write -- stream order keeps those two apart.
WGRAD_STREAMS = max(1, int(os.environ.get("ABR_WGRAD_STREAMS", "2")))
_wg_owner = {}
_wg_keep = {}    # {raw handle of the stream that produced them: [operands of the weight gradients queued on side streams since that stream's last join]}
_wg_lock = threading.Lock()


def _wg_hold(main, item):
    lst = _wg_keep.get(main)
    if lst is None:
        with _wg_lock:
            lst = _wg_keep.setdefault(main, [])
    lst.append(item)


_wgrad_keys = {}


def _wgrad_stream(dev, i):
    key = _wgrad_keys.get((dev, i))
    if key is None:
        key = _wgrad_keys[(dev, i)] = dev if i == 0 else (dev, "wgrad%d" % i)
    return side_stream(key)


def _wgrad_owner(dw):
    """index of the side stream that takes every gradient accumulated into the buffer dw (first-seen round-robin, see WGRAD_STREAMS)"""
    owner = _wg_owner.get(dw.data_ptr())
    if owner is None:
        owner = _wg_owner[dw.data_ptr()] = len(_wg_owner) % WGRAD_STREAMS
    return owner


def _arm_join():
    """the first weight gradient of a backward pass queues the join as an engine callback: from here to the join, main-stream launches share
    the device with the side streams"""
    if not _join_pending[0]:
        _join_pending[0] = True
        L.lib().abr_prof_mark_overlap(1)
        torch.autograd.Variable._execution_engine.queue_callback(join_side_stream)


def join_side_stream():
    """Make the current stream wait for everything queued on the side stream(s) (queued automatically as an end-of-backward
    callback by conv_wgrad_async; FusedSGD.step calls it again before touching the gradients)."""
    if _join_pending[0]:
        L.lib().abr_prof_mark_overlap(0)
    _join_pending[0] = False
    if torch.cuda.is_available():
        dev = torch.cuda.current_device()
        for i in range(WGRAD_STREAMS):
            s = _side_streams.get(dev if i == 0 else (dev, "wgrad%d" % i))
            if s is not None:
                torch.cuda.current_stream().wait_stream(s)
    # (after the waits: see conv_wgrad_async.)  Only the operands that belong to THIS stream go: another host thread's backward pass on another
    # stream has not waited for its side kernels yet, and its blocks would return to a pool whose stream is not ordered behind them.
    lst = _wg_keep.get(L.stream()) if torch.cuda.is_available() else None
    if lst:
        del lst[:]


def conv_wgrad_async(x, gy, dw, stride=1, pad=0, scale=None, math=MATH_F32, wino_v=None):
    """conv_wgrad on the side stream.  Only for use inside an autograd backward (the join is an engine callback)."""
    if not WGRAD_SIDE_STREAM:
        return conv_wgrad(x, gy, dw, stride, pad, scale, math, wino_v)
    side = _wgrad_stream(x.device.index, _wgrad_owner(dw))
    _arm_join()
    # The operands are made contiguous, and their amax words reduced, HERE -- on the stream that produced them and before the side stream's wait is
    # recorded: a copy or a reduction issued after that event would not be ordered before the side stream's kernel.  The copies are what the
    # kernel reads, so they are what is kept alive until the join.  The dgrad that follows on this stream shares gy's word, and the side stream
    # (ordered behind this point by the wait below) is handed both: a word reduced there would not be ordered before this stream's later readers.
    x, gy = L.f32c(x), L.f32c(gy)
    refs = amax_wgrad_operands(x, gy, wino_v) if uses_amax(math) else None
    # x, gy (and the zeroed gradient buffer) are produced on the current stream: the side stream is ordered behind it, and the launch names the
    # side stream itself (side.wait_stream(cur) + `with torch.cuda.stream(side)` cost ~30 us of Python per gradient, ~60 gradients per step)
    raw = side.cuda_stream
    main = L.stream()
    L.check(L.lib().abr_stream_wait_stream(raw, main), "stream_wait_stream")
    conv_wgrad(x, gy, dw, stride, pad, scale, math, wino_v, amax_refs=refs, stream=raw)
    # The caching allocator must not recycle the operands for the main stream while the side kernel still reads them: they are kept alive until
    # the join (join_side_stream: the main stream waits for the side streams, THEN the references go), so their blocks return to the main
    # stream's pool ordered behind the gradients.  (tensor.record_stream did the same at ~2 us per call plus an event per block at free time,
    # three tensors per gradient.)
    _wg_hold(main, (x, gy, wino_v))
    return dw


# ---- one library call for a conv's whole backward pass (round 5): the weight gradient on its side stream and the input gradient on the current
# stream are the per-conv calls above (conv_wgrad_async + conv_forward on the dgrad copy) -- ~40 us of interpreter / binding time together,
# ~40 convs per step.  The three-entry abr_conv_run table [side stream waits for this one, weight gradient, input gradient] of a (weight, shapes,
# geometry) is kept with everything constant filled in; a call writes this step's pointers and amax words.  Same kernels, same arguments,
# same order on each stream: bit-identical to the two calls.
_bwd_plans = {}


def conv_backward(x, gy, dw, wt, stride, pad, scale=None, math=MATH_F32, w_version=0, wino_v=None, dgrad=True, mask=None, residual=None,
                  out=None, out_hw=None, out_stride=(1, 1)):
    """dw += scale * gy^T im2col(x) on dw's side stream, and (dgrad) returns dL/dx = conv(gy, wt, stride 1, pad R-1-pad) with the epilogue
    options of conv_forward (mask / residual / out / the strided scatter of a stride-2 conv).  x, gy contiguous NHWC fp32; wt = the flipped,
    scaled dgrad copy [Cin,R,S,Cout] of the weight whose gradient buffer dw is.  Only inside an autograd backward (see conv_wgrad_async)."""
    if not (WGRAD_SIDE_STREAM and H3_TAGS and x.is_contiguous() and gy.is_contiguous() and x.dtype == _f32 and gy.dtype == _f32):
        conv_wgrad_async(x, gy, dw, stride, pad, scale=scale, math=math, wino_v=wino_v)
        if not dgrad:
            return None
        return conv_forward(gy, wt, 1, dw.shape[1] - 1 - pad, mask=mask, residual=residual, out=out, out_hw=out_hw, out_stride=out_stride,
                            math=math, w_version=w_version)
    key = (dw.data_ptr(), x.shape, gy.shape, stride, pad, math, dgrad, out_hw, out_stride, wino_v is not None)
    plan = _bwd_plans.get(key)
    wtp = wt.data_ptr() if dgrad else 0
    scp = scale.data_ptr() if scale is not None else 0
    if plan is None or plan[2] != wtp or plan[3] != scp:
        if len(_bwd_plans) > 4096:
            _bwd_plans.clear()
        arr = (L.ConvOp * 3)()
        arr[0].kind = L.OP_STREAM_WAIT
        arr[1].kind = L.OP_WGRAD
        arr[1].desc = conv_desc(x.shape, dw.shape, stride, pad, scale=scale, math=math)
        arr[1].out = dw.data_ptr()
        if dgrad:
            arr[2].kind = L.OP_FORWARD
            arr[2].desc = conv_desc(gy.shape, wt.shape, 1, dw.shape[1] - 1 - pad, out_hw=out_hw, out_stride=out_stride, math=math)
            arr[2].b = wtp
        plan = _bwd_plans[key] = (arr, C.cast(arr, C.c_void_p), wtp, scp, _wgrad_owner(dw), (scale, dw), threading.Lock())
    arr, ptr, _, _, owner, _, lock = plan
    with lock:     # (the table is shared by every host thread that runs this conv's backward pass; abr_conv_run releases the GIL)
        return _conv_backward_run(arr, ptr, owner, x, gy, dw, math, wino_v, dgrad, mask, residual, out, out_hw, w_version)


def _conv_backward_run(arr, ptr, owner, x, gy, dw, math, wino_v, dgrad, mask, residual, out, out_hw, w_version):
    side = _wgrad_stream(x.device.index, owner).cuda_stream
    _arm_join()
    main = L.stream()
    h3 = uses_amax(math)
    xp, gp = x.data_ptr(), gy.data_ptr()
    a0, a1 = arr[0], arr[1]
    a0.stream, a0.other = side, main
    a1.a, a1.b, a1.stream = xp, gp, side
    d1 = a1.desc
    d1.wino_v = wino_v.data_ptr() if wino_v is not None else None
    if h3:   # (the table is kept from call to call: every word it holds is rewritten)
        (d1.x_amax, d1.x_amax_epoch), (gw, ge) = amax_wgrad_operands(x, gy, wino_v)
        d1.gy_amax, d1.gy_amax_epoch = gw, ge
    if dgrad:
        a2 = arr[2]
        d2 = a2.desc
        fresh = out is None
        ow, oe = amax_new() if conv_out_emits(out, residual, d2.out_sh, d2.out_sw, None, math) else (None, 0)
        if h3:
            d2.x_amax, d2.x_amax_epoch, d2.out_amax, d2.out_amax_epoch = gw, ge, ow, oe
        if fresh:
            out = _conv_result(d2, out_hw is not None, x.device)
        a2.a, a2.out, a2.stream = gp, out.data_ptr(), main
        d2.residual = residual.data_ptr() if residual is not None else None
        d2.mask = mask.data_ptr() if mask is not None else None
        d2.w_version = int(w_version)
    L.check(L.lib().abr_conv_run(ptr, 3 if dgrad else 2), "conv_run (conv backward)")
    if dgrad:
        conv_out_done(out, fresh, ow, oe, d2.out_sh, d2.out_sw)
    _wg_hold(main, (x, gy, wino_v))
    return out if dgrad else None


def pack_weights(w, out=None):
    """w [Cout,R,S,Cin] (or any [rows, K] fp32 matrix, K % 16 == 0) -> its fragment-packed exact bf16x3 planes (uint8 buffer of
    abr_conv_packed_bytes bytes) for conv_forward(..., math=MATH_BF16X6, w_planes=): the weights-direct bf16x6 kernel loads weight
    fragments straight from them (include/abr_iod_hip.h, abr_conv_pack_weights)."""
    L.require_cuda(w)
    w = L.f32c(w)
    rows, K = w.shape[0], w.numel() // w.shape[0]
    n = int(L.lib().abr_conv_packed_bytes(rows, K))
    if n <= 0:
        raise RuntimeError("pack_weights: K = {} is not a positive multiple of 16".format(K))
    if out is None:
        out = torch.empty(n, dtype=torch.uint8, device=w.device)
    L.check(L.lib().abr_conv_pack_weights(L.ptr(w), rows, K, L.ptr(out), L.stream()), "conv_pack_weights")
    return out


def conv_dgrad_weights(w, scale=None, out=None):
    """w [Cout,R,S,Cin] -> [Cin,R,S,Cout] flipped, scaled by scale[Cout]"""
    w = L.f32c(w)
    Cout, R, S, Cin = w.shape
    if out is None:
        out = _empty((Cin, R, S, Cout), w)
    L.check(L.lib().abr_conv_dgrad_weights(L.ptr(w), L.ptr(scale), Cout, R, S, Cin, L.ptr(out), L.stream()), "dgrad_weights")
    return out


def bias_grad(gy, db):
    gy = L.f32c(gy)
    Ch = gy.shape[-1]
    L.check(L.lib().abr_bias_grad(L.ptr(gy), gy.numel() // Ch, Ch, L.ptr(db), L.stream()), "bias_grad")
    return db


# ---- deformable 3x3 conv (DCNv1 / v2 of the R-50-C4 body): columns for the 1x1 conv route and their gradient (csrc/deform.hip)
def deform_im2col(x, om, dg=1, modulated=False):
    """x [B,H,W,C], om [B,H,W,Com] (offsets, v2: + mask logits) -> cols [B,H,W,9C].  Bilinear weights sum to at most 1 and the mask lies in
    (0, 1): x's amax word bounds cols, which inherits it (no reduction pass for the f16x3 consumer)."""
    L.require_cuda(x, om)
    x, om = L.f32c(x), L.f32c(om)
    B, H, W, Ch = x.shape
    if tuple(om.shape[:3]) != (B, H, W):
        raise RuntimeError(f"deform_im2col: offsets {tuple(om.shape)} do not match x {tuple(x.shape)}")
    cols = _empty((B, H, W, 9 * Ch), x)
    L.check(L.lib().abr_deform_im2col(L.ptr(x), L.ptr(om), B, H, W, Ch, om.shape[3], int(dg), int(bool(modulated)), L.ptr(cols), L.stream()),
            "deform_im2col")
    return amax_carry_bound(cols, x)


def deform_col2im_coord(dcol, x, om, dg=1, modulated=False):
    """Backward of deform_im2col: (dx [B,H,W,C] from fp32 atomics -- not bit-reproducible, d_om [B,H,W,Com], deterministic, its padding
    channels zero).  d_om carries an amax word written by the kernel."""
    L.require_cuda(dcol, x, om)
    dcol, x, om = L.f32c(dcol), L.f32c(x), L.f32c(om)
    B, H, W, Ch = x.shape
    if tuple(dcol.shape) != (B, H, W, 9 * Ch) or tuple(om.shape[:3]) != (B, H, W):
        raise RuntimeError(f"deform_col2im_coord: dcol {tuple(dcol.shape)} / offsets {tuple(om.shape)} do not match x {tuple(x.shape)}")
    dx = torch.zeros_like(x)
    d_om = _empty(tuple(om.shape), om)
    w, e = amax_new() if H3_TAGS else (None, 0)
    L.check(L.lib().abr_deform_col2im_coord(L.ptr(dcol), L.ptr(x), L.ptr(om), B, H, W, Ch, om.shape[3], int(dg), int(bool(modulated)),
                                            L.ptr(dx), L.ptr(d_om), w, e, L.stream()), "deform_col2im_coord")
    if w is not None:
        amax_tag(d_om, w, e)
    return dx, d_om


# ---- the general deformable conv (layers/dcn, _C.deform_conv_* / _C.modulated_deform_conv_*): any kernel, stride, padding, dilation, groups
def deform_out_size(H, W, kernel, stride, padding, dilation):
    """(Ho, Wo) of deform_conv_func.py:134-147 / :249-258; all arguments pairs"""
    return tuple((n + 2 * p - (d * (k - 1) + 1)) // s + 1 for n, k, s, p, d in zip((H, W), kernel, stride, padding, dilation))


def _deform_general_args(name, x, offset, mask, kernel, stride, padding, dilation, groups, dg):
    B, H, W, Ch = x.shape
    K = kernel[0] * kernel[1]
    Ho, Wo = offset.shape[1], offset.shape[2]
    if tuple(offset.shape) != (B, Ho, Wo, dg * 2 * K):
        raise RuntimeError(f"{name}: offset {tuple(offset.shape)} is not [{B}, Ho, Wo, {dg * 2 * K}]")
    if mask is not None and tuple(mask.shape) != (B, Ho, Wo, dg * K):
        raise RuntimeError(f"{name}: mask {tuple(mask.shape)} is not [{B}, {Ho}, {Wo}, {dg * K}]")
    return (B, H, W, Ch, Ho, Wo, kernel[0], kernel[1], stride[0], stride[1], padding[0], padding[1], dilation[0], dilation[1], int(groups), int(dg))


def deform_im2col_general(x, offset, mask=None, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, dg=1):
    """x [B,H,W,C], offset [B,Ho,Wo,dg*2*K], mask [B,Ho,Wo,dg*K] or None -> cols [groups, B*Ho*Wo, K*C/groups] (include/abr_iod_hip.h,
    abr_deform_im2col_general).  Without a mask the bilinear weights sum to at most 1: x's amax word bounds cols, which inherits it.  A
    caller's mask may exceed 1, so with one cols stays untagged and its consumer reduces it."""
    L.require_cuda(x, offset, mask)
    x, offset = L.f32c(x), L.f32c(offset)
    mask = None if mask is None else L.f32c(mask)
    a = _deform_general_args("deform_im2col_general", x, offset, mask, kernel, stride, padding, dilation, groups, dg)
    B, Ch, Ho, Wo, K = a[0], a[3], a[4], a[5], a[6] * a[7]
    cols = _empty((int(groups), B * Ho * Wo, K * (Ch // int(groups))), x)
    L.check(L.lib().abr_deform_im2col_general(L.ptr(x), L.ptr(offset), L.ptr(mask), *a, L.ptr(cols), L.stream()), "deform_im2col_general")
    return amax_carry_bound(cols, x) if mask is None else cols


def deform_col2im_coord_general(dcol, x, offset, mask=None, kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1), groups=1, dg=1):
    """Backward of deform_im2col_general: (dx [B,H,W,C] from fp32 atomics into zeros -- not bit-reproducible --, d_offset like offset,
    d_mask like mask or None: both deterministic)."""
    L.require_cuda(dcol, x, offset, mask)
    dcol, x, offset = L.f32c(dcol), L.f32c(x), L.f32c(offset)
    mask = None if mask is None else L.f32c(mask)
    a = _deform_general_args("deform_col2im_coord_general", x, offset, mask, kernel, stride, padding, dilation, groups, dg)
    B, Ch, Ho, Wo, K = a[0], a[3], a[4], a[5], a[6] * a[7]
    if tuple(dcol.shape) != (int(groups), B * Ho * Wo, K * (Ch // int(groups))):
        raise RuntimeError(f"deform_col2im_coord_general: dcol {tuple(dcol.shape)} is not [{groups}, {B * Ho * Wo}, {K * (Ch // int(groups))}]")
    dx = torch.zeros_like(x)
    d_offset = _empty(tuple(offset.shape), offset)
    d_mask = None if mask is None else _empty(tuple(mask.shape), mask)
    L.check(L.lib().abr_deform_col2im_coord_general(L.ptr(dcol), L.ptr(x), L.ptr(offset), L.ptr(mask), *a, L.ptr(dx), L.ptr(d_offset),
                                                    L.ptr(d_mask), L.stream()), "deform_col2im_coord_general")
    return dx, d_offset, d_mask


def _deform_group_weights(w, groups):
    """OHWI w [Cout,kh,kw,C/groups] -> ([groups, Cop, K*C/groups], Cout/groups, Cop): group g's rows as the 1x1 conv's weight over its columns,
    the per-group output width padded with zero rows to a multiple of 4 (the contraction kernels' unit, as Conv2d(cout_pad=) does)"""
    Cout, kh, kw, Cg = w.shape
    Cog = Cout // groups
    Cop = (Cog + 3) // 4 * 4
    wm = w.reshape(groups, Cog, kh * kw * Cg)
    if Cop != Cog:
        wp = w.new_zeros((groups, Cop, kh * kw * Cg))
        wp[:, :Cog].copy_(wm)
        wm = wp
    return wm, Cog, Cop


def _deform_group_cols(cols, g, B, Ho, Wo):
    v = cols[g].view(B, Ho, Wo, cols.shape[2])
    return amax_carry_bound(v, cols)     # (a group's columns are a subset of the tensor's: its amax word, if it has one, bounds them)


def deform_conv_forward(x, offset, mask, w, bias, kernel, stride, padding, dilation, groups=1, dg=1, math=None):
    """The whole general deformable conv on NHWC / OHWI tensors: columns, then one 1x1 conv per group with the bias in its epilogue.
    x [B,H,W,C], offset [B,Ho,Wo,dg*2K], mask [B,Ho,Wo,dg*K] or None, w [Cout,kh,kw,C/groups], bias [Cout] or None
    -> (y [B,Ho,Wo,Cout], cols): cols is what deform_conv_backward's weight gradient contracts over.  math None: default_conv_math()."""
    math = default_conv_math() if math is None else math
    w = L.f32c(w)
    Cout = w.shape[0]
    if Cout % groups or tuple(w.shape[1:3]) != tuple(kernel) or w.shape[3] * groups != x.shape[3]:
        raise RuntimeError(f"deform_conv_forward: weight {tuple(w.shape)} does not fit x {tuple(x.shape)}, kernel {tuple(kernel)}, groups {groups}")
    cols = deform_im2col_general(x, offset, mask, kernel, stride, padding, dilation, groups, dg)
    B, Ho, Wo = offset.shape[:3]
    wm, Cog, Cop = _deform_group_weights(w, groups)
    KC = wm.shape[2]
    if groups == 1 and Cop == Cog:
        return conv_forward(_deform_group_cols(cols, 0, B, Ho, Wo), wm[0].view(Cop, 1, 1, KC), bias=bias, math=math), cols
    bp = None
    if bias is not None:
        bp = bias.new_zeros((groups, Cop))
        bp[:, :Cog].copy_(bias.view(groups, Cog))
    y = _empty((B, Ho, Wo, Cout), x)
    for g in range(groups):
        yg = conv_forward(_deform_group_cols(cols, g, B, Ho, Wo), wm[g].view(Cop, 1, 1, KC), bias=None if bp is None else bp[g], math=math)
        y[..., g * Cog:(g + 1) * Cog].copy_(yg[..., :Cog])
    return y, cols


def deform_conv_backward(gy, x, offset, mask, w, cols, kernel, stride, padding, dilation, groups=1, dg=1, math=None,
                         need_input=True, need_weight=True, need_bias=False):
    """Backward of deform_conv_forward from gy [B,Ho,Wo,Cout]: per group the 1x1 dgrad (the columns' gradient) and the weight gradient over
    (cols, gy); the bias gradient; the col2im + coord kernel.  -> (dx, d_offset, d_mask, dw [Cout,kh,kw,C/groups], db [Cout]), None where
    not asked for (need_input covers dx, d_offset and d_mask)."""
    math = default_conv_math() if math is None else math
    w, gy = L.f32c(w), L.f32c(gy)
    Cout, kh, kw, Cg = w.shape
    B, Ho, Wo = offset.shape[:3]
    wm, Cog, Cop = _deform_group_weights(w, groups)
    KC = wm.shape[2]
    dcol = torch.empty_like(cols) if need_input else None
    dw = wm.new_zeros(wm.shape) if need_weight else None
    for g in range(groups):
        if groups == 1 and Cop == Cog:
            gyg = gy
        else:
            gyg = gy.new_zeros((B, Ho, Wo, Cop))
            gyg[..., :Cog].copy_(gy[..., g * Cog:(g + 1) * Cog])
        if need_input:
            conv_forward(gyg, conv_dgrad_weights(wm[g].view(Cop, 1, 1, KC)), out=dcol[g].view(B, Ho, Wo, KC), math=math)
        if need_weight:
            conv_wgrad(_deform_group_cols(cols, g, B, Ho, Wo), gyg, dw[g].view(Cop, 1, 1, KC), math=math)
    db = None
    if need_bias:
        db = gy.new_zeros((Cout,))
        bias_grad(gy, db)
    dx = d_offset = d_mask = None
    if need_input:
        dx, d_offset, d_mask = deform_col2im_coord_general(dcol, x, offset, mask, kernel, stride, padding, dilation, groups, dg)
    if need_weight:
        dw = dw[:, :Cog].reshape(Cout, kh, kw, Cg)
    return dx, d_offset, d_mask, dw, db


# ----------------------------------------------------------------------------------------------- pointwise
def nchw_to_nhwc(x, cpad=None):
    x = L.f32c(x)
    B, Ch, H, W = x.shape
    cpad = cpad or Ch
    out = _empty((B, H, W, cpad), x)
    L.check(L.lib().abr_nchw_to_nhwc_pad(L.ptr(x), B, Ch, H, W, cpad, L.ptr(out), L.stream()), "nchw_to_nhwc")
    return out


def nhwc_to_nchw(x):
    x = L.f32c(x)
    B, H, W, Ch = x.shape
    out = _empty((B, Ch, H, W), x)
    L.check(L.lib().abr_nhwc_to_nchw(L.ptr(x), B, Ch, H, W, L.ptr(out), L.stream()), "nhwc_to_nchw")
    return out


def maxpool3x3s2(x):
    x = L.f32c(x)
    B, H, W, Ch = x.shape
    out = _empty((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Ch), x)
    L.check(L.lib().abr_maxpool3x3s2(L.ptr(x), B, H, W, Ch, L.ptr(out), L.stream()), "maxpool")
    return amax_carry_bound(out, x)   # (every input pixel lies in some window: max |pooled| <= max |x|, equal for a ReLU's output)


def maxpool3x3s2_backward(y, g_pool):
    """Backward of maxpool3x3s2 fused with the ReLU that produced its input y [B,H,W,C] (the stem's): g_pool [B,Ho,Wo,C] -> g_y [B,H,W,C],
    each window's gradient routed to the element maxpool3x3s2 selected (torch's rule), zero where y <= 0.  Deterministic gather, no atomics."""
    L.require_cuda(y, g_pool)
    y, g_pool = L.f32c(y), L.f32c(g_pool)
    B, H, W, Ch = y.shape
    if tuple(g_pool.shape) != (B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, Ch):
        raise RuntimeError(f"maxpool3x3s2_backward: g_pool {tuple(g_pool.shape)} does not match y {tuple(y.shape)}")
    out = _empty(y.shape, y)
    L.check(L.lib().abr_maxpool3x3s2_backward(L.ptr(y), L.ptr(g_pool), B, H, W, Ch, L.ptr(out), L.stream()), "maxpool3x3s2_backward")
    return out


def avgpool_forward(x):
    """x [N,h,w,C] -> [N,C]"""
    x = L.f32c(x)
    N, Ch = x.shape[0], x.shape[-1]
    HW = x.shape[1:-1].numel()
    out = _empty((N, Ch), x)
    L.check(L.lib().abr_avgpool_forward(L.ptr(x), N, HW, Ch, L.ptr(out), L.stream()), "avgpool_forward")
    return out


def avgpool_backward(g, shape, relu_of=None, emit_amax=False):
    """g [N, C] -> [N, H, W, C] / (H*W); relu_of = the pooled tensor itself when it is a ReLU's output: that ReLU's backward rides along
    (gx = relu_of > 0 ? g / HW : 0) and the caller's gradient is already masked"""
    g = L.f32c(g)
    N, Ch = g.shape
    gx = _empty(shape, g)
    HW = gx.numel() // (N * Ch) if N else 1
    if relu_of is not None:
        assert tuple(relu_of.shape) == tuple(shape) and relu_of.is_contiguous()
        if emit_amax and H3_TAGS:
            aw, ae = amax_new()
            L.check(L.lib().abr_avgpool_relu_backward_amax(L.ptr(g), L.ptr(relu_of), N, HW, Ch, L.ptr(gx), aw, ae, L.stream()), "avgpool_relu_backward")
            amax_tag(gx, aw, ae)
        else:
            L.check(L.lib().abr_avgpool_relu_backward(L.ptr(g), L.ptr(relu_of), N, HW, Ch, L.ptr(gx), L.stream()), "avgpool_relu_backward")
    else:
        L.check(L.lib().abr_avgpool_backward(L.ptr(g), N, HW, Ch, L.ptr(gx), L.stream()), "avgpool_backward")
    return gx


def channel_mean(x):
    """x [..., C] contiguous -> mean over the last (channel) axis, shape x.shape[:-1]"""
    L.require_cuda(x)
    x = L.f32c(x)
    out = torch.empty(x.shape[:-1], dtype=_f32, device=x.device)
    L.check(L.lib().abr_channel_mean(L.ptr(x), out.numel(), x.shape[-1], L.ptr(out), L.stream()), "channel_mean")
    return out


def relu_backward(g, y, inplace=False):
    """g * (y > 0); a new tensor unless inplace (one pass either way: no clone + in-place pair)"""
    g = L.f32c(g)
    out = g if inplace else torch.empty_like(g)
    L.check(L.lib().abr_relu_backward(L.ptr(g), L.ptr(y), g.numel(), L.ptr(out), L.stream()), "relu_backward")
    if not inplace:
        amax_carry_bound(out, g)   # (masking only removes elements: g's amax stays an upper bound, which is all a split scale needs)
    return out


def relu_backward_(g, y):
    return relu_backward(g, y, inplace=True)


def add_(a, b):
    L.check(L.lib().abr_add_inplace(L.ptr(a), L.ptr(b), a.numel(), L.stream()), "add_inplace")
    amax_drop(a)
    return a


class _LossSum(torch.autograd.Function):
    """total = sum_i w_i * loss_i (plus the two group sums, detached) in ONE launch, and one launch for all the terms' gradients: the
    reference's chain of python adds / muls on device scalars (train_incremental.py:91,101-128) is ~10 tiny kernels forward and as many
    autograd nodes backward"""

    @staticmethod
    def forward(ctx, weights, groups, *terms):
        n = len(terms)
        ts = [t.detach().reshape(()).contiguous() for t in terms]
        total = torch.empty((), dtype=_f32, device=ts[0].device)
        out = torch.empty((3,), dtype=_f32, device=ts[0].device)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for t in ts])
        w = (C.c_float * n)(*[float(v) for v in weights])
        g = (C.c_int32 * n)(*[int(v) for v in groups])
        L.check(L.lib().abr_loss_sum(C.cast(ptrs, C.c_void_p), C.cast(w, C.c_void_p), C.cast(g, C.c_void_p), n, L.ptr(total), L.ptr(out), L.stream()), "loss_sum")
        ctx.weights, ctx.n = [float(v) for v in weights], n
        ctx.mark_non_differentiable(out)
        return total, out

    @staticmethod
    def backward(ctx, g_total, _g_parts):
        n = ctx.n
        grads = torch.empty((n,), dtype=_f32, device=g_total.device)
        w = (C.c_float * n)(*ctx.weights)
        g_c = g_total.contiguous()   # (a local: a temporary inside the argument list would be released before the launch)
        L.check(L.lib().abr_loss_sum_backward(C.cast(w, C.c_void_p), n, L.ptr(g_c), L.ptr(grads), L.stream()), "loss_sum_backward")
        return (None, None) + tuple(grads[i] for i in range(n))


def loss_sum(terms, weights, groups):
    """-> (total (differentiable 0-dim), parts [3] = (total, group-0 sum, group-1 sum), detached)"""
    return _LossSum.apply(tuple(weights), tuple(groups), *terms)


def scale_(x, s=1.0, s_dev=None):
    """x *= s * s_dev[0] (s_dev: device scalar, e.g. the upstream gradient of a loss) -- no host sync"""
    if x is None:
        return None
    L.check(L.lib().abr_scale_inplace(L.ptr(x), x.numel(), float(s), L.ptr(s_dev), L.stream()), "scale_inplace")
    amax_drop(x)
    return x


# ----------------------------------------------------------------------------------------------- RPN glue
def grid_anchors(cell, H, W, stride, img_h, img_w, straddle=0):
    A = cell.shape[0]
    out = torch.empty((H * W * A, 4), dtype=_f32, device=cell.device)
    vis = torch.empty((H * W * A,), dtype=torch.uint8, device=cell.device)
    L.check(L.lib().abr_grid_anchors(L.ptr(cell), A, H, W, stride, img_h, img_w, straddle, L.ptr(out), L.ptr(vis),
                                     L.stream()), "grid_anchors")
    return out, vis


def topk_sigmoid(y, A, k):
    """y [N, nloc, ld] fp32 contiguous (columns 0..A-1 of every row are logits of anchors loc*A+a) -> (scores [N,k], idx [N,k] int64):
    the k largest sigmoid(logit) per image, sorted descending, ties by ascending anchor index."""
    y = L.f32c(y)
    N, nloc, ld = y.shape
    scores = torch.empty((N, k), dtype=_f32, device=y.device)
    idx = torch.empty((N, k), dtype=torch.int64, device=y.device)
    L.check(L.lib().abr_topk_sigmoid(L.ptr(y), nloc * ld, N, nloc * A, A, ld, k, L.ptr(scores), L.ptr(idx), L.stream()), "topk_sigmoid")
    return scores, idx


def box_encode_rows(gt, ex, weights, out=None):
    gt, ex = L.f32c(gt), L.f32c(ex)
    if out is None:
        out = torch.empty_like(ex)
    L.check(L.lib().abr_box_encode(L.ptr(gt), L.ptr(ex), ex.shape[0], *[float(v) for v in weights], L.ptr(out), L.stream()), "box_encode")
    return out


def rpn_decode_clip(reg, reg_col0, anchors, idx, img_hw, weights=(1.0, 1.0, 1.0, 1.0), A=1, clip=True):
    """reg [N,n_anchor/A,stride] ; idx [N,k] int64 anchor ids ; img_hw [N,2] int32 -> [N,k,4]"""
    N, nloc, rs = reg.shape
    n_anchor = nloc * A
    k = idx.shape[1]
    out = torch.empty((N, k, 4), dtype=_f32, device=reg.device)
    L.check(L.lib().abr_rpn_decode_clip(L.ptr(reg), rs, reg_col0, A, L.ptr(anchors), L.ptr(idx), N, n_anchor, k,
                                        L.ptr(img_hw) if clip else None, *[float(v) for v in weights], L.ptr(out), L.stream()), "rpn_decode_clip")
    return out


def rpn_pyramid_max_k():
    """most anchors abr_rpn_pyramid_topk ranks per (image, level): its in-LDS sort (2048)"""
    return L.lib().abr_rpn_pyramid_max_k()


def _rpn_pyramid_tables(what, ys, As, anchors=None):
    """the host arrays of the RPN pyramid entry points: ys = list of contiguous fp32 [N, nloc_l, ld_l] device tensors (fused head outputs)"""
    n = len(ys)
    if not 1 <= n <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"{what}: {n} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    if len(As) != n or (anchors is not None and len(anchors) != n):
        raise RuntimeError(f"{what}: the level lists differ in length")
    for l, y in enumerate(ys):
        L.require_cuda(y)
        if y.dtype != _f32 or y.dim() != 3 or not y.is_contiguous() or y.shape[0] != ys[0].shape[0]:
            raise RuntimeError(f"{what}: level {l} must be a contiguous float32 [N,nloc,ld] tensor with the batch of level 0, got {tuple(y.shape)} {y.dtype}")
    if anchors is not None:
        for l, a in enumerate(anchors):
            L.require_cuda(a)
            if a.dtype != _f32 or not a.is_contiguous() or tuple(a.shape) != (ys[l].shape[1] * As[l], 4):
                raise RuntimeError(f"{what}: anchors of level {l} must be a contiguous float32 [{ys[l].shape[1] * As[l]},4] tensor, got {tuple(a.shape)}")
    return ((C.c_void_p * n)(*[y.data_ptr() for y in ys]), (C.c_int * n)(*[y.shape[1] for y in ys]), (C.c_int * n)(*[int(a) for a in As]),
            (C.c_int * n)(*[y.shape[2] for y in ys]), (C.c_void_p * n)(*[a.data_ptr() for a in anchors]) if anchors is not None else None)


def rpn_pyramid_ks(ys, As, pre_nms_top_n):
    """k_l = min(pre_nms_top_n, nloc_l * A_l) of every level"""
    return [min(int(pre_nms_top_n), y.shape[1] * int(a)) for y, a in zip(ys, As)]


def rpn_pyramid_topk(ys, As, pre_nms_top_n):
    """ys: list of L fused head outputs [N, nloc_l, ld_l] -> (scores [N,L,k_max], idx [N,L,k_max] int64 level-local anchor ids): per (image, level)
    the k_l largest sigmoid(logit) as topk_sigmoid orders them, entries past k_l zero; three launches whatever N and L are."""
    ys = list(ys)
    yp, nl, Ap, ld, _ = _rpn_pyramid_tables("rpn_pyramid_topk", ys, As)
    N, k_max = ys[0].shape[0], max(rpn_pyramid_ks(ys, As, pre_nms_top_n))
    scores = torch.empty((N, len(ys), k_max), dtype=_f32, device=ys[0].device)
    idx = torch.empty((N, len(ys), k_max), dtype=torch.int64, device=ys[0].device)
    L.check(L.lib().abr_rpn_pyramid_topk(yp, nl, Ap, ld, len(ys), N, int(pre_nms_top_n), k_max, L.ptr(scores), L.ptr(idx), L.stream()), "rpn_pyramid_topk")
    return scores, idx


def rpn_pyramid_decode(ys, As, anchors, idx, scores, img_hw, pre_nms_top_n, weights=(1.0, 1.0, 1.0, 1.0), min_size=0):
    """idx / scores [N,L,k_max] from rpn_pyramid_topk, anchors: list of [nloc_l*A_l,4], img_hw [N,2] int32 -> (props [N*L,k_max,4],
    scores [N*L,k_max], counts [N*L] int32): decode + clip + remove_small_boxes, survivors in rank order without holes; one launch."""
    ys = list(ys)
    yp, nl, Ap, ld, ap = _rpn_pyramid_tables("rpn_pyramid_decode", ys, As, list(anchors))
    L.require_cuda(idx, scores, img_hw)
    N, nL, k_max = idx.shape
    assert nL == len(ys) and N == ys[0].shape[0] and idx.dtype == torch.int64 and idx.is_contiguous() and scores.is_contiguous()
    assert img_hw.dtype == torch.int32 and tuple(img_hw.shape) == (N, 2) and img_hw.is_contiguous()
    dev = ys[0].device
    props = torch.empty((N * nL, k_max, 4), dtype=_f32, device=dev)
    out_scores = torch.empty((N * nL, k_max), dtype=_f32, device=dev)
    counts = torch.empty((N * nL,), dtype=torch.int32, device=dev)
    L.check(L.lib().abr_rpn_pyramid_decode(yp, nl, Ap, ld, ap, nL, N, int(pre_nms_top_n), k_max, L.ptr(idx), L.ptr(scores), L.ptr(img_hw),
                                           *[float(v) for v in weights], float(min_size), L.ptr(props), L.ptr(out_scores), L.ptr(counts), L.stream()),
            "rpn_pyramid_decode")
    return props, out_scores, counts


def rpn_pyramid_select(props, scores, keep, n_keep, N, fpn_post_n, per_batch):
    """props [N*L,k_max,4], scores [N*L,k_max], keep [N*L,post] int32, n_keep [N*L] int32 (nms_sorted_batched over the segments) ->
    (rois [N,cap,4], scores [N,cap], src [N,cap] int32 candidate positions level*post+rank, n_out [N] int32), cap = min(fpn_post_n, L*post):
    per image the fpn_post_n best by descending score, or (per_batch) the batch's fpn_post_n best in candidate order; three launches."""
    L.require_cuda(props, scores, keep, n_keep)
    S, k_max = scores.shape
    post = keep.shape[1]
    assert N >= 0 and (S % N == 0 if N else S == 0) and tuple(props.shape) == (S, k_max, 4) and keep.shape[0] == S and n_keep.shape[0] == S
    assert props.dtype == _f32 and scores.dtype == _f32 and keep.dtype == torch.int32 and n_keep.dtype == torch.int32
    assert props.is_contiguous() and scores.is_contiguous() and keep.is_contiguous() and n_keep.is_contiguous()
    nL = S // N if N else 1
    cap = min(int(fpn_post_n), nL * post)
    dev = props.device
    rois = torch.empty((N, cap, 4), dtype=_f32, device=dev)
    out_scores = torch.empty((N, cap), dtype=_f32, device=dev)
    src = torch.empty((N, cap), dtype=torch.int32, device=dev)
    n_out = torch.empty((N,), dtype=torch.int32, device=dev)
    L.check(L.lib().abr_rpn_pyramid_select(L.ptr(props), L.ptr(scores), L.ptr(keep), L.ptr(n_keep), N, nL, k_max, post, int(fpn_post_n),
                                           1 if per_batch else 0, L.ptr(rois), L.ptr(out_scores), L.ptr(src), L.ptr(n_out), L.stream()),
            "rpn_pyramid_select")
    return rois, out_scores, src, n_out


def retina_max_candidates():
    """most candidates abr_retina_detect ranks per image, levels * pre_nms_top_n: its in-LDS sort (8192)"""
    return L.lib().abr_retina_max_candidates()


def retina_detect(cls, reg, anchors, A, num_classes, img_hw, score_thresh, pre_nms_top_n, nms_thresh, detections_per_img,
                  weights=(10.0, 10.0, 5.0, 5.0), min_size=0):
    """RetinaNet's post-processor for the whole batch (abr_retina_detect: 1 memset + 4 launches, nothing read back).  cls: list of L head outputs
    [N, nloc_l, ldc_l] (column a * C + c: anchor a, class c + 1; columns >= A * C are padding), reg: list of L [N, nloc_l, ldr_l] (columns 4a .. 4a+3),
    anchors: list of L [nloc_l * A, 4], C = num_classes foreground classes, img_hw [N,2] int32 -> (boxes [N,cap,4], scores [N,cap], labels [N,cap]
    int64, n_out [N] int32), cap = L * pre_nms_top_n: per image the classes' NMS survivors class by class, each class by descending score, cut at
    the detections_per_img-th largest score (ties kept)."""
    cls, reg, anchors = list(cls), list(reg), list(anchors)
    n, A, Cn, pre = len(cls), int(A), int(num_classes), int(pre_nms_top_n)
    if not 1 <= n <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"retina_detect: {n} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    if len(reg) != n or len(anchors) != n:
        raise RuntimeError("retina_detect: the level lists differ in length")
    if pre > rpn_pyramid_max_k():
        raise RuntimeError(f"retina_detect: MODEL.RETINANET.PRE_NMS_TOP_N = {pre} exceeds the {rpn_pyramid_max_k()} candidates ranked per (image, level)")
    if n * pre > retina_max_candidates():
        raise RuntimeError(f"retina_detect: {n} levels x MODEL.RETINANET.PRE_NMS_TOP_N = {pre} exceeds the {retina_max_candidates()} candidates ranked per image")
    N = cls[0].shape[0]
    for l in range(n):
        L.require_cuda(cls[l], reg[l], anchors[l])
        for what, t, need in (("cls", cls[l], A * Cn), ("reg", reg[l], 4 * A)):
            if t.dtype != _f32 or t.dim() != 3 or not t.is_contiguous() or t.shape[0] != N or t.shape[1] != cls[l].shape[1] or t.shape[2] < need:
                raise RuntimeError(f"retina_detect: {what} of level {l} must be a contiguous float32 [{N},nloc,>={need}] tensor, got {tuple(t.shape)} {t.dtype}")
        a = anchors[l]
        if a.dtype != _f32 or not a.is_contiguous() or tuple(a.shape) != (cls[l].shape[1] * A, 4):
            raise RuntimeError(f"retina_detect: anchors of level {l} must be a contiguous float32 [{cls[l].shape[1] * A},4] tensor, got {tuple(a.shape)}")
    L.require_cuda(img_hw)
    if img_hw.dtype != torch.int32 or tuple(img_hw.shape) != (N, 2) or not img_hw.is_contiguous():
        raise RuntimeError(f"retina_detect: img_hw must be a contiguous int32 [{N},2] tensor")
    dev, cap = cls[0].device, n * pre
    boxes = torch.empty((N, cap, 4), dtype=_f32, device=dev)
    scores = torch.empty((N, cap), dtype=_f32, device=dev)
    labels = torch.empty((N, cap), dtype=torch.int64, device=dev)
    n_out = torch.empty((N,), dtype=torch.int32, device=dev)
    vp, ci = C.c_void_p * n, C.c_int * n
    L.check(L.lib().abr_retina_detect(vp(*[t.data_ptr() for t in cls]), ci(*[t.shape[2] for t in cls]), vp(*[t.data_ptr() for t in reg]),
                                      ci(*[t.shape[2] for t in reg]), vp(*[t.data_ptr() for t in anchors]), ci(*[t.shape[1] for t in cls]), n, N, A, Cn,
                                      L.ptr(img_hw), float(score_thresh), pre, float(nms_thresh), int(detections_per_img),
                                      *[float(v) for v in weights], float(min_size), cap, L.ptr(boxes), L.ptr(scores), L.ptr(labels), L.ptr(n_out),
                                      L.stream()), "retina_detect")
    return boxes, scores, labels, n_out


def match_encode(boxes, gt, gt_labels, vis, hi, lo, allow_low_quality, weights, rpn_labels):
    """-> matched int64 [n], labels (fp32 RPN / int64 head) [n], reg_targets [n,4]"""
    boxes, gt = L.f32c(boxes), L.f32c(gt)
    n, G = boxes.shape[0], gt.shape[0]
    dev = boxes.device
    matched = torch.empty((n,), dtype=torch.int64, device=dev)
    lab_f = torch.empty((n,), dtype=_f32, device=dev) if rpn_labels else None
    lab_i = None if rpn_labels else torch.empty((n,), dtype=torch.int64, device=dev)
    tgt = torch.empty((n, 4), dtype=_f32, device=dev)
    ws = torch.empty((max(G, 1),), dtype=torch.int32, device=dev)
    L.check(L.lib().abr_match_encode(L.ptr(boxes), n, L.ptr(gt), L.ptr(gt_labels), G, L.ptr(vis), float(hi), float(lo),
                                     int(allow_low_quality), *[float(v) for v in weights], L.ptr(matched), L.ptr(lab_f),
                                     L.ptr(lab_i), L.ptr(tgt), L.ptr(ws), ws.numel() * 4, L.stream()), "match_encode")
    return matched, (lab_f if rpn_labels else lab_i), tgt


_sample_calls = [0]


def _draw_seed():
    """a sampler launch's seed: one draw from torch's default CPU generator per launch (host-side, no device sync): torch.manual_seed()
    therefore replays the sampler's choices, as it replays torch.randperm in the reference (balanced_positive_negative_sampler.py:44-49)"""
    _sample_calls[0] += 1
    return int(torch.empty((), dtype=torch.int64).random_().item()) & 0xFFFFFFFFFFFFFFFF


_ptr_tables = {}


_small_tables = {}


def _evict_oldest(cache, limit):
    """Drop the oldest half of a table cache that has reached `limit` entries.  NOT `cache.clear()`: a caller builds several tables for ONE
    launch, and clearing while it builds the second would free the first -- whose memory the second upload then reuses before the kernel
    has read it (seen once as a training step with garbage ground-truth boxes).  Callers also keep every table in a local until the
    launch is enqueued: after that a free is ordered behind the kernel on the same stream."""
    if len(cache) >= limit:
        for k in list(cache.keys())[:limit // 2]:
            del cache[k]


def _small_table(values, dtype, dev):
    """device copy of a short list of host integers, cached while the same list repeats (per-image GT counts, ...)"""
    key = (tuple(values), dtype, torch.device(dev))
    t = _small_tables.get(key)
    if t is None:
        _evict_oldest(_small_tables, 256)
        t = _small_tables[key] = h2d(list(values), dtype, dev)
    return t


def _pointer_table(tensors, dev):
    """device int64 array of the tensors' device addresses (one pinned asynchronous upload; cached while the addresses repeat)"""
    key = (tuple(t.data_ptr() for t in tensors), torch.device(dev))
    tab = _ptr_tables.get(key)
    if tab is None:
        _evict_oldest(_ptr_tables, 64)
        tab = _ptr_tables[key] = h2d(list(key[0]), torch.int64, dev)
    return tab


def _roi_head_targets_setup(N, n_prop, gt_boxes, gt_labels, batch_size, max_pos, dev):
    """the GT tables and the output dict shared by roi_head_targets and roi_head_targets_table (n_prop proposal rows per image at most)"""
    gtb = [L.f32c(b) for b in gt_boxes]
    gtl = [l.to(torch.int64).contiguous() for l in gt_labels]
    n_gt = [int(b.shape[0]) for b in gtb]
    if min(n_gt) == 0:   # matcher.py:53-57
        raise ValueError("No ground-truth boxes available for one of the images during training")
    g_max = max(n_gt)
    Pmax = n_prop + g_max
    R = batch_size
    i64, i32 = torch.int64, torch.int32
    out = dict(
        cand=torch.empty((N, Pmax, 4), dtype=_f32, device=dev), labels_all=torch.empty((N, Pmax), dtype=i64, device=dev),
        regt_all=torch.empty((N, Pmax, 4), dtype=_f32, device=dev), obj_all=torch.empty((N, Pmax), dtype=_f32, device=dev),
        n_cand=torch.empty((N,), dtype=i32, device=dev), pos_idx=torch.empty((N, max(max_pos, 1)), dtype=i64, device=dev),
        neg_idx=torch.empty((N, R), dtype=i64, device=dev), counts=torch.empty((N, 2), dtype=i32, device=dev),
        rois=torch.empty((N * R, 5), dtype=_f32, device=dev), labels=torch.empty((N * R,), dtype=i64, device=dev),
        reg_targets=torch.empty((N * R, 4), dtype=_f32, device=dev), sampled_idx=torch.empty((N, R), dtype=i64, device=dev),
        n_valid=torch.empty((1,), dtype=_f32, device=dev), obj=torch.empty((N * R,), dtype=_f32, device=dev),
        pos_rows=torch.empty((N * R,), dtype=i64, device=dev), col0=torch.empty((N * R,), dtype=i64, device=dev),
        n_gt=n_gt, g_max=g_max, keepalive=(gtb, gtl))
    ngt_dev = _small_table(n_gt, i32, dev)
    gtb_tab, gtl_tab = _pointer_table(gtb, dev), _pointer_table(gtl, dev)   # (held by the caller until the launch is enqueued: _evict_oldest)
    return out, (gtb_tab, gtl_tab, ngt_dev)


def roi_head_targets(props, scores, keep, n_keep, gt_boxes, gt_labels, hi, lo, weights, batch_size, max_pos, num_classes, cls_agnostic=False,
                     seed=None):
    """Box-head training targets for the whole batch, on device, no host round trip (include/abr_iod_hip.h, abr_roi_head_targets).
    props [N,k,4] / scores [N,k] / keep [N,post] int32 / n_keep [N] int32: the RPN selector's raw output; gt_boxes / gt_labels: per-image
    tensors.  Returns a dict of fixed-size tensors (batch_size rows per image)."""
    N, k_pre, _ = props.shape
    post = keep.shape[1]
    R = batch_size
    out, (gtb_tab, gtl_tab, ngt_dev) = _roi_head_targets_setup(N, post, gt_boxes, gt_labels, R, max_pos, props.device)
    if seed is None:
        seed = _draw_seed()
    L.check(L.lib().abr_roi_head_targets(
        L.ptr(props), L.ptr(keep), L.ptr(n_keep), N, k_pre, post, L.ptr(gtb_tab), L.ptr(gtl_tab), L.ptr(ngt_dev),
        out["g_max"], float(hi), float(lo), *[float(v) for v in weights], R, max_pos, seed, L.ptr(out["cand"]), L.ptr(out["labels_all"]),
        L.ptr(out["regt_all"]), L.ptr(out["n_cand"]), L.ptr(out["pos_idx"]), L.ptr(out["neg_idx"]), L.ptr(out["counts"]), L.ptr(out["rois"]),
        L.ptr(out["labels"]), L.ptr(out["reg_targets"]), L.ptr(out["sampled_idx"]), L.ptr(out["n_valid"]), L.ptr(scores), L.ptr(out["obj_all"]),
        L.ptr(out["obj"]), L.ptr(out["pos_rows"]), L.ptr(out["col0"]), int(num_classes), int(bool(cls_agnostic)), L.stream()), "roi_head_targets")
    return out


def roi_head_targets_table(rois, scores, n_out, gt_boxes, gt_labels, hi, lo, weights, batch_size, max_pos, num_classes, cls_agnostic=False,
                           seed=None):
    """roi_head_targets for the pyramid selector's output (rpn_pyramid_select): rois [N,cap,4] / scores [N,cap] / n_out [N] int32, image i's
    proposals being rows [0, n_out[i]) -- no keep lists (include/abr_iod_hip.h, abr_roi_head_targets_table).  Same dict, same three launches,
    no host round trip; the same bits as roi_head_targets given the same candidates and seed."""
    L.require_cuda(rois, scores, n_out)
    if rois.dim() != 3 or rois.shape[2] != 4 or tuple(scores.shape) != tuple(rois.shape[:2]) or n_out.numel() != rois.shape[0]:
        raise ValueError("roi_head_targets_table: rois [N,cap,4], scores [N,cap], n_out [N]; got {}, {}, {}".format(
            tuple(rois.shape), tuple(scores.shape), tuple(n_out.shape)))
    if n_out.dtype != torch.int32:
        raise ValueError("roi_head_targets_table: n_out must be int32, got {}".format(n_out.dtype))
    rois, scores, n_out = L.f32c(rois), L.f32c(scores), n_out.contiguous()
    N, cap, _ = rois.shape
    R = batch_size
    out, (gtb_tab, gtl_tab, ngt_dev) = _roi_head_targets_setup(N, cap, gt_boxes, gt_labels, R, max_pos, rois.device)
    if seed is None:
        seed = _draw_seed()
    L.check(L.lib().abr_roi_head_targets_table(
        L.ptr(rois), L.ptr(scores), L.ptr(n_out), N, cap, L.ptr(gtb_tab), L.ptr(gtl_tab), L.ptr(ngt_dev),
        out["g_max"], float(hi), float(lo), *[float(v) for v in weights], R, max_pos, seed, L.ptr(out["cand"]), L.ptr(out["labels_all"]),
        L.ptr(out["regt_all"]), L.ptr(out["n_cand"]), L.ptr(out["pos_idx"]), L.ptr(out["neg_idx"]), L.ptr(out["counts"]), L.ptr(out["rois"]),
        L.ptr(out["labels"]), L.ptr(out["reg_targets"]), L.ptr(out["sampled_idx"]), L.ptr(out["n_valid"]), L.ptr(out["obj_all"]),
        L.ptr(out["obj"]), L.ptr(out["pos_rows"]), L.ptr(out["col0"]), int(num_classes), int(bool(cls_agnostic)), L.stream()),
        "roi_head_targets_table")
    return out


def rpn_targets_batched(anchors, vis_list, gt_boxes, hi, lo, weights):
    """RPN labels [N,n] (fp32 1 / 0 / -1) and regression targets [N,n,4] for the whole batch in two launches (abr_rpn_targets_batched);
    anchors [n,4] shared, vis_list / gt_boxes per image"""
    n, N, dev = anchors.shape[0], len(gt_boxes), anchors.device
    gtb = [L.f32c(b) for b in gt_boxes]
    n_gt = [int(b.shape[0]) for b in gtb]
    if min(n_gt) == 0:   # matcher.py:53-57
        raise ValueError("No ground-truth boxes available for one of the images during training")
    g_max = max(n_gt)
    labels = torch.empty((N, n), dtype=_f32, device=dev)
    tgt = torch.empty((N, n, 4), dtype=_f32, device=dev)
    ws = torch.empty((N * g_max,), dtype=torch.int32, device=dev)
    gtb_tab, ngt_tab, vis_tab = _pointer_table(gtb, dev), _small_table(n_gt, torch.int32, dev), _pointer_table(vis_list, dev)
    L.check(L.lib().abr_rpn_targets_batched(L.ptr(anchors), n, N, L.ptr(gtb_tab), L.ptr(ngt_tab), g_max,
                                            L.ptr(vis_tab), float(hi), float(lo), *[float(v) for v in weights], L.ptr(labels),
                                            L.ptr(tgt), L.ptr(ws), ws.numel() * 4, L.stream()), "rpn_targets_batched")
    return labels, tgt, (gtb,)


def rpn_loss_indices(pos, neg, counts, A, Cf):
    """-> (samp [n_pos+n_neg], obj_flat, pos_row [n_pos], pos_col [n_pos], denom [1] fp32) from the sampler's padded lists (one launch)"""
    pos, neg = pos.reshape(-1), neg.reshape(-1)
    n_pos, n_neg, dev = pos.numel(), neg.numel(), pos.device
    samp = torch.empty((n_pos + n_neg,), dtype=torch.int64, device=dev)
    obj_flat = torch.empty_like(samp)
    pos_row = torch.empty((n_pos,), dtype=torch.int64, device=dev)
    pos_col = torch.empty_like(pos_row)
    denom = torch.empty((1,), dtype=_f32, device=dev)
    L.check(L.lib().abr_rpn_loss_indices(L.ptr(pos), n_pos, L.ptr(neg), n_neg, L.ptr(counts), counts.shape[0], int(A), int(Cf), L.ptr(samp),
                                         L.ptr(obj_flat), L.ptr(pos_row), L.ptr(pos_col), L.ptr(denom), L.stream()), "rpn_loss_indices")
    return samp, obj_flat, pos_row, pos_col, denom


def _rpn_pyramid_loss_tables(what, ys, A):
    """host arrays of the pyramid loss's entry points; ys: the levels' contiguous fp32 [N,H_l,W_l,Cf] (or [N,nloc_l,Cf]) fused head outputs"""
    nL = len(ys)
    if not 1 <= nL <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"{what}: {nL} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    N, Cf = ys[0].shape[0], ys[0].shape[-1]
    for l, y in enumerate(ys):
        L.require_cuda(y)
        if y.dtype != _f32 or y.dim() not in (3, 4) or not y.is_contiguous() or y.shape[0] != N or y.shape[-1] != Cf:
            raise RuntimeError(f"{what}: level {l} must be a contiguous float32 [N,H,W,Cf] tensor with the batch and width of level 0, got "
                               f"{tuple(y.shape)} {y.dtype}")
    nloc = [y.numel() // (N * Cf) if N else 1 for y in ys]
    return (C.c_void_p * nL)(*[y.data_ptr() for y in ys]), (C.c_int * nL)(*nloc), nloc, N, Cf


def rpn_pyramid_loss(ys, A, labels, reg_targets, pos, neg, counts, want_grad=False):
    """The RPN loss over L levels in one launch (abr_rpn_pyramid_loss).  ys: list of L fused head outputs NHWC [N,H_l,W_l,Cf]; labels [N,n] fp32 and
    reg_targets [N,n,4] over the levels' concatenated anchors (n = A * sum H_l W_l); pos [N,max_pos] / neg [N,batch] / counts [N,2] as sample_pos_neg
    returns them with index_offset_per_image = n.  -> (losses [2] = objectness, box regression; records or None).  The records (dst int64, val fp32)
    are what rpn_pyramid_loss_backward scatters."""
    ys = list(ys)
    yp, nl, nloc, N, Cf = _rpn_pyramid_loss_tables("rpn_pyramid_loss", ys, A)
    L.require_cuda(labels, reg_targets, pos, neg, counts)
    n = int(A) * sum(nloc)
    if labels.dtype != _f32 or not labels.is_contiguous() or labels.numel() != N * n:
        raise RuntimeError(f"rpn_pyramid_loss: labels must be contiguous float32 [{N},{n}], got {tuple(labels.shape)} {labels.dtype}")
    if reg_targets.dtype != _f32 or not reg_targets.is_contiguous() or reg_targets.numel() != N * n * 4:
        raise RuntimeError(f"rpn_pyramid_loss: reg_targets must be contiguous float32 [{N},{n},4], got {tuple(reg_targets.shape)} {reg_targets.dtype}")
    if pos.dtype != torch.int64 or neg.dtype != torch.int64 or counts.dtype != torch.int32 or pos.dim() != 2 or neg.dim() != 2 \
            or pos.shape[0] != N or neg.shape[0] != N or tuple(counts.shape) != (N, 2) \
            or not (pos.is_contiguous() and neg.is_contiguous() and counts.is_contiguous()):
        raise RuntimeError("rpn_pyramid_loss: pos [N,max_pos] / neg [N,batch] int64 and counts [N,2] int32, contiguous, as sample_pos_neg returns them")
    max_pos, batch, dev = pos.shape[1], neg.shape[1], ys[0].device
    losses = torch.empty((2,), dtype=_f32, device=dev)
    rec = None
    if want_grad:
        S, P = N * (max_pos + batch), N * max_pos
        rec = (torch.empty((S + P,), dtype=torch.int64, device=dev), torch.empty((S + 4 * P,), dtype=_f32, device=dev))
    L.check(L.lib().abr_rpn_pyramid_loss(yp, nl, len(ys), N, int(A), Cf, L.ptr(labels), L.ptr(reg_targets), L.ptr(pos), max_pos, L.ptr(neg), batch,
                                         L.ptr(counts), L.ptr(losses), L.ptr(rec[0]) if rec else None, L.ptr(rec[1]) if rec else None, L.stream()),
            "rpn_pyramid_loss")
    return losses, rec


def rpn_pyramid_loss_backward(shapes, A, rec, max_pos, batch, g_obj, g_box, device):
    """shapes: the levels' NHWC shapes (N,H_l,W_l,Cf); rec: rpn_pyramid_loss's records; g_obj / g_box: the upstream gradients of the two losses
    (device scalars).  -> list of L [N,H_l,W_l,Cf] views of ONE zero-filled allocation (levels back to back) holding the dense gradient."""
    shapes = [tuple(int(v) for v in s) for s in shapes]
    nL = len(shapes)
    if not 1 <= nL <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"rpn_pyramid_loss_backward: {nL} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    N, Cf = shapes[0][0], shapes[0][-1]
    nloc = [s[1] * s[2] for s in shapes]
    g_obj, g_box = L.f32c(g_obj), L.f32c(g_box)
    L.require_cuda(rec[0], rec[1], g_obj, g_box)
    S, P = N * (max_pos + batch), N * max_pos
    assert rec[0].numel() == S + P and rec[1].numel() == S + 4 * P and rec[0].dtype == torch.int64 and rec[1].dtype == _f32
    grad = torch.empty((N * sum(nloc) * Cf,), dtype=_f32, device=device)
    L.check(L.lib().abr_rpn_pyramid_loss_backward((C.c_int * nL)(*nloc), nL, N, int(A), Cf, L.ptr(rec[0]), L.ptr(rec[1]), int(max_pos), int(batch),
                                                  L.ptr(g_obj), L.ptr(g_box), L.ptr(grad), L.stream()), "rpn_pyramid_loss_backward")
    out, o = [], 0
    for s, nl in zip(shapes, nloc):
        out.append(grad[o: o + N * nl * Cf].view(s))
        o += N * nl * Cf
    return out


def retina_targets(anchors, gt_boxes, gt_labels, hi, lo, weights=(10.0, 10.0, 5.0, 5.0)):
    """RetinaNet's labelled anchor targets for the whole batch (abr_retina_targets: two launches, nothing read back).  anchors [n,4]: the levels'
    anchors concatenated, shared by the images; gt_boxes / gt_labels: per image [G_i,4] fp32 and [G_i] integer classes (G_i may be 0: every
    anchor of that image is background) -> (labels [N,n] int32: class / 0 background / -1 ignored, reg_targets [N,n,4], n_pos [1] int32)"""
    gt_boxes, gt_labels = list(gt_boxes), list(gt_labels)
    N, dev = len(gt_boxes), anchors.device
    if len(gt_labels) != N:
        raise RuntimeError(f"retina_targets: {N} box tables and {len(gt_labels)} label tables")
    L.require_cuda(anchors, *gt_boxes, *gt_labels)
    anchors = L.f32c(anchors)
    if anchors.dim() != 2 or anchors.shape[1] != 4:
        raise RuntimeError(f"retina_targets: anchors must be [n,4], got {tuple(anchors.shape)}")
    n = anchors.shape[0]
    gtb = [L.f32c(b).reshape(-1, 4) for b in gt_boxes]
    gtl = [l.to(torch.int64).contiguous() for l in gt_labels]
    n_gt = [int(b.shape[0]) for b in gtb]
    if any(l.numel() != g for l, g in zip(gtl, n_gt)):
        raise RuntimeError("retina_targets: every image needs one label per ground-truth box")
    labels = torch.empty((N, n), dtype=torch.int32, device=dev)
    tgt = torch.empty((N, n, 4), dtype=_f32, device=dev)
    n_pos = torch.zeros((1,), dtype=torch.int32, device=dev)
    if N == 0:
        return labels, tgt, n_pos
    gtb_tab, gtl_tab, ngt_tab = _pointer_table(gtb, dev), _pointer_table(gtl, dev), _small_table(n_gt, torch.int32, dev)
    L.check(L.lib().abr_retina_targets(L.ptr(anchors), n, N, L.ptr(gtb_tab), L.ptr(gtl_tab), L.ptr(ngt_tab), max(n_gt), float(hi), float(lo),
                                       *[float(v) for v in weights], L.ptr(labels), L.ptr(tgt), L.ptr(n_pos), L.stream()), "retina_targets")
    del gtb, gtl    # (kept alive until the launch is enqueued: a free is then ordered behind the kernels on this stream)
    return labels, tgt, n_pos


def _retina_loss_tables(what, cls, reg, A, num_classes, labels, reg_targets, n_pos):
    """checks and host tables shared by retina_loss and retina_loss_backward; cls / reg: the levels' contiguous fp32 NHWC head outputs
    [N,H_l,W_l,ld] (or [N,nloc_l,ld])"""
    cls, reg = list(cls), list(reg)
    nL = len(cls)
    if not 1 <= nL <= MAX_PYRAMID_LEVELS:
        raise RuntimeError(f"{what}: {nL} levels, need 1 .. {MAX_PYRAMID_LEVELS}")
    if len(reg) != nL:
        raise RuntimeError(f"{what}: the level lists differ in length")
    N = cls[0].shape[0]
    nloc = []
    for l in range(nL):
        L.require_cuda(cls[l], reg[l])
        for name, t in (("cls", cls[l]), ("reg", reg[l])):
            if t.dtype != _f32 or t.dim() not in (3, 4) or not t.is_contiguous() or t.shape[0] != N:
                raise RuntimeError(f"{what}: {name} of level {l} must be a contiguous float32 [{N},H,W,ld] tensor, got {tuple(t.shape)} {t.dtype}")
        nloc.append(cls[l][0, ..., 0].numel() if N and cls[l].shape[-1] else 1)
        if N and reg[l].shape[-1] and reg[l][0, ..., 0].numel() != nloc[l]:
            raise RuntimeError(f"{what}: cls and reg of level {l} differ in their locations: {tuple(cls[l].shape)} and {tuple(reg[l].shape)}")
    n = int(A) * sum(nloc)
    L.require_cuda(labels, reg_targets, n_pos)
    if labels.dtype != torch.int32 or not labels.is_contiguous() or tuple(labels.shape) != (N, n):
        raise RuntimeError(f"{what}: labels must be contiguous int32 [{N},{n}], got {tuple(labels.shape)} {labels.dtype}")
    if reg_targets.dtype != _f32 or not reg_targets.is_contiguous() or tuple(reg_targets.shape) != (N, n, 4):
        raise RuntimeError(f"{what}: reg_targets must be contiguous float32 [{N},{n},4], got {tuple(reg_targets.shape)} {reg_targets.dtype}")
    if n_pos.dtype != torch.int32 or n_pos.numel() != 1:
        raise RuntimeError(f"{what}: n_pos must be one int32, got {tuple(n_pos.shape)} {n_pos.dtype}")
    vp, ci = C.c_void_p * nL, C.c_int * nL
    tabs = (vp(*[t.data_ptr() for t in cls]), ci(*[t.shape[-1] for t in cls]), vp(*[t.data_ptr() for t in reg]), ci(*[t.shape[-1] for t in reg]),
            ci(*nloc), nL, N, int(A), int(num_classes))
    return cls, reg, nloc, N, tabs


def retina_loss(cls, reg, A, num_classes, labels, reg_targets, n_pos, gamma, alpha, beta, regress_norm):
    """RetinaNet's two losses over L levels in one launch (abr_retina_loss).  cls / reg: lists of L NHWC head outputs [N,H_l,W_l,ldc] (column
    a * C + c; columns >= A * C never read) / [N,H_l,W_l,ldr] (columns 4a .. 4a+3); labels [N,n] int32, reg_targets [N,n,4], n_pos [1] int32 as
    retina_targets returns them -> losses [2] = (focal sum / (n_pos + N), smooth-L1 sum over the positives / max(1, n_pos * regress_norm))"""
    cls, reg, nloc, N, tabs = _retina_loss_tables("retina_loss", cls, reg, A, num_classes, labels, reg_targets, n_pos)
    losses = torch.zeros((2,), dtype=_f32, device=cls[0].device)
    L.check(L.lib().abr_retina_loss(*tabs, L.ptr(labels), L.ptr(reg_targets), L.ptr(n_pos), float(gamma), float(alpha), float(beta),
                                    float(regress_norm), L.ptr(losses), L.stream()), "retina_loss")
    return losses


def retina_loss_backward(cls, reg, A, num_classes, labels, reg_targets, n_pos, gamma, alpha, beta, regress_norm, g_cls, g_reg, out=None):
    """The gradient of retina_loss's two losses times their upstream gradients g_cls / g_reg (device scalars), recomputed from the logits
    (abr_retina_loss_backward: one launch that writes every element) -> (list of L views shaped like cls, list of L views shaped like reg) of
    ONE allocation each, the levels back to back.  out = (d_cls, d_reg): flat fp32 buffers to write into (tests: sentinels)."""
    cls, reg, nloc, N, tabs = _retina_loss_tables("retina_loss_backward", cls, reg, A, num_classes, labels, reg_targets, n_pos)
    dev = cls[0].device
    g_cls, g_reg = L.f32c(g_cls), L.f32c(g_reg)
    L.require_cuda(g_cls, g_reg)
    nc, nr = sum(t.numel() for t in cls), sum(t.numel() for t in reg)
    if out is None:
        out = (torch.empty((nc,), dtype=_f32, device=dev), torch.empty((nr,), dtype=_f32, device=dev))
    d_cls, d_reg = out
    if d_cls.numel() != nc or d_reg.numel() != nr or d_cls.dtype != _f32 or d_reg.dtype != _f32 or not (d_cls.is_contiguous() and d_reg.is_contiguous()):
        raise RuntimeError(f"retina_loss_backward: out must be contiguous float32 buffers of {nc} and {nr} elements")
    L.check(L.lib().abr_retina_loss_backward(*tabs, L.ptr(labels), L.ptr(reg_targets), L.ptr(n_pos), float(gamma), float(alpha), float(beta),
                                             float(regress_norm), L.ptr(g_cls), L.ptr(g_reg), L.ptr(d_cls), L.ptr(d_reg), L.stream()),
            "retina_loss_backward")
    views = []
    for buf, ts in ((d_cls, cls), (d_reg, reg)):
        o, vs = 0, []
        for t in ts:
            vs.append(buf[o: o + t.numel()].view(t.shape))
            o += t.numel()
        views.append(vs)
    return views[0], views[1]


def gather_proposals(props, scores, keep, picks, P):
    """rois [N*P,5] = (i, props[i, keep[i, picks[i*P+j]]]), obj [N*P]: P picked rows per image of the post-NMS lists"""
    N, k_pre, _ = props.shape
    rois = torch.empty((N * P, 5), dtype=_f32, device=props.device)
    obj = torch.empty((N * P,), dtype=_f32, device=props.device)
    L.check(L.lib().abr_gather_proposals(L.ptr(props), L.ptr(scores), L.ptr(keep), N, k_pre, keep.shape[1], L.ptr(picks), P, L.ptr(rois), L.ptr(obj),
                                         L.stream()), "gather_proposals")
    return rois, obj


def sample_pos_neg(labels, batch_size, max_pos, index_offset_per_image=0, seed=None):
    """labels [N,n] (fp32 or int64, rows contiguous) -> pos_idx [N,max_pos] int64, neg_idx [N,batch_size] int64 (-1 padded,
    ascending), counts [N,2] int32 -- all on device, no sync."""
    if labels.dim() == 1:
        labels = labels.view(1, -1)
    N, n = labels.shape
    dev = labels.device
    pos = torch.empty((N, max(max_pos, 1)), dtype=torch.int64, device=dev)
    neg = torch.empty((N, batch_size), dtype=torch.int64, device=dev)
    counts = torch.empty((N, 2), dtype=torch.int32, device=dev)
    if seed is None:
        seed = _draw_seed()
    is64 = labels.dtype == torch.int64
    if not is64 and labels.dtype != _f32:
        raise RuntimeError("sample_pos_neg: labels must be float32 or int64")
    L.check(L.lib().abr_sample_pos_neg(L.ptr(labels), int(is64), N, n, labels.stride(0), batch_size, max_pos, seed, 0,
                                       index_offset_per_image, L.ptr(pos), L.ptr(neg), L.ptr(counts), L.stream()), "sample_pos_neg")
    return pos, neg, counts


# ----------------------------------------------------------------------------------------------- optimiser
def sgd_momentum_(p, g, m, seg_end, lr, wd, momentum, gscale=1.0, first_step=False):
    L.check(L.lib().abr_sgd_momentum(L.ptr(p), L.ptr(g), L.ptr(m), p.numel(), L.ptr(seg_end), L.ptr(lr), L.ptr(wd),
                                     seg_end.numel(), float(momentum), float(gscale), int(first_step), L.stream()), "sgd")


# ----------------------------------------------------------------------------------------------- test-time detections (F4)
def det_softmax_decode(logits, deltas, rois, C, img_hw, weights, cls_agnostic=False):
    """logits [K,>=C] / deltas [K,4C] (row-strided views of the fused predictor output are fine), rois [K,5], img_hw [N,2] int32
    -> prob [K,C], boxes [K,C,4]   (roi_heads/box_head/inference.py:55-70)"""
    L.require_cuda(logits, deltas, rois, img_hw)
    K = logits.shape[0]
    if logits.stride(-1) != 1 or logits.dtype != _f32:
        logits = L.f32c(logits)
    if deltas.stride(-1) != 1 or deltas.dtype != _f32:
        deltas = L.f32c(deltas)
    rois = L.f32c(rois)
    prob = torch.empty((K, C), dtype=_f32, device=logits.device)
    boxes = torch.empty((K, C, 4), dtype=_f32, device=logits.device)
    ld_l = logits.stride(0) if K > 1 else max(logits.shape[1], C)
    ld_d = deltas.stride(0) if K > 1 else max(deltas.shape[1], 4)
    agn = deltas.shape[1] - 4 if cls_agnostic else -1
    L.check(L.lib().abr_det_softmax_decode(L.ptr(logits), ld_l, L.ptr(deltas), ld_d, 0, agn, L.ptr(rois), K, C, L.ptr(img_hw),
                                           *[float(w) for w in weights], L.ptr(prob), L.ptr(boxes), L.stream()), "det_softmax_decode")
    return prob, boxes


def det_select(prob, boxes, row_off, N, C, r_max, score_thresh, nms_thresh, detections_per_img, background=True):
    """filter_results for the batch (inference.py:106-151) -> out_boxes [N,cap,4], out_scores [N,cap], out_labels [N,cap] int64,
    out_count [N] int32, bg_boxes [N,r_max,4], bg_scores [N,r_max], bg_count [N]"""
    L.require_cuda(prob, boxes, row_off)
    dev = prob.device
    cap = (C - 1) * r_max
    ob = torch.empty((N, cap, 4), dtype=_f32, device=dev)
    os_ = torch.empty((N, cap), dtype=_f32, device=dev)
    ol = torch.empty((N, cap), dtype=torch.int64, device=dev)
    oc = torch.empty((N,), dtype=torch.int32, device=dev)
    bb = torch.empty((N, r_max, 4), dtype=_f32, device=dev) if background else None
    bs = torch.empty((N, r_max), dtype=_f32, device=dev) if background else None
    bc = torch.empty((N,), dtype=torch.int32, device=dev) if background else None
    ws_bytes = L.lib().abr_det_select_workspace_bytes(N, C, r_max)
    ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=dev)
    L.check(L.lib().abr_det_select(L.ptr(L.f32c(prob)), L.ptr(L.f32c(boxes)), L.ptr(row_off), N, C, r_max, float(score_thresh),
                                   float(nms_thresh), int(detections_per_img), cap, L.ptr(ob), L.ptr(os_), L.ptr(ol), L.ptr(oc),
                                   L.ptr(bb), L.ptr(bs), L.ptr(bc), L.ptr(ws), ws_bytes, L.stream()), "det_select")
    return ob, os_, ol, oc, bb, bs, bc


# ----------------------------------------------------------------------------------------------- ablation distillation losses
def feat_distill(src, tgt, want_grad=False):
    """normalized_filtered_l1 between two feature maps of equal size (any layout, both the same) -> (loss[1], d_tgt or None)"""
    L.require_cuda(src, tgt)
    assert src.numel() == tgt.numel()
    loss = torch.empty((1,), dtype=_f32, device=tgt.device)
    stats = torch.empty((3,), dtype=_f32, device=tgt.device)
    d = torch.empty_like(tgt, memory_format=torch.preserve_format) if want_grad else None
    L.check(L.lib().abr_feat_distill(L.ptr(src), L.ptr(tgt), tgt.numel(), L.ptr(loss), L.ptr(stats), 1.0, L.ptr(d), L.stream()), "feat_distill")
    return loss, d


def rpn_distill(obj_s, reg_s, obj_t, reg_t, thr, use_bbox, want_grad=False):
    """obj_* [N,H,W,A] / reg_* [N,H,W,4A] NHWC views (row-strided slices of the fused head outputs are fine) ->
    (loss[1], d_obj_t [N,H,W,A] or None, d_reg_t [N,H,W,4A] or None)"""
    L.require_cuda(obj_s, reg_s, obj_t, reg_t)
    N, H, W, A = obj_t.shape
    for t in (obj_s, reg_s, obj_t, reg_t):
        assert t.stride(-1) == 1 and t.stride(0) == H * W * t.stride(2) and t.stride(1) == W * t.stride(2), "expected row-strided NHWC views"
    loss = torch.empty((1,), dtype=_f32, device=obj_t.device)
    d_o = torch.empty((N, H, W, A), dtype=_f32, device=obj_t.device) if want_grad else None
    d_r = torch.empty((N, H, W, 4 * A), dtype=_f32, device=obj_t.device) if want_grad else None
    L.check(L.lib().abr_rpn_distill(L.ptr(obj_s), L.ptr(reg_s), obj_s.stride(2), reg_s.stride(2), L.ptr(obj_t), L.ptr(reg_t), obj_t.stride(2),
                                    reg_t.stride(2), N * H * W, A, float(thr), int(bool(use_bbox)), L.ptr(loss), 1.0, L.ptr(d_o), L.ptr(d_r),
                                    A, 4 * A, L.stream()), "rpn_distill")
    return loss, d_o, d_r


# ----------------------------------------------------------------------------------------------- mask head (csrc/mask.hip)
def mask_compact_pos(labels, p_max):
    """rows with labels > 0 in ascending order, nothing read back: -> (pos_rows [p_max] int64, -1 padded; pos_labels [p_max]; inv [K] =
    position of each row in pos_rows or -1; n_pos int32 [1])"""
    L.require_cuda(labels)
    labels = labels.to(torch.int64).contiguous()
    K, dev = labels.numel(), labels.device
    pos_rows = torch.empty((p_max,), dtype=torch.int64, device=dev)
    pos_labels = torch.empty((p_max,), dtype=torch.int64, device=dev)
    inv = torch.empty((K,), dtype=torch.int64, device=dev)
    n_pos = torch.empty((1,), dtype=torch.int32, device=dev)
    L.check(L.lib().abr_mask_compact_pos(L.ptr(labels), K, int(p_max), L.ptr(pos_rows), L.ptr(pos_labels), L.ptr(inv), L.ptr(n_pos), L.stream()),
            "mask_compact_pos")
    return pos_rows, pos_labels, inv, n_pos


def mask_gather_rows(x, rows):
    """x [n, ...] contiguous fp32 -> [len(rows), ...]: row rows[p] of x, zeros where rows[p] < 0"""
    L.require_cuda(x, rows)
    x = L.f32c(x)
    n_out = rows.numel()
    row = x.numel() // max(x.shape[0], 1) if x.shape[0] else int(torch.Size(x.shape[1:]).numel())
    out = torch.empty((n_out,) + tuple(x.shape[1:]), dtype=_f32, device=x.device)
    L.check(L.lib().abr_mask_gather_rows(L.ptr(x), L.ptr(rows), x.shape[0], n_out, row, L.ptr(out), L.stream()), "mask_gather_rows")
    return out


def mask_targets(masks, gt_boxes, rois, pos_rows, M):
    """masks: per-image [n,H,W] device tensors (all uint8 or all float32), gt_boxes: per-image [n,4]; rois [K,5]; pos_rows [P] -> [P,M,M]"""
    L.require_cuda(rois, pos_rows, *masks)
    dev = rois.device
    u8 = masks[0].dtype == torch.uint8
    for m, g in zip(masks, gt_boxes):
        if m.dtype != (torch.uint8 if u8 else _f32) or m.dim() != 3:
            raise RuntimeError("mask_targets: instance masks must be [n,H,W] tensors, all uint8 or all float32")
        if m.shape[0] != g.shape[0]:
            raise RuntimeError("mask_targets: {} masks for {} ground-truth boxes".format(m.shape[0], g.shape[0]))
    ms = [m.contiguous() for m in masks]
    gs = [L.f32c(g) for g in gt_boxes]
    rois = L.f32c(rois)
    P = pos_rows.numel()
    out = torch.empty((P, M, M), dtype=_f32, device=dev)
    dims = _small_table([v for m in ms for v in m.shape], torch.int32, dev)
    mtab, gtab = _pointer_table(ms, dev), _pointer_table(gs, dev)     # (held in locals until the launch is enqueued: _evict_oldest)
    L.check(L.lib().abr_mask_targets(L.ptr(mtab), L.ptr(dims), int(u8), L.ptr(gtab), L.ptr(rois), L.ptr(pos_rows), P, rois.shape[0], len(ms), int(M),
                                     L.ptr(out), L.stream()), "mask_targets")
    return out


def mask_d2s_bias_relu(y, bias):
    """y [P,h,w,4*Cm] (the deconvolution's GEMM, columns (dy*2+dx)*Cm + co) -> relu(depth_to_space(y) + bias) [P,2h,2w,Cm]"""
    y, bias = L.f32c(y), L.f32c(bias)
    P, h, w, c4 = y.shape
    Cm = c4 // 4
    out = torch.empty((P, 2 * h, 2 * w, Cm), dtype=_f32, device=y.device)
    L.check(L.lib().abr_mask_d2s_bias_relu(L.ptr(y), L.ptr(bias), P, h, w, Cm, L.ptr(out), L.stream()), "mask_d2s_bias_relu")
    return out


def mask_d2s_bias_relu_backward(g, out):
    """g, out [P,2h,2w,Cm] -> the GEMM output's gradient [P,h,w,4*Cm] (ReLU mask of `out` applied)"""
    g, out = L.f32c(g), L.f32c(out)
    P, h2, w2, Cm = out.shape
    gy = torch.empty((P, h2 // 2, w2 // 2, 4 * Cm), dtype=_f32, device=g.device)
    L.check(L.lib().abr_mask_d2s_bias_relu_backward(L.ptr(g), L.ptr(out), P, h2 // 2, w2 // 2, Cm, L.ptr(gy), L.stream()), "mask_d2s_bias_relu_backward")
    return gy


def mask_loss(logits, num_classes, labels, targets, n_pos=None, gscale=1.0, want_grad=False):
    """logits [P,M,M,ldk] NHWC (ldk >= num_classes, % 4 == 0), labels [P] int64 (<= 0: row skipped), targets [P,M,M]; n_pos: device int32
    count of the mean's rows (None: P) -> (loss [1], grad like logits or None)"""
    L.require_cuda(logits, labels, targets)
    logits, targets = L.f32c(logits), L.f32c(targets)
    P, M1, M2, ldk = logits.shape
    loss = _empty((1,), logits)
    grad = torch.empty_like(logits) if want_grad else None
    L.check(L.lib().abr_mask_loss(L.ptr(logits), ldk, int(num_classes), L.ptr(labels), L.ptr(targets), P, M1 * M2, L.ptr(n_pos), L.ptr(loss),
                                  float(gscale), L.ptr(grad), L.stream()), "mask_loss")
    return loss, grad


def mask_select_sigmoid(logits, num_classes, labels):
    """logits [D,M,M,ldk] NHWC, labels [D] -> [D,1,M,M] = sigmoid of channel labels[d]"""
    L.require_cuda(logits, labels)
    logits = L.f32c(logits)
    D, M1, M2, ldk = logits.shape
    out = torch.empty((D, 1, M1, M2), dtype=_f32, device=logits.device)
    L.check(L.lib().abr_mask_select_sigmoid(L.ptr(logits), ldk, int(num_classes), L.ptr(labels.to(torch.int64).contiguous()), D, M1 * M2, L.ptr(out),
                                            L.stream()), "mask_select_sigmoid")
    return out


def mask_paste(prob, boxes, im_h, im_w, thresh=0.5):
    """prob [D,1,M,M], boxes [D,4] xyxy -> uint8 [D,1,im_h,im_w] (Masker, padding 1)"""
    L.require_cuda(prob, boxes)
    prob, boxes = L.f32c(prob), L.f32c(boxes)
    D, M = prob.shape[0], prob.shape[-1]
    out = torch.empty((D, 1, im_h, im_w), dtype=torch.uint8, device=prob.device)
    L.check(L.lib().abr_mask_paste(L.ptr(prob), L.ptr(boxes), D, M, int(im_h), int(im_w), float(thresh), L.ptr(out), L.stream()), "mask_paste")
    return out


# ----------------------------------------------------------------------------------------------- mask evaluation (csrc/mask_eval.hip)
def mask_words_per_row(width):
    return (int(width) + 63) // 64


def _mask_result(op, n, h, w, packed, out, device):
    """(shape, dtype) of `op`'s instance masks -- uint8 [n,h,w], or packed the int64 [n,h,ceil(w/64)] words of mask_pack_bits -- after checking
    a caller's `out` against them (`device` without an index, as in "cuda": any device of that type)"""
    shape = (n, h, mask_words_per_row(w)) if packed else (n, h, w)
    dtype = torch.int64 if packed else torch.uint8
    if out is not None and (tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous() or out.device.type != device.type
                            or (device.index is not None and out.device != device)):
        raise RuntimeError("{}: `out` must be a contiguous {} tensor of shape {} on {}".format(op, dtype, shape, device))
    return shape, dtype


def _pack_bits_host(m, w):
    """CPU uint8 masks [n,h,w] -> their mask_pack_bits words, for the host codecs' packed=True"""
    n, h, wq = m.shape[0], m.shape[1], mask_words_per_row(w)
    px = torch.zeros((n, h, wq * 64), dtype=torch.int64)
    px[:, :, :w] = m
    return (px.reshape(n, h, wq, 64) << torch.arange(64, dtype=torch.int64)).sum(-1)


def mask_pack_bits(masks):
    """masks [n,H,W] uint8 or float32 -> int64 [n,H,ceil(W/64)]: bit x % 64 of word x // 64 is set iff masks[i,y,x] == 1"""
    L.require_cuda(masks)
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, _f32):
        raise RuntimeError("mask_pack_bits: expected [n,H,W] uint8 or float32 masks, got {} {}".format(tuple(masks.shape), masks.dtype))
    masks = masks.contiguous()
    n, H, W = masks.shape
    bits = torch.empty((n, H, mask_words_per_row(W)), dtype=torch.int64, device=masks.device)
    L.check(L.lib().abr_mask_pack_bits(L.ptr(masks), int(masks.dtype == torch.uint8), n, H, W, L.ptr(bits), L.stream()), "mask_pack_bits")
    return bits


def mask_resize_pack_bits(masks, height, width):
    """uint8 masks [n,Hs,Ws] -> the packed bits [n,height,ceil(width/64)] of their bilinear resize (align_corners=False, truncated to
    uint8, == 1): what BinaryMaskList.resize((width, height)) followed by mask_pack_bits gives, without the resized image"""
    L.require_cuda(masks)
    if masks.dim() != 3 or masks.dtype != torch.uint8:
        raise RuntimeError("mask_resize_pack_bits: expected [n,H,W] uint8 masks, got {} {}".format(tuple(masks.shape), masks.dtype))
    masks = masks.contiguous()
    n, Hs, Ws = masks.shape
    bits = torch.empty((n, int(height), mask_words_per_row(width)), dtype=torch.int64, device=masks.device)
    L.check(L.lib().abr_mask_resize_pack_bits(L.ptr(masks), n, Hs, Ws, int(height), int(width), L.ptr(bits), L.stream()), "mask_resize_pack_bits")
    return bits


def mask_pair_counts(pred_bits, gt_bits, width, pred_labels=None, gt_labels=None):
    """pred_bits [P,H,Wq], gt_bits [T,H,Wq] (mask_pack_bits of masks `width` wide) -> (inter [P,T], area_p [P], area_t [T]) int32 pixel
    counts; with both label vectors, pairs of different labels are 0 and are not read"""
    L.require_cuda(pred_bits, gt_bits)
    if pred_bits.dtype != torch.int64 or gt_bits.dtype != torch.int64 or pred_bits.dim() != 3 or pred_bits.shape[1:] != gt_bits.shape[1:]:
        raise RuntimeError("mask_pair_counts: expected int64 [P,H,Wq] and [T,H,Wq] of one image size")
    if (pred_labels is None) != (gt_labels is None):
        raise RuntimeError("mask_pair_counts: labels must be given for both sides or neither")
    pred_bits, gt_bits = pred_bits.contiguous(), gt_bits.contiguous()
    P, H, Wq = pred_bits.shape
    T, dev = gt_bits.shape[0], pred_bits.device
    if P == 0 or T == 0:
        z = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)    # noqa: E731
        return z(P, T), z(P), z(T)
    if pred_labels is not None:
        pred_labels = pred_labels.to(device=dev, dtype=torch.int64).contiguous()
        gt_labels = gt_labels.to(device=dev, dtype=torch.int64).contiguous()
        if pred_labels.numel() != P or gt_labels.numel() != T:
            raise RuntimeError("mask_pair_counts: {} / {} labels for {} / {} masks".format(pred_labels.numel(), gt_labels.numel(), P, T))
    inter = torch.empty((P, T), dtype=torch.int32, device=dev)
    area_p = torch.empty((P,), dtype=torch.int32, device=dev)
    area_t = torch.empty((T,), dtype=torch.int32, device=dev)
    L.check(L.lib().abr_mask_pair_counts(L.ptr(pred_bits), L.ptr(gt_bits), L.ptr(pred_labels), L.ptr(gt_labels), P, T, H, int(width), H * Wq,
                                         L.ptr(inter), L.ptr(area_p), L.ptr(area_t), L.stream()), "mask_pair_counts")
    return inter, area_p, area_t


# ----------------------------------------------------------------------------------------------- COCO run-length masks (csrc/rle.hip)
_RLE_ERRORS = {-1: "the last value of the counts string is cut short", -2: "a character of the counts string is outside [48, 111]",
               -3: "a value of the counts string is longer than 7 characters or outside int32", -4: "a negative run length"}


def _rle_payload(rles, h, w):
    """checks each dict's "size" and -> (compressed?, [bytes or int32 array per instance])"""
    import numpy as np
    from .structures.rle import RLEError, counts_to_string
    items = []
    for i, r in enumerate(rles):
        if not isinstance(r, dict) or "counts" not in r or "size" not in r:
            raise RLEError("RLE instance {}: expected a dict with 'size' and 'counts', got {!r}".format(i, type(r).__name__))
        if tuple(int(v) for v in r["size"]) != (h, w):
            raise RLEError("RLE instance {}: its size {} is not the expected (h, w) = {}".format(i, list(r["size"]), (h, w)))
        c = r["counts"]
        items.append(c.encode("ascii") if isinstance(c, str) else (bytes(c) if isinstance(c, (bytes, bytearray)) else [int(v) for v in c]))
    compressed = any(isinstance(c, bytes) for c in items)
    if compressed:        # (a list among strings: one form per call, so it is written as a string here)
        items = [c if isinstance(c, bytes) else counts_to_string(c).encode("ascii") for c in items]
        return True, [np.frombuffer(c, np.uint8) for c in items]
    for i, c in enumerate(items):
        if any(v < 0 or v > 0x7fffffff for v in c):
            raise RLEError("RLE instance {}: a negative run length".format(i) if min(c) < 0 else "RLE instance {}: a run length outside int32".format(i))
    return False, [np.asarray(c, np.int32).reshape(-1) for c in items]


def rle_decode(rles, size, device="cuda", packed=False, out=None):
    """list of COCO RLE dicts of one image -> its instance masks on `device`: uint8 [n,h,w] of 0 / 1, or with packed=True the int64
    [n,h,ceil(w/64)] words of mask_pack_bits (the bytes are never written).  size = (h, w) as in the dicts' "size".  counts may be str, bytes
    or a list of ints.  One upload (offsets + counts), one launch chain, one [n]-element read-back of the sums that tells a malformed
    annotation: structures.rle.RLEError names the instance.  `out`: a contiguous tensor of the result's shape and dtype to decode into.
    device "cpu": the host codec (structures/rle.py)."""
    import numpy as np
    from .structures.rle import RLEError
    h, w = int(size[0]), int(size[1])
    device = torch.device(device)
    n = len(rles)
    shape, dtype = _mask_result("rle_decode", n, h, w, packed, out, device)
    if device.type == "cpu":
        from .structures import rle as host
        m = torch.from_numpy(host.decode(list(rles), (h, w)))
        if packed:
            m = _pack_bits_host(m, w)
        return m if out is None else out.copy_(m)
    if h <= 0 or w <= 0 or h * w >= 2 ** 31:
        raise RuntimeError("rle_decode: bad size {}".format((h, w)))
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    if n == 0:
        return out
    compressed, items = _rle_payload(rles, h, w)
    lens = np.array([len(c) for c in items], np.int64)
    offsets = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    n_items = int(offsets[-1])
    item = 1 if compressed else 4
    host = np.zeros(8 * (n + 1) + (n_items * item + 7) // 8 * 8, np.uint8)          # offsets, then the items: ONE upload
    host[: 8 * (n + 1)] = offsets.view(np.uint8)
    if n_items:
        host[8 * (n + 1): 8 * (n + 1) + n_items * item] = np.concatenate(items).view(np.uint8)
    with torch.cuda.device(device):
        buf = torch.from_numpy(host).to(device)
        payload = buf[8 * (n + 1):]
        ws_bytes = L.lib().abr_rle_decode_workspace_bytes(n, n_items)
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=device)
        totals = torch.empty((n,), dtype=torch.int64, device=device)
        L.check(L.lib().abr_rle_decode(L.ptr(payload) if compressed else None, None if compressed else L.ptr(payload), L.ptr(buf), n, n_items, h, w,
                                       None if packed else L.ptr(out), L.ptr(out) if packed else None, L.ptr(totals), L.ptr(ws), ws_bytes, L.stream()),
                "rle_decode")
        got = totals.cpu().tolist()
    for i, t in enumerate(got):
        if t != h * w:
            raise RLEError("RLE instance {}: {}".format(i, _RLE_ERRORS.get(t, "its counts sum to {}, not to h * w = {}".format(t, h * w))))
    return out


def rle_encode(masks, width=None):
    """uint8 [n,h,w] device masks (a pixel is set iff it == 1), a PackedMasks, or int64 packed words [n,h,ceil(width/64)] with `width` ->
    list of {"size": [h, w], "counts": str}, encoded on the device.  Capacity protocol (abr_rle_encode): the call gets room for
    max(1024, h * w / 16) characters per instance; the per-instance offsets are read back (one small copy), and only when their last entry
    says the room was too small -- masks close to noise -- the call is repeated with exactly that many bytes; then the characters are
    downloaded, exactly as many as were written."""
    if hasattr(masks, "bits") and hasattr(masks, "size"):
        masks, width = masks.bits, masks.size[0]
    L.require_cuda(masks)
    if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.int64) or (masks.dtype == torch.int64 and width is None):
        raise RuntimeError("rle_encode: expected uint8 [n,h,w] masks, a PackedMasks, or int64 words with `width`; got {} {}".format(
            tuple(masks.shape), masks.dtype))
    masks = masks.contiguous()
    is_bits = masks.dtype == torch.int64
    n, h = int(masks.shape[0]), int(masks.shape[1])
    w = int(width) if is_bits else int(masks.shape[2])
    if is_bits and masks.shape[2] != mask_words_per_row(w):
        raise RuntimeError("rle_encode: words of shape {} do not pack masks {} wide".format(tuple(masks.shape), w))
    if n == 0:
        return []
    dev = masks.device
    head = 8 * (n + 1) + (4 * n + 7) // 8 * 8
    with torch.cuda.device(dev):
        ws_bytes = L.lib().abr_rle_encode_workspace_bytes(n, h, w)
        if ws_bytes < 0:
            raise RuntimeError("rle_encode: bad size {}".format((h, w)))
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)
        capacity = n * max(1024, h * w // 16)
        while True:
            buf = torch.empty((head + capacity,), dtype=torch.uint8, device=dev)     # offsets [n+1] int64 | nruns [n] int32 | characters
            L.check(L.lib().abr_rle_encode(None if is_bits else L.ptr(masks), L.ptr(masks) if is_bits else None, n, h, w, L.ptr(buf[head:]), capacity,
                                           L.ptr(buf), L.ptr(buf[8 * (n + 1):]), L.ptr(ws), ws_bytes, L.stream()), "rle_encode")
            offsets = buf[: 8 * (n + 1)].cpu().numpy().view("int64")
            total = int(offsets[-1])
            if total <= capacity:
                break
            capacity = total
        chars = buf[head: head + total].cpu().numpy().tobytes()
    return [{"size": [h, w], "counts": chars[int(offsets[i]): int(offsets[i + 1])].decode("ascii")} for i in range(n)]


# ----------------------------------------------------------------------------------------------- polygon masks (csrc/poly.hip)
def poly_rasterize(polys, packed=False, out=None, return_status=False):
    """PolygonList of one image -> its instance masks where the list is: uint8 [n,h,w] of 0 / 1, or with packed=True the int64
    [n,h,ceil(w/64)] words of mask_pack_bits (the bytes are never written).  What pycocotools' frPyObjects + merge + decode give
    (DESIGN.md §4); an instance is the OR of its polygons.  `out`: a contiguous tensor of the result's shape and dtype to write into.
    return_status=True: -> (masks, status int32 [n]), status[i] != 0 when a polygon of instance i was left out by the guard (a non-finite
    coordinate: 1, one beyond +-32768 pixels: 2); nothing is read back.  A list on the CPU: the host codec (structures/polygon.py)."""
    w, h = polys.int_size()
    device = polys.coords.device
    n = len(polys)
    shape, dtype = _mask_result("poly_rasterize", n, h, w, packed, out, device)
    if device.type == "cpu":
        from .structures import polygon as host
        m, st = host.rasterize(polys.coords.numpy(), polys._po, polys._io, h, w)
        m, status = torch.from_numpy(m), torch.from_numpy(st)
        if packed:
            m = _pack_bits_host(m, w)
        m = m if out is None else out.copy_(m)
        return (m, status) if return_status else m
    if h * w >= 2 ** 31 - 64:
        raise RuntimeError("poly_rasterize: bad size {}".format((h, w)))
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=device)
    status = torch.zeros((n,), dtype=torch.int32, device=device)
    if n:
        coords = L.f32c(polys.coords)
        po, io = polys.poly_offsets.contiguous(), polys.inst_offsets.contiguous()
        n_poly = po.numel() - 1
        with torch.cuda.device(device):
            ws_bytes = L.lib().abr_poly_rasterize_workspace_bytes(n_poly, h, w)
            ws = torch.empty((max(ws_bytes, 8),), dtype=torch.uint8, device=device)
            L.check(L.lib().abr_poly_rasterize(L.ptr(coords), L.ptr(po), L.ptr(io), n, n_poly, coords.shape[0], h, w, None if packed else L.ptr(out),
                                               L.ptr(out) if packed else None, L.ptr(status), L.ptr(ws), ws_bytes, L.stream()), "poly_rasterize")
    return (out, status) if return_status else out


def poly_mask_targets(polys_per_image, gt_boxes, rois, pos_rows, M):
    """polys_per_image: per-image PolygonList on the device, gt_boxes: per-image [n,4]; rois [K,5]; pos_rows [P] -> [P,M,M]: for each row the
    polygons of the matched instance (first maximum IoU, as mask_targets) through PolygonInstance.crop(box).resize((M, M)), rasterised on the
    M x M grid -- the reference's project_masks_on_boxes (mask_head/loss.py:11-42) for polygon targets, one launch for the batch"""
    L.require_cuda(rois, pos_rows, *[p.coords for p in polys_per_image])
    dev = rois.device
    if len(polys_per_image) != len(gt_boxes) or not len(gt_boxes):
        raise RuntimeError("poly_mask_targets: {} polygon lists for {} images".format(len(polys_per_image), len(gt_boxes)))
    dims = []
    for p, g in zip(polys_per_image, gt_boxes):
        if len(p) != g.shape[0]:
            raise RuntimeError("poly_mask_targets: {} polygon instances for {} ground-truth boxes".format(len(p), g.shape[0]))
        w, h = p.int_size()
        dims += [len(p), len(p._po) - 1, int(p.coords.shape[0]), h, w]
    if int(M) > 64:
        raise RuntimeError("poly_mask_targets: M = {} (the kernel's grid holds M <= 64)".format(M))
    cs = [L.f32c(p.coords) for p in polys_per_image]
    pos = [p.poly_offsets.contiguous() for p in polys_per_image]
    ios = [p.inst_offsets.contiguous() for p in polys_per_image]
    gs = [L.f32c(g) for g in gt_boxes]
    rois = L.f32c(rois)
    N, P = len(gs), pos_rows.numel()
    out = torch.empty((P, M, M), dtype=_f32, device=dev)
    dtab = h2d(dims, torch.int32, dev)
    tab = _pointer_table(cs + pos + ios + gs, dev)     # ONE upload: four tables of N addresses (held in locals until the launch: _evict_oldest)
    t0 = L.ptr(tab)
    L.check(L.lib().abr_poly_mask_targets(t0, t0 + 8 * N, t0 + 16 * N, L.ptr(dtab), t0 + 24 * N, L.ptr(rois), L.ptr(pos_rows), P, rois.shape[0], N, int(M),
                                          L.ptr(out), L.stream()), "poly_mask_targets")
    return out


# ----------------------------------------------------------------------------------------------- keypoint head (csrc/keypoint.hip)
def kp_pad(K):
    """the planar heat maps' channel count: K rounded up to a multiple of 4"""
    return (int(K) + 3) // 4 * 4


def kp_select_targets(rois, labels, gt_boxes, keypoints, M, p_max):
    """rois [R,5] / labels [R]: the box head's sampled set; gt_boxes: per-image [n,4]; keypoints: per-image [n,K,3] (x, y, visibility)
    -> dict(pos_rows [p_max] int64 (-1 padded, ascending), inv [R], n_pos int32 [1], targets [p_max,K] int64, valid [p_max,K] uint8,
    n_valid int32 [1]): the positives whose matched instance has a visible keypoint inside its box, and their heat-map indices on the
    M x M map (abr_kp_select_targets); nothing is read back"""
    L.require_cuda(rois, labels, *keypoints)
    dev = rois.device
    if len(gt_boxes) != len(keypoints) or not len(gt_boxes):
        raise RuntimeError("kp_select_targets: {} keypoint tensors for {} images".format(len(keypoints), len(gt_boxes)))
    K = int(keypoints[0].shape[1])
    for k, g in zip(keypoints, gt_boxes):
        if k.dim() != 3 or k.shape[1] != K or k.shape[2] != 3 or k.shape[0] != g.shape[0]:
            raise RuntimeError("kp_select_targets: keypoints must be [n,{},3] with one row per ground-truth box, got {} for {} boxes".format(
                K, tuple(k.shape), g.shape[0]))
    ks, gs = [L.f32c(k) for k in keypoints], [L.f32c(g) for g in gt_boxes]
    rois, labels = L.f32c(rois), labels.to(torch.int64).contiguous()
    R, N, p_max = labels.numel(), len(gs), int(p_max)
    i64 = torch.int64
    out = dict(pos_rows=torch.empty((p_max,), dtype=i64, device=dev), inv=torch.empty((R,), dtype=i64, device=dev),
               n_pos=torch.empty((1,), dtype=torch.int32, device=dev), targets=torch.empty((p_max, K), dtype=i64, device=dev),
               valid=torch.empty((p_max, K), dtype=torch.uint8, device=dev), n_valid=torch.empty((1,), dtype=torch.int32, device=dev))
    n_gt = _small_table([int(g.shape[0]) for g in gs], torch.int32, dev)
    tab = _pointer_table(gs + ks, dev)       # ONE upload: two tables of N addresses (held in a local until the launch: _evict_oldest)
    t0 = L.ptr(tab)
    L.check(L.lib().abr_kp_select_targets(L.ptr(rois), L.ptr(labels), R, t0, t0 + 8 * N, L.ptr(n_gt), N, K, int(M), p_max, L.ptr(out["pos_rows"]),
                                          L.ptr(out["inv"]), L.ptr(out["n_pos"]), L.ptr(out["targets"]), L.ptr(out["valid"]),
                                          L.ptr(out["n_valid"]), L.stream()), "kp_select_targets")
    return out


def kp_deconv_fold(y, bias):
    """y [P,h,w,16*Kp] (the deconvolution's GEMM, columns (ky*4+kx)*Kp + k), bias [K] -> planar [P,Kp,2h,2w] = ConvTranspose2d(., K, 4, 2, 1);
    the planes k >= K are zeros"""
    L.require_cuda(y, bias)
    y, bias = L.f32c(y), L.f32c(bias)
    P, h, w, c = y.shape
    K = bias.numel()
    Kp = kp_pad(K)
    if c != 16 * Kp:
        raise RuntimeError("kp_deconv_fold: {} columns for {} keypoints (want 16 * {})".format(c, K, Kp))
    out = torch.empty((P, Kp, 2 * h, 2 * w), dtype=_f32, device=y.device)
    L.check(L.lib().abr_kp_deconv_fold(L.ptr(y), L.ptr(bias), P, h, w, K, L.ptr(out), L.stream()), "kp_deconv_fold")
    return out


def kp_deconv_unfold(g, K):
    """the fold's adjoint: g [P,Kp,2h,2w] -> [P,h,w,16*Kp] (zeros outside the map and in the columns k >= K)"""
    L.require_cuda(g)
    g = L.f32c(g)
    P, Kp, H, W = g.shape
    if Kp != kp_pad(K) or H % 2 or W % 2:
        raise RuntimeError("kp_deconv_unfold: a {} gradient for {} keypoints".format(tuple(g.shape), K))
    gy = torch.empty((P, H // 2, W // 2, 16 * Kp), dtype=_f32, device=g.device)
    L.check(L.lib().abr_kp_deconv_unfold(L.ptr(g), P, H // 2, W // 2, int(K), L.ptr(gy), L.stream()), "kp_deconv_unfold")
    return gy


def kp_upsample2x(x, K):
    """planar x [P,Kp,H,W] -> [P,K,2H,2W]: interpolate(scale_factor=2, mode="bilinear", align_corners=False) of the first K channels"""
    L.require_cuda(x)
    x = L.f32c(x)
    P, Kp, H, W = x.shape
    if Kp != kp_pad(K):
        raise RuntimeError("kp_upsample2x: {} channels for {} keypoints".format(Kp, K))
    out = torch.empty((P, int(K), 2 * H, 2 * W), dtype=_f32, device=x.device)
    L.check(L.lib().abr_kp_upsample2x(L.ptr(x), P, int(K), H, W, L.ptr(out), L.stream()), "kp_upsample2x")
    return out


def kp_loss(x, K, targets, valid, n_valid, gscale=1.0, want_grad=False):
    """x [P,Kp,H,W] planar low-resolution maps; targets [P,K] int64 / valid [P,K] uint8 on the UPSAMPLED 2H x 2W map; n_valid device int32
    -> (loss [1], grad like x or None, row_sum [P,Kp] or None): 2x bilinear upsampling + cross-entropy over each valid row's 4 H W logits,
    mean over n_valid rows (0: loss 0, zero gradients); the gradient is with respect to x"""
    L.require_cuda(x, targets, valid, n_valid)
    x = L.f32c(x)
    P, Kp, H, W = x.shape
    if Kp != kp_pad(K) or tuple(targets.shape) != (P, K) or tuple(valid.shape) != (P, K):
        raise RuntimeError("kp_loss: maps {} with targets {} / valid {} for {} keypoints".format(tuple(x.shape), tuple(targets.shape), tuple(valid.shape), K))
    if targets.dtype != torch.int64 or valid.dtype != torch.uint8 or n_valid.dtype != torch.int32:
        raise RuntimeError("kp_loss: targets int64, valid uint8, n_valid int32")
    loss = _empty((1,), x)
    grad = torch.empty_like(x) if want_grad else None
    row_sum = torch.empty((P, Kp), dtype=_f32, device=x.device) if want_grad else None
    L.check(L.lib().abr_kp_loss(L.ptr(x), P, int(K), H, W, L.ptr(targets.contiguous()), L.ptr(valid.contiguous()), L.ptr(n_valid), float(gscale),
                                L.ptr(loss), L.ptr(grad), L.ptr(row_sum), L.stream()), "kp_loss")
    return loss, grad, row_sum


def kp_decode(maps, boxes):
    """maps [D,K,Hm,Wm] (each plane contiguous), boxes [D,4] xyxy -> (keypoints [D,K,3] = (x, y, 1), logits [D,K]): heatmaps_to_keypoints
    (keypoint_head/inference.py:40-94) on the device -- the bicubic resize to the RoI restated, first maximum in row-major order"""
    L.require_cuda(maps, boxes)
    if maps.dtype != _f32 or maps.dim() != 4:
        raise RuntimeError("kp_decode: maps must be float32 [D,K,Hm,Wm]")
    D, K, Hm, Wm = maps.shape
    if D and (maps.stride(3) != 1 or maps.stride(2) != Wm):
        maps = maps.contiguous()
    boxes = L.f32c(boxes)
    if tuple(boxes.shape) != (D, 4):
        raise RuntimeError("kp_decode: {} boxes for {} maps".format(tuple(boxes.shape), D))
    xy = torch.empty((D, K, 3), dtype=_f32, device=maps.device)
    logit = torch.empty((D, K), dtype=_f32, device=maps.device)
    if D:
        L.check(L.lib().abr_kp_decode(L.ptr(maps), maps.stride(0), maps.stride(1), L.ptr(boxes), D, K, Hm, Wm, L.ptr(xy), L.ptr(logit), L.stream()),
                "kp_decode")
    return xy, logit


# ----------------------------------------------------------------------------------------------- COCO scoring (csrc/coco_eval.hip)
COCO_MATCH_MAX_GT = 128      # ABR_COCO_MATCH_MAX_GT: the ground truths per group coco_match's kernel holds


def _coco_offsets(counts, dev):
    """per-group counts -> (int64 numpy [n+1] offsets, the same on `dev`)"""
    import numpy as np
    off = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(np.asarray(counts, np.int64), out=off[1:])
    return off, torch.from_numpy(off).to(dev)


def _f64_dev(a, dev, shape):
    import numpy as np
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.float64).reshape(shape).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(shape))).to(dev)


def _u8_dev(a, dev):
    import numpy as np
    if isinstance(a, torch.Tensor):
        return a.to(device=dev, dtype=torch.uint8).reshape(-1).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(np.uint8).reshape(-1))).to(dev)


def coco_box_iou(det, gt, gt_crowd, det_counts, gt_counts, device="cuda"):
    """pycocotools' bbIou for every group of a batch in one launch.  det [D_total,4], gt [G_total,4] xywh (float64; numpy or tensors),
    gt_crowd [G_total]; det_counts / gt_counts: detections / ground truths per group.  -> (iou float64 device [sum D_k * G_k], the groups'
    row-major D_k x G_k matrices one after the other; iou_off int64 numpy [n+1])"""
    import numpy as np
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("coco_box_iou runs on the device; the host restatement is evaluation/coco/coco_eval_host.py")
    det_counts, gt_counts = np.asarray(det_counts, np.int64).reshape(-1), np.asarray(gt_counts, np.int64).reshape(-1)
    if det_counts.shape != gt_counts.shape or (det_counts < 0).any() or (gt_counts < 0).any():
        raise RuntimeError("coco_box_iou: one non-negative detection count and ground-truth count per group")
    n = len(det_counts)
    with torch.cuda.device(dev):
        det_off, det_off_d = _coco_offsets(det_counts, dev)
        gt_off, gt_off_d = _coco_offsets(gt_counts, dev)
        iou_off, iou_off_d = _coco_offsets(det_counts * gt_counts, dev)
        det, gt, crowd = _f64_dev(det, dev, (-1, 4)), _f64_dev(gt, dev, (-1, 4)), _u8_dev(gt_crowd, dev)
        if det.shape[0] != det_off[-1] or gt.shape[0] != gt_off[-1] or crowd.numel() != gt_off[-1]:
            raise RuntimeError("coco_box_iou: {} detections / {} ground truths / {} crowd flags for counts that sum to {} / {}".format(
                det.shape[0], gt.shape[0], crowd.numel(), det_off[-1], gt_off[-1]))
        total = int(iou_off[-1])
        iou = torch.empty((total,), dtype=torch.float64, device=dev)
        if n and total:
            L.check(L.lib().abr_coco_box_iou(L.ptr(det), L.ptr(gt), L.ptr(crowd), L.ptr(det_off_d), L.ptr(gt_off_d), L.ptr(iou_off_d), n, total,
                                             L.ptr(iou), L.stream()), "coco_box_iou")
    return iou, iou_off


def coco_mask_iou(inter, area_p, area_t, gt_crowd):
    """the int32 counts of mask_pair_counts for one image + gt_crowd [T] -> float64 [P,T] mask IoU as pycocotools' rleIou defines it:
    inter / (area_p + area_t - inter), inter / area_p for a crowd ground truth, 0 where the masks do not meet"""
    L.require_cuda(inter, area_p, area_t)
    if inter.dtype != torch.int32 or area_p.dtype != torch.int32 or area_t.dtype != torch.int32 or inter.dim() != 2:
        raise RuntimeError("coco_mask_iou: expected the int32 [P,T], [P], [T] counts of mask_pair_counts")
    P, T = inter.shape
    dev = inter.device
    crowd = _u8_dev(gt_crowd, dev)
    if area_p.numel() != P or area_t.numel() != T or crowd.numel() != T:
        raise RuntimeError("coco_mask_iou: {} / {} areas and {} crowd flags for {} x {} counts".format(area_p.numel(), area_t.numel(), crowd.numel(), P, T))
    iou = torch.empty((P, T), dtype=torch.float64, device=dev)
    if P and T:
        with torch.cuda.device(dev):
            L.check(L.lib().abr_coco_mask_iou(L.ptr(inter.contiguous()), L.ptr(area_p.contiguous()), L.ptr(area_t.contiguous()), L.ptr(crowd), P, T,
                                              L.ptr(iou), L.stream()), "coco_mask_iou")
    return iou


def coco_oks(det_kp, gt_kp, gt_box, gt_area, sigmas, det_counts, gt_counts, device="cuda"):
    """pycocotools' computeOks for every group of a batch in one launch.  det_kp [D_total,K,3], gt_kp [G_total,K,3] (x, y, visibility),
    gt_box [G_total,4] xywh, gt_area [G_total], sigmas [K] (float64; numpy or tensors); det_counts / gt_counts: detections / ground truths
    per group.  -> (oks float64 device [sum D_k * G_k] in coco_box_iou's layout, iou_off int64 numpy [n+1])"""
    import numpy as np
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("coco_oks runs on the device; the host restatement is evaluation/coco/coco_eval_host.py")
    det_counts, gt_counts = np.asarray(det_counts, np.int64).reshape(-1), np.asarray(gt_counts, np.int64).reshape(-1)
    if det_counts.shape != gt_counts.shape or (det_counts < 0).any() or (gt_counts < 0).any():
        raise RuntimeError("coco_oks: one non-negative detection count and ground-truth count per group")
    n = len(det_counts)
    with torch.cuda.device(dev):
        var = (_f64_dev(sigmas, dev, (-1,)) * 2) ** 2
        K = var.numel()
        if K < 1:
            raise RuntimeError("coco_oks: no sigmas (one per keypoint)")
        det_off, det_off_d = _coco_offsets(det_counts, dev)
        gt_off, gt_off_d = _coco_offsets(gt_counts, dev)
        iou_off, iou_off_d = _coco_offsets(det_counts * gt_counts, dev)
        det_kp, gt_kp = _f64_dev(det_kp, dev, (-1, K, 3)), _f64_dev(gt_kp, dev, (-1, K, 3))
        gt_box, gt_area = _f64_dev(gt_box, dev, (-1, 4)), _f64_dev(gt_area, dev, (-1,))
        if det_kp.shape[0] != det_off[-1] or gt_kp.shape[0] != gt_off[-1] or gt_box.shape[0] != gt_off[-1] or gt_area.numel() != gt_off[-1]:
            raise RuntimeError("coco_oks: {} detections / {} ground truths / {} boxes / {} areas of {} keypoints for counts that sum to {} / {}".format(
                det_kp.shape[0], gt_kp.shape[0], gt_box.shape[0], gt_area.numel(), K, det_off[-1], gt_off[-1]))
        total = int(iou_off[-1])
        oks = torch.empty((total,), dtype=torch.float64, device=dev)
        if n and total:
            L.check(L.lib().abr_coco_oks(L.ptr(det_kp), L.ptr(gt_kp), L.ptr(gt_box), L.ptr(gt_area), L.ptr(var), K, L.ptr(det_off_d), L.ptr(gt_off_d),
                                         L.ptr(iou_off_d), n, total, L.ptr(oks), L.stream()), "coco_oks")
    return oks, iou_off


def coco_match(iou, det_counts, gt_counts, det_area, gt_area, gt_crowd, area_rng, thrs, device="cuda", gt_ignore=None):
    """pycocotools' evaluateImg for every group of a batch, all area ranges and all IoU thresholds in one launch.  iou: the flat float64
    matrices of coco_box_iou's layout (device tensor or numpy); det_area [D_total], gt_area [G_total], gt_crowd [G_total]; area_rng [A,2]
    (inclusive); thrs [T] float64, used as given.  -> dict of numpy arrays:
        dt_gt   int32 [A,T,D_total]  the matched ground truth's row in its group, -1 = unmatched
        dt_ig   bool  [A,T,D_total]  the detection is ignored
        gt_ig   bool  [A,G_total]    the ground truth is ignored
    gt_ignore [G_total]: the protocol's `ignore` flag of a ground truth (keypoints: crowd or no labelled keypoint); None = gt_crowd, as
    for boxes and masks.  It decides beside the area range whether a ground truth is ignored; gt_crowd alone lets one match again.
        n_fallback                   groups with more than COCO_MATCH_MAX_GT ground truths: scored by the host restatement
                                     (coco_eval_host.evaluate_img), never truncated
    Matches are recorded by row, not by annotation id."""
    import numpy as np
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("coco_match runs on the device; the host restatement is evaluation/coco/coco_eval_host.py")
    det_counts, gt_counts = np.asarray(det_counts, np.int64).reshape(-1), np.asarray(gt_counts, np.int64).reshape(-1)
    if det_counts.shape != gt_counts.shape or (det_counts < 0).any() or (gt_counts < 0).any():
        raise RuntimeError("coco_match: one non-negative detection count and ground-truth count per group")
    area_rng, thrs = np.asarray(area_rng, np.float64).reshape(-1, 2), np.asarray(thrs, np.float64).reshape(-1)
    A, T, n = area_rng.shape[0], thrs.shape[0], len(det_counts)
    if not (1 <= A <= 8 and T >= 1 and A * T <= 64):
        raise RuntimeError("coco_match: {} area ranges x {} thresholds (the kernel gives each pair one lane of a wave: A <= 8, A * T <= 64)".format(A, T))
    with torch.cuda.device(dev):
        det_off, det_off_d = _coco_offsets(det_counts, dev)
        gt_off, gt_off_d = _coco_offsets(gt_counts, dev)
        iou_off, iou_off_d = _coco_offsets(det_counts * gt_counts, dev)
        Dt, Gt = int(det_off[-1]), int(gt_off[-1])
        iou_d = _f64_dev(iou, dev, (-1,))
        d_area, g_area, crowd = _f64_dev(det_area, dev, (-1,)), _f64_dev(gt_area, dev, (-1,)), _u8_dev(gt_crowd, dev)
        ignore = None if gt_ignore is None else _u8_dev(gt_ignore, dev)
        if iou_d.numel() != iou_off[-1] or d_area.numel() != Dt or g_area.numel() != Gt or crowd.numel() != Gt or (
                ignore is not None and ignore.numel() != Gt):
            raise RuntimeError("coco_match: the flat arrays do not have the lengths the counts sum to")
        iou_arg = iou_d if iou_d.numel() else torch.zeros((1,), dtype=torch.float64, device=dev)      # (no pair at all: still a valid address)
        dt_gt = torch.full((A, T, Dt), -1, dtype=torch.int32, device=dev)
        dt_ig = torch.zeros((A, T, Dt), dtype=torch.uint8, device=dev)
        gt_ig = torch.zeros((A, Gt), dtype=torch.uint8, device=dev)
        n_over = torch.zeros((1,), dtype=torch.int32, device=dev)
        if n:
            rng_d, thr_d = torch.from_numpy(area_rng.copy()).to(dev), torch.from_numpy(thrs.copy()).to(dev)
            head = (L.ptr(iou_arg), L.ptr(iou_off_d), L.ptr(det_off_d), L.ptr(gt_off_d), L.ptr(d_area), L.ptr(g_area), L.ptr(crowd))
            tail = (n, Dt, Gt, L.ptr(rng_d), A, L.ptr(thr_d), T, L.ptr(dt_gt), L.ptr(dt_ig), L.ptr(gt_ig), L.ptr(n_over), L.stream())
            if ignore is None:
                L.check(L.lib().abr_coco_match(*head, *tail), "coco_match")
            else:
                L.check(L.lib().abr_coco_match_ig(*head, L.ptr(ignore), *tail), "coco_match")
        out = {"dt_gt": dt_gt.cpu().numpy(), "dt_ig": dt_ig.cpu().numpy().astype(bool), "gt_ig": gt_ig.cpu().numpy().astype(bool)}
        skipped = int(n_over.cpu().item())
    over = np.nonzero(gt_counts > COCO_MATCH_MAX_GT)[0]
    if skipped != len(over):
        raise RuntimeError("coco_match: the kernel left {} groups to the host, the tables say {}".format(skipped, len(over)))
    if len(over):
        from .data.datasets.evaluation.coco import coco_eval_host as H
        iou_h = iou_d.cpu().numpy() if any(det_counts[k] for k in over) else None
        d_area_h, g_area_h, crowd_h = d_area.cpu().numpy(), g_area.cpu().numpy(), crowd.cpu().numpy().astype(bool)
        ignore_h = None if ignore is None else ignore.cpu().numpy().astype(bool)
        for k in over:
            D, G = int(det_counts[k]), int(gt_counts[k])
            ds, gs = slice(det_off[k], det_off[k + 1]), slice(gt_off[k], gt_off[k + 1])
            mat = iou_h[iou_off[k]: iou_off[k + 1]].reshape(D, G) if D else np.zeros((0, G))
            r = H.evaluate_img(mat, d_area_h[ds], g_area_h[gs], crowd_h[gs], area_rng, thrs, None if ignore_h is None else ignore_h[gs])
            out["dt_gt"][:, :, ds], out["dt_ig"][:, :, ds], out["gt_ig"][:, gs] = r["dt_gt"], r["dt_ig"], r["gt_ig"]
    out["n_fallback"] = len(over)
    return out


# ----------------------------------------------------------------------------------------------- proposal recall (csrc/proposal_recall.hip)
PROPOSAL_COVER_MAX_PROP = 1024      # ABR_PROPOSAL_COVER_MAX_PROP: the proposals per image proposal_cover's kernel holds


def _f32_dev(a, dev, shape):
    import numpy as np
    if isinstance(a, torch.Tensor):
        if a.dtype != torch.float32:
            raise RuntimeError("proposal_cover: expected float32 tensors, got {}".format(a.dtype))
        return a.to(dev).reshape(shape).contiguous()
    a = np.asarray(a)
    if a.dtype != np.float32:
        raise RuntimeError("proposal_cover: expected float32 arrays, got {} (the protocol's arithmetic is float32: round on purpose)".format(a.dtype))
    return torch.from_numpy(np.ascontiguousarray(a.reshape(shape))).to(dev)


def proposal_cover(prop, gt, gt_area, prop_counts, gt_counts, area_rng, limits, thrs, device="cuda"):
    """evaluate_box_proposals' greedy cover for every image, proposal limit and area range of a dataset in one launch.  prop float32
    [P_total,4] xyxy in rank order at the original image size (cut at the largest limit), gt float32 [G_total,4] xyxy (non-crowd), gt_area
    float32 [G_total] (numpy or tensors; float32 is required, not converted to: the protocol compares the rounded areas); prop_counts /
    gt_counts: proposals / ground truths per image; area_rng [A,2] (inclusive), limits [L], thrs [T] float32, used as given.
    -> dict of numpy arrays:
        overlaps  float32 [L,A,G_total]  per image segment: the cell's recorded overlaps in round order, zeros up to the number of ground
                                         truths in range, then -1; all -1 where the cell has no proposal or no ground truth in range
        hits      int32 [L,A,T]          how many overlaps of the cell vectors are >= thrs[t]
        num_pos   int32 [A]              ground truths in range
        n_fallback                       images with more than PROPOSAL_COVER_MAX_PROP proposals or COCO_MATCH_MAX_GT ground truths:
                                         scored by the host restatement (coco_eval_host.proposal_cover), never truncated"""
    import numpy as np
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError("proposal_cover runs on the device; the host restatement is evaluation/coco/coco_eval_host.py")
    prop_counts, gt_counts = np.asarray(prop_counts, np.int64).reshape(-1), np.asarray(gt_counts, np.int64).reshape(-1)
    if prop_counts.shape != gt_counts.shape or (prop_counts < 0).any() or (gt_counts < 0).any():
        raise RuntimeError("proposal_cover: one non-negative proposal count and ground-truth count per image")
    area_rng = np.asarray(area_rng, np.float32).reshape(-1, 2)
    limits = np.asarray(limits, np.int64).reshape(-1)
    thrs = (thrs.detach().cpu().numpy() if isinstance(thrs, torch.Tensor) else np.asarray(thrs)).reshape(-1)
    if thrs.dtype != np.float32:
        raise RuntimeError("proposal_cover: the thresholds are float32 and used as given, got {}".format(thrs.dtype))
    A, Ln, T, n = area_rng.shape[0], limits.shape[0], thrs.shape[0], len(prop_counts)
    if not (1 <= A <= 8 and 1 <= Ln <= 4 and 1 <= T <= 16):
        raise RuntimeError("proposal_cover: {} area ranges, {} limits, {} thresholds (1 <= A <= 8, 1 <= L <= 4, 1 <= T <= 16)".format(A, Ln, T))
    if (limits < 1).any() or (limits >= 2 ** 31).any():
        raise RuntimeError("proposal_cover: limits must be positive int32 values, got {}".format(limits.tolist()))
    with torch.cuda.device(dev):
        p_off, p_off_d = _coco_offsets(prop_counts, dev)
        g_off, g_off_d = _coco_offsets(gt_counts, dev)
        Pt, Gt = int(p_off[-1]), int(g_off[-1])
        prop_d, gt_d, area_d = _f32_dev(prop, dev, (-1, 4)), _f32_dev(gt, dev, (-1, 4)), _f32_dev(gt_area, dev, (-1,))
        if prop_d.shape[0] != Pt or gt_d.shape[0] != Gt or area_d.numel() != Gt:
            raise RuntimeError("proposal_cover: {} proposals / {} ground truths / {} areas for counts that sum to {} / {}".format(
                prop_d.shape[0], gt_d.shape[0], area_d.numel(), Pt, Gt))
        overlaps = torch.empty((Ln, A, Gt), dtype=_f32, device=dev)
        hits = torch.zeros((Ln, A, T), dtype=torch.int32, device=dev)
        num_pos = torch.zeros((A,), dtype=torch.int32, device=dev)
        n_over = torch.zeros((1,), dtype=torch.int32, device=dev)
        if n and Gt:
            rng_d, thr_d = torch.from_numpy(area_rng.copy()).to(dev), torch.from_numpy(thrs.copy()).to(dev)
            lim_d = torch.from_numpy(limits.astype(np.int32)).to(dev)
            L.check(L.lib().abr_proposal_cover(L.ptr(prop_d), L.ptr(gt_d), L.ptr(area_d), L.ptr(p_off_d), L.ptr(g_off_d), n, Pt, Gt, L.ptr(rng_d), A,
                                               L.ptr(lim_d), Ln, L.ptr(thr_d), T, L.ptr(overlaps), L.ptr(hits), L.ptr(num_pos), L.ptr(n_over),
                                               L.stream()), "proposal_cover")
        out = {"overlaps": overlaps.cpu().numpy(), "hits": hits.cpu().numpy(), "num_pos": num_pos.cpu().numpy()}
        skipped = int(n_over.cpu().item())
    over = np.nonzero((gt_counts > 0) & ((gt_counts > COCO_MATCH_MAX_GT) | (prop_counts > PROPOSAL_COVER_MAX_PROP)))[0]
    if skipped != len(over):
        raise RuntimeError("proposal_cover: the kernel left {} images to the host, the tables say {}".format(skipped, len(over)))
    if len(over):
        from .data.datasets.evaluation.coco import coco_eval_host as H
        prop_h, gt_h, area_h = prop_d.cpu(), gt_d.cpu(), area_d.cpu()
        thr_h = torch.from_numpy(thrs.copy())
        for k in over:
            ps, gs = slice(p_off[k], p_off[k + 1]), slice(g_off[k], g_off[k + 1])
            for a in range(A):
                valid = (area_h[gs] >= float(area_rng[a, 0])) & (area_h[gs] <= float(area_rng[a, 1]))
                Gv = int(valid.sum())
                out["num_pos"][a] += Gv
                for li in range(Ln):
                    seg = out["overlaps"][li, a, gs]
                    seg[:] = -1
                    boxes = prop_h[ps][: int(limits[li])]
                    if Gv == 0 or len(boxes) == 0:
                        continue
                    vec = H.proposal_cover(boxes, gt_h[gs][valid])
                    seg[:Gv] = vec.numpy()
                    out["hits"][li, a] += (vec[None, :] >= thr_h[:, None]).sum(1).to(torch.int32).numpy()
    out["n_fallback"] = len(over)
    return out

"""Mirror of maskrcnn_benchmark/modeling/poolers.py: LevelMapper (:11-42), Pooler (:45-105), make_pooler (:108-117).

The reference pools a feature pyramid with a Python loop over the levels: per level a `torch.nonzero` (a device-to-host sync), a row
gather, one ROIAlign launch and an indexed write into a zero-filled result; its backward is one atomic ROIAlign backward per level
behind index kernels.  Here a RoI's level is chosen inside the kernel (abr_iod_amd/csrc/roi_align.hip: a workgroup belongs to one RoI,
so the level is a workgroup-uniform choice of map), and the whole pooler is ONE launch forward and ONE launch backward: no host
round trip, no index tensors, no zero-filled intermediate.  Same results: a row has the bits the single-level ROIAlign gives it on its
level's map, and a row without a level (NaN or negative area -- it matches no level in the reference) is zero.

The C4 heads keep their own single-level Pooler (modeling/roi_heads/box_head/box_head.py) with its bin_step and joint-pass paths.
"""
import torch
from torch import nn
from torch.autograd import Function
from torch.autograd.function import once_differentiable

from .. import ops
from ..layers import ROIAlign
from ..layers._layout import as_nhwc, from_nhwc


def _roi_table(boxes):
    """poolers.py:73-78: [K,5] = (index of the BoxList, x1, y1, x2, y2)"""
    concat = torch.cat([b.convert("xyxy").bbox for b in boxes], dim=0)
    ids = torch.cat([torch.full((len(b), 1), i, dtype=concat.dtype, device=concat.device) for i, b in enumerate(boxes)], dim=0)
    return torch.cat([ids, concat], dim=1)


class LevelMapper(object):
    """poolers.py:11-42: the FPN paper's Eqn. (1), evaluated on the device by ops.fpn_levels"""

    def __init__(self, k_min, k_max, canonical_scale=224, canonical_level=4, eps=1e-6):
        self.k_min, self.k_max = k_min, k_max
        self.s0, self.lvl0, self.eps = canonical_scale, canonical_level, eps

    def __call__(self, boxlists):
        """list of BoxLists (or a ready [K,5] RoI table) -> int64 [K] on the device: 0 .. k_max - k_min, -1 for a box without a level"""
        rois = boxlists if torch.is_tensor(boxlists) else _roi_table(boxlists)
        return ops.fpn_levels(rois, self.k_min, self.k_max, self.s0, self.lvl0, self.eps).to(torch.int64)


class _PyramidROIAlign(Function):
    """(rois, rows, geometry, level rule, *maps logical [B,C,H_l,W_l]) -> logical [K,C,ph,pw]; a gradient for every level's map.
    rows: None, or an int64 [P] device list of table rows (entries < 0 are padding) -> logical [P,C,ph,pw], zero at the padding"""

    @staticmethod
    def forward(ctx, rois, rows, output_size, scales, sampling_ratio, rule, *feats):
        xs = [as_nhwc(f) for f in feats]
        out = ops.roi_align_pyramid_forward(xs, rois, scales, output_size[0], output_size[1], sampling_ratio, *rule, rows=rows)
        # a pooled value is an average of bilinear samples of ONE level's map (or 0): the largest of the levels' amax words bounds the result
        # (f16x3 scales; ops.amax_carry_bound for L maps).  A level without a tag leaves the result untagged: its consumer reduces it.
        # A subset of the table's rows and zeros for padding keep that bound.
        ops.amax_bound_levels(out, xs)
        ctx.save_for_backward(rois, *(() if rows is None else (rows,)))
        ctx.geom = (tuple(output_size), tuple(scales), sampling_ratio, rule, [tuple(x.shape) for x in xs])
        return from_nhwc(out)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        rois, *rows = ctx.saved_tensors
        (ph, pw), scales, sr, rule, shapes = ctx.geom
        gs = ops.roi_align_pyramid_backward(as_nhwc(grad_output), rois, scales, ph, pw, sr, shapes, *rule, rows=rows[0] if rows else None)
        return (None, None, None, None, None, None) + tuple(from_nhwc(g) for g in gs)


class Pooler(nn.Module):
    """poolers.py:45-105.  x: list of logical [B,C,H_l,W_l] maps, one per scale -> logical [K,C,ph,pw] (channels-last memory)"""

    def __init__(self, output_size, scales, sampling_ratio):
        super().__init__()
        self.poolers = nn.ModuleList([ROIAlign(output_size, spatial_scale=s, sampling_ratio=sampling_ratio) for s in scales])
        self.output_size = output_size
        # the levels of the first and the last map, from the scales as fp32 (poolers.py:69-71)
        lvl_min = -torch.log2(torch.tensor(scales[0], dtype=torch.float32)).item()
        lvl_max = -torch.log2(torch.tensor(scales[-1], dtype=torch.float32)).item()
        self.map_levels = LevelMapper(lvl_min, lvl_max)

    def convert_to_roi_format(self, boxes):
        return _roi_table(boxes)

    def forward(self, x, boxes, rows=None):
        """boxes: list of BoxLists (poolers.py:80-105) or an [K,5] RoI table (batch index, x1, y1, x2, y2) already on the device.
        rows: an int64 [P] device list of rows of that table -> [P,C,ph,pw]: only those rows are pooled, in one launch and without a gathered
        copy; an entry < 0 (the padding of ops.mask_compact_pos) gives a zero row and takes no gradient."""
        rois = boxes if torch.is_tensor(boxes) else self.convert_to_roi_format(boxes)
        if len(self.poolers) == 1 and rows is None:
            return self.poolers[0](x[0], rois)
        if len(x) != len(self.poolers):
            raise RuntimeError(f"Pooler: {len(x)} feature maps for {len(self.poolers)} scales")
        return _PyramidROIAlign.apply(rois, rows, *self.geometry(), *x)

    def geometry(self):
        """(output size, scales, sampling ratio, level rule): what the ops.roi_align_pyramid_* calls take -- for a head that folds the pooler
        into its own autograd node (roi_heads/pyramid_extractor.py)"""
        m = self.map_levels
        output_size = self.output_size if isinstance(self.output_size, (tuple, list)) else (self.output_size, self.output_size)
        return (tuple(output_size), tuple(p.spatial_scale for p in self.poolers), self.poolers[0].sampling_ratio,
                (m.k_min, m.k_max, m.s0, m.lvl0, m.eps))


def make_pooler(cfg, head_name):
    """poolers.py:108-117"""
    resolution = cfg.MODEL[head_name].POOLER_RESOLUTION
    return Pooler(output_size=(resolution, resolution), scales=cfg.MODEL[head_name].POOLER_SCALES,
                  sampling_ratio=cfg.MODEL[head_name].POOLER_SAMPLING_RATIO)

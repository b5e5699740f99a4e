"""PolygonList: instance masks given as polygons, the normal form of a COCO-format "segmentation" (mirror of PolygonInstance / PolygonList,
maskrcnn_benchmark/structures/segmentation_mask.py:182-443), stored FLAT so that the device reads it in place:
    coords        float32 [V,2]          every vertex (x, y) of every polygon of every instance of one image
    poly_offsets  int64   [n_poly+1]     polygon p owns vertices [poly_offsets[p], poly_offsets[p+1])
    inst_offsets  int64   [n_inst+1]     instance i owns polygons [inst_offsets[i], inst_offsets[i+1])
    size          (width, height)
A BoxList carries it as its "masks" field beside SegmentationMask and PackedMasks; SegmentationMask(..., mode="poly") keeps raising.
transpose / crop / resize are the reference's torch expressions on `coords` (an fp32 tensor with a Python scalar: the scalar is rounded to
fp32), on whatever device the tensors are.  Rasterising is ops.poly_rasterize: csrc/poly.hip on the device, the host codec below when the
list is on the CPU.  The training step never rasterises whole images: its M x M targets come from ops.poly_mask_targets.

The host codec is a numpy restatement of pycocotools' rleFrPoly + merge + decode, used on the CPU and as the reference the
kernels are tested against.  pycocotools cannot be installed where this project is built, so compatibility rests on the restatement and
its known answers (tests/test_poly_host.py), not on a comparison with pycocotools itself.

Divergences from the reference, both deliberate: an instance left without a polygon (all of its polygons had fewer than 3 vertices) STAYS
in the list and rasterises to zeros -- the reference drops it from the list, which silently misaligns "masks" with the boxes, or fails
inside pycocotools; and a polygon with a non-finite coordinate or one beyond +-32768 pixels contributes nothing and is reported in a
status word (the guard that bounds every loop of the kernels)."""
import numpy as np
import torch

from .segmentation_mask import FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM

UPSAMPLE = 5                      # rleFrPoly's scale
COORD_LIMIT = 5.0 * 32768.0       # the guard: |5 c| beyond this (or a non-finite c) and the polygon contributes nothing
STATUS_NONFINITE, STATUS_RANGE = 1, 2


# ----------------------------------------------------------------------------------------------------------------- host codec
def polygon_status(xy):
    """guard flags of one polygon, xy [k,2]: STATUS_NONFINITE | STATUS_RANGE, 0 = fine"""
    a = np.asarray(xy, np.float32).astype(np.float64).reshape(-1)
    finite = np.isfinite(a)
    flags = 0 if finite.all() else STATUS_NONFINITE
    if (np.abs(5.0 * a[finite]) > COORD_LIMIT).any():
        flags |= STATUS_RANGE
    return flags


def _trunc(a):
    return np.asarray(a, np.float64).astype(np.int64)      # C's (int): toward zero


def polygon_crossings(xy, h, w):
    """the column-major positions x * h + yd of the crossings of one polygon (xy float32 [k,2], k >= 1) on an h x w grid; each toggles
    every pixel from its position on"""
    a = np.asarray(xy, np.float32).astype(np.float64).reshape(-1, 2)
    k = a.shape[0]
    X = _trunc(UPSAMPLE * a[:, 0] + 0.5).tolist()
    Y = _trunc(UPSAMPLE * a[:, 1] + 0.5).tolist()
    X.append(X[0])
    Y.append(Y[0])
    us, vs = [], []
    for j in range(k):
        xs, xe, ys, ye = X[j], X[j + 1], Y[j], Y[j + 1]
        dx, dy = abs(xe - xs), abs(ys - ye)
        flip = (dx >= dy and xs > xe) or (dx < dy and ys > ye)
        if flip:
            xs, xe, ys, ye = xe, xs, ye, ys
        length = max(dx, dy)
        if length == 0:                                   # one point; its 0 / 0 slope is never formed
            us.append(np.array([xs], np.int64))
            vs.append(np.array([ys], np.int64))
            continue
        d = np.arange(length + 1, dtype=np.int64)
        t = length - d if flip else d
        tf = t.astype(np.float64)
        if dx >= dy:
            s = float(ye - ys) / float(dx)
            us.append(t + xs)
            vs.append(_trunc((float(ys) + s * tf) + 0.5))
        else:
            s = float(xe - xs) / float(dy)
            vs.append(t + ys)
            us.append(_trunc((float(xs) + s * tf) + 0.5))
    u, v = np.concatenate(us), np.concatenate(vs)
    u0, u1, v0, v1 = u[:-1], u[1:], v[:-1], v[1:]
    moved = u1 != u0
    u0, u1, v0, v1 = u0[moved], u1[moved], v0[moved], v1[moved]
    xd = (np.where(u1 < u0, u1, u1 - 1).astype(np.float64) + 0.5) / UPSAMPLE - 0.5
    keep = (np.floor(xd) == xd) & (xd >= 0) & (xd <= w - 1)
    yd = (np.minimum(v1, v0).astype(np.float64) + 0.5) / UPSAMPLE - 0.5
    yd = np.ceil(np.clip(yd, 0.0, float(h)))
    return (xd[keep] * h + yd[keep]).astype(np.int64)


def rasterize_polygon(xy, h, w):
    """one polygon -> (uint8 [h,w] mask of 0 / 1, status)"""
    h, w = int(h), int(w)
    status = polygon_status(xy)
    if status or len(xy) == 0:
        return np.zeros((h, w), np.uint8), status
    toggles = np.bincount(polygon_crossings(xy, h, w), minlength=h * w + 1)
    filled = np.cumsum(toggles)[: h * w] & 1               # parity over the LINEAR position: it carries from column to column
    return filled.astype(np.uint8).reshape(w, h).T.copy(), 0


def rasterize(coords, poly_offsets, inst_offsets, h, w):
    """flat storage of one image -> (uint8 [n,h,w] masks, int32 [n] status); an instance is the OR of its polygons"""
    coords = np.asarray(coords, np.float32).reshape(-1, 2)
    n = len(inst_offsets) - 1
    masks = np.zeros((n, int(h), int(w)), np.uint8)
    status = np.zeros((n,), np.int32)
    for i in range(n):
        for p in range(int(inst_offsets[i]), int(inst_offsets[i + 1])):
            m, st = rasterize_polygon(coords[int(poly_offsets[p]): int(poly_offsets[p + 1])], h, w)
            masks[i] |= m
            status[i] |= st
    return masks, status


# ----------------------------------------------------------------------------------------------------------------- the structure
def _as_xy(p):
    a = (p.detach().cpu().numpy() if isinstance(p, torch.Tensor) else np.asarray(p)).astype(np.float32).reshape(-1)
    if a.size % 2:
        raise ValueError("a polygon is a flat list x0, y0, x1, y1, ...: got {} numbers".format(a.size))
    return a.reshape(-1, 2)


class PolygonList(object):
    def __init__(self, polygons, size, device=None):
        """polygons: a list (instances) of lists (polygons) of flat x0, y0, x1, y1, ... number lists, or a PolygonList; size = (width,
        height); device: where the tensors are put (None: the CPU, or where the given PolygonList is).  Polygons with fewer than 6 numbers
        are dropped (segmentation_mask.py:196-202); an instance left with none stays and rasterises to zeros."""
        if isinstance(polygons, PolygonList):
            src = polygons if device is None else polygons.to(device)
            self.coords, self.poly_offsets, self.inst_offsets = src.coords, src.poly_offsets, src.inst_offsets
            self._po, self._io, self.size = src._po, src._io, src.size     # (the reference takes the given list's size too, :354-356)
            self.mode = "poly"
            return
        if not isinstance(polygons, (list, tuple)):
            raise TypeError("PolygonList: expected a list of instances (lists of polygons) or a PolygonList, got {}".format(type(polygons).__name__))
        assert isinstance(size, (list, tuple)) and len(size) == 2, str(type(size))
        chunks, po, io = [], [0], [0]
        for i, inst in enumerate(polygons):
            if not isinstance(inst, (list, tuple)):
                raise TypeError("PolygonList: instance {} is a {}, expected a list of polygons".format(i, type(inst).__name__))
            for p in inst:
                if not isinstance(p, (list, tuple, np.ndarray, torch.Tensor)):
                    raise TypeError("PolygonList: instance {} holds a {}, expected flat coordinate lists".format(i, type(p).__name__))
                if len(p) >= 6:      # 3 * 2 coordinates
                    xy = _as_xy(p)
                    chunks.append(xy)
                    po.append(po[-1] + xy.shape[0])
            io.append(len(po) - 1)
        coords = torch.from_numpy(np.concatenate(chunks) if chunks else np.zeros((0, 2), np.float32))
        self._set(coords.to(device) if device is not None else coords, po, io, tuple(size))

    def _set(self, coords, po, io, size, like=None):
        """like: a PolygonList with the same offsets on the same device, whose offset tensors are shared instead of uploaded again"""
        self.coords, self._po, self._io, self.size = coords, list(po), list(io), size
        if like is not None and like.poly_offsets.device == coords.device:
            self.poly_offsets, self.inst_offsets = like.poly_offsets, like.inst_offsets
        else:
            from ..ops import h2d       # (a pinned asynchronous upload on the device; a plain tensor on the CPU)
            self.poly_offsets = h2d(self._po, torch.int64, coords.device)
            self.inst_offsets = h2d(self._io, torch.int64, coords.device)
        self.mode = "poly"
        return self

    @classmethod
    def _make(cls, coords, po, io, size, like=None):
        return cls.__new__(cls)._set(coords, po, io, size, like)

    @property
    def instances(self):       # (the reference's SegmentationMask wraps a PolygonList with the same methods)
        return self

    @property
    def device(self):
        return self.coords.device

    def polygons_of(self, i):
        """the polygons of instance i as float32 [k,2] tensors (views of coords)"""
        return [self.coords[self._po[p]: self._po[p + 1]] for p in range(self._io[i], self._io[i + 1])]

    def int_size(self):
        """(width, height) as ints: the grid to rasterise on; a cropped list has float sizes and is resized before it is rasterised"""
        w, h = (float(s) for s in self.size)
        if w != int(w) or h != int(h) or w <= 0 or h <= 0:
            raise ValueError("a PolygonList of size {} cannot be rasterised: resize it to an integer size first".format(self.size))
        return int(w), int(h)

    # --- geometry: the reference's expressions
    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        width, height = self.size
        dim, idx = (width, 0) if method == FLIP_LEFT_RIGHT else (height, 1)
        c = self.coords.clone()
        TO_REMOVE = 1
        c[:, idx] = dim - self.coords[:, idx] - TO_REMOVE
        return PolygonList._make(c, self._po, self._io, self.size, like=self)

    def crop(self, box):
        assert isinstance(box, (list, tuple, torch.Tensor)), str(type(box))
        current_width, current_height = self.size
        xmin, ymin, xmax, ymax = map(float, box)
        assert xmin <= xmax and ymin <= ymax, str(box)
        xmin = min(max(xmin, 0), current_width - 1)
        ymin = min(max(ymin, 0), current_height - 1)
        xmax = min(max(xmax, 0), current_width)
        ymax = min(max(ymax, 0), current_height)
        xmax = max(xmax, xmin + 1)
        ymax = max(ymax, ymin + 1)
        w, h = xmax - xmin, ymax - ymin
        c = self.coords.clone()
        c[:, 0] = c[:, 0] - xmin
        c[:, 1] = c[:, 1] - ymin
        return PolygonList._make(c, self._po, self._io, (float(w), float(h)), like=self)      # the clamped size, a pair of floats (PolygonInstance's, :272)

    def resize(self, size, *args, **kwargs):
        try:
            iter(size)
        except TypeError:
            assert isinstance(size, (int, float))
            size = size, size
        ratios = tuple(float(s) / float(s_orig) for s, s_orig in zip(size, self.size))
        if ratios[0] == ratios[1]:
            c = self.coords * ratios[0]
        else:
            c = self.coords.clone()
            c[:, 0] *= ratios[0]
            c[:, 1] *= ratios[1]
        return PolygonList._make(c, self._po, self._io, tuple(size), like=self)

    # --- rasterising
    def convert(self, mode):
        if mode == "poly":
            return self
        if mode != "mask":
            raise NotImplementedError("Unknown mode: %s" % str(mode))
        from .. import ops
        from .segmentation_mask import SegmentationMask
        return SegmentationMask(ops.poly_rasterize(self), self.int_size(), mode="mask")

    def pack(self):
        """-> PackedMasks: rasterised straight into bits, the masks never exist as bytes"""
        from .. import ops
        from .segmentation_mask import PackedMasks
        return PackedMasks(ops.poly_rasterize(self, packed=True), self.int_size())

    def get_mask_tensor(self):
        return self.convert("mask").get_mask_tensor()

    # --- container
    def to(self, device):
        if torch.device(device) == self.coords.device:
            return self
        return PolygonList._make(self.coords.to(device), self._po, self._io, self.size)

    def __len__(self):
        return len(self._io) - 1

    def __getitem__(self, item):
        n = len(self)
        if isinstance(item, (int, np.integer)):
            picked = [range(n)[int(item)]]
        elif isinstance(item, slice):
            picked = list(range(n))[item]
        else:
            if isinstance(item, torch.Tensor):
                if item.dtype == torch.bool:
                    if item.numel() != n:
                        raise IndexError("a bool index of {} entries for {} instances".format(item.numel(), n))
                    item = item.nonzero().reshape(-1)
                item = item.reshape(-1).tolist()
            item = list(item)
            if item and all(isinstance(i, (bool, np.bool_)) for i in item):      # a list of bools is a mask, as a bool tensor is
                if len(item) != n:
                    raise IndexError("a bool index of {} entries for {} instances".format(len(item), n))
                item = [i for i, keep in enumerate(item) if keep]
            elif any(isinstance(i, (bool, np.bool_)) for i in item):
                raise IndexError("an index list mixes bools and integers")
            picked = [range(n)[int(i)] for i in item]
        po, io, spans = [0], [0], []
        for i in picked:
            for p in range(self._io[i], self._io[i + 1]):
                spans.append(np.arange(self._po[p], self._po[p + 1], dtype=np.int64))
                po.append(po[-1] + self._po[p + 1] - self._po[p])
            io.append(len(po) - 1)
        index = torch.from_numpy(np.concatenate(spans) if spans else np.zeros((0,), np.int64)).to(self.coords.device)
        return PolygonList._make(self.coords[index], po, io, self.size)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def __repr__(self):
        return "PolygonList(num_instances={}, image_width={}, image_height={})".format(len(self), self.size[0], self.size[1])

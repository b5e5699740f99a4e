"""SegmentationMask over binary instance masks (mirror of maskrcnn_benchmark/structures/segmentation_mask.py:33-179, 445-545 for
mode="mask"): ONE tensor [n,H,W] (uint8 or float32) on any device, with the reference's crop / resize / transpose / indexing, so that BoxList
indexing, flipping and resizing carry a "masks" field as they do there.  This is the data path's API; the training step never calls it per
RoI -- its targets come from ops.mask_targets.  mode="poly" raises: polygons live in structures/polygon.py's PolygonList.  COCO run-length annotations (a list of RLE dicts, what the reference hands to
pycocotools' mask_utils.decode, segmentation_mask.py:57-63) are decoded by ops.rle_decode: on the device when one is given, else by the host codec
(structures/rle.py)."""
import torch

FLIP_LEFT_RIGHT = 0
FLIP_TOP_BOTTOM = 1


def _decode_rles(rles, size, device, packed):
    from .. import ops
    for i, inst in enumerate(rles):     # the reference's check, segmentation_mask.py:59-61
        assert isinstance(inst, dict) and "size" in inst and "counts" in inst, "RLE instance %d: expected a dict with 'size' and 'counts'" % i
        assert (size[1], size[0]) == tuple(inst["size"]), "RLE instance %d: %s != %s" % (i, (size[1], size[0]), tuple(inst["size"]))
    return ops.rle_decode(list(rles), (size[1], size[0]), device if device is not None else "cpu", packed=packed)


class SegmentationMask(object):
    def __init__(self, instances, size, mode="mask", device=None):
        """instances: [n,H,W] tensor, [H,W] tensor, list of [H,W] tensors, list of COCO RLE dicts or a SegmentationMask; size = (width, height);
        device: where RLE dicts are decoded (None: the CPU); tensors stay where they are"""
        if mode == "poly":
            raise NotImplementedError("SegmentationMask mode 'poly': polygons have a class of their own here, structures.polygon.PolygonList(polygons, "
                                      "size); a BoxList carries it as its 'masks' field and .convert('mask') rasterises it")
        if mode != "mask":
            raise NotImplementedError("Unknown mode: %s" % str(mode))
        assert isinstance(size, (list, tuple)) and len(size) == 2
        size = tuple(int(s.item()) if isinstance(s, torch.Tensor) else s for s in size)
        if isinstance(instances, SegmentationMask):
            masks = instances.masks
        elif isinstance(instances, (list, tuple)) and len(instances) and isinstance(instances[0], dict):
            masks = _decode_rles(instances, size, device, packed=False)
        elif isinstance(instances, (list, tuple)):
            masks = torch.stack(list(instances), dim=0) if len(instances) else torch.zeros((0, int(size[1]), int(size[0])), dtype=torch.uint8,
                                                                                           device=device if device is not None else "cpu")
        else:
            masks = instances
        if masks.dim() == 2:
            masks = masks.unsqueeze(0)
        assert masks.dim() == 3
        assert masks.shape[1] == size[1], "%s != %s" % (masks.shape[1], size[1])
        assert masks.shape[2] == size[0], "%s != %s" % (masks.shape[2], size[0])
        if masks.dtype not in (torch.uint8, torch.float32):
            raise TypeError("SegmentationMask holds uint8 or float32 masks, got {}".format(masks.dtype))
        self.masks = masks
        self.size = size
        self.mode = mode

    @property
    def instances(self):   # (the reference wraps a BinaryMaskList with the same methods)
        return self

    def transpose(self, method):
        if method not in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
            raise NotImplementedError("Only FLIP_LEFT_RIGHT and FLIP_TOP_BOTTOM implemented")
        return SegmentationMask(self.masks.flip(1 if method == FLIP_TOP_BOTTOM else 2), self.size, self.mode)

    def crop(self, box):
        """box xyxy; corners through Python's round (half to even), clamped as segmentation_mask.py:99-106"""
        assert isinstance(box, (list, tuple, torch.Tensor)), str(type(box))
        current_width, current_height = self.size
        xmin, ymin, xmax, ymax = [round(float(b)) for b in box]
        assert xmin <= xmax and ymin <= ymax, str(box)
        xmin = min(max(xmin, 0), current_width - 1)
        ymin = min(max(ymin, 0), current_height - 1)
        xmax = min(max(xmax, 0), current_width)
        ymax = min(max(ymax, 0), current_height)
        xmax = max(xmax, xmin + 1)
        ymax = max(ymax, ymin + 1)
        return SegmentationMask(self.masks[:, ymin:ymax, xmin:xmax], (xmax - xmin, ymax - ymin), self.mode)

    def resize(self, size, *args, **kwargs):
        try:
            iter(size)
        except TypeError:
            assert isinstance(size, (int, float))
            size = size, size
        width, height = map(int, size)
        assert width > 0 and height > 0
        if len(self.masks) > 0:
            resized = torch.nn.functional.interpolate(self.masks.unsqueeze(0).float(), size=(height, width), mode="bilinear",
                                                      align_corners=False)[0].type_as(self.masks)
        else:
            resized = torch.zeros(0, height, width).type_as(self.masks)
        return SegmentationMask(resized, (width, height), self.mode)

    def convert(self, mode):
        if mode == self.mode:
            return self
        return SegmentationMask(self.masks, self.size, mode)    # raises for "poly"

    def to(self, device):
        return SegmentationMask(self.masks.to(device), self.size, self.mode)

    def get_mask_tensor(self):
        return self.masks.squeeze(0)     # ([H,W] when there is one instance, segmentation_mask.py:512-517)

    def __len__(self):
        return len(self.masks)

    def __getitem__(self, item):
        return SegmentationMask(self.masks[item], self.size, self.mode)

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]

    def __repr__(self):
        return "SegmentationMask(num_instances={}, image_width={}, image_height={}, mode={})".format(len(self), self.size[0], self.size[1], self.mode)


class PackedMasks(object):
    """Binary instance masks as bits: `bits` int64 [n,H,ceil(W/64)], bit x % 64 of word x // 64 of row y set iff the pixel is 1
    (ops.mask_pack_bits), and size = (width, height).  What the test loop keeps per image when mask AP is asked for (engine/inference.py):
    one eighth of the uint8 masks' bytes, already at the original image size and ready for ops.mask_pair_counts.  A BoxList carries it as a
    non-tensor field like SegmentationMask."""

    def __init__(self, bits, size):
        size = tuple(int(s) for s in size)
        assert bits.dim() == 3 and bits.dtype == torch.int64, "PackedMasks holds int64 [n,H,Wq] words"
        assert bits.shape[1] == size[1] and bits.shape[2] == (size[0] + 63) // 64, "{} does not pack masks of size {}".format(tuple(bits.shape), size)
        self.bits = bits
        self.size = size
        self.mode = "packed"

    @classmethod
    def from_rle(cls, rles, size, device=None):
        """list of COCO RLE dicts, size = (width, height) -> PackedMasks on `device` (None: the CPU): the words are written by the decoder,
        the masks never exist as bytes (ground truth for mask AP)"""
        size = tuple(int(s) for s in size)
        if len(rles) == 0:
            bits = torch.zeros((0, size[1], (size[0] + 63) // 64), dtype=torch.int64, device=device if device is not None else "cpu")
        else:
            bits = _decode_rles(rles, size, device, packed=True)
        return cls(bits, size)

    @property
    def instances(self):
        return self

    def to(self, device):
        return PackedMasks(self.bits.to(device), self.size)

    def resize(self, size, *args, **kwargs):
        try:
            size = tuple(int(s) for s in size)
        except TypeError:
            size = (int(size), int(size))
        if size != self.size:
            raise ValueError("PackedMasks of size {} cannot be resized to {}: bits are packed at their final size (resize the "
                             "SegmentationMask first, or pack with ops.mask_resize_pack_bits)".format(self.size, size))
        return self

    def unpack(self):
        """-> uint8 [n,H,W] (tests and debugging)"""
        n, H, Wq = self.bits.shape
        shifts = torch.arange(64, dtype=torch.int64, device=self.bits.device)
        px = (self.bits.unsqueeze(-1) >> shifts) & 1
        return px.reshape(n, H, Wq * 64)[:, :, : self.size[0]].to(torch.uint8)

    def __len__(self):
        return self.bits.shape[0]

    def __getitem__(self, item):
        bits = self.bits[item]
        return PackedMasks(bits.unsqueeze(0) if bits.dim() == 2 else bits, self.size)

    def __repr__(self):
        return "PackedMasks(num_instances={}, image_width={}, image_height={})".format(len(self), self.size[0], self.size[1])

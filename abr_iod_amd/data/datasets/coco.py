"""COCODataset(ann_file, root, remove_images_without_annotations, transforms=None): detection and instance segmentation from a COCO
annotation file (mirror of maskrcnn_benchmark/data/datasets/coco.py's COCODataset).

The reference sits on torchvision's CocoDetection and pycocotools' COCO index; the index is a few dicts, built here with plain `json`:
images by id, annotations by image id in file order, categories in file order.  Kept from the reference:
  * ids sorted; with remove_images_without_annotations an image is kept only when it has a valid annotation: not empty, not all boxes
    with a side <= 1 (crowd annotations count here), and, for keypoint files, at least 10 visible keypoints;
  * a sample's target: the image's NON-crowd annotations; boxes xywh -> xyxy; "labels" = contiguous category ids (1 .. number of
    categories, in the file's category order; 0 is the background); "masks" = the polygons as a structures.polygon.PolygonList on the
    dataset's device (only with with_masks=True); clip_to_image(remove_empty=True);
  * json_category_id_to_contiguous_id and its inverse, id_to_img_map, get_img_info.
The reference's class-incremental remapping of category ids (its alphabetical order, the first-70 / last-10 split hard-wired in the
file) is not carried: labels follow the annotation file.
For the evaluator (evaluation/coco): get_annotations(index) -- ALL annotations of the image, crowds included, as the file gives them --
annotation_masks(index, device, packed) -- their masks, run-length ones through ops.rle_decode and polygons through
ops.poly_rasterize -- and get_groundtruth(index), the same as a BoxList with "labels", "iscrowd" and "area".
Samples have this package's form (data/datasets/voc.py): (uint8 device image, target, flip flag, index), for GPUTransform.collate."""
import json
import os

import torch

from ...structures.bounding_box import BoxList
from ...structures.polygon import PolygonList

min_keypoints_per_image = 10


def _count_visible_keypoints(anno):
    return sum(sum(1 for v in ann["keypoints"][2::3] if v > 0) for ann in anno)


def _has_only_empty_bbox(anno):
    return all(any(o <= 1 for o in obj["bbox"][2:]) for obj in anno)


def has_valid_annotation(anno):
    if len(anno) == 0:
        return False
    if _has_only_empty_bbox(anno):
        return False
    if "keypoints" not in anno[0]:
        return True
    return _count_visible_keypoints(anno) >= min_keypoints_per_image


class COCODataset(object):
    def __init__(self, ann_file, root, remove_images_without_annotations, transforms=None, with_masks=False, device="cuda"):
        self.root, self.transforms, self.with_masks, self.device = root, transforms, with_masks, device
        with open(ann_file) as f:
            data = json.load(f)
        self.imgs = {img["id"]: img for img in data.get("images", [])}
        self.cats = {cat["id"]: cat for cat in data.get("categories", [])}
        self.img_to_anns = {i: [] for i in self.imgs}
        for ann in data.get("annotations", []):
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)
        self.ids = sorted(self.imgs)
        if remove_images_without_annotations:
            self.ids = [i for i in self.ids if has_valid_annotation(self.img_to_anns[i])]
        self.json_category_id_to_contiguous_id = {v: i + 1 for i, v in enumerate(self.cats)}
        self.contiguous_category_id_to_json_id = {v: k for k, v in self.json_category_id_to_contiguous_id.items()}
        self.id_to_img_map = {k: v for k, v in enumerate(self.ids)}

    def __len__(self):
        return len(self.ids)

    def _load_image(self, img_id):
        from PIL import Image
        return Image.open(os.path.join(self.root, self.imgs[img_id]["file_name"])).convert("RGB")

    def _boxlist(self, anno, size):
        boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)   # guard against no boxes
        target = BoxList(boxes, size, mode="xywh").convert("xyxy")
        target.add_field("labels", torch.tensor([self.json_category_id_to_contiguous_id[obj["category_id"]] for obj in anno], dtype=torch.int64))
        return target

    def get_target(self, index, size=None):
        """the training target of image `index` at `size` = (width, height) (default: the file's): crowds dropped, clipped, empty boxes removed"""
        info = self.get_img_info(index)
        size = (int(info["width"]), int(info["height"])) if size is None else tuple(size)
        anno = [obj for obj in self.img_to_anns[self.ids[index]] if obj.get("iscrowd", 0) == 0]
        target = self._boxlist(anno, size)
        if self.with_masks:
            segs = [obj["segmentation"] for obj in anno]
            if any(not isinstance(s, (list, tuple)) for s in segs):
                raise ValueError("image {}: a non-crowd annotation whose segmentation is not a polygon list".format(self.ids[index]))
            target.add_field("masks", PolygonList(segs, size, device=self.device))
        if anno and "keypoints" in anno[0]:      # coco.py:258-261: a person-keypoint file hands its keypoints to the model (MODEL.KEYPOINT_ON)
            from ...structures.keypoint import PersonKeypoints
            target.add_field("keypoints", PersonKeypoints(torch.tensor([obj["keypoints"] for obj in anno], dtype=torch.float32).to(self.device), size))
        return target.clip_to_image(remove_empty=True)

    def __getitem__(self, index):
        from ..gpu_transforms import to_device_u8
        img = self._load_image(self.ids[index])
        target = self.get_target(index, img.size)
        img = to_device_u8(img, self.device)
        if self.transforms is not None:
            img, target, flip = self.transforms(img, target)
        else:
            flip = False
        return img, target, flip, index

    def get_img_info(self, index):
        return self.imgs[self.id_to_img_map[index]]

    def get_img_id(self, index):
        return self.id_to_img_map[index]

    # --- for the evaluator: everything the file holds for the image, crowds included
    def get_annotations(self, index):
        return self.img_to_anns[self.id_to_img_map[index]]

    def annotation_masks(self, index, device="cuda", packed=True):
        """the masks of get_annotations(index) at the image's size on `device`: packed int64 bits [n,h,ceil(w/64)] (ops.mask_pack_bits'
        layout) or uint8 [n,h,w].  Run-length annotations (the crowds) are decoded by ops.rle_decode, polygons rasterised by ops.poly_rasterize."""
        from ... import ops
        info = self.get_img_info(index)
        w, h = int(info["width"]), int(info["height"])
        anno = self.get_annotations(index)
        device = torch.device(device)
        shape, dtype = ops._mask_result("annotation_masks", len(anno), h, w, packed, None, device)
        out = torch.zeros(shape, dtype=dtype, device=device)
        poly = [i for i, a in enumerate(anno) if isinstance(a["segmentation"], (list, tuple))]
        rle = [i for i in range(len(anno)) if i not in set(poly)]
        if poly:
            out[torch.tensor(poly, device=device)] = ops.poly_rasterize(PolygonList([anno[i]["segmentation"] for i in poly], (w, h), device=device),
                                                                        packed=packed)
        if rle:
            out[torch.tensor(rle, device=device)] = ops.rle_decode([anno[i]["segmentation"] for i in rle], (h, w), device, packed=packed)
        return out

    def get_groundtruth(self, index):
        """all annotations of the image (crowds included, unclipped) as a BoxList with "labels", "iscrowd" and "area" """
        info = self.get_img_info(index)
        anno = self.get_annotations(index)
        target = self._boxlist(anno, (int(info["width"]), int(info["height"])))
        target.add_field("iscrowd", torch.tensor([int(obj.get("iscrowd", 0)) for obj in anno], dtype=torch.uint8))
        target.add_field("area", torch.tensor([float(obj["area"]) for obj in anno], dtype=torch.float64))
        return target

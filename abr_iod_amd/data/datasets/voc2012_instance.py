"""PASCAL VOC 2012 instance segmentation from a COCO-format JSON (mirror of maskrcnn_benchmark/data/datasets/voc2012_Instance.py:73-328).

The reference sits on torchvision's CocoDetection and pycocotools' COCO index; the index is a few dicts, built here with plain `json`:
images by id, annotations by image id in file order.  Kept from the reference:
  * ids sorted; an image is used when it has a valid annotation among its NON-crowd annotations (not empty, not all boxes with a side <= 1,
    no keypoints) and at least one of them is of a NEW class (training) or of a new or old class (testing) (:80-100);
  * a sample's annotations are ALL of the image's (crowd included, :114-115) filtered to those classes (:124-130); boxes xywh -> xyxy, labels
    = category ids, "masks" = the annotations' run-length "segmentation" decoded by ops.rle_decode on the dataset's device (the reference:
    pycocotools on the host), or, when the "segmentation"s are polygons, a PolygonList (structures/polygon.py), then
    clip_to_image(remove_empty=False) (:131-147);
  * get_groundtruth (unclipped, :158-232), get_img_info (the JSON's image record), get_img_id, map_class_id_to_class_name.
Samples have this package's form (data/datasets/voc.py): (uint8 device image, target, flip flag, index), for GPUTransform.collate."""
import json
import os

import torch

from ...structures.bounding_box import BoxList
from ...structures.polygon import PolygonList
from ...structures.segmentation_mask import PackedMasks, SegmentationMask
from ..gpu_transforms import to_device_u8
from .voc import CLASSES


def _has_only_empty_bbox(anno):
    return all(any(o <= 1 for o in obj["bbox"][2:]) for obj in anno)


def has_valid_annotation(anno):
    if len(anno) == 0:
        return False
    if _has_only_empty_bbox(anno):
        return False
    return "keypoints" not in anno[0]


class PascalVOCDataset2012(object):
    CLASSES = CLASSES

    def __init__(self, data_dir, ann_file, split=None, use_difficult=False, transforms=None, old_classes=(), new_classes=(), excluded_classes=(),
                 is_train=True, device="cuda"):
        self.root, self.transforms, self.device, self.is_train = data_dir, transforms, device, is_train
        self.old_classes, self.new_classes = list(old_classes), list(new_classes)
        with open(ann_file) as f:
            data = json.load(f)
        self.imgs = {img["id"]: img for img in data.get("images", [])}
        self.img_to_anns = {i: [] for i in self.imgs}
        for ann in data.get("annotations", []):
            self.img_to_anns.setdefault(ann["image_id"], []).append(ann)
        self.ids = sorted(self.imgs)
        wanted = self._wanted()
        self.final_ids = []
        for img_id in self.ids:
            anno = [a for a in self.img_to_anns[img_id] if not a.get("iscrowd", 0)]
            if has_valid_annotation(anno) and any(CLASSES[a["category_id"]] in wanted for a in anno):
                self.final_ids.append(img_id)
        self.num_img = len(self.final_ids)
        self.id_to_img_map = dict(enumerate(self.final_ids))
        self.class_to_ind = dict(zip(CLASSES, range(len(CLASSES))))

    def _wanted(self):
        return self.new_classes if self.is_train else self.new_classes + self.old_classes

    def __len__(self):
        return len(self.final_ids)

    def _load_image(self, img_id):
        from PIL import Image
        return Image.open(os.path.join(self.root, self.imgs[img_id]["file_name"])).convert("RGB")

    def _load_target(self, img_id):
        wanted = self._wanted()
        return [a for a in self.img_to_anns[img_id] if CLASSES[a["category_id"]] in wanted]

    def _target(self, img_id, size, packed=False):
        anno = self._load_target(img_id)
        boxes = torch.as_tensor([obj["bbox"] for obj in anno], dtype=torch.float32).reshape(-1, 4)   # guard against no boxes
        target = BoxList(boxes, size, mode="xywh").convert("xyxy")
        target.add_field("labels", torch.tensor([obj["category_id"] for obj in anno], dtype=torch.int64))
        segs = [obj["segmentation"] for obj in anno]
        target.add_field("masks", self._masks(segs, size, packed))
        return target

    def _masks(self, segs, size, packed):
        """run-length dicts: decoded (as ever); polygons (a list of flat coordinate lists per annotation): a PolygonList on the dataset's
        device, or with packed=True rasterised straight into bits; an image that mixes both: the polygons are rasterised and everything
        becomes one SegmentationMask (PackedMasks with packed=True)"""
        poly = [i for i, seg in enumerate(segs) if isinstance(seg, (list, tuple))]
        if not poly:
            return PackedMasks.from_rle(segs, size, self.device) if packed else SegmentationMask(segs, size, mode="mask", device=self.device)
        polys = PolygonList([segs[i] for i in poly], size, device=self.device)
        if len(poly) == len(segs):
            return polys.pack() if packed else polys
        rle = [i for i in range(len(segs)) if i not in set(poly)]
        rles = [segs[i] for i in rle]
        a = polys.pack().bits if packed else polys.convert("mask").masks
        b = PackedMasks.from_rle(rles, size, self.device).bits if packed else SegmentationMask(rles, size, mode="mask", device=self.device).masks
        both = a.new_empty((len(segs),) + tuple(a.shape[1:]))
        both[torch.tensor(poly, device=a.device)] = a
        both[torch.tensor(rle, device=a.device)] = b
        return PackedMasks(both, size) if packed else SegmentationMask(both, size, mode="mask")

    def get_groundtruth(self, index, packed=False):
        """the image's target at its original size; packed=True: "masks" as PackedMasks decoded straight into bits (evaluation)"""
        img_id = self.final_ids[index]
        info = self.imgs[img_id]
        return self._target(img_id, (int(info["width"]), int(info["height"])), packed)

    def __getitem__(self, index):
        img_id = self.final_ids[index]
        img = self._load_image(img_id)
        target = self._target(img_id, img.size).clip_to_image(remove_empty=False)
        img = to_device_u8(img, self.device)
        if self.transforms is not None:
            img, target, flip = self.transforms(img, target)
        else:
            flip = False
        return img, target, flip, index

    def get_img_info(self, index):
        return self.imgs[self.final_ids[index]]

    def get_img_id(self, index):
        return self.final_ids[index]

    def map_class_id_to_class_name(self, class_id):
        return CLASSES[class_id]

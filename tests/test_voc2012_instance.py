"""CPU: PascalVOCDataset2012 (COCO-format JSON with run-length masks) on a generated 3-image annotation file, against a hand-written
expectation: which images and annotations a task sees, boxes, labels, masks and ground truth."""
import json
import os

import numpy as np
import pytest
import torch

from abr_iod_amd.structures import rle as R


def _rect(h, w, x0, y0, x1, y1):
    m = np.zeros((h, w), np.uint8)
    m[y0:y1 + 1, x0:x1 + 1] = 1
    return m


def _write(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(0)
    sizes = {7: (40, 60), 3: (50, 30), 5: (32, 32)}         # id: (h, w); ids out of order on purpose
    images, annos = [], []
    for img_id in (7, 3, 5):
        h, w = sizes[img_id]
        name = "img{}.png".format(img_id)
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(os.path.join(str(tmp_path), name))
        images.append({"id": img_id, "file_name": name, "height": h, "width": w})

    def ann(aid, img_id, cat, box, crowd=0, counts_as="str"):
        h, w = sizes[img_id]
        x0, y0, x1, y1 = box
        rle = R.encode_one(_rect(h, w, x0, y0, x1, y1))
        if counts_as == "list":
            rle["counts"] = R.string_to_counts(rle["counts"])
        annos.append({"id": aid, "image_id": img_id, "category_id": cat, "bbox": [x0, y0, x1 - x0 + 1, y1 - y0 + 1], "iscrowd": crowd,
                      "area": (x1 - x0 + 1) * (y1 - y0 + 1), "segmentation": rle})

    # image 3: a dog (12, new), a person (15, old), and a cat (8, neither); image 5: a person only; image 7: a dog whose box is degenerate
    # plus a crowd dog -- the non-crowd annotations are "only empty boxes", so the image is dropped
    ann(1, 3, 12, (2, 3, 20, 30))
    ann(2, 3, 15, (5, 10, 29, 49), counts_as="list")        # touches the border: clip_to_image leaves it
    ann(3, 3, 8, (0, 0, 4, 4))
    ann(4, 5, 15, (1, 1, 30, 30))
    ann(5, 7, 12, (10, 10, 10, 20))                           # width 1
    ann(6, 7, 12, (0, 0, 50, 30), crowd=1)
    path = os.path.join(str(tmp_path), "inst.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": annos, "categories": []}, f)
    return path, sizes


def _ds(tmp_path, **kw):
    from abr_iod_amd.data.datasets import PascalVOCDataset2012
    path, sizes = _write(tmp_path)
    return PascalVOCDataset2012(str(tmp_path), path, device="cpu", **kw), sizes


def test_training_split_sees_new_classes_only(tmp_path):
    ds, sizes = _ds(tmp_path, new_classes=["dog"], old_classes=["person"], is_train=True)
    assert ds.ids == [3, 5, 7] and ds.final_ids == [3] and len(ds) == 1
    assert ds.get_img_id(0) == 3 and ds.get_img_info(0) == {"id": 3, "file_name": "img3.png", "height": 50, "width": 30}
    assert ds.map_class_id_to_class_name(12) == "dog"
    img, target, flip, index = ds[0]
    assert tuple(img.shape) == (50, 30, 3) and img.dtype == torch.uint8 and flip is False and index == 0
    assert target.size == (30, 50) and target.mode == "xyxy"
    assert target.bbox.tolist() == [[2.0, 3.0, 20.0, 30.0]]
    assert target.get_field("labels").tolist() == [12] and target.get_field("labels").dtype == torch.int64
    masks = target.get_field("masks")
    assert masks.size == (30, 50) and np.array_equal(masks.masks.numpy(), _rect(50, 30, 2, 3, 20, 30)[None])


def test_test_split_sees_new_and_old_classes(tmp_path):
    ds, sizes = _ds(tmp_path, new_classes=["dog"], old_classes=["person"], is_train=False)
    assert ds.final_ids == [3, 5] and ds.id_to_img_map == {0: 3, 1: 5}
    gt = ds.get_groundtruth(0)
    assert gt.bbox.tolist() == [[2.0, 3.0, 20.0, 30.0], [5.0, 10.0, 29.0, 49.0]] and gt.get_field("labels").tolist() == [12, 15]
    want = np.stack([_rect(50, 30, 2, 3, 20, 30), _rect(50, 30, 5, 10, 29, 49)])
    assert np.array_equal(gt.get_field("masks").masks.numpy(), want)
    packed = ds.get_groundtruth(0, packed=True).get_field("masks")
    assert packed.size == (30, 50) and np.array_equal(packed.unpack().numpy(), want)
    _, target, _, _ = ds[0]
    assert target.bbox.tolist() == gt.bbox.tolist()          # nothing to clip
    gt1 = ds.get_groundtruth(1)
    assert gt1.bbox.tolist() == [[1.0, 1.0, 30.0, 30.0]] and gt1.get_field("labels").tolist() == [15]


def test_crowd_only_and_degenerate_boxes_drop_the_image(tmp_path):
    ds, _ = _ds(tmp_path, new_classes=["dog", "person", "cat"], is_train=True)
    assert 7 not in ds.final_ids and ds.final_ids == [3, 5]
    assert ds.get_groundtruth(0).get_field("labels").tolist() == [12, 15, 8]


def test_a_wrong_size_annotation_is_named(tmp_path):
    path, _ = _write(tmp_path)
    data = json.load(open(path))
    data["annotations"][0]["segmentation"]["size"] = [30, 50]
    json.dump(data, open(path, "w"))
    from abr_iod_amd.data.datasets import PascalVOCDataset2012
    ds = PascalVOCDataset2012(str(tmp_path), path, new_classes=["dog"], device="cpu")
    with pytest.raises(AssertionError, match="instance 0"):
        ds[0]

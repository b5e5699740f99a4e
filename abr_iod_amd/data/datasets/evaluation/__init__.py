"""evaluate(dataset, predictions, output_folder, **kwargs) (mirror of maskrcnn_benchmark/data/datasets/evaluation/__init__.py): a
COCODataset is scored by the COCO protocol (evaluation/coco), everything else by the PASCAL VOC protocol (every configs/voc YAML evaluates
with it).  The reference picks the VOC instance metric by its PascalVOCDataset2012 class; that choice is made here by what its drivers set
from MODEL.MASK_ON: "segm" in iou_types."""
from .coco import coco_evaluation
from .voc import voc_evaluation, voc_evaluation_inst


def evaluate(dataset, predictions, output_folder, **kwargs):
    from ..coco import COCODataset
    args = dict(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    if isinstance(dataset, COCODataset):
        return coco_evaluation(**args)
    if "segm" in (kwargs.get("iou_types") or ()):
        return voc_evaluation_inst(**args)
    return voc_evaluation(**args)

"""evaluate(dataset, predictions, output_folder, **kwargs) (mirror of maskrcnn_benchmark/data/datasets/evaluation/__init__.py):
only the PASCAL VOC protocol is on this path (every configs/voc YAML evaluates with it).  The reference picks the instance metric by its
PascalVOCDataset2012 class; that reader is not carried here, so the choice is made by what its drivers set from MODEL.MASK_ON: "segm" in
iou_types."""
from .voc import voc_evaluation, voc_evaluation_inst


def evaluate(dataset, predictions, output_folder, **kwargs):
    args = dict(dataset=dataset, predictions=predictions, output_folder=output_folder, **kwargs)
    if "segm" in (kwargs.get("iou_types") or ()):
        return voc_evaluation_inst(**args)
    return voc_evaluation(**args)

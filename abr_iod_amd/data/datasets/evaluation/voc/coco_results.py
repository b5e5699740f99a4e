"""COCO-format mask results (mirror of maskrcnn_benchmark/data/datasets/evaluation/coco/coco_eval.py:159-210): one
{"image_id", "category_id", "segmentation", "score"} dict per predicted instance, "segmentation" a compressed run-length dict.  The
reference pastes with Masker and encodes with pycocotools on the host; here the masks are what inference(..., iou_types=("bbox", "segm"))
leaves in the predictions -- PackedMasks at the original image size -- or pasted uint8 masks, and ops.rle_encode encodes them on the device."""
import torch


def prepare_for_coco_segmentation(predictions, dataset, device="cuda"):
    from ..... import ops
    from .....structures.segmentation_mask import PackedMasks, SegmentationMask
    from .voc_eval_inst import _prediction_bits
    id_map = getattr(dataset, "id_to_img_map", None)
    json_ids = getattr(dataset, "contiguous_category_id_to_json_id", None)
    coco_results = []
    for image_id, prediction in enumerate(predictions):
        original_id = id_map[image_id] if id_map is not None else dataset.get_img_id(image_id)
        if len(prediction) == 0:
            continue
        info = dataset.get_img_info(image_id)
        width, height = int(info["width"]), int(info["height"])
        field = prediction.get_field("mask")
        if not isinstance(field, (PackedMasks, SegmentationMask, torch.Tensor)):
            raise TypeError("cannot encode a 'mask' field of type {}".format(type(field).__name__))
        bits = _prediction_bits(field, (width, height), torch.device(device))     # (uint8 masks of another size are resized as the metric does)
        rles = ops.rle_encode(bits, width=width)
        scores = prediction.get_field("scores").tolist()
        labels = prediction.get_field("labels").tolist()
        mapped = [json_ids[i] for i in labels] if json_ids is not None else labels
        coco_results.extend({"image_id": original_id, "category_id": mapped[k], "segmentation": rle, "score": scores[k]}
                            for k, rle in enumerate(rles))
    return coco_results

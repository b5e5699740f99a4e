from .coco_eval import do_coco_evaluation


def coco_evaluation(dataset, predictions, output_folder, box_only=False, iou_types=("bbox",), expected_results=(), expected_results_sigma_tol=4,
                    **kwargs):
    """evaluation/coco/__init__.py:4-22.  engine.inference hands every evaluator `alphabetical_order`, the VOC class-order switch; COCO labels
    follow the annotation file (data/datasets/coco.py), so it has nothing to decide here."""
    kwargs.pop("alphabetical_order", None)
    return do_coco_evaluation(dataset=dataset, predictions=predictions, box_only=box_only, output_folder=output_folder, iou_types=iou_types,
                              expected_results=expected_results, expected_results_sigma_tol=expected_results_sigma_tol, **kwargs)

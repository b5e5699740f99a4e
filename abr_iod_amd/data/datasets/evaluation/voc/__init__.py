import logging

from .coco_results import prepare_for_coco_segmentation  # noqa: F401
from .voc_eval import do_voc_evaluation
from .voc_eval_inst import do_voc_evaluation_inst


def voc_evaluation(dataset, predictions, output_folder, box_only=False, **_):
    """evaluation/voc/__init__.py:6-16"""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    if box_only:
        logger.warning("voc evaluation doesn't support box_only, ignored.")
    logger.info("performing voc evaluation, ignored iou_types.")
    return do_voc_evaluation(dataset=dataset, predictions=predictions, output_folder=output_folder, logger=logger)


def voc_evaluation_inst(dataset, predictions, output_folder, box_only=False, **_):
    """box and instance-mask AP (the reference's evaluation of its VOC2012 instance dataset, evaluation/__init__.py:25-28)"""
    logger = logging.getLogger("maskrcnn_benchmark.inference")
    if box_only:
        logger.warning("voc evaluation doesn't support box_only, ignored.")
    logger.info("performing voc instance evaluation (box and mask AP).")
    return do_voc_evaluation_inst(dataset=dataset, predictions=predictions, output_folder=output_folder, logger=logger)

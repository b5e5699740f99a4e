"""CPU: COCO's box_only evaluates proposal recall instead of raising NotImplementedError, and says what it needs when the predictions
carry no "objectness"."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def test_rpn_only_default_is_off_and_build_roi_heads_gives_an_empty_list():
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    assert cfg.MODEL.RPN_ONLY is False
    c = cfg.clone()
    c.merge_from_list(["MODEL.RPN_ONLY", True, "MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21])
    assert build_roi_heads(c, 1024) == []


def test_box_only_no_longer_raises_not_implemented():
    from coco_eval_common import tiny, tiny_predictions
    from abr_iod_amd.data.datasets.evaluation.coco import coco_eval
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import COCOResults, do_coco_evaluation
    assert COCOResults.METRICS["box_proposal"] == ["AR@100", "ARs@100", "ARm@100", "ARl@100", "AR@1000", "ARs@1000", "ARm@1000", "ARl@1000"]
    assert "Not carried" not in coco_eval.__doc__
    ds = tiny()
    preds = tiny_predictions(ds, perfect=True)
    for p in preds:
        p.add_field("objectness", p.get_field("scores").float())
    results, second = do_coco_evaluation(ds, preds, True, None, ("bbox",), (), 4, device="cpu")
    assert second is None and set(results.results) == {"box_proposal"}


def test_detections_without_objectness_are_a_value_error_naming_the_field():
    from coco_eval_common import tiny, tiny_predictions
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import MissingObjectness, do_coco_evaluation
    ds = tiny()
    with pytest.raises(ValueError, match='"objectness"') as e:
        do_coco_evaluation(ds, tiny_predictions(ds, perfect=True), True, None, ("bbox",), (), 4, device="cpu")
    assert isinstance(e.value, MissingObjectness) and "scores" in str(e.value)      # (its fields are named)

#!/usr/bin/env python3
"""R-101-C4 state-dict golden FROM THE REFERENCE (in-container only): the ordered keys, shapes, dtypes and requires_grad of the reference's
own R-101-C4 GeneralizedRCNN (ResNet101StagesTo4, modeling/backbone/resnet.py:60-64, :443-453) at the default FREEZE_CONV_BODY_AT 2, for the
21-class target detector of the 15-5 task.  Full width: the shapes are the ones a real R-101-C4 checkpoint holds.

The reference's GeneralizedRCNN cannot be built with CONV_BODY "R-101-C4" as it stands: its ResNet50Conv5ROIFeatureExtractor
(roi_heads/box_head/roi_box_feature_extractors.py:23-29) sets the layer4 StageSpec only for "R-50-C4" / "R-50-C5" and raises
UnboundLocalError for any other body.  Both branches build the same 3-block layer4 head, and so does upstream maskrcnn-benchmark for every
C4 body.  So the detector is built with "R-50-C4" and its `backbone` is replaced by the reference's own build_backbone() of the "R-101-C4"
cfg (modeling/backbone/backbone.py:12-19), in place: the module order, and with it the state-dict order, is the detector's.

Stored as tests/golden/r101_state_dict_shapes.json: {"overrides": [...], "entries": [[key, shape, dtype, requires_grad], ...]} in
state_dict() order; requires_grad is null for buffers."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

OVERRIDES = ["MODEL.DEVICE", "cpu", "MODEL.BACKBONE.CONV_BODY", "R-101-C4", "MODEL.BACKBONE.FREEZE_CONV_BODY_AT", 2,
             "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21]


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.backbone import build_backbone
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    cfg = rh.default_cfg(overrides=OVERRIDES)
    cfg50 = cfg.clone()
    cfg50.MODEL.BACKBONE.CONV_BODY = "R-50-C4"
    model = build_detection_model(cfg50)
    model.backbone = build_backbone(cfg)
    assert len(model.backbone.body.layer3) == 23 and len(model.roi_heads.box.feature_extractor.head.layer4) == 3
    params = dict(model.named_parameters())
    entries = [[k, list(v.shape), str(v.dtype).replace("torch.", ""), bool(params[k].requires_grad) if k in params else None]
               for k, v in model.state_dict().items()]
    with open(os.path.join(HERE, "r101_state_dict_shapes.json"), "w") as f:
        json.dump({"overrides": OVERRIDES, "entries": entries}, f, indent=0)
        f.write("\n")


if __name__ == "__main__":
    main()

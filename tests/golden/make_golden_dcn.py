#!/usr/bin/env python3
"""Deformable-conv state-dict golden FROM THE REFERENCE (in-container only): the key names and shapes of the reference's own
GeneralizedRCNN.state_dict() (modeling/backbone/resnet.py:105-125, :289-312; layers/misc.py:114-190) for the tiny detector of
tests/test_checkpoint.py (21 classes) under each STAGE_WITH_DCN / WITH_MODULATED_DCN / DEFORMABLE_GROUPS case of tests/test_dcn_config.py.
Stored as tests/golden/dcn_state_dict_shapes.json: {case name: {"overrides": [...], "shapes": {key: shape}}}."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import ref_harness as rh  # noqa: E402

TINY = ["MODEL.DEVICE", "cpu", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16, "MODEL.RESNETS.RES2_OUT_CHANNELS", 32,
        "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 128, "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21]

CASES = {
    "default": [],
    "v1_FTTF": ["MODEL.RESNETS.STAGE_WITH_DCN", (False, True, True, False)],
    "v2_TTTT": ["MODEL.RESNETS.STAGE_WITH_DCN", (True, True, True, True), "MODEL.RESNETS.WITH_MODULATED_DCN", True],
    "v1_dg2_FTFF": ["MODEL.RESNETS.STAGE_WITH_DCN", (False, True, False, False), "MODEL.RESNETS.DEFORMABLE_GROUPS", 2],
}


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.detector import build_detection_model
    out = {}
    for name, extra in CASES.items():
        cfg = rh.default_cfg(overrides=TINY + extra)
        model = build_detection_model(cfg)
        out[name] = {"overrides": [list(v) if isinstance(v, tuple) else v for v in extra],
                     "shapes": {k: list(v.shape) for k, v in model.state_dict().items()}}
    with open(os.path.join(HERE, "dcn_state_dict_shapes.json"), "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    main()

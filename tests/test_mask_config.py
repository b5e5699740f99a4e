"""CPU: the mask head's configuration, state-dict boundary and SegmentationMask against values recorded from the reference
(tests/golden/make_golden_mask.py)."""
import json
import os

import numpy as np
import pytest
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _cfg(*overrides):
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(["MODEL.MASK_ON", True, "MODEL.DEVICE", "cpu", "MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21] + list(overrides))
    return c


def test_defaults_equal_the_references():
    from abr_iod_amd.config import cfg
    want = json.load(open(os.path.join(GOLD, "mask_defaults.json")))
    got = {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in cfg.MODEL.ROI_MASK_HEAD.items()}
    assert got == want
    assert cfg.MODEL.MASK_ON is False


@pytest.mark.parametrize("key,value", [("FEATURE_EXTRACTOR", "MaskRCNNFPNFeatureExtractor"), ("PREDICTOR", "MaskRCNNConv1x1Predictor"), ("USE_GN", True),
                                       ("DILATION", 2), ("SHARE_BOX_FEATURE_EXTRACTOR", False), ("POOLER_RESOLUTION", 7),
                                       ("POOLER_SAMPLING_RATIO", 2), ("POOLER_SCALES", (0.125,))])
def test_unsupported_keys_raise_and_name_themselves(key, value):
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    with pytest.raises(NotImplementedError, match="ROI_MASK_HEAD." + key):
        build_roi_heads(_cfg("MODEL.ROI_MASK_HEAD." + key, value), 1024)


def test_resolution_must_fit_the_pooler():
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    with pytest.raises(ValueError, match="RESOLUTION"):
        build_roi_heads(_cfg("MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 7), 1024)
    heads = build_roi_heads(_cfg("MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", 7, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", 7,
                                 "MODEL.ROI_MASK_HEAD.RESOLUTION", 8), 1024)
    assert "mask" in heads


def test_state_dict_names_and_shapes_equal_the_references():
    from abr_iod_amd.modeling.detector.generalized_rcnn import GeneralizedRCNN
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict, reference_state_dict
    want = json.load(open(os.path.join(GOLD, "mask_state_dict_shapes.json")))
    model = GeneralizedRCNN(_cfg())
    sd = reference_state_dict(model)
    assert {k: list(v.shape) for k, v in sd.items()} == want
    assert any(k.startswith("roi_heads.mask.feature_extractor.head.layer4") for k in sd)
    # round trip (the duplicate keys are accepted), and MASK_ON = False keeps its keys
    other = GeneralizedRCNN(_cfg())
    load_reference_state_dict(other, sd)
    back = reference_state_dict(other)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    off = _cfg()
    off.MODEL.MASK_ON = False
    assert not any("mask" in k for k in reference_state_dict(GeneralizedRCNN(off)))


def test_grown_head_copies_the_old_rows_of_mask_fcn_logits():
    from abr_iod_amd.modeling.detector.generalized_rcnn import GeneralizedRCNN
    from abr_iod_amd.utils.checkpoint import load_state_dict, reference_state_dict
    small = GeneralizedRCNN(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 11))
    big = GeneralizedRCNN(_cfg("MODEL.ROI_BOX_HEAD.NUM_CLASSES", 16))
    before = reference_state_dict(big)
    sd = reference_state_dict(small)
    load_state_dict(big, sd)
    after = reference_state_dict(big)
    for name in ("roi_heads.mask.predictor.mask_fcn_logits", "roi_heads.box.predictor.cls_score"):
        for part in ("weight", "bias"):
            k = "{}.{}".format(name, part)
            assert after[k].shape[0] == 16 and torch.equal(after[k][:11], sd[k]) and torch.equal(after[k][11:], before[k][11:]), k
    k = "roi_heads.mask.predictor.conv5_mask.weight"
    assert torch.equal(after[k], sd[k])


@pytest.mark.parametrize("tag", ["u8", "f32"])
def test_segmentation_mask_against_the_reference(tag):
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    g = np.load(os.path.join(GOLD, "mask_segmentation.npz"))
    inst = torch.from_numpy(g[tag + "_masks"])
    W, H = inst.shape[2], inst.shape[1]
    sm = SegmentationMask(inst, (W, H), mode="mask")
    assert len(sm) == 3 and sm.get_mask_tensor().shape == (3, H, W)
    for i, b in enumerate(g["crop_boxes"]):
        c = sm.crop(torch.from_numpy(b))
        assert np.array_equal(c.masks.numpy(), g["%s_crop%d" % (tag, i)]) and c.size == (c.masks.shape[2], c.masks.shape[1])
        r = c.resize((14, 9))
        assert r.masks.dtype == inst.dtype and r.size == (14, 9)
        assert np.array_equal(r.masks.numpy(), g["%s_crop%d_resize" % (tag, i)])
    assert np.array_equal(sm.transpose(0).masks.numpy(), g[tag + "_flip0"])
    assert np.array_equal(sm.transpose(1).masks.numpy(), g[tag + "_flip1"])
    assert np.array_equal(sm[torch.tensor([2, 0])].masks.numpy(), g[tag + "_index"])
    assert np.array_equal(sm.resize((50, 40)).masks.numpy(), g[tag + "_resize"])
    assert sm[1].get_mask_tensor().shape == (H, W)
    # BoxList carries the field through indexing, flipping and resizing
    bl = BoxList(torch.tensor([[1.0, 2.0, 30.0, 40.0], [5.0, 5.0, 60.0, 50.0], [0.0, 0.0, 9.0, 9.0]]), (W, H))
    bl.add_field("masks", sm)
    assert np.array_equal(bl[torch.tensor([2, 0])].get_field("masks").masks.numpy(), g[tag + "_index"])
    assert np.array_equal(bl.transpose(0).get_field("masks").masks.numpy(), g[tag + "_flip0"])
    assert np.array_equal(bl.resize((50, 40)).get_field("masks").masks.numpy(), g[tag + "_resize"])
    with pytest.raises(NotImplementedError):
        SegmentationMask([[0, 0, 1, 1, 2, 2]], (W, H), mode="poly")


def test_synthetic_masks_are_opt_in_and_leave_the_batch_unchanged():
    from abr_iod_amd.engine.synthetic import synthetic_batch
    im0, t0 = synthetic_batch(2, 64, 96, seed=5, device="cpu", max_boxes=3)
    for shape, dt in (("ellipse", torch.uint8), ("rect", torch.float32)):
        im1, t1 = synthetic_batch(2, 64, 96, seed=5, device="cpu", max_boxes=3, masks=shape, mask_dtype=dt)
        assert torch.equal(im0, im1)
        for a, b in zip(t0, t1):
            assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("labels"), b.get_field("labels")) and not a.has_field("masks")
            m = b.get_field("masks")
            assert len(m) == len(b) and m.masks.dtype == dt and m.size == (96, 64) and bool(m.masks.flatten(1).any(1).all())

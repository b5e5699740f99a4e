"""CPU: MODEL.ROI_KEYPOINT_HEAD's defaults, what the keypoint head refuses, and its checkpoint layout, against the reference's recorded
defaults and state_dict shapes (tests/golden/make_golden_keypoint.py)."""
import json
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ON = ["MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False, "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 56]


def _cfg(extra=()):
    from abr_iod_amd.config import cfg
    c = cfg.clone()
    c.merge_from_list(ON + list(extra))
    return c


def test_defaults_equal_the_reference():
    from abr_iod_amd.config import cfg
    want = json.load(open(os.path.join(GOLDEN, "keypoint_defaults.json")))
    got = {k: (list(v) if isinstance(v, (tuple, list)) else v) for k, v in cfg.MODEL.ROI_KEYPOINT_HEAD.items()}
    assert got == want
    assert cfg.MODEL.KEYPOINT_ON is False


@pytest.mark.parametrize("key,value", [("FEATURE_EXTRACTOR", "KeypointRCNNFPNFeatureExtractor"), ("PREDICTOR", "Other"), ("SHARE_BOX_FEATURE_EXTRACTOR", True),
                                       ("POOLER_SCALES", (0.25, 0.125)), ("POOLER_SCALES", (0.125,)), ("CONV_LAYERS", (512, 510)), ("CONV_LAYERS", ()),
                                       ("POOLER_RESOLUTION", 17), ("POOLER_RESOLUTION", 34)])
def test_unsupported_settings_name_their_key(key, value):
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    extra = ["MODEL.ROI_KEYPOINT_HEAD." + key, value]
    if key == "POOLER_RESOLUTION":
        extra += ["MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 4 * value]
    with pytest.raises(NotImplementedError, match="ROI_KEYPOINT_HEAD." + key):
        build_roi_heads(_cfg(extra), 1024)


def test_resolution_mismatch_names_the_value_to_set():
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    with pytest.raises(ValueError, match="set RESOLUTION to 56"):
        build_roi_heads(_cfg(["MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 14]), 1024)
    with pytest.raises(ValueError, match="set RESOLUTION to 28"):
        build_roi_heads(_cfg(["MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", 7]), 1024)
    with pytest.raises(NotImplementedError):
        build_roi_heads(_cfg(["MODEL.RETINANET_ON", True]), 1024)


def test_keypoint_off_builds_nothing_new():
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.roi_heads.roi_heads import build_roi_heads
    heads = build_roi_heads(cfg.clone(), 1024)
    assert list(heads.keys()) == ["box"]


def test_state_dict_names_shapes_and_round_trip():
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.utils.checkpoint import load_reference_state_dict, reference_state_dict
    want = json.load(open(os.path.join(GOLDEN, "keypoint_state_dict_shapes.json")))
    cfg = _cfg(["MODEL.ROI_BOX_HEAD.NUM_CLASSES", 21, "MODEL.DEVICE", "cpu"])
    torch.manual_seed(0)
    model = build_detection_model(cfg)
    sd = reference_state_dict(model)
    assert {k: list(v.shape) for k, v in sd.items()} == want
    kp = {k: v for k, v in sd.items() if k.startswith("roi_heads.keypoint.")}
    assert len(kp) == 18 and tuple(kp["roi_heads.keypoint.predictor.kps_score_lowres.weight"].shape) == (512, 17, 4, 4)
    assert tuple(kp["roi_heads.keypoint.predictor.kps_score_lowres.bias"].shape) == (17,)
    torch.manual_seed(1)
    other = build_detection_model(cfg)
    assert not torch.equal(reference_state_dict(other)["roi_heads.keypoint.feature_extractor.conv_fcn3.weight"], kp["roi_heads.keypoint.feature_extractor.conv_fcn3.weight"])
    load_reference_state_dict(other, sd)
    back = reference_state_dict(other)
    assert sorted(back) == sorted(sd) and all(torch.equal(back[k], sd[k]) for k in sd)
    # the padding rows of the deconvolution's GEMM weight and bias stay zero
    dc = other.roi_heads.keypoint.predictor.kps_score_lowres
    assert dc.kp == 20 and torch.all(dc.weight.detach().view(4, 4, 20, 512)[:, :, 17:] == 0) and torch.all(dc.bias.detach()[17:] == 0)


def test_coco_target_carries_keypoints(tmp_path):
    """a person-keypoint COCO file: the target gets a "keypoints" field (PersonKeypoints [n,17,3]) that follows the boxes through resize,
    flip and indexing; a file without keypoints gets none"""
    from abr_iod_amd.data.datasets.coco import COCODataset
    from abr_iod_amd.structures.keypoint import PersonKeypoints

    def kps(x0, y0, vis):
        return [v for k in range(17) for v in ((x0 + 2 * k, y0 + k, 2) if k < vis else (0, 0, 0))]

    anns = [dict(id=1, image_id=7, category_id=1, bbox=[10, 20, 60, 40], area=2400.0, iscrowd=0, keypoints=kps(12, 22, 12), num_keypoints=12),
            dict(id=2, image_id=7, category_id=1, bbox=[50, 5, 30, 30], area=900.0, iscrowd=0, keypoints=kps(52, 8, 3), num_keypoints=3),
            dict(id=3, image_id=7, category_id=1, bbox=[0, 0, 20, 20], area=400.0, iscrowd=1, keypoints=kps(1, 1, 17), num_keypoints=17)]
    doc = dict(images=[dict(id=7, file_name="a.jpg", width=100, height=80)], annotations=anns, categories=[dict(id=1, name="person")])
    f = tmp_path / "kp.json"
    f.write_text(json.dumps(doc))
    ds = COCODataset(str(f), str(tmp_path), True, device="cpu")
    assert len(ds) == 1                       # 15 visible keypoints on non-crowd annotations... the filter counts every annotation: kept
    t = ds.get_target(0)
    kp = t.get_field("keypoints")
    assert isinstance(kp, PersonKeypoints) and tuple(kp.keypoints.shape) == (2, 17, 3) and kp.size == (100, 80)
    assert kp.keypoints[0, 1].tolist() == [14.0, 23.0, 2.0] and kp.keypoints[1, 3].tolist() == [0.0, 0.0, 0.0]
    half = t.resize((50, 40)).get_field("keypoints")
    assert half.keypoints[0, 1].tolist() == [7.0, 11.5, 2.0] and half.size == (50, 40)
    flip = t.transpose(0).get_field("keypoints")
    assert flip.keypoints[0, 2].tolist() == [100 - 14.0 - 1, 23.0, 2.0]          # left_eye <-> right_eye
    assert tuple(t[[1]].get_field("keypoints").keypoints.shape) == (1, 17, 3)
    for a in anns:
        del a["keypoints"]
    f.write_text(json.dumps(doc))
    assert not COCODataset(str(f), str(tmp_path), True, device="cpu").get_target(0).has_field("keypoints")


def test_abr_paste_refuses_keypoint_targets():
    """the mixup / mosaic rebuild their targets from boxes and labels: with a "keypoints" field they raise and say so, before any draw"""
    from abr_iod_amd.data.abr import BoxRehearsalABR
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.keypoint import PersonKeypoints
    t = BoxList(torch.tensor([[1., 2, 30, 40]]), (64, 48))
    t.add_field("labels", torch.tensor([1]))
    t.add_field("keypoints", PersonKeypoints(torch.zeros(1, 17, 3), (64, 48)))
    with pytest.raises(NotImplementedError, match="keypoints"):
        BoxRehearsalABR.transform_current_data_with_ABR(None, None, t)

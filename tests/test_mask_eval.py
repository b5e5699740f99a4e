"""CPU: the host side of the instance-mask evaluation (evaluation/voc/voc_eval_inst.py, PackedMasks, the dispatch in evaluate) against
tests/golden/mask_eval.npz, which tests/golden/make_golden_mask_eval.py wrote from the reference's own voc_eval_inst.py.  The bound 1e-12
is tests/test_voc_eval.py's for the same float64 arithmetic."""
import logging

import numpy as np
import pytest
import torch

from abr_iod_amd.data.datasets.evaluation import evaluate
from abr_iod_amd.data.datasets.evaluation.voc import voc_eval_inst as V
from abr_iod_amd.structures.bounding_box import BoxList
from abr_iod_amd.structures.segmentation_mask import PackedMasks, SegmentationMask

from mask_eval_common import FakeInstDataset, check_tables, lists, reference_mask_iou
from test_voc_eval import _FakeVOC, _lists


def _records(g):
    preds, gts, _ = lists(g)
    recs = []
    for i, (p, t) in enumerate(zip(preds, gts)):
        boxes = p.copy_with_fields(["labels", "scores"]).resize(t.size)
        np.testing.assert_array_equal(boxes.bbox.numpy(), g["rb%d" % i])      # the reference's own resized boxes
        recs.append(V.image_record(boxes, t, reference_mask_iou(g, i)))
    return recs


def test_matching_and_ap_reproduce_the_reference(gold):
    g = gold("mask_eval")
    check_tables(g, _records(g))


def test_summary_text_and_return_value(gold, tmp_path, capsys):
    g = gold("mask_eval")
    _, _, dataset = lists(g)
    res, ap_boxes, ap_masks = V.summarise(dataset, _records(g), str(tmp_path), logging.getLogger("test"))
    np.testing.assert_allclose(ap_boxes, g["ap_box"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(ap_masks, g["ap_mask"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(res["mask"], g["ret_mask"], rtol=0, atol=1e-12)
    assert res["box"] == str(g["ret_box"])
    assert (tmp_path / "result.txt").read_text() == str(g["result_txt"])
    out = capsys.readouterr().out
    assert "BOX: " in out and "MSK: " in out


def test_mask_iou_from_counts_edges():
    iou = V.mask_iou_from_counts([[1, 0], [0, 0]], [1, 0], [2, 0])
    assert iou[0, 0] == 0.5 and iou[0, 1] == 0.0 and iou[1, 0] == 0.0
    assert iou[1, 1] == 0.0                      # empty union: the reference's `break` path
    assert V._claim(np.array([[0.5]]), 0.5) == [1]          # unmatched iff max < thresh: equality matches
    assert V._claim(np.array([[0.7, 0.7], [0.7, 0.7]]), 0.5) == [1, 0]      # first maximum; a claimed ground truth is not credited again


def test_bbox_only_dispatch_is_unchanged(gold, tmp_path):
    g = gold("voc_eval")
    preds, gts = _lists(g)
    r = evaluate(_FakeVOC(gts, 1), preds, str(tmp_path), box_only=False, iou_types=("bbox",))
    assert set(r) == {"ap", "map"}
    np.testing.assert_allclose(r["ap"], g["ap_area"], atol=1e-12, equal_nan=True)
    assert (tmp_path / "result.txt").read_text().startswith("mAP: ")


def test_segm_reaches_the_instance_metric(monkeypatch, tmp_path):
    from abr_iod_amd.data.datasets.evaluation import voc
    seen = {}

    def fake(dataset, predictions, output_folder, logger):
        seen["args"] = (dataset, predictions, output_folder)
        return {"mask": np.zeros(1), "box": ""}

    monkeypatch.setattr(voc, "do_voc_evaluation_inst", fake)
    r = evaluate("dataset", ["p"], str(tmp_path), box_only=False, iou_types=("bbox", "segm"))
    assert set(r) == {"mask", "box"} and seen["args"] == ("dataset", ["p"], str(tmp_path))


def _packed(n=3, w=70, h=5):
    bits = torch.arange(n * h * 2, dtype=torch.int64).reshape(n, h, 2) * 0x0101010101
    bits[:, :, 1] &= (1 << (w - 64)) - 1
    return PackedMasks(bits, (w, h))


def test_packed_masks_container():
    pm = _packed()
    assert len(pm) == 3 and pm.instances is pm and pm.unpack().shape == (3, 5, 70) and pm.unpack().dtype == torch.uint8
    want = np.unpackbits(pm.bits.numpy().view(np.uint8).reshape(3, 5, 16), axis=-1, bitorder="little")[:, :, :70]
    np.testing.assert_array_equal(pm.unpack().numpy(), want)
    assert len(pm[torch.tensor([2, 0])]) == 2 and torch.equal(pm[torch.tensor([2, 0])].bits, pm.bits[[2, 0]])
    assert len(pm[1:]) == 2 and len(pm[torch.tensor([True, False, True])]) == 2
    b = BoxList(torch.tensor([[0.0, 0, 9, 4], [1, 1, 5, 3], [2, 0, 60, 4]]), (70, 5))
    b.add_field("labels", torch.tensor([1, 2, 3]))
    b.add_field("mask", pm)
    sub = b[torch.tensor([2, 1])]
    assert isinstance(sub.get_field("mask"), PackedMasks) and torch.equal(sub.get_field("mask").bits, pm.bits[[2, 1]])
    assert isinstance(b.to("cpu").get_field("mask"), PackedMasks)
    assert b.resize((70, 5)).get_field("mask").size == (70, 5)
    with pytest.raises(ValueError):
        b.resize((140, 10))
    with pytest.raises(ValueError):
        pm.resize((35, 5))
    with pytest.raises(AssertionError):
        PackedMasks(pm.bits, (200, 5))


def test_entry_points_reject_bad_arguments_without_a_gpu():
    from abr_iod_amd import _lib
    L = _lib.lib()
    cases = [
        (L.abr_mask_pack_bits, (None, 1, 2, 4, 4, None, None), b"mask_pack_bits"),
        (L.abr_mask_pack_bits, (None, 1, 0, 65536, 32768, None, None), b"mask_pack_bits"),              # H * W = 2^31
        (L.abr_mask_pack_bits, (None, 1, -1, 4, 4, None, None), b"mask_pack_bits"),
        (L.abr_mask_resize_pack_bits, (None, 2, 4, 4, 8, 8, None, None), b"mask_resize_pack_bits"),
        (L.abr_mask_resize_pack_bits, (None, 0, 4, 4, 0, 8, None, None), b"mask_resize_pack_bits"),
        (L.abr_mask_resize_pack_bits, (None, 2, 4, 4, 4, 4, None, None), b"mask_pack_bits"),            # equal sizes reduce to the plain pack
        (L.abr_mask_pair_counts, (None, None, None, None, 1, 1, 4, 4, 4, None, None, None, None), b"mask_pair_counts"),
        (L.abr_mask_pair_counts, (None, None, None, None, 0, 0, 4, 4, 5, None, None, None, None), b"words"),
        (L.abr_mask_pair_counts, (None, None, None, None, 0, 0, 65536, 32768, 65536 * 512, None, None, None, None), b"2^31"),
    ]
    for fn, args, word in cases:
        rc = fn(*args)
        assert rc < 0 and word in L.abr_last_error(), (args, rc, L.abr_last_error())
    assert L.abr_mask_pair_counts(None, None, None, None, 0, 0, 4, 4, 4, None, None, None, None) == 0      # nothing to do: no launch
    assert L.abr_mask_pack_bits(None, 1, 0, 4, 4, None, None) == 0


def test_bare_probability_tensor_names_the_config_key(gold):
    g = gold("mask_eval")
    preds, gts, dataset = lists(g)
    p = preds[0].copy_with_fields(["labels", "scores"])
    p.add_field("mask", torch.rand(len(p), 1, 28, 28))
    with pytest.raises(ValueError, match="POSTPROCESS_MASKS"):
        V.do_voc_evaluation_inst(dataset, [p] + preds[1:], None, logging.getLogger("test"))

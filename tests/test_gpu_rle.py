"""GPU: the device run-length codec (csrc/rle.hip through ops.rle_decode / ops.rle_encode) against the host codec
(abr_iod_amd/structures/rle.py), its behaviour on malformed bytes, and the two paths it closes: annotation file -> dataset -> transforms ->
training step, and predictions -> COCO-format results.  Every comparison is exact: the format is integers and bytes."""
import json
import os
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _blob(rng, h, w, k):
    """a union of k random ellipses: long runs, thousands of them at 600x1000"""
    yy, xx = np.mgrid[:h, :w]
    m = np.zeros((h, w), bool)
    for _ in range(k):
        cy, cx = rng.uniform(0, h), rng.uniform(0, w)
        ry, rx = rng.uniform(2, max(3.0, h / 3)), rng.uniform(2, max(3.0, w / 3))
        m |= ((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 < 1
    return m.astype(np.uint8)


def _groups():
    """[(h, w, uint8 [n,h,w])]: a few hundred instances over the sizes that matter"""
    rng = np.random.default_rng(11)
    out = []
    for h, w in [(1, 1), (1, 70), (70, 1), (7, 63), (7, 64), (7, 65), (33, 127), (33, 128), (33, 129), (50, 37)]:
        ms = [np.zeros((h, w), np.uint8), np.ones((h, w), np.uint8)]
        single = np.zeros((h, w), np.uint8)
        single[rng.integers(h), rng.integers(w)] = 1
        ms.append(single)
        for dens in (0.02, 0.3, 0.5, 0.7, 0.98) * 4:
            ms.append((rng.random((h, w)) < dens).astype(np.uint8))
        for k in (1, 3):
            ms.append(_blob(rng, h, w, k))
        out.append((h, w, np.stack(ms)))
    out.append((375, 500, np.stack([_blob(rng, 375, 500, k) for k in (1, 2, 4, 8, 16, 32)] + [(rng.random((375, 500)) < 0.5).astype(np.uint8)])))
    big = np.stack([_blob(rng, 600, 1000, k) for k in (3, 12, 40)] + [1 - _blob(rng, 600, 1000, 25)])
    out.append((600, 1000, big))
    return out


def _unpack(bits, w):
    from abr_iod_amd.structures.segmentation_mask import PackedMasks
    return PackedMasks(bits, (w, bits.shape[1])).unpack()


def test_decode_vs_host_codec():
    from abr_iod_amd import ops
    from abr_iod_amd.structures import rle as R
    total, long_tokens, negative, max_runs = 0, 0, 0, 0
    for h, w, masks in _groups():
        rles = R.encode(masks)
        for r in rles:
            vals = [ord(c) - 48 for c in r["counts"]]
            long_tokens += any(v & 0x20 for v in vals)
            negative += any((not v & 0x20) and (v & 0x10) for v in vals)
            max_runs = max(max_runs, len(R.string_to_counts(r["counts"])))
        want = torch.from_numpy(R.decode(rles, (h, w)))
        assert np.array_equal(want.numpy(), masks)
        forms = [rles, [{"size": r["size"], "counts": r["counts"].encode("ascii")} for r in rles],
                 [{"size": r["size"], "counts": R.string_to_counts(r["counts"])} for r in rles]]
        for form in forms:
            u8 = ops.rle_decode(form, (h, w), "cuda")
            assert u8.dtype == torch.uint8 and u8.is_cuda and torch.equal(u8.cpu(), want), (h, w)
            bits = ops.rle_decode(form, (h, w), "cuda", packed=True)
            assert bits.dtype == torch.int64 and torch.equal(bits, ops.mask_pack_bits(u8)), (h, w)
            assert torch.equal(_unpack(bits, w).cpu(), want)
        total += len(rles)
    assert total >= 200 and long_tokens > 20 and negative > 20 and max_runs > 2000, (total, long_tokens, negative, max_runs)
    for packed in (False, True):
        e = ops.rle_decode([], (30, 70), "cuda", packed=packed)
        assert tuple(e.shape) == ((0, 30, 2) if packed else (0, 30, 70)) and e.is_cuda


def test_encode_vs_host_codec_and_round_trip():
    from abr_iod_amd import ops
    from abr_iod_amd.structures import rle as R
    from abr_iod_amd.structures.segmentation_mask import PackedMasks
    for h, w, masks in _groups():
        want = R.encode(masks)
        dev = torch.from_numpy(masks).cuda()
        got = ops.rle_encode(dev)
        assert got == want, (h, w)
        bits = ops.mask_pack_bits(dev)
        assert ops.rle_encode(PackedMasks(bits, (w, h))) == want and ops.rle_encode(bits, width=w) == want, (h, w)
        assert torch.equal(ops.rle_decode(got, (h, w), "cuda"), dev)
    assert ops.rle_encode(torch.zeros((0, 5, 5), dtype=torch.uint8, device="cuda")) == []
    # a mask close to noise needs more room than the first call gives: the capacity protocol's second call
    rng = np.random.default_rng(2)
    noise = (rng.random((2, 64, 512)) < 0.5).astype(np.uint8)
    want = R.encode(noise)
    assert sum(len(r["counts"]) for r in want) > 2 * max(1024, 64 * 512 // 16)
    assert ops.rle_encode(torch.from_numpy(noise).cuda()) == want


@pytest.mark.parametrize("packed", [False, True], ids=["u8", "packed"])
def test_malformed_bytes_are_reported_and_write_nothing_outside(packed):
    """a truncated token, a sum that is too large, a sum that is too small, a character outside [48,111], an over-long token, a negative
    count: the call raises naming the instance, and the guard regions around the output keep their pattern"""
    from abr_iod_amd import ops
    from abr_iod_amd.structures import rle as R
    h, w = 24, 70
    rng = np.random.default_rng(5)
    good = R.encode((rng.random((2, h, w)) < 0.4).astype(np.uint8))
    s = good[1]["counts"]
    counts = R.string_to_counts(s)
    too_large = R.counts_to_string(counts[:-1] + [counts[-1] + 100000])
    too_small = R.counts_to_string(counts[:-2])
    cases = {"truncated": s + "o", "too-large": too_large, "too-small": too_small,        # ("o": a final character that announces another one)
             "bad-char-low": s[:5] + " " + s[6:], "bad-char-high": s[:5] + "z" + s[6:], "long-token": "o" * 9 + "0" + s,
             "negative": R.counts_to_string([5, -3, h * w - 2]), "empty": "", "huge-first": R.counts_to_string([2 ** 31 - 1, 5])}
    guard = 4096
    shape = (2, h, (w + 63) // 64) if packed else (2, h, w)
    dtype = torch.int64 if packed else torch.uint8
    numel = 2 * h * shape[2]
    item = 8 if packed else 1
    for name, bad in cases.items():
        raw = torch.full((2 * guard + numel * item,), 0xA5, dtype=torch.uint8, device="cuda")
        out = raw[guard: guard + numel * item].view(dtype).view(shape)
        with pytest.raises(R.RLEError, match="instance 1"):
            ops.rle_decode([good[0], {"size": [h, w], "counts": bad}], (h, w), "cuda", packed=packed, out=out)
        torch.cuda.synchronize()
        assert bool((raw[:guard] == 0xA5).all()) and bool((raw[guard + numel * item:] == 0xA5).all()), name
        # the well-formed neighbour is decoded, the malformed instance is zeros
        want0 = torch.from_numpy(R.decode_one(good[0])).cuda()
        got0 = _unpack(out[:1], w)[0] if packed else out[0]
        assert torch.equal(got0, want0) and not bool(out[1].any()), name
    with pytest.raises(R.RLEError, match="instance 0.*size"):
        ops.rle_decode([{"size": [w, h], "counts": good[0]["counts"]}], (h, w), "cuda", packed=packed)
    # offsets that do not fit the byte buffer (only reachable through the C ABI): clamped, reported, nothing outside
    from abr_iod_amd import _lib as L
    data = torch.from_numpy(np.frombuffer(good[0]["counts"].encode("ascii"), np.uint8).copy()).cuda()
    offsets = torch.tensor([-7, 10 ** 9, 5], dtype=torch.int64, device="cuda")
    raw = torch.full((2 * guard + numel * item,), 0xA5, dtype=torch.uint8, device="cuda")
    out = raw[guard: guard + numel * item]
    totals = torch.full((2,), 12345, dtype=torch.int64, device="cuda")
    ws_bytes = L.lib().abr_rle_decode_workspace_bytes(2, data.numel())
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device="cuda")
    L.check(L.lib().abr_rle_decode(L.ptr(data), None, L.ptr(offsets), 2, data.numel(), h, w, None if packed else L.ptr(out), L.ptr(out) if packed else None,
                                   L.ptr(totals), L.ptr(ws), ws_bytes, L.stream()), "rle_decode")
    torch.cuda.synchronize()
    assert totals.tolist() == [h * w, 0]
    assert bool((raw[:guard] == 0xA5).all()) and bool((raw[guard + numel * item:] == 0xA5).all())


def test_segmentation_mask_and_packed_masks_from_rle_on_the_device():
    from abr_iod_amd.structures import rle as R
    from abr_iod_amd.structures.segmentation_mask import PackedMasks, SegmentationMask
    rng = np.random.default_rng(9)
    masks = np.stack([_blob(rng, 143, 200, k) for k in (1, 2, 5)])
    rles = R.encode(masks)
    seg = SegmentationMask(rles, (200, 143), mode="mask", device="cuda")
    assert seg.masks.is_cuda and torch.equal(seg.masks.cpu(), torch.from_numpy(masks))
    p = PackedMasks.from_rle(rles, (200, 143), device="cuda")
    assert p.bits.is_cuda and torch.equal(p.unpack().cpu(), torch.from_numpy(masks))
    with pytest.raises(AssertionError):
        SegmentationMask(rles, (143, 200), mode="mask", device="cuda")


BOXES = [[[10, 8, 60, 50], [50, 30, 100, 70]], [[5, 5, 40, 60], [60, 10, 105, 45], [30, 40, 80, 75]]]
LABELS = [[16, 18], [20, 17, 16]]


def _write_dataset(tmp_path):
    """two 80 x 112 images (h x w) whose Resize to (160, 224) is a real resize; elliptic instances inside BOXES"""
    from PIL import Image
    from abr_iod_amd.engine.synthetic import _box_masks
    from abr_iod_amd.structures import rle as R
    rng = np.random.default_rng(1)
    images, annos, masks = [], [], []
    for i, (boxes, labels) in enumerate(zip(BOXES, LABELS)):
        name = "im{}.png".format(i)
        Image.fromarray(rng.integers(0, 256, (80, 112, 3), dtype=np.uint8)).save(os.path.join(str(tmp_path), name))
        images.append({"id": i + 1, "file_name": name, "height": 80, "width": 112})
        m = _box_masks(torch.tensor(boxes, dtype=torch.float32), 80, 112, "ellipse", torch.uint8).numpy()
        masks.append(m)
        for b, l, rle in zip(boxes, labels, R.encode(m)):
            annos.append({"id": len(annos) + 1, "image_id": i + 1, "category_id": l, "iscrowd": 0,
                          "bbox": [b[0], b[1], b[2] - b[0] + 1, b[3] - b[1] + 1], "segmentation": rle})
    path = os.path.join(str(tmp_path), "inst.json")
    with open(path, "w") as f:
        json.dump({"images": images, "annotations": annos}, f)
    return path, masks


def _one_step(S, images, targets):
    from abr_iod_amd.engine import train_step
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    opt = make_optimizer(S["cfg_t"], S["mt"])
    sch = make_lr_scheduler(S["cfg_t"], opt)
    ld, _ = train_step(S["ms"], S["mt"], images, targets, opt, sch, S["cfg_t"], next_images=images)
    torch.cuda.synchronize()
    return {k: float(v.detach()) if hasattr(v, "detach") else float(v) for k, v in ld.items()}


def test_dataset_to_training_step(tmp_path):
    """PascalVOCDataset2012 -> GPUTransform (a x2 resize and a flip) -> collate -> one training step of the small mask-head setup gives the
    same losses as the same step fed the same masks as tensors"""
    from test_gpu_mask_head import _build
    from abr_iod_amd.data.abr import GPUTransform
    from abr_iod_amd.data.datasets import PascalVOCDataset2012
    from abr_iod_amd.data.datasets.voc import CLASSES, BatchCollator
    from abr_iod_amd.structures.segmentation_mask import FLIP_LEFT_RIGHT, SegmentationMask
    path, masks = _write_dataset(tmp_path)
    losses = []
    for route in ("rle", "tensors"):
        S = _build("15-5")
        cfg = S["cfg_t"].clone()
        cfg.merge_from_list(["INPUT.MIN_SIZE_TRAIN", (160,), "INPUT.MAX_SIZE_TRAIN", 224, "INPUT.FLIP_PROB_TRAIN", 1.0])
        tf = GPUTransform(cfg, is_train=True)
        ds = PascalVOCDataset2012(str(tmp_path), path, new_classes=list(CLASSES[1:]), transforms=tf, is_train=True, device="cuda")
        assert len(ds) == 2
        random.seed(0)
        batch = [ds[0], ds[1]]
        assert all(b[2] is True for b in batch)
        il, targets, idx = BatchCollator(tf, 0)(batch)
        assert tuple(il.tensors.shape) == (2, 3, 160, 224) and idx == [0, 1]
        targets = [t.to("cuda") for t in targets]
        for i, t in enumerate(targets):
            seg = t.get_field("masks")
            assert seg.size == (224, 160) and seg.masks.is_cuda and seg.masks.dtype == torch.uint8 and len(seg) == len(BOXES[i])
            assert t.get_field("labels").tolist() == LABELS[i]
            by_hand = SegmentationMask(torch.from_numpy(masks[i]).cuda(), (112, 80)).resize((224, 160)).transpose(FLIP_LEFT_RIGHT)
            assert torch.equal(seg.masks, by_hand.masks)
            if route == "tensors":
                t.add_field("masks", by_hand)
        losses.append(_one_step(S, il.tensors, targets))
    print("losses:", losses)
    assert losses[0]["loss_mask"] > 0 and losses[0]["loss_mask"] == losses[1]["loss_mask"]
    assert losses[0] == losses[1]


class _Loader(list):
    dataset = None


def test_predictions_to_coco_results(tmp_path):
    """compute_on_dataset(pack_masks=True) -- what inference(..., iou_types=("bbox", "segm")) evaluates -- -> prepare_for_coco_segmentation ->
    decode gives back the predicted masks"""
    from mask_eval_common import FakeInstDataset
    from test_gpu_mask_head import _build
    from abr_iod_amd import ops
    from abr_iod_amd.data.datasets.evaluation.voc import prepare_for_coco_segmentation
    from abr_iod_amd.engine.inference import compute_on_dataset

    class Dataset(FakeInstDataset):
        id_to_img_map = {0: 2008000008, 1: 2008000015}

    S = _build("15-5", extra=["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True])
    mt, images, targets = S["mt"], S["images"], S["targets"]
    sizes = [(200, 143), (180, 130)]
    gts = [t.to("cpu").resize(size) for t, size in zip(targets, sizes)]
    dataset = Dataset(gts, ["__background__"] + ["class%d" % i for i in range(1, 21)], n_new=5, n_old=15)
    loader = _Loader([(images, targets, (0, 1))])
    loader.dataset = dataset
    for pack in (True, False):
        preds, _ = compute_on_dataset(mt, loader, torch.device("cuda"), pack_masks=pack)
        preds = [preds[0], preds[1]]
        n = sum(len(p) for p in preds)
        assert n > 0
        results = prepare_for_coco_segmentation(preds, dataset)
        assert len(results) == n and json.loads(json.dumps(results)) == results
        k = 0
        for i, p in enumerate(preds):
            width, height = sizes[i]
            field = p.get_field("mask")
            if pack:
                want = field.unpack()
            else:       # pasted uint8 masks at the network's size: resized and thresholded as the metric does
                want = _unpack(ops.mask_resize_pack_bits(field[:, 0].cuda(), height, width), width).cpu()
            part = results[k: k + len(p)]
            k += len(p)
            assert [r["image_id"] for r in part] == [dataset.id_to_img_map[i]] * len(p)
            assert [r["category_id"] for r in part] == p.get_field("labels").tolist()       # no contiguous_category_id_to_json_id: the label
            assert [r["score"] for r in part] == p.get_field("scores").tolist()
            assert all(r["segmentation"]["size"] == [height, width] and isinstance(r["segmentation"]["counts"], str) for r in part)
            got = ops.rle_decode([r["segmentation"] for r in part], (height, width), "cuda").cpu()
            assert torch.equal(got, want)
    dataset.contiguous_category_id_to_json_id = {i: 100 + i for i in range(21)}
    mapped = prepare_for_coco_segmentation(preds, dataset)
    assert [r["category_id"] for r in mapped] == [100 + r["category_id"] for r in results]

"""GPU: the mask evaluation kernels (csrc/mask_eval.hip) and the instance metric built on them.  Every comparison is exact integer
equality unless it says otherwise; the resize is compared with torch's own CPU interpolate, and the cap on excused pixels is zero."""
import logging

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mask_eval_common import FakeInstDataset, check_tables, class_blocks, lists  # noqa: E402


def _words(bits):
    return bits.cpu().numpy().view(np.uint64)


def _np_pack(set_px):
    """bool [n,H,W] -> uint64 [n,H,ceil(W/64)], bit x % 64 of word x // 64"""
    n, H, W = set_px.shape
    Wq = (W + 63) // 64
    padded = np.zeros((n, H, Wq * 64), np.uint8)
    padded[:, :, :W] = set_px
    return np.packbits(padded, axis=-1, bitorder="little").view(np.uint64).reshape(n, H, Wq)


@pytest.mark.parametrize("W", [1, 63, 64, 65, 500])
@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_pack_bits_vs_numpy(dtype, W):
    from abr_iod_amd import ops
    rng = np.random.default_rng(W)
    vals = np.array([0, 1, 255, 1, 0, 1], np.uint8) if dtype == "u8" else np.array([0.0, 1.0, 255.0, 0.5, 1.0, 0.0], np.float32)
    m = vals[rng.integers(0, len(vals), size=(3, 7, W))]
    got = ops.mask_pack_bits(torch.from_numpy(m).cuda())
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, 7, (W + 63) // 64)
    np.testing.assert_array_equal(_words(got), _np_pack(m == 1))
    empty = ops.mask_pack_bits(torch.from_numpy(m[:0]).cuda())
    assert tuple(empty.shape) == (0, 7, (W + 63) // 64)


def _shape(rng, kind, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    if kind == 0:      # blob
        m = ((xs - rng.uniform(0, W)) / (W / 3 + 0.5)) ** 2 + ((ys - rng.uniform(0, H)) / (H / 3 + 0.5)) ** 2 <= 1
    elif kind == 1:    # thin lines
        m = (xs % 7 == int(rng.integers(0, 7))) | (ys % 5 == int(rng.integers(0, 5)))
    elif kind == 2:    # noise
        m = rng.random((H, W)) < 0.6
    else:              # all set, with a few 255s (not "set", and they pull neighbours off 1)
        m = np.ones((H, W), bool)
    m = m.astype(np.uint8)
    if kind == 3:
        m[rng.random((H, W)) < 0.01] = 255
    return m


def _size_pairs():
    rng = np.random.default_rng(2024)
    pairs = [(600, 1000, 375, 500), (600, 1000, 333, 500), (160, 224, 143, 200), (375, 500, 600, 1000), (100, 100, 64, 64), (100, 100, 64, 65),
             (37, 53, 37, 53), (1, 1, 1, 1), (1, 9, 5, 1), (9, 1, 1, 70), (1, 1, 40, 90), (50, 70, 1, 1), (64, 64, 128, 128), (3, 200, 2, 127)]
    while len(pairs) < 240:
        hi = int(rng.choice([8, 70, 140, 320]))
        pairs.append(tuple(int(v) for v in rng.integers(1, hi, 4)))
    return pairs


def test_resize_pack_bits_vs_torch_cpu_interpolate():
    """240 seeded (source, destination) size pairs: identity, 1-pixel sides, up- and down-scaling by non-integer ratios, on both sides of
    the output size at which torch changes its CPU kernel; blobs, thin lines, noise, 255s.  Zero differing pixels are allowed."""
    from abr_iod_amd import ops
    rng = np.random.default_rng(5)
    bad = []
    for k, (Hs, Ws, Hd, Wd) in enumerate(_size_pairs()):
        n = 1 + k % 4
        m = np.stack([_shape(rng, (k + j) % 4, Hs, Ws) for j in range(n)])
        want = torch.nn.functional.interpolate(torch.from_numpy(m)[None].float(), size=(Hd, Wd), mode="bilinear",
                                               align_corners=False)[0].to(torch.uint8).numpy() == 1
        got = _words(ops.mask_resize_pack_bits(torch.from_numpy(m).cuda(), Hd, Wd))
        diff = int(np.unpackbits((got ^ _np_pack(want)).view(np.uint8)).sum())
        if diff:
            bad.append(((Hs, Ws, Hd, Wd), diff))
    print("size pairs with differing pixels:", bad)
    assert not bad
    same = torch.from_numpy(_shape(rng, 2, 37, 53)[None]).cuda()
    assert torch.equal(ops.mask_resize_pack_bits(same, 37, 53), ops.mask_pack_bits(same))
    assert tuple(ops.mask_resize_pack_bits(same[:0], 20, 70).shape) == (0, 20, 2)


@pytest.mark.parametrize("P,T,H,W", [(5, 3, 33, 70), (100, 40, 375, 500), (3, 17, 20, 64), (0, 4, 10, 10), (4, 0, 10, 10)])
def test_pair_counts_vs_numpy(P, T, H, W):
    from abr_iod_amd import ops
    rng = np.random.default_rng(P * 100 + T)
    pm, gm = rng.random((P, H, W)) < 0.4, rng.random((T, H, W)) < 0.3
    if P:
        pm[0] = False
    pb, gb = ops.mask_pack_bits(torch.from_numpy(pm.astype(np.uint8)).cuda()), ops.mask_pack_bits(torch.from_numpy(gm.astype(np.uint8)).cuda())
    want = (pm.reshape(P, 1, -1) & gm.reshape(1, T, -1)).sum(-1) if P and T else np.zeros((P, T), np.int64)
    inter, ap, at = ops.mask_pair_counts(pb, gb, W)
    assert inter.dtype == torch.int32 and tuple(inter.shape) == (P, T)
    np.testing.assert_array_equal(inter.cpu().numpy(), want)
    if P and T:
        np.testing.assert_array_equal(ap.cpu().numpy(), pm.reshape(P, -1).sum(-1))
        np.testing.assert_array_equal(at.cpu().numpy(), gm.reshape(T, -1).sum(-1))
    pl, gl = torch.from_numpy(rng.integers(1, 4, P)), torch.from_numpy(rng.integers(1, 4, T))
    inter_l, ap_l, at_l = ops.mask_pair_counts(pb, gb, W, pl.cuda(), gl)
    np.testing.assert_array_equal(inter_l.cpu().numpy(), want * (pl.numpy()[:, None] == gl.numpy()[None, :]))
    assert torch.equal(ap_l, ap) and torch.equal(at_l, at)
    again = ops.mask_pair_counts(pb, gb, W, pl.cuda(), gl)
    assert all(torch.equal(a, b) for a, b in zip(again, (inter_l, ap_l, at_l)))


def _check_fixture_route(g, preds, gts, dataset, tmp_path):
    from abr_iod_amd.data.datasets.evaluation.voc import voc_eval_inst as V
    for i, (p, t) in enumerate(zip(preds, gts)):
        c = V.image_mask_counts(p, t, t.size)
        iou = V.mask_iou_from_counts(c["inter"], c["area_p"], c["area_t"])
        for l, rows, cols, block in class_blocks(g, i):
            assert (iou[np.ix_(rows, cols)] == block).all(), (i, l, iou[np.ix_(rows, cols)], block)
    records = V.prepare_records(dataset, preds)
    check_tables(g, records)
    res = V.do_voc_evaluation_inst(dataset, preds, str(tmp_path), logging.getLogger("test"))
    np.testing.assert_allclose(res["mask"], g["ret_mask"], rtol=0, atol=1e-12)
    assert res["box"] == str(g["ret_box"])
    assert (tmp_path / "result.txt").read_text() == str(g["result_txt"])
    return res


@pytest.mark.parametrize("where", ["device", "host"])
def test_instance_metric_on_the_reference_fixture(gold, tmp_path, where):
    g = gold("mask_eval")
    preds, gts, dataset = lists(g, "cuda" if where == "device" else "cpu")
    _check_fixture_route(g, preds, gts, dataset, tmp_path)


def test_packed_route_gives_identical_tables(gold, tmp_path):
    """the predictions packed first, as compute_on_dataset packs them, then sent to the host"""
    from abr_iod_amd.engine.inference import _pack_masks
    from abr_iod_amd.structures.segmentation_mask import PackedMasks
    g = gold("mask_eval")
    preds, gts, dataset = lists(g, "cuda")
    raw = []
    for p in preds:       # as the detector returns them: a bare [n,1,H,W] uint8 tensor
        q = p.copy_with_fields(["labels", "scores"])
        q.add_field("mask", p.get_field("mask").masks[:, None])
        raw.append(q)
    packed = [o.to("cpu") for o in _pack_masks(raw, list(range(len(raw))), dataset)]
    for o, t in zip(packed, gts):
        f = o.get_field("mask")
        assert isinstance(f, PackedMasks) and f.size == t.size and not f.bits.is_cuda
    _check_fixture_route(g, packed, gts, dataset, tmp_path)


class _Loader(list):
    dataset = None


def test_inference_end_to_end_box_and_mask_ap(tmp_path):
    from test_gpu_mask_head import _build
    from abr_iod_amd.data.datasets.evaluation.voc import voc_eval_inst as V
    from abr_iod_amd.engine.inference import compute_on_dataset, inference
    from abr_iod_amd.structures.segmentation_mask import PackedMasks, SegmentationMask
    S = _build("15-5", extra=["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True])
    mt, images, targets = S["mt"], S["images"], S["targets"]
    sizes = [(200, 143), (180, 130)]          # original (width, height): 224x160 is a non-integer multiple of both
    gts = []
    for t, size in zip(targets, sizes):
        gt = t.to("cpu").resize(size)
        gt.add_field("difficult", torch.zeros(len(gt), dtype=torch.uint8))
        gts.append(gt)
    # the reference sizes its AP tables by the largest class id seen (voc_eval_inst.py:191) and by the class lists (:27): they agree only
    # when the last class occurs, as it does on every VOC split
    gts[0].get_field("labels")[0] = 20
    dataset = FakeInstDataset(gts, ["__background__"] + ["class%d" % i for i in range(1, 21)], n_new=5, n_old=15)
    loader = _Loader([(images, targets, (0, 1))])
    loader.dataset = dataset

    res = inference(mt, loader, "synthetic", iou_types=("bbox", "segm"), output_folder=str(tmp_path))
    assert set(res) == {"mask", "box"} and res["mask"].shape == (20,) and res["box"].startswith("mAP OD\n")
    assert "mAP IS" in (tmp_path / "result.txt").read_text()

    plain, _ = compute_on_dataset(mt, loader, torch.device("cuda"))
    packed, _ = compute_on_dataset(mt, loader, torch.device("cuda"), pack_masks=True)
    assert sum(len(plain[i]) for i in (0, 1)) > 0
    wrapped = []
    for i in (0, 1):
        m = plain[i].get_field("mask")
        assert isinstance(m, torch.Tensor) and m.dtype == torch.uint8 and tuple(m.shape) == (len(plain[i]), 1, 160, 224)
        f = packed[i].get_field("mask")
        assert isinstance(f, PackedMasks) and f.size == sizes[i] and len(f) == len(plain[i])
        want = SegmentationMask(m[:, 0], (224, 160)).resize(sizes[i]).masks == 1        # torch's own resize on the host
        assert torch.equal(f.unpack().bool(), want)
        q = plain[i].copy_with_fields(["labels", "scores"])
        q.add_field("mask", SegmentationMask(m[:, 0], (224, 160)))
        wrapped.append(q)
    ref = V.do_voc_evaluation_inst(dataset, wrapped, None, logging.getLogger("test"))
    np.testing.assert_allclose(res["mask"], ref["mask"], rtol=0, atol=1e-12)
    assert res["box"] == ref["box"]

    box_only = inference(mt, loader, "synthetic", iou_types=("bbox",), output_folder=str(tmp_path))
    assert set(box_only) == {"ap", "map"}
    from abr_iod_amd.data.datasets.evaluation.voc.voc_eval import do_voc_evaluation
    want_box = do_voc_evaluation(dataset, [plain[0], plain[1]], None, logging.getLogger("test"))
    np.testing.assert_array_equal(box_only["ap"], want_box["ap"])

"""GPU: the polygon kernels (csrc/poly.hip) against the host codec (abr_iod_amd/structures/polygon.py, itself pinned to the plain
restatement and the known answers by tests/test_poly_host.py).  Every comparison is exact and no case is skipped."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_poly_host import KNOWN, forced_cases, known_mask, random_cases  # noqa: E402


def _both(instances, h, w):
    """-> (host masks, host status, device masks, device bits unpacked, device status)"""
    from abr_iod_amd import ops
    from abr_iod_amd.structures.polygon import PolygonList
    from abr_iod_amd.structures.segmentation_mask import PackedMasks
    pl = PolygonList(instances, (w, h))
    hm, hs = ops.poly_rasterize(pl, return_status=True)
    dl = pl.to("cuda")
    dm, ds = ops.poly_rasterize(dl, return_status=True)
    db, ds2 = ops.poly_rasterize(dl, packed=True, return_status=True)
    assert dm.is_cuda and dm.dtype == torch.uint8 and db.dtype == torch.int64 and tuple(db.shape) == (len(pl), h, (w + 63) // 64)
    assert torch.equal(ds, ds2) and ds.dtype == torch.int32
    return hm, hs, dm.cpu(), PackedMasks(db, (w, h)).unpack().cpu(), ds.cpu()


@pytest.mark.parametrize("name,xy,h,w,rows", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers_on_the_device(name, xy, h, w, rows):
    hm, hs, dm, db, ds = _both([[xy]], h, w)
    want = torch.from_numpy(known_mask(rows))[None]
    assert torch.equal(dm, want) and torch.equal(db, want) and torch.equal(hm, want) and ds.tolist() == [0]


def test_rasterize_equals_host_codec_on_forced_and_random_polygons():
    cases = forced_cases() + random_cases(2000)
    bad = []
    for name, xy, h, w in cases:
        hm, hs, dm, db, ds = _both([[xy]], h, w)
        if not (torch.equal(dm, hm) and torch.equal(db, hm) and torch.equal(ds, hs)):
            bad.append((name, int((dm != hm).sum()), int((db != hm).sum())))
    print("cases:", len(cases), "differing:", bad[:10])
    assert not bad


def _random_instances(rng, n, h, w, max_vertices, max_polys=3):
    out = []
    for _ in range(n):
        polys = []
        for _ in range(int(rng.integers(1, max_polys + 1))):
            k = int(rng.integers(8, max_vertices + 1))
            cx, cy = rng.uniform(0, w), rng.uniform(0, h)
            r = rng.uniform(0.05, 0.6) * min(h, w) * rng.uniform(0.6, 1.4, k)
            a = np.sort(rng.uniform(0, 2 * np.pi, k))
            polys.append(np.stack((cx + r * np.cos(a), cy + r * np.sin(a)), 1).astype(np.float32).reshape(-1).tolist())
        out.append(polys)
    return out


@pytest.mark.parametrize("h,w,n,max_vertices", [(600, 1000, 32, 200), (600, 1000, 7, 200), (375, 500, 32, 60), (375, 500, 1, 8)])
def test_rasterize_whole_images(h, w, n, max_vertices):
    rng = np.random.default_rng(h + n)
    inst = _random_instances(rng, n, h, w, max_vertices)
    inst[0] = [[-50, -50, w + 50, -50, w + 50, h + 50, -50, h + 50]]          # everything set
    if n > 2:
        inst[1] = []                                                            # an instance without polygons
        inst[2] = inst[2] + [[3, 3, float("nan"), 9, 20, 30]]                   # a guarded polygon beside good ones
    hm, hs, dm, db, ds = _both(inst, h, w)
    assert torch.equal(dm, hm) and torch.equal(db, hm) and torch.equal(ds, hs)
    assert hm[0].all() and (n <= 2 or (not hm[1].any() and hs[2] == 1 and hm[2].any()))
    assert 0.02 < hm[3:].float().mean() < 0.98 if n > 3 else True


@pytest.mark.parametrize("w", [63, 64, 65, 127, 128, 129])
def test_bit_layout_edges(w):
    rng = np.random.default_rng(w)
    h = 21
    inst = _random_instances(rng, 5, h, w, 12) + [[[w - 2.5, -1, w + 3, -1, w + 3, h + 1, w - 2.5, h + 1]], [[61.5, 2, 66.5, 2, 66.5, 19, 61.5, 19]]]
    hm, hs, dm, db, ds = _both(inst, h, w)
    assert torch.equal(dm, hm) and torch.equal(db, hm) and ds.tolist() == [0] * 7
    assert hm[5][:, w - 1].all() and hm[5][:, : w - 3].sum() == 0


def test_status_empty_list_and_out():
    from abr_iod_amd import ops
    from abr_iod_amd.structures.polygon import PolygonList
    ok = [2, 2, 17, 2, 17, 11, 2, 11]
    inst = [[ok], [[2, 2, float("nan"), 2, 17, 11]], [[2, 2, 1e9, 2, 17, 11]], [ok, [2, 2, float("inf"), 5, -1e9, 11]], [], [[0, 0, 32768.0, 0, 0, 9]]]
    hm, hs, dm, db, ds = _both(inst, 16, 24)
    assert hs.tolist() == [0, 1, 2, 3, 0, 0] and torch.equal(ds, hs) and torch.equal(dm, hm) and torch.equal(db, hm)
    assert not dm[1].any() and not dm[2].any() and torch.equal(dm[3], dm[0]) and dm[5].any()
    assert torch.equal(PolygonList(inst, (24, 16)).pack().unpack(), hm)        # the host's own packing
    empty = PolygonList([], (24, 16), device="cuda")
    m, st = ops.poly_rasterize(empty, return_status=True)
    assert tuple(m.shape) == (0, 16, 24) and m.is_cuda and tuple(st.shape) == (0,)
    assert tuple(ops.poly_rasterize(empty, packed=True).shape) == (0, 16, 1)
    pl = PolygonList(inst, (24, 16), device="cuda")
    out = torch.full((6, 16, 24), 7, dtype=torch.uint8, device="cuda")
    assert ops.poly_rasterize(pl, out=out) is out and torch.equal(out.cpu(), hm)
    bits = torch.full((6, 16, 1), -1, dtype=torch.int64, device="cuda")
    assert ops.poly_rasterize(pl, packed=True, out=bits) is bits and torch.equal(bits, ops.mask_pack_bits(out))
    with pytest.raises(RuntimeError):
        ops.poly_rasterize(pl, out=torch.zeros((6, 16, 25), dtype=torch.uint8, device="cuda"))
    assert torch.equal(pl.convert("mask").masks.cpu(), hm) and torch.equal(pl.pack().bits, bits)


# ------------------------------------------------------------------------------------------------------------ M x M targets
def _match(gt, b):
    """index of the GT box with the first maximum IoU (boxlist_iou, TO_REMOVE = 1, torch.max's tie rule), in fp32 as the reference"""
    area1 = (gt[:, 2] - gt[:, 0] + 1) * (gt[:, 3] - gt[:, 1] + 1)
    area2 = (b[2] - b[0] + 1) * (b[3] - b[1] + 1)
    lt, rb = torch.max(gt[:, :2], b[:2]), torch.min(gt[:, 2:], b[2:])
    wh = (rb - lt + 1).clamp(min=0)
    inter = wh[:, 0] * wh[:, 1]
    return int((inter / (area1 + area2 - inter)).max(0)[1])


def _host_targets(polys, gts, rois, pos_rows, M):
    """the reference's per-RoI procedure (mask_head/loss.py:11-42, 55-66) on the host through the PolygonList API: IoU argmax (first
    maximum), crop(box), resize((M, M)), rasterise; zeros for the -1 padding rows"""
    out = torch.zeros((len(pos_rows), M, M))
    for p, row in enumerate(pos_rows.tolist()):
        if row < 0:
            continue
        img = int(rois[row, 0])
        b = rois[row, 1:]
        out[p] = polys[img][_match(gts[img], b)].crop(b).resize((M, M)).get_mask_tensor().float()
    return out


def _target_case(seed):
    from abr_iod_amd.structures.polygon import PolygonList
    rng = np.random.default_rng(seed)
    sizes = [(224, 160), (200, 143), (333, 250), (97, 61)]          # (width, height)
    counts = [3, 1, 6, 2]                                            # different instance counts; the second image has one GT
    polys, gts, rois = [], [], []
    for img, ((W, H), n) in enumerate(zip(sizes, counts)):
        inst = _random_instances(rng, n, H, W, 24, max_polys=2)
        pl = PolygonList(inst, (W, H))
        gt = []
        for i in range(n):
            c = torch.cat(pl.polygons_of(i))
            gt.append([float(c[:, 0].min()), float(c[:, 1].min()), float(c[:, 0].max()), float(c[:, 1].max())])
        gt = torch.tensor(gt, dtype=torch.float32)
        polys.append(pl)
        gts.append(gt)
        for i in range(n):                                           # jittered copies of the GT boxes
            for _ in range(4):
                j = gt[i] + torch.from_numpy(rng.normal(0, 6, 4)).float()
                rois.append([img, min(j[0], j[2]), min(j[1], j[3]), max(j[0], j[2]), max(j[1], j[3])])
        rois += [[img, -30.5, -20.25, W * 0.6, H * 0.7], [img, W * 0.4, H * 0.3, W + 40.0, H + 25.5], [img, -10.0, -10.0, W + 10.0, H + 10.0],   # over every edge
                 [img, W * 0.5, H * 0.5, W * 0.5 + 0.3, H * 0.5 + 0.2], [img, 10.25, 12.5, 10.25, 12.5], [img, W - 0.5, H - 0.5, W + 5.0, H + 5.0],  # sub-pixel
                 [img, 0.0, 0.0, float(W - 1), float(H - 1)], [img, 8.0, 8.0, 36.0, 36.0]]                                                    # integer corners
    rois = torch.tensor([[float(v) for v in r] for r in rois], dtype=torch.float32)
    order = rng.permutation(len(rois))
    pos_rows = torch.from_numpy(np.concatenate((order[: len(order) * 3 // 4], [-1, -1, -1]))).long()
    return polys, gts, rois, pos_rows


@pytest.mark.parametrize("M", [8, 14, 28])
def test_poly_mask_targets_equal_the_per_roi_host_procedure(M):
    from abr_iod_amd import ops
    polys, gts, rois, pos_rows = _target_case(M)
    want = _host_targets(polys, gts, rois, pos_rows, M)
    got = ops.poly_mask_targets([p.to("cuda") for p in polys], [g.cuda() for g in gts], rois.cuda(), pos_rows.cuda(), M)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(pos_rows), M, M)
    got = got.cpu()
    differing = [(p, int(pos_rows[p]), int((got[p] != want[p]).sum())) for p in range(len(pos_rows)) if not torch.equal(got[p], want[p])]
    print("rows:", len(pos_rows), "differing:", differing[:10])
    assert not differing
    assert not got[-3:].any() and 0.05 < float(want[:-3].mean()) < 0.95
    assert set(got.unique().tolist()) <= {0.0, 1.0}
    # an image with a single GT, alone in the batch; and an empty row list
    one = (rois[:, 0] == 1).nonzero().flatten()
    r1 = rois[one].clone()
    r1[:, 0] = 0
    rows1 = torch.arange(len(one))
    got1 = ops.poly_mask_targets([polys[1].to("cuda")], [gts[1].cuda()], r1.cuda(), rows1.cuda(), M).cpu()
    assert torch.equal(got1, _host_targets([polys[1]], [gts[1]], r1, rows1, M))
    assert tuple(ops.poly_mask_targets([polys[1].to("cuda")], [gts[1].cuda()], r1.cuda(), rows1[:0].cuda(), M).shape) == (0, M, M)
    with pytest.raises(RuntimeError):
        ops.poly_mask_targets([polys[0].to("cuda")], [gts[1].cuda()], r1.cuda(), rows1.cuda(), M)      # 3 instances for 1 box


@pytest.mark.parametrize("M", [8, 14])
def test_bitmask_and_polygon_routes_agree_where_the_host_proves_it(M):
    """ops.mask_targets on PolygonList.convert("mask") resizes a rasterised mask bilinearly, ops.poly_mask_targets rasterises scaled
    vertices: in general they differ.  For an M x M RoI on integer corners both reduce to a shift by whole pixels (the crop is M wide, the
    resize is the identity, the ratio is 1), so there the HOST procedures (SegmentationMask.crop / resize against PolygonList.crop / resize)
    are compared first, and wherever they agree the two device routes must agree too.  The rectangles on integer corners are built so that
    they do; the count compared is asserted, not assumed."""
    from abr_iod_amd import ops
    from abr_iod_amd.structures.polygon import PolygonList
    rng = np.random.default_rng(M)
    W, H = 96, 64
    rect = lambda x0, y0, x1, y1: [[x0, y0, x1, y0, x1, y1, x0, y1]]      # noqa: E731
    inst = [rect(10, 8, 40, 30), rect(50, 20, 90, 60), rect(3, 40, 20, 61)] + _random_instances(rng, 2, H, W, 16, max_polys=1)
    pl = PolygonList(inst, (W, H))
    gt = torch.tensor([[10, 8, 40, 30], [50, 20, 90, 60], [3, 40, 20, 61], [0, 0, W - 1, H - 1], [20, 10, 70, 50]], dtype=torch.float32)
    corners = [(8, 6), (12, 10), (30, 20), (48, 18), (60, 30), (80, 48), (2, 38), (10, 45), (35, 25), (0, 0), (W - M, H - M), (40, 2)]
    rois = torch.tensor([[0.0, x, y, x + M, y + M] for x, y in corners if x + M <= W and y + M <= H], dtype=torch.float32)
    rows = torch.arange(len(rois))
    seg = pl.convert("mask")
    want = _host_targets([pl], [gt], rois, rows, M)
    poly = ops.poly_mask_targets([pl.to("cuda")], [gt.cuda()], rois.cuda(), rows.cuda(), M).cpu()
    bit = ops.mask_targets([seg.masks.cuda()], [gt.cuda()], rois.cuda(), rows.cuda(), M).cpu()
    assert torch.equal(poly, want)
    compared = 0
    for p in range(len(rois)):
        b = rois[p, 1:]
        host_bit = seg[_match(gt, b)].crop(b).resize((M, M)).get_mask_tensor().float()
        if torch.equal(host_bit, want[p]):      # proved on the host first
            compared += 1
            assert torch.equal(bit[p], poly[p]), p
    print("RoIs:", len(rois), "compared across the routes:", compared)
    assert compared >= len(rois) // 2 and float(want.mean()) > 0.1


# ------------------------------------------------------------------------------------------------------------ end to end
def test_training_step_on_polygon_targets():
    """one training step of the mask-on detector on synthetic_batch(..., masks="poly").  Every positive RoI's target is compared with the host
    polygon procedure (crop, resize, rasterise).  The bitmask route (ops.mask_targets on PolygonList.convert("mask")) resizes a rasterised
    mask bilinearly where this route rasterises scaled vertices, so the two legitimately differ; they are compared only for RoIs with
    integer corners for which the HOST proves the two procedures agree (SegmentationMask.crop / resize against PolygonList.crop / resize),
    and the count of such RoIs is printed."""
    import math
    from test_gpu_mask_head import _build
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.roi_heads.box_head.box_head import convert_to_roi_format
    from abr_iod_amd.structures.polygon import PolygonList
    from abr_iod_amd.engine.synthetic import synthetic_batch
    S = _build("finetune", res=7)
    mt, cfg = S["mt"], S["cfg_t"]
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=(16, 21), masks="poly")     # _build's batch, with polygons
    assert torch.equal(images, S["images"]) and all(t.get_field("masks").coords.is_cuda for t in targets)
    M = cfg.MODEL.ROI_MASK_HEAD.RESOLUTION
    mt.flat.zero_grad()
    loss_dict = mt(images, targets)[0]
    assert "loss_mask" in loss_dict
    sum(loss_dict.values()).backward()
    torch.cuda.synchronize()
    assert all(math.isfinite(float(v)) for v in loss_dict.values()), loss_dict
    grads = [p.grad for n, p in mt.named_parameters() if "roi_heads.mask.predictor" in n and p.requires_grad]
    assert len(grads) == 4 and all(g is not None and bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)

    det_props = mt.roi_heads.box.loss_evaluator._proposals
    rois = convert_to_roi_format(det_props).cpu()
    labels = torch.cat([p.get_field("labels") for p in det_props]).cpu()
    pos = (labels > 0).nonzero().flatten()
    sel = mt.roi_heads.mask.last_selection
    assert len(pos) > 0 and int(sel["n_pos"]) == len(pos) and torch.equal(sel["pos_rows"].cpu()[: len(pos)], pos)
    polys = [t.get_field("masks").to("cpu") for t in targets]
    assert all(isinstance(p, PolygonList) for p in polys)
    gts = [t.bbox.cpu() for t in targets]
    got = sel["mask_targets"].cpu()
    want = _host_targets(polys, gts, rois, pos, M)
    assert torch.equal(got[: len(pos)], want), "mask targets differ from the per-RoI polygon crop + resize + rasterise"
    assert not got[len(pos):].any() and 0.05 < float(want.mean()) < 0.95

    # the bitmask route on the same instances, for the integer-cornered RoIs where the host shows the two procedures agree
    segs = [p.convert("mask") for p in polys]
    bit = ops.mask_targets([s.masks.cuda() for s in segs], [g.cuda() for g in gts], rois.cuda(), sel["pos_rows"], M).cpu()
    integer, agree = 0, 0
    for p, row in enumerate(pos.tolist()):
        b = rois[row, 1:]
        if not bool((b == b.round()).all()):
            continue
        integer += 1
        img = int(rois[row, 0])
        host_bit = segs[img][_match(gts[img], b)].crop(b).resize((M, M)).get_mask_tensor().float()
        if torch.equal(host_bit, want[p]):      # (proved on the host first)
            agree += 1
            assert torch.equal(bit[p], got[p])
    print("positive RoIs:", len(pos), "with integer corners:", integer, "of which the host procedures agree:", agree)


class _Loader(list):
    dataset = None


def test_mask_ap_is_the_same_from_polygon_and_run_length_ground_truth(tmp_path):
    from mask_eval_common import FakeInstDataset
    from test_gpu_mask_head import _build
    from abr_iod_amd import ops
    from abr_iod_amd.engine.inference import inference
    from abr_iod_amd.structures.polygon import PolygonList
    from abr_iod_amd.structures.segmentation_mask import PackedMasks
    from abr_iod_amd.engine.synthetic import synthetic_batch
    S = _build("15-5", extra=["MODEL.ROI_MASK_HEAD.POSTPROCESS_MASKS", True])
    mt = S["mt"]
    images, targets = synthetic_batch(2, 160, 224, seed=3, max_boxes=3, label_range=(16, 21), masks="poly")
    sizes = [(200, 143), (180, 130)]
    names = ["__background__"] + ["class%d" % i for i in range(1, 21)]
    results = {}
    for kind in ("poly", "rle"):
        gts = []
        for t, size in zip(targets, sizes):
            gt = t.to("cpu").resize(size)
            f = gt.get_field("masks")
            assert isinstance(f, PolygonList) and f.size == size
            if kind == "rle":
                rles = ops.rle_encode(f.to("cuda").convert("mask").masks)
                gt.add_field("masks", PackedMasks.from_rle(rles, size, "cuda"))
            gt.add_field("difficult", torch.zeros(len(gt), dtype=torch.uint8))
            gts.append(gt)
        gts[0].get_field("labels")[0] = 20          # (see test_gpu_mask_eval.py: the AP tables are sized by the largest class id seen)
        loader = _Loader([(images, targets, (0, 1))])
        loader.dataset = FakeInstDataset(gts, names, n_new=5, n_old=15)
        out = tmp_path / kind
        out.mkdir()
        res = inference(mt, loader, "synthetic", iou_types=("bbox", "segm"), output_folder=str(out))
        text = (out / "result.txt").read_text()
        assert "mAP IS" in text
        results[kind] = (res, text[text.index("mAP IS"):])
    np.testing.assert_array_equal(results["poly"][0]["mask"], results["rle"][0]["mask"])
    assert results["poly"][1] == results["rle"][1] and results["poly"][0]["box"] == results["rle"][0]["box"]
    logging.getLogger("test").info("mAP IS from polygons: %s", results["poly"][1].splitlines()[:2])

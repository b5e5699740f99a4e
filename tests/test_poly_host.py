"""CPU: polygon instance masks -- the host codec (abr_iod_amd/structures/polygon.py) against the plain restatement (tests/poly_ref.py) and
the known answers of DESIGN.md §4, PolygonList's geometry against the reference's torch expressions, and the dataset's field types.
Every comparison is exact.  pycocotools cannot be imported where this project is built; the three known answers below were computed from
the restated algorithm and are asserted for every implementation (the device too, tests/test_gpu_poly.py)."""
import json
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poly_ref  # noqa: E402

from abr_iod_amd.structures.bounding_box import BoxList  # noqa: E402
from abr_iod_amd.structures.polygon import PolygonList  # noqa: E402
from abr_iod_amd.structures.segmentation_mask import FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, PackedMasks, SegmentationMask  # noqa: E402

KNOWN = [
    ("rectangle", [1, 1, 4, 1, 4, 3, 1, 3], 5, 6, ["000000", "011100", "011100", "000000", "000000"]),
    ("triangle", [0.5, 0.5, 6.5, 1.0, 3.0, 5.5], 7, 8, ["00000000", "01111100", "00111000", "00111000", "00010000", "00000000", "00000000"]),
    # leaves the grid on all four sides: negative truncation, the yd == h carry, dropped columns; every pixel but (x=0, y=5)
    ("quadrilateral", [-2.3, 1.2, 4.6, -1.5, 9.9, 3.3, 3.1, 8.7], 6, 7, ["1111111"] * 5 + ["0111111"]),
]


def known_mask(rows):
    return np.array([[int(c) for c in r] for r in rows], np.uint8)


def host_masks(instances, h, w, **kw):
    """list (instances) of lists (polygons) of flat lists -> what ops.poly_rasterize gives for the list on the CPU"""
    from abr_iod_amd import ops
    return ops.poly_rasterize(PolygonList(instances, (w, h)), **kw)


# ------------------------------------------------------------------------------------------------------------ cases (shared with the GPU tests)
def forced_cases():
    """(name, flat polygon, h, w)"""
    return [
        ("repeated last vertex", [2.2, 3.1, 20.7, 4.4, 11.3, 17.9, 2.2, 3.1], 24, 30),
        ("duplicate consecutive vertices", [2.2, 3.1, 2.2, 3.1, 20.7, 4.4, 20.7, 4.4, 20.7, 4.4, 11.3, 17.9], 24, 30),
        ("dx == dy edges", [3, 3, 13, 13, 23, 3, 13, -7], 20, 30),
        ("dx == dy edges, fractional", [3.3, 3.3, 13.3, 13.3, 23.3, 3.3], 20, 30),
        ("axis-aligned on integers", [2, 2, 17, 2, 17, 11, 2, 11], 16, 24),
        ("axis-aligned on .5", [2.5, 2.5, 17.5, 2.5, 17.5, 11.5, 2.5, 11.5], 16, 24),
        ("axis-aligned over the border", [-3, -2.5, 40, -2.5, 40, 7, -3, 7], 16, 24),
        ("entirely outside", [40, 40, 60, 41, 50, 70], 16, 24),
        ("entirely outside, negative", [-40, -40, -6, -41, -5, -7], 16, 24),
        ("covering everything", [-10, -10, 50, -10, 50, 50, -10, 50], 16, 24),
        ("one pixel grid", [-1, -1, 3, -1, 3, 3, -1, 3], 1, 1),
        ("self-intersecting", [1, 1, 20, 14, 20, 1, 1, 14], 16, 24),
        ("sliver", [1.0, 1.0, 22.0, 1.2, 1.0, 1.4], 16, 24),
    ]


def random_cases(count, seed=7):
    """sizes 1x1 .. 64x64 plus a few 375x500, 3..40 vertices, coordinates over -0.5 .. 1.5 of the image size"""
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(count):
        if i % 250 == 249:
            h, w = 375, 500
        elif i < 20:
            h, w = 1 + i % 4, 1 + i // 4
        else:
            h, w = int(rng.integers(1, 65)), int(rng.integers(1, 65))
        k = int(rng.integers(3, 41))
        xy = rng.uniform(-0.5, 1.5, (k, 2)) * [w, h]
        if i % 3 == 1:
            xy = np.round(xy * 2) / 2         # integer and .5 coordinates: axis-aligned and diagonal edges, crossings on pixel centres
        cases.append(("random %d" % i, xy.astype(np.float32).reshape(-1).tolist(), h, w))
    return cases


# ------------------------------------------------------------------------------------------------------------ the rasteriser
@pytest.mark.parametrize("name,xy,h,w,rows", KNOWN, ids=[k[0] for k in KNOWN])
def test_known_answers(name, xy, h, w, rows):
    want = known_mask(rows)
    np.testing.assert_array_equal(np.array(poly_ref.rasterize_polygon(xy, h, w), np.uint8), want)
    got, status = host_masks([[xy]], h, w, return_status=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1, h, w) and status.tolist() == [0]
    np.testing.assert_array_equal(got[0].numpy(), want)


def test_host_codec_equals_plain_restatement_on_random_and_forced_polygons():
    cases = forced_cases() + random_cases(2000)
    assert len(cases) >= 2000
    bad, odd_columns = [], 0
    for name, xy, h, w in cases:
        want = np.array(poly_ref.rasterize_polygon(xy, h, w), np.uint8)
        got = host_masks([[xy]], h, w)[0].numpy()
        if not np.array_equal(got, want):
            bad.append((name, int((got != want).sum())))
        odd_columns += bool(want[-1].any())
    print("polygons that leave the grid through the bottom row:", odd_columns, "of", len(cases))
    assert not bad, bad[:10]
    assert odd_columns > 100          # the carry across columns is exercised, not assumed
    for name, xy, h, w in forced_cases():
        m = host_masks([[xy]], h, w)[0].numpy()
        if name.startswith("entirely outside"):
            assert not m.any(), name
        if name in ("covering everything", "one pixel grid"):
            assert m.all(), name
    a, b = forced_cases()[0], forced_cases()[1]
    plain = host_masks([[[2.2, 3.1, 20.7, 4.4, 11.3, 17.9]]], 24, 30)
    assert torch.equal(host_masks([[a[1]]], 24, 30), plain) and torch.equal(host_masks([[b[1]]], 24, 30), plain)


def test_an_instance_is_the_union_of_its_polygons():
    rng = np.random.default_rng(3)
    h, w = 40, 52
    for _ in range(30):
        polys = [(rng.uniform(-0.3, 1.3, (int(rng.integers(3, 12)), 2)) * [w, h]).astype(np.float32).reshape(-1).tolist() for _ in range(int(rng.integers(2, 5)))]
        whole = host_masks([polys], h, w)[0]
        parts = host_masks([[p] for p in polys], h, w)
        assert torch.equal(whole, parts.max(0)[0])
        np.testing.assert_array_equal(whole.numpy(), np.array(poly_ref.rasterize_instance(polys, h, w), np.uint8))
    # two nested squares of the same orientation: a union keeps the inner square filled, even-odd across polygons would cut a hole
    outer, inner = [4, 4, 30, 4, 30, 30, 4, 30], [10, 10, 20, 10, 20, 20, 10, 20]
    ring = host_masks([[outer, inner]], 36, 36)[0]
    assert torch.equal(ring, host_masks([[outer]], 36, 36)[0]) and ring[15, 15] == 1 and ring.sum() == 26 * 26
    pm = PolygonList([[outer, inner], [inner]], (36, 36)).pack()
    assert isinstance(pm, PackedMasks) and torch.equal(pm.unpack(), host_masks([[outer, inner], [inner]], 36, 36))


def test_guard_gives_zeros_and_a_status_word():
    ok = [2, 2, 17, 2, 17, 11, 2, 11]
    m, st = host_masks([[ok], [[2, 2, float("nan"), 2, 17, 11]], [[2, 2, 1e9, 2, 17, 11]], [ok, [2, 2, float("inf"), 5, -1e9, 11]], []], 16, 24,
                       return_status=True)
    assert st.dtype == torch.int32 and st.tolist() == [0, 1, 2, 3, 0]
    assert m[0].sum() == 15 * 9 and not m[1].any() and not m[2].any() and not m[4].any()
    assert torch.equal(m[3], m[0])                 # the guarded polygon is left out, the instance's other polygon stays
    edge = 32768.0                                 # |5 c| == 5 * 32768 is still inside
    m, st = host_masks([[[0, 0, edge, 0, 0, 9]], [[0, 0, np.nextafter(np.float32(edge), np.float32(np.inf)), 0, 0, 9]]], 4, 4, return_status=True)
    assert st.tolist() == [0, 2] and m[0].any()
    np.testing.assert_array_equal(np.array(poly_ref.rasterize_polygon([2, 2, 1e9, 2, 17, 11], 16, 24)), 0)


# ------------------------------------------------------------------------------------------------------------ the structure
def _example():
    return [[[10.25, 5.5, 60.75, 7.125, 33.0, 41.5], [1, 2, 3, 4]],                       # (its second polygon has < 6 numbers: dropped)
            [[5, 5, 5.5, 30.25, 31, 29.0, 30, 4.75], [40.5, 20, 66, 21, 50, 39.5]],
            [[0, 0, 69.9, 0, 69.9, 44.9]]]


def _same(plist, want):
    """want: per instance a list of [k,2] tensors"""
    assert len(plist) == len(want)
    for i, polys in enumerate(want):
        got = plist.polygons_of(i)
        assert len(got) == len(polys)
        for a, b in zip(got, polys):
            assert a.dtype == torch.float32 and torch.equal(a, b), (i, a, b)


def test_polygon_list_geometry_is_the_reference_expressions():
    """the reference's PolygonInstance keeps one flat float32 tensor p per polygon, x at p[0::2], y at p[1::2] (segmentation_mask.py):
         transpose  p[idx::2] = dim - p[idx::2] - 1                                  (:238-242)
         crop       p[0::2] = p[0::2] - xmin, p[1::2] = p[1::2] - ymin with the box as Python floats clamped against the size (:251-270)
         resize     p * ratio when both ratios are equal, else p[0::2] *= ratio_w, p[1::2] *= ratio_h, ratios float(s) / float(s_orig) (:281-294)"""
    W, H = 70, 45
    pl = PolygonList(_example(), (W, H))
    flat = [[torch.as_tensor(p, dtype=torch.float32) for p in inst if len(p) >= 6] for inst in _example()]
    xy = lambda p: torch.stack((p[0::2], p[1::2]), 1)     # noqa: E731
    assert pl.coords.dtype == torch.float32 and tuple(pl.coords.shape) == (13, 2) and pl.size == (W, H)
    assert pl.poly_offsets.tolist() == [0, 3, 7, 10, 13] and pl.inst_offsets.tolist() == [0, 1, 3, 4] and pl.poly_offsets.dtype == torch.int64
    _same(pl, [[xy(p) for p in inst] for inst in flat])

    for method, dim, idx in ((FLIP_LEFT_RIGHT, W, 0), (FLIP_TOP_BOTTOM, H, 1)):
        want = []
        for inst in flat:
            want.append([])
            for p in inst:
                q = p.clone()
                q[idx::2] = dim - p[idx::2] - 1
                want[-1].append(xy(q))
        t = pl.transpose(method)
        _same(t, want)
        assert t.size == (W, H)
    with pytest.raises(NotImplementedError):
        pl.transpose(2)

    for box in ([5.2, 3.7, 50.5, 30.1], torch.tensor([-4.5, -2.0, 90.0, 44.2]), [12.3, 8.1, 12.4, 8.15], [69.7, 44.6, 80.0, 50.0]):
        xmin, ymin, xmax, ymax = map(float, box)
        xmin, ymin = min(max(xmin, 0), W - 1), min(max(ymin, 0), H - 1)
        xmax, ymax = min(max(xmax, 0), W), min(max(ymax, 0), H)
        xmax, ymax = max(xmax, xmin + 1), max(ymax, ymin + 1)
        want = []
        for inst in flat:
            want.append([])
            for p in inst:
                q = p.clone()
                q[0::2] = q[0::2] - xmin
                q[1::2] = q[1::2] - ymin
                want[-1].append(xy(q))
        c = pl.crop(box)
        _same(c, want)
        assert c.size == (xmax - xmin, ymax - ymin) and all(isinstance(s, float) for s in c.size)
        # ... and the resize the mask loss applies to the crop: ratios of floats, a different one per axis
        M = 14
        rw, rh = float(M) / float(xmax - xmin), float(M) / float(ymax - ymin)
        want_r = []
        for inst in want:
            want_r.append([])
            for p in inst:
                q = p.reshape(-1).clone()
                if rw == rh:
                    q = q * rw
                else:
                    q[0::2] *= rw
                    q[1::2] *= rh
                want_r[-1].append(xy(q))
        r = c.resize((M, M))
        _same(r, want_r)
        assert r.size == (M, M)

    both = pl.resize((140, 90))         # equal ratios: the reference's first branch
    _same(both, [[xy(p * 2.0) for p in inst] for inst in flat])
    assert pl.resize(35).size == (35, 35)


def test_polygon_list_container():
    W, H = 70, 45
    pl = PolygonList(_example(), (W, H))
    assert len(pl) == 3 and [len(pl.polygons_of(i)) for i in range(3)] == [1, 2, 1]
    assert pl.instances is pl and "num_instances=3" in repr(pl) and "image_width=70" in repr(pl)
    items = list(pl)
    assert len(items) == 3 and all(isinstance(p, PolygonList) and len(p) == 1 and p.size == (W, H) for p in items)
    full = pl.convert("mask")
    assert isinstance(full, SegmentationMask) and full.masks.dtype == torch.uint8 and tuple(full.masks.shape) == (3, H, W) and full.size == (W, H)
    assert pl.convert("poly") is pl
    for item, rows in ((1, [1]), (-1, [2]), (slice(0, 2), [0, 1]), (slice(None, None, -1), [2, 1, 0]), ([2, 0], [2, 0]), ([], []),
                       (torch.tensor([2, 2, 1]), [2, 2, 1]), (torch.tensor([True, False, True]), [0, 2]), (torch.tensor([False] * 3), [])):
        sub = pl[item]
        assert len(sub) == len(rows) and sub.size == (W, H)
        assert torch.equal(sub.convert("mask").masks, full.masks[rows])
        for j, i in enumerate(rows):
            assert all(torch.equal(a, b) for a, b in zip(sub.polygons_of(j), pl.polygons_of(i)))
    assert torch.equal(pl[[True, False, True]].coords, pl[[0, 2]].coords)      # a list of bools is a mask, not the indices 1, 0, 1
    with pytest.raises(IndexError):
        pl[[True, 1, 0]]
    with pytest.raises(IndexError):
        pl[3]
    with pytest.raises(IndexError):
        pl[torch.tensor([True, False])]
    assert torch.equal(items[1].get_mask_tensor(), full.masks[1])
    moved = pl.to("cpu")
    assert moved.coords.device.type == "cpu" and torch.equal(moved.coords, pl.coords) and len(moved) == 3
    again = PolygonList(pl, (1, 1))
    assert again.size == (W, H) and torch.equal(again.coords, pl.coords)       # a PolygonList brings its own size, as in the reference

    empty = PolygonList([], (W, H))
    assert len(empty) == 0 and list(empty) == [] and tuple(empty.coords.shape) == (0, 2)
    assert tuple(empty.convert("mask").masks.shape) == (0, H, W) and tuple(empty.pack().bits.shape) == (0, H, 2)
    assert len(empty[[]]) == 0 and len(empty.transpose(FLIP_LEFT_RIGHT).resize((7, 9))) == 0

    # fewer than 6 numbers: the polygon is dropped; the instance stays and rasterises to zeros
    short = PolygonList([[[1, 1, 5, 5]], [[1, 1, 9, 1, 9, 9, 1, 9], [3, 3]], [[]]], (12, 12))
    assert len(short) == 3 and [len(short.polygons_of(i)) for i in range(3)] == [0, 1, 0]
    m = short.convert("mask").masks
    assert not m[0].any() and m[1].sum() == 64 and not m[2].any()
    with pytest.raises(ValueError):
        PolygonList([[[1, 1, 5, 5, 3, 3, 2]]], (12, 12))
    with pytest.raises(ValueError):
        pl.crop([5.2, 3.7, 50.5, 30.1]).convert("mask")      # a float size: resize first
    with pytest.raises(NotImplementedError):
        pl.convert("rle")


def test_boxlist_carries_a_polygon_list():
    W, H = 70, 45
    boxes = torch.tensor([[10.0, 5.0, 61.0, 42.0], [5.0, 4.0, 66.0, 40.0], [0.0, 0.0, 69.0, 44.0]])
    t = BoxList(boxes, (W, H), mode="xyxy")
    t.add_field("labels", torch.tensor([3, 1, 2]))
    pl = PolygonList(_example(), (W, H))
    t.add_field("masks", pl)
    for item in ([2, 0], torch.tensor([True, False, True]), slice(1, 3)):
        s = t[item]
        assert isinstance(s.get_field("masks"), PolygonList) and torch.equal(s.get_field("masks").coords, pl[item].coords) and len(s.get_field("masks")) == len(s)
    for method in (FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM):
        f = t.transpose(method).get_field("masks")
        assert isinstance(f, PolygonList) and torch.equal(f.coords, pl.transpose(method).coords)
    r = t.resize((140, 100))
    f = r.get_field("masks")
    assert isinstance(f, PolygonList) and f.size == (140, 100) == r.size and torch.equal(f.coords, pl.resize((140, 100)).coords)
    c = t.clip_to_image(remove_empty=False)
    assert c.get_field("masks") is pl
    assert isinstance(t.to("cpu").get_field("masks"), PolygonList)
    kept = t.clip_to_image(remove_empty=True)
    assert len(kept.get_field("masks")) == len(kept)


def test_segmentation_mask_poly_mode_still_raises():
    with pytest.raises(NotImplementedError) as e:
        SegmentationMask([[[0, 0, 1, 1, 2, 2]]], (10, 10), mode="poly")
    assert "PolygonList" in str(e.value)
    with pytest.raises(NotImplementedError):
        SegmentationMask(torch.zeros(1, 10, 10, dtype=torch.uint8), (10, 10)).convert("poly")


def test_synthetic_poly_masks_are_opt_in():
    from abr_iod_amd.engine.synthetic import synthetic_batch
    im0, t0 = synthetic_batch(2, 96, 128, seed=3, device="cpu", max_boxes=3)
    im1, t1 = synthetic_batch(2, 96, 128, seed=3, device="cpu", max_boxes=3, masks="poly")
    im2, t2 = synthetic_batch(2, 96, 128, seed=3, device="cpu", max_boxes=3, masks="ellipse")
    assert torch.equal(im0, im1)
    for a, b, c in zip(t0, t1, t2):
        assert torch.equal(a.bbox, b.bbox) and torch.equal(a.get_field("labels"), b.get_field("labels")) and not a.has_field("masks")
        f = b.get_field("masks")
        assert isinstance(f, PolygonList) and len(f) == len(b) and f.size == (128, 96) and f.poly_offsets.tolist() == [24 * i for i in range(len(b) + 1)]
        poly, ell = f.convert("mask").masks.bool(), c.get_field("masks").masks.bool()
        # a 24-gon inscribed in the ellipse: inside it up to the rasteriser's half-pixel conventions, and at least 90 % of it
        assert (poly & ~ell).sum() <= 0.05 * ell.sum() and (poly & ell).sum() >= 0.9 * ell.sum()
    with pytest.raises(ValueError):
        synthetic_batch(1, 96, 128, device="cpu", masks="triangle")


# ------------------------------------------------------------------------------------------------------------ the dataset
def _write_json(path):
    from abr_iod_amd.structures import rle as R
    W, H = 60, 40
    sq = lambda x, y, s: [x, y, x + s, y, x + s, y + s, x, y + s]      # noqa: E731
    rle_mask = np.zeros((H, W), np.uint8)
    rle_mask[5:20, 7:33] = 1
    rle = R.encode_one(rle_mask)
    rle2_mask = np.zeros((H, W), np.uint8)
    rle2_mask[20:39, 1:9] = 1
    rle2 = R.encode_one(rle2_mask)
    images = [dict(id=i, width=W, height=H, file_name="%d.jpg" % i) for i in (1, 2, 3)]
    ann = lambda i, img, cat, bbox, seg: dict(id=i, image_id=img, category_id=cat, bbox=bbox, segmentation=seg, iscrowd=0, area=float(bbox[2] * bbox[3]))  # noqa: E731
    annotations = [
        ann(1, 1, 16, [4, 4, 20, 20], [sq(4.5, 4.5, 20)]),                                  # image 1: polygons only
        ann(2, 1, 17, [30, 10, 25, 25], [sq(30, 10, 10), [45.5, 20, 55, 21.5, 50, 34.75]]),
        ann(3, 2, 16, [7, 5, 26, 15], rle),                                                 # image 2: run-length only
        ann(4, 3, 18, [7, 5, 26, 15], rle),                                                 # image 3: mixed, in this order
        ann(5, 3, 16, [2, 2, 30, 30], [sq(2, 2, 30)]),
        ann(6, 3, 17, [1, 20, 8, 19], rle2),
        ann(7, 3, 20, [40, 3, 15, 15], [sq(40.25, 3.5, 15), sq(44, 7, 4)]),
    ]
    with open(path, "w") as f:
        json.dump(dict(images=images, annotations=annotations, categories=[]), f)
    return (W, H), rle_mask, rle2_mask, annotations


def test_dataset_gives_polygon_lists_rle_masks_and_mixed_masks(tmp_path):
    from abr_iod_amd.data.datasets.voc import CLASSES
    from abr_iod_amd.data.datasets.voc2012_instance import PascalVOCDataset2012
    (W, H), rle_mask, rle2_mask, annotations = _write_json(str(tmp_path / "inst.json"))
    ds = PascalVOCDataset2012(str(tmp_path), str(tmp_path / "inst.json"), new_classes=list(CLASSES[16:21]), old_classes=list(CLASSES[1:16]), device="cpu")
    assert len(ds) == 3
    # polygons only -> a PolygonList; packed -> PackedMasks equal to pack() of it
    t = ds.get_groundtruth(0)
    f = t.get_field("masks")
    assert isinstance(f, PolygonList) and len(f) == 2 == len(t) and f.size == (W, H) and [len(f.polygons_of(i)) for i in (0, 1)] == [1, 2]
    want = host_masks([a["segmentation"] for a in annotations[:2]], H, W)
    assert torch.equal(f.convert("mask").masks, want) and want[0].sum() == 400
    p = ds.get_groundtruth(0, packed=True).get_field("masks")
    assert isinstance(p, PackedMasks) and p.size == (W, H) and torch.equal(p.bits, f.pack().bits) and torch.equal(p.unpack(), want)
    # run-length only: exactly as before
    f = ds.get_groundtruth(1).get_field("masks")
    assert isinstance(f, SegmentationMask) and f.mode == "mask" and torch.equal(f.masks, torch.from_numpy(rle_mask)[None])
    p = ds.get_groundtruth(1, packed=True).get_field("masks")
    assert isinstance(p, PackedMasks) and torch.equal(p.unpack(), torch.from_numpy(rle_mask)[None])
    # mixed: one SegmentationMask in annotation order
    t = ds.get_groundtruth(2)
    f = t.get_field("masks")
    assert isinstance(f, SegmentationMask) and f.mode == "mask" and f.masks.dtype == torch.uint8 and tuple(f.masks.shape) == (4, H, W)
    polys = host_masks([annotations[4]["segmentation"], annotations[6]["segmentation"]], H, W)
    want = torch.stack([torch.from_numpy(rle_mask), polys[0], torch.from_numpy(rle2_mask), polys[1]])
    assert torch.equal(f.masks, want) and t.get_field("labels").tolist() == [18, 16, 17, 20]
    p = ds.get_groundtruth(2, packed=True).get_field("masks")
    assert isinstance(p, PackedMasks) and torch.equal(p.unpack(), want)

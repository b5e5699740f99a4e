"""GPU: the pixel kernels of csrc/imgproc.hip at their edges, bit for bit -- resize (1-pixel axes, one-pass calls through the C ABI, 2669-tap
filters, images that drive bicubic into both clips, guard bytes round `dst`), normalise into the batch (every flip x to_bgr255 x mean/std
combination, all 256 byte values, neighbouring slots untouched, +0.0 padding), blend / copy / fill (every byte pair, 1-pixel and empty
rectangles, every refusal), the four ColorJitter ops (the whole 2^24 colour cube through hue, means of exactly k + 0.5 and a luma sum past 2^32
through contrast) and one case past every launcher's grid cap of 16384 x 256 work items, where the grid-stride loops take a second trip.

References: oracle/abr_data_ref.py (pinned to Pillow by tests/test_oracle_data.py) and Pillow itself through `R.pil_resize`.  Everything is
integer or correctly rounded IEEE arithmetic, so every comparison is for equality.  Output buffers handed to the C ABI are stale: 0xA5 bytes
(uint8) or NaN (fp32), and every element must come back written.

The refusal cases only pass arguments that the launchers' own ABR_REQUIRE lines turn away before any launch."""
import functools
import random

import numpy as np
import pytest
import torch

from oracle import abr_data_ref as R

pytestmark = pytest.mark.gpu

STALE = 0xA5
GUARD = 64
FILTERS = [R.BILINEAR, R.BICUBIC]


def _G():
    from abr_iod_amd.data import gpu_transforms as G
    return G


def _abi():
    from abr_iod_amd._lib import lib, ptr, stream
    return lib(), ptr, stream


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _guarded(nbytes):
    """a stale uint8 buffer of `nbytes` with GUARD bytes on each side -> (whole buffer, pointer of the payload)"""
    buf = torch.full((GUARD + nbytes + GUARD,), STALE, dtype=torch.uint8, device="cuda")
    return buf, buf.data_ptr() + GUARD


def _guards_intact(buf):
    b = buf.cpu().numpy()
    return bool((b[:GUARD] == STALE).all() and (b[-GUARD:] == STALE).all())


def _payload(buf, shape):
    return buf.cpu().numpy()[GUARD:-GUARD].reshape(shape)


# ------------------------------------------------------------------------------------------------------------------------------ resize
def _images(H, W, seed):
    """random bytes; all 255; a 0 / 255 checkerboard (bicubic's over- and undershoot meet both clips)"""
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    board = np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    return [("random", rs.randint(0, 256, (H, W, 3), dtype=np.uint8)), ("white", np.full((H, W, 3), 255, np.uint8)),
            ("board", np.ascontiguousarray(board))]


def _abi_resize(img, ow, oh, name):
    """abr_img_resample_u8 into a stale guarded buffer; a direction that does not change gets NULL tables, and a single pass gets tmp = NULL"""
    G = _G()
    L, ptr, stream = _abi()
    H, W, _ = img.shape
    src = _dev(img)
    nil = (None, None, 0)
    bh, kh, nh = G._dev_table(W, ow, name, src.device) if ow != W else nil
    bv, kv, nv = G._dev_table(H, oh, name, src.device) if oh != H else nil
    tmp = torch.full((H, ow, 3), STALE, dtype=torch.uint8, device="cuda") if (ow != W and oh != H) else None
    buf, dst = _guarded(oh * ow * 3)
    rc = L.abr_img_resample_u8(ptr(src), H, W, dst, oh, ow, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), stream())
    assert rc == 0, L.abr_last_error()
    assert _guards_intact(buf), (H, W, ow, oh, name)
    assert np.array_equal(src.cpu().numpy(), img)                 # the source is read only
    return _payload(buf, (oh, ow, 3))


RESIZE_SHAPES = [(1, 1, 5, 7), (1, 9, 4, 1), (5, 1, 1, 5), (2000, 3, 3, 3), (3, 2000, 2, 3), (7, 5, 800, 600), (64, 64, 64, 1)]


@pytest.mark.parametrize("name", FILTERS)
@pytest.mark.parametrize("shape", RESIZE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_resize_edge_shapes_vs_pillow_and_restatement(shape, name):
    """1-pixel sources and outputs, 2669-tap rows (2000 -> 3), big enlargements; three images each; the wrapper and the C ABI with guards"""
    G = _G()
    H, W, ow, oh = shape
    for kind, img in _images(H, W, seed=H * 131 + W):
        pil = R.pil_resize(img, ow, oh, name)
        ref = R.resample_u8(img, ow, oh, name)
        assert np.array_equal(pil, ref), ("Pillow and its restatement differ: a Pillow-version matter, not the kernel's", kind)
        got = G.resize(_dev(img), ow, oh, name).cpu().numpy()
        assert got.shape == (oh, ow, 3) and got.dtype == np.uint8
        assert np.array_equal(got, ref), (kind, int((got != ref).sum()))
        got = _abi_resize(img, ow, oh, name)
        assert np.array_equal(got, ref), (kind, int((got != ref).sum()))


@pytest.mark.parametrize("name", FILTERS)
def test_resize_one_pass_and_identity_through_the_abi(name):
    """width only and height only: tmp = NULL and the other direction's tables NULL; the identity size is a copy; guards stay"""
    for (H, W, ow, oh) in [(9, 31, 13, 9), (9, 31, 70, 9), (31, 9, 9, 13), (31, 9, 9, 70), (1, 40, 7, 1), (40, 1, 1, 7), (9, 31, 31, 9), (1, 1, 1, 1)]:
        for kind, img in _images(H, W, seed=W * 7 + ow):
            got = _abi_resize(img, ow, oh, name)
            assert np.array_equal(got, R.pil_resize(img, ow, oh, name)), (H, W, ow, oh, kind)
            assert np.array_equal(got, R.resample_u8(img, ow, oh, name)), (H, W, ow, oh, kind)


def test_resize_refusals_launch_nothing():
    """missing tables of a direction that changes, and two passes without the intermediate: refused, `dst` untouched"""
    G = _G()
    L, ptr, stream = _abi()
    img = _images(6, 8, 1)[0][1]
    src = _dev(img)
    bh, kh, nh = G._dev_table(8, 5, R.BILINEAR, src.device)
    bv, kv, nv = G._dev_table(6, 4, R.BILINEAR, src.device)
    tmp = torch.full((6, 5, 3), STALE, dtype=torch.uint8, device="cuda")
    buf, dst = _guarded(4 * 5 * 3)
    st = stream()
    calls = [
        (ptr(src), 6, 8, dst, 4, 5, None, ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), None, nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), ptr(kh), 0, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, None, ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), None, nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), 0, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, None, st),
        (ptr(src), 0, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, dst, 4, 0, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (None, 6, 8, dst, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
        (ptr(src), 6, 8, None, 4, 5, ptr(bh), ptr(kh), nh, ptr(bv), ptr(kv), nv, ptr(tmp), st),
    ]
    for i, args in enumerate(calls):
        assert L.abr_img_resample_u8(*args) != 0, i
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == STALE).all() and (tmp.cpu().numpy() == STALE).all()


@pytest.mark.parametrize("name", FILTERS)
def test_resize_past_the_grid_cap(name):
    """2100 x 1400 -> 2049 x 2048: 2100 * 2048 items in the horizontal pass and 2049 * 2048 in the vertical one, both above 16384 * 256"""
    G = _G()
    H, W, ow, oh = 2100, 1400, 2048, 2049
    assert H * ow > 16384 * 256 and oh * ow > 16384 * 256
    img = np.random.RandomState(11).randint(0, 256, (H, W, 3), dtype=np.uint8)
    got = G.resize(_dev(img), ow, oh, name).cpu().numpy()
    ref = R.pil_resize(img, ow, oh, name)
    assert got.shape == ref.shape and np.array_equal(got, ref), int((got != ref).sum())


# --------------------------------------------------------------------------------------------------------------------------- normalise
NORMS = [([102.9801, 115.9465, 122.7717], [1.0, 1.0, 1.0]),
         ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225]),
         ([0.0, 0.0, 0.0], [57.375, 57.12, 58.395])]
NORM_SHAPES = [(1, 1, 1, 1), (1, 1, 3, 5), (5, 1, 5, 1), (7, 13, 7, 13), (7, 13, 32, 32), (33, 65, 64, 96)]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _normalize_case(img, HP, WP, mean, std, bgr, flip):
    """the middle slot of a NaN-filled [3,3,HP,WP] batch: the reference inside [h,w], +0.0 outside, the neighbours still all NaN"""
    G = _G()
    h, w, _ = img.shape
    batch = torch.full((3, 3, HP, WP), float("nan"), dtype=torch.float32, device="cuda")
    src = _dev(img)
    G.normalize_into(src, batch[1], mean, std, to_bgr255=bgr, flip=flip)
    assert bool(batch[0].isnan().all()) and bool(batch[2].isnan().all()), "a neighbouring slot was written"
    got = batch[1].cpu().numpy()
    ref = R.to_tensor_normalize(img, mean, std, bgr, flip)
    assert ref.shape == (3, h, w) and ref.dtype == np.float32
    inside = _bits(got[:, :h, :w])
    assert np.array_equal(inside, _bits(ref)), (h, w, HP, WP, int((inside != _bits(ref)).sum()))
    pad = _bits(got).copy()
    pad[:, :h, :w] = 0
    assert not pad.any(), "the padding is not +0.0 everywhere"
    assert np.array_equal(src.cpu().numpy(), img)


def _permutation_image():
    """16 x 16, each channel another permutation of 0..255: every byte value through every channel"""
    rs = np.random.RandomState(21)
    img = np.stack([np.arange(256), rs.permutation(256), rs.permutation(256)[::-1]], -1).astype(np.uint8).reshape(16, 16, 3)
    assert all(sorted(img[..., c].ravel().tolist()) == list(range(256)) for c in range(3))
    assert not np.array_equal(img[..., 0], img[..., 1]) and not np.array_equal(img[..., 1], img[..., 2]) and not np.array_equal(img[..., 0], img[..., 2])
    return np.ascontiguousarray(img)


@pytest.mark.parametrize("norm", range(3))
@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("flip", [False, True])
def test_normalize_into_batch_every_combination(flip, bgr, norm):
    mean, std = NORMS[norm]
    rs = np.random.RandomState(31 + norm)
    for (h, w, HP, WP) in NORM_SHAPES:
        _normalize_case(rs.randint(0, 256, (h, w, 3), dtype=np.uint8), HP, WP, mean, std, bgr, flip)
    perm = _permutation_image()
    _normalize_case(perm, 16, 16, mean, std, bgr, flip)
    _normalize_case(perm, 17, 19, mean, std, bgr, flip)


@pytest.mark.parametrize("flip,bgr,norm", [(True, False, 1), (False, True, 2)])
def test_normalize_past_the_grid_cap(flip, bgr, norm):
    """2049 x 2048 plane positions: above 16384 * 256"""
    assert 2049 * 2048 > 16384 * 256
    img = np.random.RandomState(41).randint(0, 256, (2048, 2047, 3), dtype=np.uint8)
    _normalize_case(img, 2049, 2048, NORMS[norm][0], NORMS[norm][1], bgr, flip)


# -------------------------------------------------------------------------------------------------------------------- blend, copy, fill
LAMS = [0.0, 1.0, 0.5, 1.0 / 3.0, 0.1, float(np.float32(0.2871)), float(np.nextafter(1.0, 0.0))]
_draws = random.Random(2050)
LAMS += [_draws.betavariate(2.0, 5.0) for _ in range(16)]            # the draw of voc_abr.py's mixup, seeded


@pytest.mark.parametrize("lam", LAMS, ids=lambda v: repr(v))
def test_blend_every_byte_pair(lam):
    """image byte = row index, crop byte = column index: all 65536 (image byte, crop byte) pairs in every channel"""
    G = _G()
    img = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None], (256, 256, 3)))
    crop = np.ascontiguousarray(np.broadcast_to(np.arange(256, dtype=np.uint8)[None, :, None], (256, 256, 3)))
    want = R.blend_paste(img.copy(), crop, 0, 0, 256, 256, 0, 0, lam)
    cd = _dev(crop)
    got = G.blend_paste_(_dev(img), cd, 0, 0, 256, 256, 0, 0, lam).cpu().numpy()
    assert np.array_equal(got, want), (lam, int((got != want).sum()))
    assert np.array_equal(cd.cpu().numpy(), crop)


IH, IW = 37, 53          # the image of the geometry cases
BIG, SMALL = (41, 59), (11, 13)      # a crop larger than the image, and one smaller
# (crop, x0, y0, rw, rh, off_x, off_y)
GEOMETRY = [
    ("small", 0, 0, 1, 1, 0, 0), ("small", IW - 1, 0, 1, 1, 12, 0), ("small", 0, IH - 1, 1, 1, 0, 10), ("small", IW - 1, IH - 1, 1, 1, 12, 10),
    ("big", 0, 0, IW, IH, 3, 2),                       # the whole image
    ("big", 0, 0, IW, IH, 59 - IW, 41 - IH),           # the whole image from the crop's far corner
    ("small", 5, 7, 13, 11, 0, 0),                     # the whole crop
    ("small", IW - 10, IH - 9, 10, 9, 3, 2),           # touches the right and bottom edges of image and crop
    ("small", IW - 13, 0, 13, 1, 0, 10),               # one row along the right edge
    ("small", 0, IH - 11, 1, 11, 12, 0),               # one column along the bottom edge
    ("small", 5, 5, 0, 4, 1, 1), ("small", 5, 5, 4, 0, 1, 1), ("small", 5, 5, 0, 0, 1, 1),      # empty: success, nothing written
    ("small", IW, IH, 0, 0, 13, 11),
]


def _geometry_inputs():
    rs = np.random.RandomState(51)
    img = rs.randint(0, 256, (IH, IW, 3), dtype=np.uint8)
    crops = {"big": rs.randint(0, 256, BIG + (3,), dtype=np.uint8), "small": rs.randint(0, 256, SMALL + (3,), dtype=np.uint8)}
    return img, crops


def test_blend_rectangles_write_nothing_outside():
    G = _G()
    img, crops = _geometry_inputs()
    for lam in (float(np.float32(0.2871)), 1.0 / 3.0, 0.0):
        for (ck, x0, y0, rw, rh, ox, oy) in GEOMETRY:
            crop = crops[ck]
            want = R.blend_paste(img.copy(), crop, x0, y0, x0 + rw, y0 + rh, ox, oy, lam) if rw and rh else img
            got = G.blend_paste_(_dev(img), _dev(crop), x0, y0, x0 + rw, y0 + rh, ox, oy, lam).cpu().numpy()
            assert np.array_equal(got, want), (lam, ck, x0, y0, rw, rh, ox, oy)


def test_copy_rectangles_write_nothing_outside():
    G = _G()
    img, crops = _geometry_inputs()
    for (ck, x0, y0, rw, rh, ox, oy) in GEOMETRY:
        crop = crops[ck]
        want = img.copy()
        want[y0:y0 + rh, x0:x0 + rw] = crop[oy:oy + rh, ox:ox + rw]
        cd = _dev(crop)
        got = G.copy_rect_(_dev(img), cd, x0, y0, ox, oy, rw, rh).cpu().numpy()
        assert np.array_equal(got, want), (ck, x0, y0, rw, rh, ox, oy)
        assert np.array_equal(cd.cpu().numpy(), crop)


# one bound broken by one pixel each, image 37 x 53, crop 11 x 13: (x0, y0, rw, rh, off_x, off_y)
REFUSED_RECTS = [
    (-1, 4, 5, 4, 2, 2),               # x0 >= 0
    (6, -1, 5, 4, 2, 2),               # y0 >= 0
    (IW - 4, 4, 5, 4, 2, 2),           # x0 + rw <= W
    (6, IH - 3, 5, 4, 2, 2),           # y0 + rh <= H
    (6, 4, 5, 4, -1, 2),               # off_x >= 0
    (6, 4, 5, 4, 2, -1),               # off_y >= 0
    (6, 4, 5, 4, 13 - 4, 2),           # off_x + rw <= CW
    (6, 4, 5, 4, 2, 11 - 3),           # off_y + rh <= CH
    (6, 4, -1, 4, 2, 2),               # rw >= 0
    (6, 4, 5, -1, 2, 2),               # rh >= 0
    (6, 4, -1, -1, 2, 2),
]


@pytest.mark.parametrize("rect", REFUSED_RECTS, ids=lambda r: "_".join(map(str, r)))
def test_blend_and_copy_refuse_rectangles_outside(rect):
    """each bound of abr_img_blend_paste_u8 and abr_img_copy_rect_u8 missed by one pixel: RuntimeError before any launch, the image as it was"""
    G = _G()
    img, crops = _geometry_inputs()
    crop = crops["small"]
    x0, y0, rw, rh, ox, oy = rect
    d, cd = _dev(img), _dev(crop)
    with pytest.raises(RuntimeError):
        G.blend_paste_(d, cd, x0, y0, x0 + rw, y0 + rh, ox, oy, 0.5)
    with pytest.raises(RuntimeError):
        G.copy_rect_(d, cd, x0, y0, ox, oy, rw, rh)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), img) and np.array_equal(cd.cpu().numpy(), crop)
    # the same rectangle moved back inside by that pixel is accepted
    G.copy_rect_(d, cd, 6, 4, 2, 2, 5, 4)
    want = img.copy()
    want[4:8, 6:11] = crop[2:6, 2:7]
    assert np.array_equal(d.cpu().numpy(), want)


@pytest.mark.parametrize("value", [0, 114, 255])
def test_fill_lengths_round_one_block(value):
    L, ptr, stream = _abi()
    for n in (0, 1, 255, 256, 257):
        buf, dst = _guarded(n)
        assert L.abr_img_fill_u8(dst, n, value, stream()) == 0
        b = buf.cpu().numpy()
        assert (b[GUARD:GUARD + n] == value).all() and (b[:GUARD] == STALE).all() and (b[GUARD + n:] == STALE).all(), n


def test_fill_refuses_values_that_are_no_byte():
    G = _G()
    L, ptr, stream = _abi()
    buf, dst = _guarded(256)
    for value in (256, -1):
        assert L.abr_img_fill_u8(dst, 256, value, stream()) != 0
        with pytest.raises(RuntimeError):
            G.full_canvas(4, 4, value, "cuda")
    assert L.abr_img_fill_u8(dst, -1, 7, stream()) != 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == STALE).all()


def test_fill_past_the_grid_cap():
    """a 1399 x 1000 mosaic canvas is 4,197,000 bytes: 2,696 more than 16384 * 256"""
    G = _G()
    L, ptr, stream = _abi()
    n = 1399 * 1000 * 3
    assert n > 16384 * 256
    buf, dst = _guarded(n)
    assert L.abr_img_fill_u8(dst, n, 114, stream()) == 0
    inner = buf[GUARD:GUARD + n]
    assert int((inner != 114).sum()) == 0, int((inner != 114).sum())
    assert _guards_intact(buf)
    del inner
    buf.fill_(STALE)
    del buf                                                    # (the allocator hands the stale block to the canvas below, as a rule)
    canvas = G.full_canvas(1399, 1000, 114, "cuda")
    assert tuple(canvas.shape) == (1399, 1000, 3) and canvas.dtype == torch.uint8
    assert int((canvas != 114).sum()) == 0


def test_blend_and_copy_past_the_grid_cap():
    """a 2048 x 2049 rectangle (4,196,352 pixels) inside a 2050 x 2060 image"""
    G = _G()
    H, W, rw, rh, x0, y0, ox, oy = 2050, 2060, 2048, 2049, 7, 1, 1, 0
    assert rw * rh > 16384 * 256
    rs = np.random.RandomState(61)
    img = rs.randint(0, 256, (H, W, 3), dtype=np.uint8)
    crop = rs.randint(0, 256, (2049, 2050, 3), dtype=np.uint8)
    cd = _dev(crop)
    lam = float(np.float32(0.2871))
    want = R.blend_paste(img.copy(), crop, x0, y0, x0 + rw, y0 + rh, ox, oy, lam)
    got = G.blend_paste_(_dev(img), cd, x0, y0, x0 + rw, y0 + rh, ox, oy, lam).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    want = img.copy()
    want[y0:y0 + rh, x0:x0 + rw] = crop[oy:oy + rh, ox:ox + rw]
    got = G.copy_rect_(_dev(img), cd, x0, y0, ox, oy, rw, rh).cpu().numpy()
    assert np.array_equal(got, want), int((got != want).sum())


# -------------------------------------------------------------------------------------------------------------------------- ColorJitter
def _slab(s):
    """colours (r, g, b) with r in [32 s, 32 s + 32), every g and b: [8192, 256, 3]; the eight slabs are the whole 2^24 cube"""
    r = np.arange(32 * s, 32 * s + 32, dtype=np.uint8)
    v = np.arange(256, dtype=np.uint8)
    return np.ascontiguousarray(np.stack(np.meshgrid(r, v, v, indexing="ij"), -1).reshape(8192, 256, 3))


HUE_EXTRA = [0.004, 0.17, -0.23, 0.31, -0.4]
HUE_FACTORS = {s: (0.0, 0.5, -0.5, HUE_EXTRA[(2 * s) % 5], HUE_EXTRA[(2 * s + 1) % 5]) for s in range(8)}


def test_hue_factors_cover_the_list():
    assert {f for s in range(8) for f in HUE_FACTORS[s][3:]} == set(HUE_EXTRA)
    assert all(HUE_FACTORS[s][3] != HUE_FACTORS[s][4] for s in range(8))


@pytest.mark.parametrize("s", range(8))
def test_hue_whole_colour_cube(s):
    """every colour through RGB -> HSV -> shift -> RGB: the float quotients, the fmod and the round() of the device build against the host's"""
    G = _G()
    cube = _slab(s)
    dev = _dev(cube)
    for f in HUE_FACTORS[s]:
        got = G.color_jitter_(dev.clone(), "hue", f).cpu().numpy()
        want = R.adjust_hue(cube, f)
        assert np.array_equal(got, want), (s, f, int((got != want).any(-1).sum()))


BLEND_FACTORS = (0.0, 0.3, 1.0, 1.6, 3.0, 255.0)


@pytest.mark.parametrize("s", [0, 7])
@pytest.mark.parametrize("op", ["saturation", "brightness"])
def test_saturation_and_brightness_on_cube_slabs(op, s):
    G = _G()
    fn = {"saturation": R.adjust_saturation, "brightness": R.adjust_brightness}[op]
    cube = _slab(s)
    dev = _dev(cube)
    for f in BLEND_FACTORS:
        got = G.color_jitter_(dev.clone(), op, f).cpu().numpy()
        want = fn(cube, f)
        assert np.array_equal(got, want), (op, s, f, int((got != want).any(-1).sum()))


def _gray(*lumas):
    """a 1 x n image of gray pixels: L of (v, v, v) is v"""
    img = np.repeat(np.array(lumas, np.uint8)[None, :, None], 3, axis=2)
    assert R.rgb_to_l(img).ravel().tolist() == list(lumas)
    return np.ascontiguousarray(img)


def _contrast(img, f):
    return _G().color_jitter_(_dev(img), "contrast", f).cpu().numpy()


def test_contrast_mean_of_exactly_one_half_and_one_pixel():
    two, three = _gray(10, 11), _gray(10, 10, 11)
    assert (R.adjust_contrast(two, 0.0) == 11).all()          # mean 10.5 -> int(10.5 + 0.5) = 11
    assert (R.adjust_contrast(three, 0.0) == 10).all()        # mean 10.33 -> 10
    one = np.array([[[200, 17, 93]]], np.uint8)
    cases = [two, three, one, _gray(0), _gray(255), _gray(254, 255), _gray(0, 1), _gray(0, 0, 0, 1), _gray(3, 4, 4, 4)]
    for img in cases:
        for f in (0.0, 0.45, 1.0, 1.6):
            want = R.adjust_contrast(img, f)
            got = _contrast(img, f)
            assert np.array_equal(got, want), (img[..., 0].tolist(), f, got.tolist(), want.tolist())


def test_contrast_scratch_is_zeroed_between_calls():
    """two calls in a row on images of different sizes give what each call gives alone"""
    rs = np.random.RandomState(71)
    big = rs.randint(128, 256, (97, 131, 3), dtype=np.uint8)
    small = rs.randint(0, 64, (3, 5, 3), dtype=np.uint8)
    wb, ws = R.adjust_contrast(big, 0.45), R.adjust_contrast(small, 0.45)
    for first, second, w1, w2 in ((big, small, wb, ws), (small, big, ws, wb), (small, small, ws, ws)):
        g1 = _contrast(first, 0.45)
        g2 = _contrast(second, 0.45)
        assert np.array_equal(g1, w1) and np.array_equal(g2, w2)


@functools.lru_cache(maxsize=1)
def _bright_image():
    """4200 x 4100, 255 everywhere except a band of 100 random rows: the luma sum (about 4.39e9) is above 2^32"""
    img = np.full((4200, 4100, 3), 255, np.uint8)
    img[2000:2100] = np.random.RandomState(81).randint(0, 256, (100, 4100, 3), dtype=np.uint8)
    total = int(R.rgb_to_l(img[2000:2100]).astype(np.int64).sum()) + 255 * 4100 * 4100
    mean = int(total / (4200 * 4100) + 0.5)
    assert total > 2 ** 32 and mean > 250 and int((total % 2 ** 32) / (4200 * 4100) + 0.5) < 10
    return img, mean


@pytest.mark.parametrize("f", [0.0, 0.45])
def test_contrast_luma_sum_past_32_bits(f):
    img, mean = _bright_image()
    want = R.adjust_contrast(img, f)
    assert int(want[0, 0, 0]) == int(np.float32(mean) + np.float32(f) * (np.float32(255) - np.float32(mean)))     # (the reference did not truncate)
    got = _contrast(img, f)
    assert np.array_equal(got, want), (f, mean, int(got[0, 0, 0]), int(want[0, 0, 0]))


@pytest.mark.parametrize("op,f", [("brightness", 1.37), ("contrast", 0.45), ("saturation", 1.6), ("hue", 0.17)])
def test_color_jitter_past_the_grid_cap(op, f):
    """2049 x 2048 pixels: above 16384 * 256"""
    G = _G()
    assert 2049 * 2048 > 16384 * 256
    fn = {"brightness": R.adjust_brightness, "contrast": R.adjust_contrast, "saturation": R.adjust_saturation, "hue": R.adjust_hue}[op]
    img = np.random.RandomState(91).randint(0, 256, (2049, 2048, 3), dtype=np.uint8)
    got = G.color_jitter_(_dev(img), op, f).cpu().numpy()
    want = fn(img, f)
    assert np.array_equal(got, want), (op, int((got != want).any(-1).sum()))


def test_color_jitter_empty_images_and_wrapper_refusals():
    G = _G()
    L, ptr, stream = _abi()
    buf = torch.full((4, 5, 3), STALE, dtype=torch.uint8, device="cuda")
    scratch = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    for op, f in ((0, 1.3), (1, 0.4), (2, 1.6), (3, 0.2)):
        for (H, W) in ((0, 5), (4, 0), (0, 0)):
            assert L.abr_img_color_jitter_u8(ptr(buf), H, W, op, f, ptr(scratch), stream()) == 0
            assert L.abr_img_color_jitter_u8(None, H, W, op, f, None, stream()) == 0
    torch.cuda.synchronize()
    assert (buf.cpu().numpy() == STALE).all() and int(scratch.item()) == 0x5A5A5A5A
    img = torch.zeros((6, 8, 3), dtype=torch.uint8, device="cuda")
    for bad in (img[:, ::2], img.permute(1, 0, 2), img.float(), img.to(torch.int8), img[..., :2], img[0]):
        with pytest.raises(ValueError):
            G.color_jitter_(bad, "brightness", 1.2)
    assert int(img.sum()) == 0


def test_color_jitter_refusals_launch_nothing():
    """op 4 and -1, a negative or NaN enhancement factor, a hue factor just outside [-0.5, 0.5] or NaN, contrast without its scratch"""
    G = _G()
    L, ptr, stream = _abi()
    img = np.random.RandomState(95).randint(0, 256, (6, 8, 3), dtype=np.uint8)
    d = _dev(img)
    scratch = torch.full((1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda")
    nan = float("nan")
    calls = [(4, 1.0), (-1, 1.0), (0, -0.1), (1, -0.1), (2, -0.1), (0, -1e-300), (0, nan), (1, nan), (2, nan), (3, nan),
             (3, 0.5000001), (3, -0.5000001), (-1, nan), (4, 0.2)]
    for op, f in calls:
        assert L.abr_img_color_jitter_u8(ptr(d), 6, 8, op, f, ptr(scratch), stream()) != 0, (op, f)
    assert L.abr_img_color_jitter_u8(ptr(d), 6, 8, 1, 0.5, None, stream()) != 0
    assert L.abr_img_color_jitter_u8(None, 6, 8, 0, 0.5, ptr(scratch), stream()) != 0
    assert L.abr_img_color_jitter_u8(ptr(d), -1, 8, 0, 0.5, ptr(scratch), stream()) != 0
    assert L.abr_img_color_jitter_u8(ptr(d), 6, -1, 0, 0.5, ptr(scratch), stream()) != 0
    for op, f in (("hue", 0.5000001), ("hue", -0.5000001), ("hue", nan), ("brightness", -0.1), ("contrast", nan), ("saturation", -1.0)):
        with pytest.raises(RuntimeError):
            G.color_jitter_(d, op, f)
    torch.cuda.synchronize()
    assert np.array_equal(d.cpu().numpy(), img) and int(scratch.item()) == 0x5A5A5A5A
    # the edge of the hue range itself is accepted
    for f in (0.5, -0.5):
        assert np.array_equal(G.color_jitter_(_dev(img), "hue", f).cpu().numpy(), R.adjust_hue(img, f))

"""CPU: the host run-length codec (abr_iod_amd/structures/rle.py) against the format's known answers, its round trips and its errors, and
SegmentationMask / PackedMasks built from RLE dicts on the CPU.  All comparisons are exact: the format is integers and bytes."""
import numpy as np
import pytest
import torch

from abr_iod_amd.structures import rle as R
from abr_iod_amd.structures.segmentation_mask import FLIP_LEFT_RIGHT, FLIP_TOP_BOTTOM, PackedMasks, SegmentationMask


def _box_mask():
    m = np.zeros((4, 5), np.uint8)      # 4x5 (h x w), rows 1-2, columns 1-3 set
    m[1:3, 1:4] = 1
    return m


def test_known_answers_both_directions():
    assert R.mask_counts(_box_mask()) == [5, 2, 2, 2, 2, 2, 5]
    assert R.encode_one(_box_mask()) == {"size": [4, 5], "counts": "5220003"}
    assert np.array_equal(R.decode_one({"size": [4, 5], "counts": "5220003"}), _box_mask())
    assert R.string_to_counts("5220003") == [5, 2, 2, 2, 2, 2, 5]
    ones = np.ones((3, 2), np.uint8)
    assert R.mask_counts(ones) == [0, 6]
    assert R.encode_one(ones) == {"size": [3, 2], "counts": "06"}
    assert np.array_equal(R.decode_one({"size": [3, 2], "counts": "06"}), ones)
    # the varint alone: single stored values
    assert R.counts_to_string([1000]) == "Xo0" and R.string_to_counts("Xo0") == [1000]
    assert R.counts_to_string([-2]) == "N" and R.string_to_counts("N") == [-2]


def test_counts_forms_accepted():
    want = _box_mask()
    for counts in ("5220003", b"5220003", [5, 2, 2, 2, 2, 2, 5]):
        assert np.array_equal(R.decode_one({"size": [4, 5], "counts": counts}), want), counts
    got = R.decode([{"size": [4, 5], "counts": "5220003"}, {"size": [4, 5], "counts": [20]}, {"size": [4, 5], "counts": b"0d0"}])
    assert got.shape == (3, 4, 5) and got.dtype == np.uint8
    assert np.array_equal(got[0], want) and not got[1].any() and got[2].all()
    assert R.decode([], (4, 5)).shape == (0, 4, 5)


def _cases():
    rng = np.random.default_rng(7)
    out = {"zeros": np.zeros((5, 9), np.uint8), "ones": np.ones((5, 9), np.uint8)}
    single = np.zeros((6, 7), np.uint8)
    single[4, 2] = 1
    out["single"] = single
    first = np.zeros((6, 7), np.uint8)
    first[0, 0] = 1
    out["first-pixel"] = first
    last = np.zeros((6, 7), np.uint8)
    last[5, 6] = 1
    out["last-pixel"] = last
    for h, w in [(1, 17), (23, 1), (1, 1), (9, 63), (9, 64), (9, 65), (5, 127), (5, 128), (5, 129), (40, 70)]:
        for dens in (0.1, 0.5, 0.9):
            out["rand-{}x{}-{}".format(h, w, dens)] = (rng.random((h, w)) < dens).astype(np.uint8)
    blob = np.zeros((300, 200), np.uint8)          # long runs: multi-character values and deltas of both signs
    yy, xx = np.mgrid[:300, :200]
    blob[((yy - 140) / 120.0) ** 2 + ((xx - 90) / 70.0) ** 2 < 1] = 1
    out["blob"] = blob
    return out


@pytest.mark.parametrize("name", sorted(_cases()))
def test_round_trip(name):
    m = _cases()[name]
    rle = R.encode_one(m)
    assert rle["size"] == list(m.shape) and isinstance(rle["counts"], str)
    assert all(48 <= ord(ch) <= 111 for ch in rle["counts"])
    counts = R.string_to_counts(rle["counts"])
    assert counts == R.mask_counts(m) and sum(counts) == m.size and all(c > 0 for c in counts[1:])
    assert np.array_equal(R.decode_one(rle), m)
    assert np.array_equal(R.decode_one({"size": rle["size"], "counts": counts}), m)
    assert R.counts_to_string(counts) == rle["counts"]


def test_blob_has_long_tokens_and_negative_deltas():
    s = R.encode_one(_cases()["blob"])["counts"]
    vals = [ord(c) - 48 for c in s]
    assert any(v & 0x20 for v in vals), "no multi-character value"
    assert any((not v & 0x20) and (v & 0x10) for v in vals), "no negative stored value"


def test_malformed_annotations_name_the_instance():
    good = {"size": [4, 5], "counts": "5220003"}
    with pytest.raises(R.RLEError, match="instance 1.*sum to 19"):
        R.decode([good, {"size": [4, 5], "counts": [5, 2, 2, 2, 2, 2, 4]}])
    with pytest.raises(R.RLEError, match="instance 2.*sum to 21"):
        R.decode([good, good, {"size": [4, 5], "counts": "5220004"}])
    with pytest.raises(R.RLEError, match="instance 1.*size"):
        R.decode([good, {"size": [5, 4], "counts": "5220003"}], (4, 5))
    with pytest.raises(R.RLEError, match="instance 0.*cut short"):
        R.decode([{"size": [4, 5], "counts": "522000X"}])
    with pytest.raises(R.RLEError, match="instance 0.*outside"):
        R.decode([{"size": [4, 5], "counts": "52 0003"}])
    assert issubclass(R.RLEError, ValueError)


def test_ops_rle_decode_on_the_cpu_is_the_host_codec():
    from abr_iod_amd import ops
    masks = np.stack([_cases()["rand-9x65-0.5"], _cases()["rand-9x65-0.1"]])
    rles = R.encode(masks)
    got = ops.rle_decode(rles, (9, 65), "cpu")
    assert got.dtype == torch.uint8 and np.array_equal(got.numpy(), masks)
    bits = ops.rle_decode(rles, (9, 65), "cpu", packed=True)
    assert bits.dtype == torch.int64 and tuple(bits.shape) == (2, 9, 2)
    assert np.array_equal(PackedMasks(bits, (65, 9)).unpack().numpy(), masks)


def test_segmentation_mask_from_rle_dicts_on_the_cpu():
    """the construction the reference's dataset performs (SegmentationMask(list of RLE dicts, size, mode='mask')); before the codec
    existed it ended in a TypeError from torch.stack"""
    rng = np.random.default_rng(3)
    masks = (rng.random((3, 37, 70)) < 0.4).astype(np.uint8)
    rles = R.encode(masks)
    rles[1] = {"size": rles[1]["size"], "counts": rles[1]["counts"].encode("ascii")}
    rles[2] = {"size": rles[2]["size"], "counts": R.string_to_counts(rles[2]["counts"])}
    a = SegmentationMask(rles, (70, 37), mode="mask")
    b = SegmentationMask(torch.from_numpy(masks), (70, 37), mode="mask")
    assert len(a) == 3 and a.size == (70, 37) and a.masks.dtype == torch.uint8 and a.masks.device.type == "cpu"
    assert torch.equal(a.masks, b.masks)
    for f in (lambda s: s.crop([5.2, 3.7, 50.5, 30.1]), lambda s: s.resize((101, 55)), lambda s: s.transpose(FLIP_LEFT_RIGHT),
              lambda s: s.transpose(FLIP_TOP_BOTTOM), lambda s: s[[2, 0]]):
        x, y = f(a), f(b)
        assert x.size == y.size and torch.equal(x.masks, y.masks)
    with pytest.raises(AssertionError):           # the reference's size check: (size[1], size[0]) == tuple(inst["size"])
        SegmentationMask(rles, (37, 70), mode="mask")
    with pytest.raises(NotImplementedError):
        SegmentationMask(rles, (70, 37), mode="poly")
    p = PackedMasks.from_rle(rles, (70, 37))
    assert torch.equal(p.unpack(), b.masks) and len(PackedMasks.from_rle([], (70, 37))) == 0

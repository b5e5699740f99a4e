"""COCO run-length masks on the host: a numpy / Python restatement of the format, used when the device is the CPU and as the
reference the device codec (csrc/rle.hip, ops.rle_decode / ops.rle_encode) is tested against.  pycocotools cannot be installed where this
project is built, so compatibility with its mask_utils.decode / encode rests on this restatement of the format and on its known answers,
not on a comparison with pycocotools itself.

An RLE is {"size": [h, w], "counts": C}.  Pixels are visited in column-major order p = x * h + y; the counts are the lengths of alternating
runs, the first of zeros (0 when pixel (0, 0) is set), and sum to h * w.  C is a list of ints, or the compressed str / bytes: the i-th
stored value is counts[i] - counts[i-2] for i > 2 and counts[i] otherwise, written 5 bits per character, low bits first; bit 0x20 says
another character follows, bit 0x10 of the last character is the sign; a character is its 6-bit value + 48."""
import numpy as np


class RLEError(ValueError):
    """a malformed run-length annotation; the message names the instance"""


def _where(instance):
    return "RLE instance {}".format(instance) if instance is not None else "RLE"


def counts_to_string(counts):
    """list of run lengths -> the compressed str"""
    out = []
    for i, c in enumerate(counts):
        x = int(c) - (int(counts[i - 2]) if i > 2 else 0)
        more = True
        while more:
            ch = x & 0x1f
            x >>= 5                                       # (Python's >> is arithmetic)
            more = (x != -1) if (ch & 0x10) else (x != 0)
            if more:
                ch |= 0x20
            out.append(chr(ch + 48))
    return "".join(out)


def string_to_counts(s, instance=None):
    """compressed str / bytes -> list of run lengths"""
    data = s.encode("ascii") if isinstance(s, str) else bytes(s)
    counts = []
    p, n = 0, len(data)
    while p < n:
        x, k, more = 0, 0, True
        while more:
            if p >= n:
                raise RLEError("{}: the last value of the counts string is cut short".format(_where(instance)))
            c = data[p] - 48
            if c < 0 or c > 63:
                raise RLEError("{}: character {!r} of the counts string is outside [48, 111]".format(_where(instance), chr(data[p])))
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_counts(rle, size=None, instance=None):
    """the run lengths of one RLE dict, checked: "size" equals size = (h, w) when given, no negative count, the counts sum to h * w"""
    if not isinstance(rle, dict) or "counts" not in rle or "size" not in rle:
        raise RLEError("{}: expected a dict with 'size' and 'counts', got {!r}".format(_where(instance), type(rle).__name__))
    h, w = (int(v) for v in rle["size"])
    if size is not None and (h, w) != (int(size[0]), int(size[1])):
        raise RLEError("{}: its size {} is not the expected (h, w) = {}".format(_where(instance), [h, w], (int(size[0]), int(size[1]))))
    c = rle["counts"]
    counts = string_to_counts(c, instance) if isinstance(c, (str, bytes, bytearray)) else [int(v) for v in c]
    if any(v < 0 for v in counts):
        raise RLEError("{}: a negative run length".format(_where(instance)))
    if sum(counts) != h * w:
        raise RLEError("{}: its counts sum to {}, not to h * w = {}".format(_where(instance), sum(counts), h * w))
    return counts


def decode_one(rle, size=None, instance=None):
    """one RLE dict -> uint8 [h, w] numpy mask of 0 / 1"""
    counts = rle_counts(rle, size, instance)
    h, w = (int(v) for v in rle["size"])
    values = (np.arange(len(counts)) & 1).astype(np.uint8)
    return np.repeat(values, counts).reshape(w, h).T.copy()     # column-major run order


def decode(rles, size=None):
    """list of RLE dicts (all of one size; size = (h, w) is needed when the list is empty) -> uint8 [n, h, w] numpy masks"""
    if len(rles) == 0:
        if size is None:
            raise ValueError("decode: an empty list needs size = (h, w)")
        return np.zeros((0, int(size[0]), int(size[1])), np.uint8)
    size = tuple(int(v) for v in (size if size is not None else rles[0]["size"]))
    return np.stack([decode_one(r, size, i) for i, r in enumerate(rles)])


def mask_counts(mask):
    """[h, w] mask (a pixel is set iff it == 1) -> list of run lengths"""
    m = np.asarray(mask)
    if m.ndim != 2:
        raise ValueError("mask_counts: expected an [h, w] mask, got shape {}".format(m.shape))
    flat = (m == 1).T.reshape(-1)                                # column-major
    starts = np.flatnonzero(np.diff(np.concatenate(([False], flat)).astype(np.int8)))   # where the value changes, against a 0 before pixel 0
    edges = np.concatenate(([0], starts, [flat.size]))
    return [int(v) for v in np.diff(edges)]


def encode_one(mask):
    m = np.asarray(mask)
    return {"size": [int(m.shape[0]), int(m.shape[1])], "counts": counts_to_string(mask_counts(m))}


def encode(masks):
    """[n, h, w] masks -> list of {"size": [h, w], "counts": str}"""
    return [encode_one(m) for m in np.asarray(masks)]

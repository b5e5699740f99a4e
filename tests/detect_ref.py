"""float64 reference of the test-time softmax + box decode (abr_iod_amd/csrc/detect.hip: det_softmax_decode_kernel) and the seeded case
builders its two suites share (tests/test_detect_ref.py on the CPU, tests/test_gpu_detect_post.py on the GPU).  Plain numpy: nothing here
imports the library under test.

  * `softmax_decode_f64` promotes the float32 inputs to float64 and evaluates softmax(logits), BoxCoder.decode of every class's deltas
    against the proposal and clip_to_image(remove_empty=False) there.  The clamp of dw / dh is float32(log(1000 / 16)) promoted -- the
    value a float32 kernel holds -- so a delta one float above or below clamp * weight lands on the same side in both.  Next to `prob` and
    `boxes` it returns the MAGNITUDES the error bounds are relative to (`prob_bound`, `box_bound`).
  * `softmax_cases()` builds every input the two suites run: the shape grid C x K with rows cycling through all logit / delta / proposal
    families, one case per family (so a maximum can be printed per family), several images of different sizes with empty ones first, in the
    middle and last, and the class-agnostic heads.
  * the selection (det_select) has no second reference here: oracle.torch_ref.det_filter_results is it.  `grid_boxes` and the score
    builders below only make inputs on which that comparison is about the thing under test: integer boxes on a non-overlapping grid (every
    IoU is exactly 0) and scores with chosen bit patterns.
"""
from collections import namedtuple

import numpy as np

EPS = 2.0 ** -24                                        # half a float32 ulp, relative
CLIP32 = np.float32(np.log(1000.0 / 16))                # box_coder.py:20 as a float32 kernel holds it
CLIP = float(CLIP32)
WEIGHTS = (10.0, 10.0, 5.0, 5.0)

Ref = namedtuple("Ref", "prob boxes prob_mag box_mag")


# --------------------------------------------------------------------------------------------------------------------- reference
def softmax_decode_f64(logits, deltas, rois, img_hw, weights=WEIGHTS, cls_agnostic=False):
    """logits [K, C], deltas [K, 4C] (class-agnostic: any width >= 4, the LAST four columns are the box), rois [K, 5] = (image, x1, y1, x2,
    y2), img_hw [N, 2] (height, width) -> Ref(prob [K, C], boxes [K, C, 4], prob_mag [K, C], box_mag [K, C, 4]), all float64.

    prob_mag = |x_j - max_c x_c| + C + 4                                            (relative to prob: see prob_bound)
    box_mag  = |dx| |w| + |cx| + 0.5 e^dw |w| (1 + |dw|) + 1  for x1 / x2, likewise for y1 / y2 (absolute: see box_bound)"""
    x = np.asarray(logits, np.float32).astype(np.float64)
    K, C = x.shape
    rel = x - x.max(axis=1, keepdims=True)
    e = np.exp(rel)
    prob = e / e.sum(axis=1, keepdims=True)
    d = np.asarray(deltas, np.float32).astype(np.float64)
    d = np.tile(d[:, -4:], (1, C)) if cls_agnostic else d[:, :4 * C]
    d = d.reshape(K, C, 4)
    r = np.asarray(rois, np.float32).astype(np.float64)
    wx, wy, ww, wh = [float(np.float32(v)) for v in weights]
    w, h = (r[:, 3] - r[:, 1] + 1)[:, None], (r[:, 4] - r[:, 2] + 1)[:, None]
    cx, cy = r[:, 1:2] + 0.5 * w, r[:, 2:3] + 0.5 * h
    dx, dy = d[..., 0] / wx, d[..., 1] / wy
    dw, dh = np.minimum(d[..., 2] / ww, CLIP), np.minimum(d[..., 3] / wh, CLIP)
    pcx, pcy = dx * w + cx, dy * h + cy
    pw, ph = np.exp(dw) * w, np.exp(dh) * h
    raw = np.stack([pcx - 0.5 * pw, pcy - 0.5 * ph, pcx + 0.5 * pw - 1, pcy + 0.5 * ph - 1], -1)
    img = r[:, 0].astype(np.int64)
    hw = np.asarray(img_hw, np.int64).reshape(-1, 2)
    W1, H1 = (hw[img, 1] - 1).astype(np.float64)[:, None], (hw[img, 0] - 1).astype(np.float64)[:, None]
    hi = np.stack([W1, H1, W1, H1], -1) + np.zeros_like(raw)
    boxes = np.minimum(np.maximum(raw, 0.0), hi)
    mx = np.abs(dx) * np.abs(w) + np.abs(cx) + 0.5 * np.exp(dw) * np.abs(w) * (1 + np.abs(dw)) + 1
    my = np.abs(dy) * np.abs(h) + np.abs(cy) + 0.5 * np.exp(dh) * np.abs(h) * (1 + np.abs(dh)) + 1
    return Ref(prob, boxes, np.abs(rel) + C + 4, np.stack([mx, my, mx, my], -1))


def prob_bound(ref):
    """|got - want| <= EPS (|x_j - max| + C + 4) want + 2^-126"""
    return EPS * ref.prob_mag * ref.prob + 2.0 ** -126


def box_bound(ref):
    """|got - want| <= 8 EPS (|dx| w + |cx| + 0.5 e^dw w (1 + |dw|) + 1)"""
    return 8 * EPS * ref.box_mag


def measure(got_prob, got_boxes, ref):
    """-> (worst prob error as a fraction of prob_bound, worst prob error in units of EPS * want over the normal results, worst box error
    as a fraction of box_bound, worst box error in units of EPS * box_mag); 0 for empty inputs"""
    if ref.prob.size == 0:
        return 0.0, 0.0, 0.0, 0.0
    ep = np.abs(np.asarray(got_prob, np.float64) - ref.prob)
    eb = np.abs(np.asarray(got_boxes, np.float64) - ref.boxes)
    normal = ref.prob >= 2.0 ** -126
    ulps = float((ep[normal] / (EPS * ref.prob[normal])).max()) if normal.any() else 0.0
    return float((ep / prob_bound(ref)).max()), ulps, float((eb / box_bound(ref)).max()), float((eb / (EPS * ref.box_mag)).max())


# --------------------------------------------------------------------------------------------------------------------- softmax cases
LOGIT_FAMILIES = ("normal", "equal", "plus88", "plus1e4", "minus100")
DELTA_FAMILIES = ("normal", "clamp", "pm60", "out_left", "out_right", "out_top", "out_bottom")
PROP_FAMILIES = ("normal", "one_pixel", "inverted", "border")

# (width, height): an ordinary image, 1 x 1, 7 x 1000, 600 x 9; images 0, 3 and 6 never get a row (empty first, in the middle, last)
SIZES_WH = [(800, 600), (1000, 600), (1, 1), (640, 480), (7, 1000), (600, 9), (333, 500)]

Case = namedtuple("Case", "name C counts sizes_wh logits deltas rois img_hw cls_agnostic families")


def _counts(K):
    small = min(K // 8, 16)
    c = [0, 0, small, 0, K // 8, K // 8, 0]
    c[1] = K - sum(c)
    return c


def _proposals(rng, fam, W, H):
    """one float32 proposal of family `fam` inside a W x H image, corners >= 0"""
    x1, y1 = rng.uniform(0, max(W - 1, 0)), rng.uniform(0, max(H - 1, 0))
    x2, y2 = rng.uniform(x1, max(W - 1, 0)), rng.uniform(y1, max(H - 1, 0))
    if fam == "one_pixel":
        x2, y2 = x1, y1
    elif fam == "inverted":
        x1, x2, y1, y2 = x2 + rng.integers(0, 3), x1, y2 + rng.integers(0, 3), y1      # x2 <= x1; w = x2 - x1 + 1 can be 0 or negative
    elif fam == "border":
        side = rng.integers(0, 4)
        x1, y1 = (0.0, y1) if side == 0 else (x1, 0.0) if side == 1 else (x1, y1)
        x2, y2 = (float(W - 1), y2) if side == 2 else (x2, float(H - 1)) if side == 3 else (x2, y2)
    return np.float32([x1, y1, x2, y2])


def _logits(rng, fam, C):
    if fam == "normal":
        return (rng.standard_normal(C) * 3).astype(np.float32)
    if fam == "equal":
        return np.full(C, np.float32(rng.standard_normal() * 3), np.float32)
    x = (rng.standard_normal(C) * 0.25).astype(np.float32)
    j = rng.integers(0, C)
    x[j] += np.float32({"plus88": 88.0, "plus1e4": 1e4, "minus100": -100.0}[fam])
    return x


def _deltas(rng, fam, n4, box, W, H, weights):
    """n4 = number of 4-column groups; `box` the float32 proposal the deltas are decoded against"""
    d = (rng.standard_normal((n4, 4)) * 0.7).astype(np.float32)
    if fam == "clamp":
        for col, wt in ((2, weights[2]), (3, weights[3])):
            c = CLIP32 * np.float32(wt)
            d[:, col] = np.float32([c, np.nextafter(c, np.float32(np.inf)), np.nextafter(c, np.float32(-np.inf))])[rng.integers(0, 3, n4)]
    elif fam == "pm60":
        # +-60 as a delta (dw = +-12) and as dw itself (the delta is +-60 * weight)
        d[:, 2] = np.float32([60.0, -60.0, 60.0 * weights[2], -60.0 * weights[2]])[rng.integers(0, 4, n4)]
        d[:, 3] = np.float32([60.0, -60.0, 60.0 * weights[3], -60.0 * weights[3]])[rng.integers(0, 4, n4)]
    elif fam.startswith("out_"):
        # the centre moves two image sizes plus two decoded box sizes past the side: both corners clip to 0 or to W - 1 / H - 1
        d[:, 2:] = (rng.standard_normal((n4, 2)) * 0.3).astype(np.float32)
        b = box.astype(np.float64)
        w, h = b[2] - b[0] + 1, b[3] - b[1] + 1
        horiz = fam in ("out_left", "out_right")
        ext, L, col, wt = (w, W, 0, weights[0]) if horiz else (h, H, 1, weights[1])
        sign = -1.0 if fam in ("out_left", "out_top") else 1.0
        if ext != 0:
            grow = np.exp(d[:, col + 2].astype(np.float64) / weights[col + 2])
            d[:, col] = (sign * (2 * L + 2 * abs(ext) * grow + 4) / ext * wt).astype(np.float32)
    return d


def _pick(fams, which, r):
    return fams[r % len(fams)] if which == "mix" else which


def make_case(name, C, counts, sizes_wh, seed, logit="mix", delta="mix", prop="mix", cls_agnostic=False, delta_cols=None, weights=WEIGHTS):
    """rows cycle through the families when a family is "mix" (with co-prime periods, so every combination comes up in a long case)"""
    rng = np.random.default_rng(seed)
    K = sum(counts)
    ncol = delta_cols if delta_cols is not None else 4 * C
    logits, deltas, rois = np.empty((K, C), np.float32), np.empty((K, ncol), np.float32), np.empty((K, 5), np.float32)
    fams = []
    r = 0
    for i, n in enumerate(counts):
        W, H = sizes_wh[i]
        for _ in range(n):
            lf, df, pf = _pick(LOGIT_FAMILIES, logit, r), _pick(DELTA_FAMILIES, delta, r // 5), _pick(PROP_FAMILIES, prop, r // 3)
            box = _proposals(rng, pf, W, H)
            logits[r] = _logits(rng, lf, C)
            deltas[r] = _deltas(rng, df, ncol // 4, box, W, H, weights).reshape(-1)
            rois[r, 0], rois[r, 1:] = i, box
            fams.append((lf, df, pf))
            r += 1
    img_hw = np.array([[h, w] for w, h in sizes_wh], np.int32)
    return Case(name, C, list(counts), list(sizes_wh), logits, deltas, rois, img_hw, cls_agnostic, fams)


def softmax_cases():
    """every softmax / decode case of both suites, in a fixed order with fixed seeds"""
    out = []
    for C in (1, 2, 21, 81):
        for K in (0, 1, 255, 256, 257, 1000):
            out.append(make_case("shape-C{}-K{}".format(C, K), C, _counts(K), SIZES_WH, seed=1000 * C + K))
    for f in LOGIT_FAMILIES:
        out.append(make_case("logits-" + f, 21, _counts(257), SIZES_WH, seed=len(out), logit=f, delta="normal", prop="normal"))
    for f in DELTA_FAMILIES:
        out.append(make_case("deltas-" + f, 21, _counts(257), SIZES_WH, seed=len(out), logit="normal", delta=f))
    for f in PROP_FAMILIES:
        out.append(make_case("props-" + f, 21, _counts(257), SIZES_WH, seed=len(out), logit="normal", delta="normal", prop=f))
    out.append(make_case("images-mixed", 21, [0, 40, 9, 0, 33, 57, 0], SIZES_WH, seed=len(out)))
    out.append(make_case("agnostic-4col", 21, _counts(257), SIZES_WH, seed=len(out), cls_agnostic=True, delta_cols=4))
    out.append(make_case("agnostic-4C", 21, _counts(257), SIZES_WH, seed=len(out), cls_agnostic=True))
    out.append(make_case("agnostic-4col-K1", 2, _counts(1), SIZES_WH, seed=len(out), cls_agnostic=True, delta_cols=4))
    return out


def proposals_per_image(case):
    """list of [n_i, 4] float32 arrays, the form the oracle takes"""
    off = np.concatenate([[0], np.cumsum(case.counts)])
    return [case.rois[off[i]:off[i + 1], 1:].copy() for i in range(len(case.counts))]


def clamp_probe():
    """-> Case of C = 1, three rows in one 4096 x 4096 image whose dw = dh = float32(delta / 5) is exactly one float below the clamp, the
    clamp, one float above it.  The proposal (0, 0, 63, 63) has w = 64 and cx = 32 and dx = dy = 0, so everything but expf() is exact in
    float32: rows 1 and 2 must decode to the same bits, row 0 to a box that is narrower by 8 ulps of x2 (e^dw changes by 4 of its ulps)."""
    c = CLIP32 * np.float32(5)
    near = [c]
    for _ in range(8):
        near = [np.nextafter(near[0], np.float32(-np.inf))] + near + [np.nextafter(near[-1], np.float32(np.inf))]
    near = np.float32(near)
    q = near / np.float32(5)
    want = [np.nextafter(CLIP32, np.float32(0)), CLIP32, np.nextafter(CLIP32, np.float32(9))]
    d = np.float32([near[np.nonzero(q == v)[0][0]] for v in want])
    deltas = np.zeros((3, 4), np.float32)
    deltas[:, 2] = deltas[:, 3] = d
    rois = np.tile(np.float32([0, 0, 0, 63, 63]), (3, 1))
    return Case("clamp-probe", 1, [3], [(4096, 4096)], np.zeros((3, 1), np.float32), deltas, rois, np.array([[4096, 4096]], np.int32), False, [])


# --------------------------------------------------------------------------------------------------------------------- selection inputs
def grid_boxes(n, C, cell=4, per_row=128):
    """[n, C, 4] float32: proposal t sits in cell (t % per_row, t // per_row) of an integer grid, one pixel short of its neighbours on every
    side, the same box for every class -- every pairwise IoU is exactly 0, so NMS keeps all of them at any threshold above 0"""
    t = np.arange(n)
    x1, y1 = (t % per_row) * cell, (t // per_row) * cell
    b = np.stack([x1, y1, x1 + cell - 2, y1 + cell - 2], -1).astype(np.float32)
    return np.repeat(b[:, None, :], C, 1).copy()


def from_bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)

"""The level rule of the feature-pyramid pooler restated in numpy, the RoI sets its two suites share (tests/test_pooler_ref.py on the CPU,
tests/test_gpu_pooler.py on the GPU) and the expected results built from the single-level references.  Nothing here imports the library
under test.

  * LEVELS: modeling/poolers.py:37-42 op by op in float32 (numpy's float32 ufuncs round every operation and never contract): area with
    TO_REMOVE = 1, sqrt, / canonical_scale, + eps, log2, canonical_level + ., floor, clamp, minus k_min.  -1 where the value is NaN (a
    negative or NaN area): the reference's row matches no level.  `level_value(.., np.float64)` is the unclamped value in float64: random rows
    whose float64 value lies within MARGIN of an integer are redrawn when the set is BUILT, so every row of a set is compared.
  * EXPECTED FORWARD: oracle.ops.roi_align_forward (the CPU oracle of the single-level operator) on each level's rows, scattered into
    zeros -- the reference Pooler's own procedure (poolers.py:99-103).
  * FLOAT64 PAIRS: roi_align_ref.forward / backward per level over that level's rows only, with S the sum of |addends|.
"""
import numpy as np

import roi_align_ref as R

SCALES = (0.25, 0.125, 0.0625, 0.03125)
K_MIN, K_MAX = 2.0, 5.0      # -log2 of the first and the last scale
MARGIN = 1e-5


def level_value(rois, canonical_scale=224, canonical_level=4, eps=1e-6, dtype=np.float32):
    """canonical_level + log2(sqrt(area) / canonical_scale + eps) before the floor, in `dtype`; NaN for a negative or NaN area"""
    ft = np.dtype(dtype).type
    r = np.asarray(rois, np.float32).astype(ft)
    with np.errstate(invalid="ignore", divide="ignore"):
        area = (r[:, 3] - r[:, 1] + ft(1)) * (r[:, 4] - r[:, 2] + ft(1))
        s = np.sqrt(area)
        v = ft(canonical_level) + np.log2(s / ft(canonical_scale) + ft(eps))
    assert v.dtype == np.dtype(dtype)
    return v


def levels(rois, k_min=K_MIN, k_max=K_MAX, canonical_scale=224, canonical_level=4, eps=1e-6):
    """int32 [K]: 0 .. k_max - k_min, -1 for a row without a level"""
    v = level_value(rois, canonical_scale, canonical_level, eps)
    nan = np.isnan(v)
    t = np.clip(np.floor(np.where(nan, np.float32(k_min), v)), np.float32(k_min), np.float32(k_max))
    return np.where(nan, -1, t.astype(np.int64) - int(k_min)).astype(np.int32)


# --------------------------------------------------------------------------------------------------------------------- RoI sets
def edge_rows(img_h, img_w):
    """[(name, x1, y1, x2, y2)] in image units: the level rule's boundaries and the rows without a level"""
    rows = []
    for side in (56, 112, 224, 448, 896):        # exactly on a boundary: the eps puts them on the UPPER level (896: on k_max)
        rows.append((f"square_{side}", 10.0, 10.0, 10.0 + side - 1, 10.0 + side - 1))
    rows.append(("224x223", 10.0, 10.0, 233.0, 232.0))      # one level lower
    rows.append(("448x447", 10.0, 10.0, 457.0, 456.0))
    rows.append(("one_by_one", 20.0, 20.0, 20.0, 20.0))
    rows.append(("far_larger_than_image", -2000.0, -1500.0, 3000.0, 2500.0))
    rows.append(("area_zero", 30.0, 30.0, 29.0, 50.0))      # x2 = x1 - 1: 4 + log2(1e-6) clamps to k_min
    rows.append(("both_sides_negative", 50.0, 50.0, 40.0, 40.0))   # positive area: pooled like any box (ROIAlign makes it 1 x 1)
    rows.append(("negative_area", 50.0, 50.0, 40.0, 60.0))  # no level
    rows.append(("nan_coordinate", float("nan"), 10.0, 50.0, 60.0))   # no level
    rows.append(("outside_the_map", img_w + 100.0, img_h + 100.0, img_w + 180.0, img_h + 150.0))
    return rows


NO_LEVEL = ("negative_area", "nan_coordinate")


def random_rows(rng, n, img_h, img_w):
    """side log-uniform in [16, 1000] px, aspect ratio in [1/3, 3], centre anywhere in the image (boxes may leave it); a row whose float64
    level value lies within MARGIN of an integer is redrawn"""
    out = np.zeros((n, 4), np.float32)
    i = 0
    while i < n:
        side = np.exp(rng.uniform(np.log(16.0), np.log(1000.0)))
        ar = np.exp(rng.uniform(np.log(1 / 3), np.log(3.0)))
        w, h = side * np.sqrt(ar), side / np.sqrt(ar)
        cx, cy = rng.uniform(0, img_w), rng.uniform(0, img_h)
        row = np.array([cx - w / 2, cy - h / 2, cx + w / 2, cy + h / 2], np.float32)
        v = level_value(np.concatenate([[0], row])[None], dtype=np.float64)[0]
        if abs(v - np.round(v)) < MARGIN:
            continue
        out[i] = row
        i += 1
    return out


def roi_set(B, img_h, img_w, maps, per_img=36, zoo=False, seed=0, scales=SCALES):
    """(rois [K,5] float32, names): the edge rows, per_img random rows for every image and, with `zoo`, roi_align_ref.edge_zoo rescaled to each
    level's scale (built for that level's map; the rule sends each row wherever its size says).  Every level gets >= 4 rows per image."""
    rng = np.random.default_rng(R._seed("pooler_roi_set", B, img_h, img_w, per_img, zoo, seed))
    rows, names = [], []
    for i, (n, x1, y1, x2, y2) in enumerate(edge_rows(img_h, img_w)):
        rows.append([i % B, x1, y1, x2, y2])
        names.append(n)
    for b in range(B):
        for j, r in enumerate(random_rows(rng, per_img, img_h, img_w)):
            rows.append([b, *r])
            names.append(f"random_{b}_{j}")
    if zoo:
        for l, ((H, W), s) in enumerate(zip(maps, scales)):
            for n, r in R.edge_zoo_named(B, H, W, s):
                rows.append(r)
                names.append(f"zoo{l}_{n}")
    rois = np.array(rows, np.float32).reshape(-1, 5)
    lv = levels(rois)
    for b in range(B):
        got = np.bincount(lv[(rois[:, 0] == b) & (lv >= 0)], minlength=len(maps))
        assert (got >= 4).all(), f"image {b}: rows per level {got.tolist()}"
    return rois, names


def make_feats(seed, B, C, maps):
    """list of [B,H,W,C] float32 standard-normal maps"""
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, H, W, C)).astype(np.float32) for H, W in maps]


# --------------------------------------------------------------------------------------------------------------------- expected results
def expected_forward(feats, rois, lv, ph, pw, sr, scales=SCALES):
    """[K,C,ph,pw] float32: the CPU oracle of the single-level operator on each level's rows, scattered into zeros; no-level rows stay zero"""
    from oracle import ops as O
    C = feats[0].shape[-1]
    out = np.zeros((len(rois), C, ph, pw), np.float32)
    for l, (f, s) in enumerate(zip(feats, scales)):
        idx = np.nonzero(lv == l)[0]
        if len(idx):
            out[idx] = O.roi_align_forward(np.ascontiguousarray(f.transpose(0, 3, 1, 2)), rois[idx], s, ph, pw, sr)
    return out


def want_forward(feats, rois, lv, ph, pw, sr, scales=SCALES):
    """float64 (want, S), each [K,ph,pw,C]"""
    C = feats[0].shape[-1]
    want, S = np.zeros((len(rois), ph, pw, C)), np.zeros((len(rois), ph, pw, C))
    for l, (f, s) in enumerate(zip(feats, scales)):
        idx = np.nonzero(lv == l)[0]
        if len(idx):
            want[idx], S[idx] = R.forward(f, rois[idx], s, ph, pw, sr)
    return want, S


def want_backward(grad, rois, lv, shapes, ph, pw, sr, scales=SCALES):
    """[(want_l, S_l)] float64 [B,H_l,W_l,C]: the transpose over that level's rows only"""
    out = []
    for l, ((B, H, W, C), s) in enumerate(zip(shapes, scales)):
        idx = np.nonzero(lv == l)[0]
        out.append(R.backward(grad[idx], rois[idx], s, ph, pw, sr, B, H, W))
    return out

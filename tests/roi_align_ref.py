"""float64 reference of RoIAlign and the seeded case builders its two suites share (tests/test_roi_align_ref.py on the CPU,
tests/test_gpu_roi_align.py on the GPU).  Plain numpy: nothing here imports the library under test.

The reference is the separable form of the operation.  A bilinear sample's four weights are the product of a y-pair and an x-pair, the
sample grid is a product grid, and a sample is rejected when its y OR its x is out of range -- so for one RoI

    out[k, ph, pw, :] = (1 / count) * sum_{y, x} Ay[k, ph, y] * Ax[k, pw, x] * feat[b, y, x, :]        count = gh * gw

with Ay[k, ph, y] the sum, over bin row ph's samples that survive the reject test, of the weight they put on feature row y.

  * GEOMETRY is float32 (float64 behind `dtype`), op by op in the association order of ROIAlign_cpu.cpp:39-45 that `roi_geom`, `make_tap` and
    `axis_tap` of abr_iod_amd/csrc/roi_align.hip restate: scaled corners, max(., 1), bin size, grid (sr > 0 ? sr : ceil), the sample coordinate
    start + p * bin + ((i + .5) * bin) / grid, the reject test (v < -1 || v > L), the clamp to 0 and the clamp of l >= L - 1.  numpy's float32
    ufuncs round every operation to float32 and never contract, so the integer taps ARE the float32 ones.
  * WEIGHTS AND SUMS are float64: the fraction lw = v - l is the float32 one widened to double, the tables sum (1 - lw) and lw in double, and
    both directions accumulate in double.
  * S, the magnitude every bound is relative to, is the same function run on |feat| (or |grad|): the per-element sum of |addends| (the weights
    are non-negative).  Both functions return (value, S) from one pass over the channels [x, |x|].

Evaluation is per RoI over its footprint with two matmuls, so the full-size case (B = 4, 38 x 63 x 1024, 2048 RoIs) stays affordable: see
tests/test_roi_align_ref.py for the measured time.
"""
import zlib
from collections import namedtuple

import numpy as np

TOL = 1e-6        # the project's rule (tests/test_gpu_loss_kernels.py): relative to the sum of |addends|, about 8 fp32 ulps
TOL_F64 = 1e-12   # the float64 NCHW pair


# --------------------------------------------------------------------------------------------------------------------- geometry
Geom = namedtuple("Geom", "b y0 x0 bh bw gh gw")
Axis = namedtuple("Axis", "lo hi lw ok")   # each [K, Po, gmax]; ok False for rejected samples and for i >= grid[k]


def roi_geom(rois, scale, PH, PW, sr, dtype=np.float32):
    ft = np.dtype(dtype).type
    r = np.asarray(rois)
    rr = r.astype(ft)
    s = ft(scale)
    sw, sh, ew, eh = rr[:, 1] * s, rr[:, 2] * s, rr[:, 3] * s, rr[:, 4] * s
    rw, rh = np.maximum(ew - sw, ft(1)), np.maximum(eh - sh, ft(1))
    bh, bw = rh / ft(PH), rw / ft(PW)
    if sr > 0:
        gh = np.full(len(r), sr, np.int64)
        gw = gh.copy()
    else:
        gh, gw = np.ceil(rh / ft(PH)).astype(np.int64), np.ceil(rw / ft(PW)).astype(np.int64)
    return Geom(r[:, 0].astype(np.int64), sh, sw, bh, bw, gh, gw)


def axis_taps(start, binsz, grid, P, step, L, dtype=np.float32):
    """samples of the kept bins 0, step, 2 step, ... of one axis for every RoI: low / high tap, the fraction on the high tap, validity"""
    ft = np.dtype(dtype).type
    K = len(start)
    p = np.arange(0, P, step)
    gmax = int(grid.max()) if K else 1
    i = np.arange(gmax)
    st, bs = start[:, None, None], binsz[:, None, None]
    v = (st + p.astype(ft)[None, :, None] * bs) + ((i.astype(ft) + ft(0.5))[None, None, :] * bs) / grid.astype(ft)[:, None, None]
    assert v.dtype == np.dtype(dtype)
    ok = (i[None, None, :] < grid[:, None, None]) & ~((v < ft(-1)) | (v > ft(L)))
    v = np.where(v <= ft(0), ft(0), v)
    lo = np.where(ok, v, ft(0)).astype(np.int64)
    top = lo >= L - 1
    lo = np.where(top, L - 1, lo)
    hi = np.where(top, L - 1, lo + 1)
    v = np.where(top, lo.astype(ft), v)
    lw = v - lo.astype(ft)
    assert lw.dtype == np.dtype(dtype)
    return Axis(lo, hi, lw.astype(np.float64), ok)


def axis_table(ax, L):
    """A[K, Po, L] float64: the weight the bin's surviving samples put on each pixel of the axis"""
    K, Po, _ = ax.ok.shape
    A = np.zeros((K, Po, L), np.float64)
    kk, pp, ii = np.nonzero(ax.ok)
    np.add.at(A, (kk, pp, ax.lo[kk, pp, ii]), 1.0 - ax.lw[kk, pp, ii])
    np.add.at(A, (kk, pp, ax.hi[kk, pp, ii]), ax.lw[kk, pp, ii])
    return A


Tables = namedtuple("Tables", "b Ay Ax count gh gw yr xr")   # yr, xr [K, 2]: inclusive footprint, (0, -1) when empty


def _span(A):
    hit = (A != 0).any(1)
    K, L = hit.shape
    first = np.where(hit.any(1), hit.argmax(1), 0)
    last = np.where(hit.any(1), L - 1 - hit[:, ::-1].argmax(1), -1)
    return np.stack([first, last], 1)


def tables(rois, H, W, scale, PH, PW, sr, bin_step=1, dtype=np.float32):
    g = roi_geom(rois, scale, PH, PW, sr, dtype)
    Ay = axis_table(axis_taps(g.y0, g.bh, g.gh, PH, bin_step, H, dtype), H)
    Ax = axis_table(axis_taps(g.x0, g.bw, g.gw, PW, bin_step, W, dtype), W)
    return Tables(g.b, Ay, Ax, (g.gh * g.gw).astype(np.float64), g.gh, g.gw, _span(Ay), _span(Ax))


def taps(rois, H, W, scale, PH, PW, sr, max_s):
    """(idx [K, PH * PW, max_s, 4] int32, grid [K, 2] int32) in the layout of oracle.ops.roi_align_taps: flat y * W + x of the four taps of
    sample s = iy * gw + ix, -1 for a rejected sample, -2 for the unused slots"""
    g = roi_geom(rois, scale, PH, PW, sr)
    K = len(g.b)
    ay = axis_taps(g.y0, g.bh, g.gh, PH, 1, H)
    ax = axis_taps(g.x0, g.bw, g.gw, PW, 1, W)
    idx = np.full((K, PH * PW, max_s, 4), -2, np.int32)
    for gh, gw in {(int(a), int(b)) for a, b in zip(g.gh, g.gw)}:
        sel = np.nonzero((g.gh == gh) & (g.gw == gw))[0]
        yl, yh, oky = (a[sel][:, :, None, :gh, None] for a in (ay.lo, ay.hi, ay.ok))    # [k, ph, 1, iy, 1]
        xl, xh, okx = (a[sel][:, None, :, None, :gw] for a in (ax.lo, ax.hi, ax.ok))    # [k, 1, pw, 1, ix]
        ok = oky & okx
        t = np.stack([np.where(ok, a * W + b, -1) for a, b in ((yl, xl), (yl, xh), (yh, xl), (yh, xh))], -1)
        t = t.reshape(len(sel), PH * PW, gh * gw, 4)[:, :, :max_s]
        idx[sel, :, :t.shape[2]] = t
    return idx, np.stack([g.gh, g.gw], 1).astype(np.int32)


# --------------------------------------------------------------------------------------------------------------------- the two directions
def forward(feat, rois, scale, PH, PW, sr, bin_step=1, dtype=np.float32):
    """feat [B, H, W, C], rois [K, 5] -> (out, S), each float64 [K, PHo, PWo, C]"""
    B, H, W, C = feat.shape
    t = tables(rois, H, W, scale, PH, PW, sr, bin_step, dtype)
    K, Po, Qo = len(t.b), t.Ay.shape[1], t.Ax.shape[1]
    f = np.asarray(feat, np.float64)
    F = np.concatenate([f, np.abs(f)], -1)
    out = np.zeros((K, Po, Qo, 2 * C), np.float64)
    for k in range(K):
        (y0, y1), (x0, x1) = t.yr[k], t.xr[k]
        if y1 < y0 or x1 < x0:
            continue
        ny, nx = y1 - y0 + 1, x1 - x0 + 1
        rows = t.Ay[k][:, y0:y1 + 1] @ F[t.b[k], y0:y1 + 1, x0:x1 + 1].reshape(ny, nx * 2 * C)    # [Po, nx * 2C]
        out[k] = np.matmul(t.Ax[k][:, x0:x1 + 1], rows.reshape(Po, nx, 2 * C)) / t.count[k]        # [Po, Qo, 2C]
    return out[..., :C], out[..., C:]


def backward(grad, rois, scale, PH, PW, sr, B, H, W, bin_step=1, dtype=np.float32):
    """grad [K, PHo, PWo, C] -> (gfeat, S), each float64 [B, H, W, C]: the transpose of `forward`"""
    K, Po, Qo, C = grad.shape
    t = tables(rois, H, W, scale, PH, PW, sr, bin_step, dtype)
    assert (Po, Qo) == (t.Ay.shape[1], t.Ax.shape[1])
    g = np.asarray(grad, np.float64)
    G = np.concatenate([g, np.abs(g)], -1)
    out = np.zeros((B, H, W, 2 * C), np.float64)
    for k in range(K):
        (y0, y1), (x0, x1) = t.yr[k], t.xr[k]
        if y1 < y0 or x1 < x0:
            continue
        ny, nx = y1 - y0 + 1, x1 - x0 + 1
        cols = np.matmul(t.Ax[k][:, x0:x1 + 1].T, G[k])                                            # [Po, nx, 2C]
        px = t.Ay[k][:, y0:y1 + 1].T @ cols.reshape(Po, nx * 2 * C)                                # [ny, nx * 2C]
        out[t.b[k], y0:y1 + 1, x0:x1 + 1] += px.reshape(ny, nx, 2 * C) / t.count[k]
    return out[..., :C], out[..., C:]


# --------------------------------------------------------------------------------------------------------------------- the one check
def worst_ratio(got, want, S):
    """max |got - want| / S over the elements with S > 0 (0.0 when there is none)"""
    got, want, S = (np.asarray(a, np.float64) for a in (got, want, S))
    live = S > 0
    return float((np.abs(got - want)[live] / S[live]).max()) if live.any() else 0.0


def check(got, want, S, what, axes="k,ph,pw,c", tol=TOL):
    """got is finite; |got - want| <= tol * S element-wise; got == 0 exactly where S == 0.  Returns the worst |err| / S."""
    got = np.asarray(got, np.float64)
    want, S = np.asarray(want, np.float64), np.asarray(S, np.float64)
    assert got.shape == want.shape == S.shape, f"{what}: shapes {got.shape} {want.shape} {S.shape}"
    if got.size == 0:
        return 0.0
    bad = ~np.isfinite(got)
    assert not bad.any(), f"{what}: non-finite at ({axes}) = {np.unravel_index(int(bad.argmax()), got.shape)}"
    dead = (S == 0) & (got != 0)
    if dead.any():
        at = np.unravel_index(int(dead.argmax()), got.shape)
        raise AssertionError(f"{what}: {got[at]!r} where no sample lands (S == 0) at ({axes}) = {tuple(int(i) for i in at)}; {int(dead.sum())} such elements")
    err = np.abs(got - want)
    over = err - tol * S
    if (over > 0).any():
        at = np.unravel_index(int(np.where(S > 0, err / np.where(S > 0, S, 1.0), 0.0).argmax()), got.shape)
        raise AssertionError(f"{what}: worst |err| / S = {err[at] / S[at]:.3e} > {tol:g} at ({axes}) = {tuple(int(i) for i in at)}: got {got[at]!r}, "
                             f"want {want[at]!r}, S {S[at]:.6g}; {int((over > 0).sum())} of {got.size} elements over the bound")
    return worst_ratio(got, want, S)


# --------------------------------------------------------------------------------------------------------------------- RoI builders
def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def random_rois(B, H, W, scale, per_img, seed=0):
    """log-uniform sizes from a quarter pixel to most of the map, corners from 1.25 pixels before the origin to past the far borders
    (tests/test_gpu_vs_reference_csrc.py::_rois, in units of the map); every image gets per_img rows"""
    rng = np.random.default_rng(_seed("random_rois", B, H, W, scale, per_img, seed))
    out = []
    for b in range(B):
        x1 = rng.uniform(-1.25, W - 0.6, per_img)
        y1 = rng.uniform(-1.25, H - 0.6, per_img)
        w = np.exp(rng.uniform(np.log(0.25), np.log(max(0.7 * W, 2.0)), per_img))
        h = np.exp(rng.uniform(np.log(0.25), np.log(max(0.8 * H, 2.0)), per_img))
        out.append(np.stack([np.full(per_img, b), x1, y1, np.minimum(x1 + w, W + 0.95), np.minimum(y1 + h, H + 0.95)], 1))
    r = np.concatenate(out) if out else np.zeros((0, 5))
    r[:, 1:] /= scale
    return r.astype(np.float32)


def outside_rows(B, H, W, scale):
    """four RoIs whose every sample is rejected, one past each side of the map (for 7 or more bins and any sampling ratio)"""
    rows = [("outside_top", 2.0, -12.0, 9.0, -3.0), ("outside_bottom", 2.0, H + 3.0, 9.0, H + 12.0),
            ("outside_left", -12.0, 1.0, -3.0, 8.0), ("outside_right", W + 3.0, 1.0, W + 12.0, 8.0)]
    return [(n, i % B, x1, y1, x2, y2) for i, (n, x1, y1, x2, y2) in enumerate(rows)]


def edge_zoo_named(B, H, W, scale):
    """[(name, [b, x1, y1, x2, y2] in image units)]: one row per edge.  The exact-coordinate rows are built for 7 bins at sampling_ratio 2
    (bin size 1, samples at +0.25 and +0.75); `scale` is a power of two, so the division below and the kernel's multiplication are exact."""
    cy, cx = H / 2.0, W / 2.0
    rows = outside_rows(B, H, W, scale)

    def add(name, x1, y1, x2, y2, b=None):
        rows.append((name, len(rows) % B if b is None else b, x1, y1, x2, y2))

    # straddling: some samples rejected (< -1 or > L), some clamped from [-1, 0] to 0, some on the last pixel
    add("straddle_top", 1.0, -3.3, 8.3, 3.9)
    add("straddle_bottom", 1.0, H - 3.7, 8.3, H + 3.4)
    add("straddle_left", -3.3, 0.5, 3.9, 7.1)
    add("straddle_right", W - 3.7, 0.5, W + 3.4, 7.1)
    add("straddle_corner", -2.6, -2.6, 2.1, 2.1)
    # y = -1.25 + 0 * 1 + 0.5 * 1 / 2 = -1.0 exactly: kept (the test is v < -1), clamped to 0
    add("sample_at_minus_one_y", 2.0, -1.25, 9.0, 5.75)
    add("sample_at_minus_one_x", -1.25, 2.0, 5.75, 9.0)
    # bin 6, sample 0: (H - 6.25) + 6 + 0.25 = H exactly: kept (the test is v > H), clamped to the last row with weight 1
    add("sample_at_H", 2.0, H - 6.25, 9.0, H + 0.75)
    add("sample_at_W", W - 6.25, 2.0, W + 0.75, 9.0)
    # bin size 2, samples at 1.5 + 2 p + {0.5, 1.5}: every sample on a pixel centre, the high taps weigh exactly 0
    add("integer_aligned", 1.5, 1.5, 15.5, 15.5)
    add("reversed_corners", cx + 3.0, cy + 2.0, cx - 3.0, cy - 2.0)
    add("zero_size", cx, cy, cx, cy)
    add("sub_pixel", cx + 0.2, cy + 0.3, cx + 0.5, cy + 0.45)
    add("whole_image", 0.0, 0.0, float(W), float(H))
    ey, ex = max(H + 8.0, 71.0) / 2, max(W + 8.0, 71.0) / 2                 # 7 bins: adaptive grid >= 11 per axis, most of it rejected
    add("larger_than_image", cx - ex, cy - ey, cx + ex, cy + ey)
    # adaptive grids (7 bins) of 4 x 8 = 32, 3 x 11 = 33 and 8 x 8 = 64 samples: the forward's chunk of 32 samples per bin and both sides of it
    add("grid_32", cx - 26.0, cy - 12.5, cx + 26.0, cy + 12.5)
    add("grid_33", cx - 36.5, cy - 9.0, cx + 36.5, cy + 9.0)
    add("grid_64", cx - 26.5, cy - 26.0, cx + 26.5, cy + 26.0)
    add("first_pixel", 0.0, 0.0, 1.0, 1.0)
    add("last_pixel", W - 1.0, H - 1.0, float(W), float(H))
    add("first_row", 0.0, 0.0, float(W), 1.0)
    add("last_row", 0.0, H - 1.0, float(W), float(H))
    add("first_column", 0.0, 0.0, 1.0, float(H))
    add("last_column", W - 1.0, 0.0, float(W), float(H))
    for i in range(300):
        add(f"same_roi_{i}", cx - 2.3, cy - 1.9, cx + 3.1, cy + 2.2, b=B - 1)
    return [(n, [b, x1 / scale, y1 / scale, x2 / scale, y2 / scale]) for n, b, x1, y1, x2, y2 in rows]


def edge_zoo(B, H, W, scale):
    return np.array([r for _, r in edge_zoo_named(B, H, W, scale)], np.float32).reshape(-1, 5)


def edge_zoo_names(B, H, W, scale):
    return [n for n, _ in edge_zoo_named(B, H, W, scale)]


def outside(B, H, W, scale):
    return np.array([[b, x1 / scale, y1 / scale, x2 / scale, y2 / scale] for _, b, x1, y1, x2, y2 in outside_rows(B, H, W, scale)], np.float32)


def layouts(B, H, W, scale):
    """{name: rois}: every RoI on one image (the others have none), a single RoI, no RoI at all"""
    one = random_rois(1, H, W, scale, 24, seed=11)
    one[:, 0] = B // 2
    single = random_rois(1, H, W, scale, 1, seed=12)
    single[:, 0] = B - 1
    return {"one_image": one, "one_roi": single, "empty": np.zeros((0, 5), np.float32)}


def rois_for(kind, B, H, W, scale):
    """the RoI sets the cases name: 'zoo', 'random', 'mixed' (zoo + random) and the three layouts"""
    if kind == "zoo":
        return edge_zoo(B, H, W, scale)
    if kind == "random":
        return random_rois(B, H, W, scale, 48)
    if kind == "mixed":
        return np.concatenate([edge_zoo(B, H, W, scale), random_rois(B, H, W, scale, 16)])
    if kind == "full":
        return random_rois(B, H, W, scale, 512)
    return layouts(B, H, W, scale)[kind]


# --------------------------------------------------------------------------------------------------------------------- cases
class Case(namedtuple("Case", "rois B H W C PH PW sr scale step")):
    """one operator call: the RoI set's name, the map, the pooler.  Inputs are seeded by the case itself."""

    @property
    def id(self):
        s = {1.0: "1", 0.25: "4", 0.125: "8", 0.0625: "16"}[self.scale]
        return f"{self.rois}-B{self.B}-{self.H}x{self.W}x{self.C}-p{self.PH}x{self.PW}-sr{self.sr}-s{s}-step{self.step}"

    @property
    def pooled(self):
        return -(-self.PH // self.step), -(-self.PW // self.step)

    def make_rois(self):
        return rois_for(self.rois, self.B, self.H, self.W, self.scale)

    def make_feat(self):
        rng = np.random.default_rng(_seed("feat", *self))
        return rng.standard_normal((self.B, self.H, self.W, self.C)).astype(np.float32)

    def make_grad(self, K):
        rng = np.random.default_rng(_seed("grad", *self))
        return rng.standard_normal((K,) + self.pooled + (self.C,)).astype(np.float32)


def case(rois="mixed", B=2, H=38, W=63, C=24, P=7, sr=0, scale=0.0625, step=1):
    PH, PW = (P, P) if isinstance(P, int) else P
    return Case(rois, B, H, W, C, PH, PW, sr, scale, step)


# The cross-section both suites walk (not the full product).  tests/test_gpu_roi_align.py says which kernel and launch shape each row reaches.
CASES = [
    # channel counts on the model's map: VEC = 1 (C % 4 != 0), every pick_shape outcome, cslices 1 and 8, gather chunk counts 1, 2, 4, 6, 8
    case(C=1), case(C=3), case(C=4), case(C=5), case(C=20), case(C=24), case(C=252), case(C=256), case(C=260),
    case(C=512, rois="random"), case(C=1024, rois="mixed"), case(C=1536, rois="random"), case(C=2048, rois="random"),
    case(C=1024, H=5, W=5, rois="mixed"), case(C=2048, H=5, W=5, rois="random"),      # C >= 1024 on a map under 2 MiB: not sliced
    case(C=70, rois="random"), case(C=250, rois="random"), case(C=514, rois="random"),  # VEC = 1 past 32 lanes, and in more than one pass
    # maps: H or W of 1, W under / on / over the 8-pixel x-tile, odd extents
    case(H=1, W=1, C=8), case(H=1, W=9, C=8), case(H=9, W=1, C=8), case(H=7, W=8, C=8), case(H=7, W=9, C=8), case(H=13, W=21, C=8),
    case(H=5, W=7, C=8, B=3),
    case(H=1, W=1, C=3), case(H=7, W=9, C=6),
    # pooled sizes and bin_step
    case(P=14, C=8), case(P=14, C=256, rois="random"), case(P=(3, 5), C=8), case(P=1, C=8), case(P=8, C=8), case(P=9, C=8), case(P=9, C=5),
    case(P=7, C=8, step=2), case(P=8, C=8, step=2), case(P=14, C=8, step=2), case(P=7, C=512, step=2, rois="random"), case(P=7, C=6, step=2),
    # sampling ratios and scales
    case(sr=1, C=8), case(sr=2, C=8), case(sr=3, C=8), case(sr=2, C=6), case(sr=2, P=14, C=12),
    case(scale=0.125, C=8, sr=2), case(scale=0.25, C=8), case(scale=1.0, C=8, sr=2),
    # RoI layouts
    case(rois="one_image", B=3, C=8), case(rois="one_roi", B=3, C=8), case(rois="empty", B=2, C=8),
    case(rois="one_image", B=3, C=256, step=2), case(rois="one_roi", B=2, C=5),
]
assert len({c.id for c in CASES}) == len(CASES)

"""numpy references of ROIPool and deformable PS-RoI pooling and the seeded case builders their suites share (tests/test_roi_pool_ref.py on the
CPU, tests/test_gpu_roi_pool.py and tests/test_gpu_deform_roi_pool.py on the GPU).  Nothing here imports the library under test; `check`,
`worst_ratio`, `random_rois` and the seeding helper are tests/roi_align_ref.py's.

ROIPool (csrc/cuda/ROIPool_cuda.cu:16-108 of the reference)
  * GEOMETRY is restated op by op in np.float32 (np.float64 behind `dtype`, the reference's double instantiation): corners rounded half away
    from zero, +1 lengths, bin = len / P, floor(ph * bin) and ceil((ph + 1) * bin) with ONE rounded product each, the RoI start added afterwards,
    clipped to the map.  `exact=True` gives the integer-exact borders floor(ph * len / P), ceil((ph + 1) * len / P) instead: the two differ on a few
    rows (tests/test_roi_pool_ref.py pins them), and the float32 ones are the contract.
  * VALUES are the map's own, so float64 holds them exactly; gradients and S, the sum of |addends|, are float64.

Deformable PS-RoI pooling (csrc/cuda/deform_pool_kernel_cuda.cu:54-264), float64 throughout; spatial_scale and trans_std are first rounded to
float32, the type the entry points take them in.  `dtype` = np.float32 gives the honest float32 restatement the CPU suite measures the bounds
with: float64 sample coordinates (the kernels compute them in double, see csrc/roi_pool.hip), fractions and bilinear weights formed in float64 and rounded once to float32, float32 after that.
Per output: out, count, S (sum of |addends| / count, times the sigmoid), n (addends) and
`near`: some sample of the output lies within NEAR of one of the four accept boundaries, where float32 and float64 may decide differently.
The part cell and the group cell of a bin are the CUDA kernel's float32 expressions, floor(float(ph) / P * part) and floor(float(ph) * G / P),
like the kernels' -- tests/test_roi_pool_ref.py asserts that they are the exact integers ph * part // P and ph * G // P for every (P, part, G)
the suites use, and lists where they are not (P = part = 22 and 23).
"""
from collections import namedtuple

import numpy as np

from roi_align_ref import TOL, _seed, random_rois

FLT_MAX = float(np.finfo(np.float32).max)
NEAR = 1e-4
EPS24 = 2.0 ** -24


def tol_of(n):
    """max(TOL, (n + 8) 2^-24): the project's rule, or the worst case of an n-term float32 sum of products in any order"""
    return np.maximum(TOL, (np.asarray(n, np.float64) + 8.0) * EPS24)


def scaled(S, n):
    """S scaled so that roi_align_ref.check(got, want, scaled(S, n)) (tolerance TOL) applies tol_of(n) * S element-wise"""
    return np.asarray(S, np.float64) * (tol_of(n) / TOL)


def round_half_away(v):
    t = np.trunc(v)
    return t + np.sign(v) * (np.abs(v - t) >= 0.5)   # v - trunc(v) is exact


# ===================================================================================================================== ROIPool
PoolBins = namedtuple("PoolBins", "b hs he ws we")   # hs, he [K, PH]; ws, we [K, PW]: clipped, [start, end)


def pool_bins(rois, scale, PH, PW, H, W, dtype=np.float32, exact=False):
    ft = np.dtype(dtype).type
    r = np.asarray(rois)
    rr, s = r.astype(ft), ft(scale)
    sw, sh, ew, eh = (round_half_away(rr[:, i] * s).astype(np.int64) for i in (1, 2, 3, 4))
    rw, rh = np.maximum(ew - sw + 1, 1), np.maximum(eh - sh + 1, 1)

    def axis(length, start, P, L):
        p = np.arange(P)
        if exact:
            lo = (p[None, :] * length[:, None]) // P
            hi = -((-(p[None, :] + 1) * length[:, None]) // P)
        else:
            binsz = length.astype(ft) / ft(P)
            a, b = p.astype(ft)[None, :] * binsz[:, None], (p + 1).astype(ft)[None, :] * binsz[:, None]
            assert a.dtype == b.dtype == np.dtype(dtype)
            lo, hi = np.floor(a).astype(np.int64), np.ceil(b).astype(np.int64)
        return np.clip(lo + start[:, None], 0, L), np.clip(hi + start[:, None], 0, L)

    hs, he = axis(rh, sh, PH, H)
    ws, we = axis(rw, sw, PW, W)
    return PoolBins(r[:, 0].astype(np.int64), hs, he, ws, we)


def pool_forward(feat, rois, scale, PH, PW, dtype=np.float32):
    """feat [B, H, W, C], rois [K, 5] -> (out float64 [K, PH, PW, C], argmax int32 [K, PH, PW, C]): row-major scan with strict > from -FLT_MAX --
    the first maximum wins, NaN never does; an empty bin gives (0, -1), a bin without a value above -FLT_MAX gives (-FLT_MAX, -1)"""
    B, H, W, C = feat.shape
    q = pool_bins(rois, scale, PH, PW, H, W, dtype)
    K = len(q.b)
    f = np.asarray(feat, np.float64)
    out = np.zeros((K, PH, PW, C), np.float64)
    arg = np.full((K, PH, PW, C), -1, np.int32)
    for k in range(K):
        for ph in range(PH):
            h0, h1 = q.hs[k, ph], q.he[k, ph]
            for pw in range(PW):
                w0, w1 = q.ws[k, pw], q.we[k, pw]
                if h1 <= h0 or w1 <= w0:
                    continue
                v = f[q.b[k], h0:h1, w0:w1].reshape(-1, C)
                pix = (np.arange(h0, h1)[:, None] * W + np.arange(w0, w1)[None, :]).reshape(-1)
                with np.errstate(invalid="ignore"):
                    cand = v > -FLT_MAX                                  # NaN and -inf never replace the initial value
                first = np.where(cand, v, -np.inf).argmax(0)             # argmax returns the FIRST maximum
                hit = cand.any(0)
                out[k, ph, pw] = np.where(hit, v[first, np.arange(C)], -FLT_MAX)
                arg[k, ph, pw] = np.where(hit, pix[first], -1)
    return out, arg


def pool_backward(grad, rois, argmax, B, H, W, dtype=np.float64):
    """grad, argmax [K, PH, PW, C] -> (grad_feat, S, n) [B, H, W, C]: grad_feat[b, argmax] += grad wherever argmax != -1; `dtype` float32 adds
    sequentially in float32 (the honest restatement)"""
    K, PH, PW, C = grad.shape
    g = np.asarray(grad, dtype)
    b = np.asarray(rois)[:, 0].astype(np.int64)
    out, S, n = np.zeros((B, H * W, C), dtype), np.zeros((B, H * W, C), np.float64), np.zeros((B, H * W, C), np.int64)
    kk, pp, qq, cc = np.nonzero(np.asarray(argmax) != -1)
    at = (b[kk], np.asarray(argmax)[kk, pp, qq, cc].astype(np.int64), cc)
    np.add.at(out, at, g[kk, pp, qq, cc])
    np.add.at(S, at, np.abs(np.asarray(grad, np.float64))[kk, pp, qq, cc])
    np.add.at(n, at, 1)
    return out.reshape(B, H, W, C), S.reshape(B, H, W, C), n.reshape(B, H, W, C)


# the rows on which float32 and integer-exact bin borders differ, for P in {2, 3, 5, 6, 7, 14} and lengths 1 .. 63: (P, length, bin, which border)
DISCRIMINATING = [(7, 57, 6, "end"), (14, 57, 13, "end"), (14, 62, 7, "start")]


def length_rows(scale=0.0625, lo=1, hi=63):
    """one RoI per length lo .. hi along x (and 1 + (length % 7) along y), starting at pixel 0: rois whose scaled corners are integers"""
    rows = [[i % 2, 0.0, 0.0, (n - 1) / scale, (n % 7) / scale] for i, n in enumerate(range(lo, hi + 1))]
    return np.array(rows, np.float32)


def rounding_rows(scale=0.0625):
    """corners at +-8 and +-24 image pixels: +-0.5 and +-1.5 map pixels, which round half away from zero to +-1 and +-2 (rintf gives 0 and +-2)"""
    rows = []
    for a in (8.0, -8.0, 24.0, -24.0):
        rows.append([0, a, a, a + 5 / scale, a + 4 / scale])
        rows.append([1, 3 / scale, 2 / scale, 9 / scale + a, 7 / scale + a])
    return np.array(rows, np.float32)


def pool_rois(kind, B, H, W, scale):
    if kind == "lengths":
        return length_rows(scale)
    if kind == "rounding":
        return rounding_rows(scale)
    if kind == "malformed":      # x2 < x1 and / or y2 < y1
        return np.array([[0, 20, 10, 5, 30], [1, 4, 30, 40, 6], [0, 30, 30, 2, 2], [1, 9, 9, 8, 8]], np.float32) / np.array([1] + [scale] * 4, np.float32)
    if kind == "outside":        # wholly outside the map: every bin empty
        return np.array([[0, -30, 2, -9, 9], [1, W + 5, 2, W + 20, 9], [0, 2, -30, 9, -9], [1, 2, H + 5, 9, H + 20]], np.float32) / np.array([1] + [scale] * 4, np.float32)
    if kind == "one_image":      # image 0 has no RoI
        r = random_rois(1, H, W, scale, 12, seed=21)
        r[:, 0] = B - 1
        return r
    if kind == "empty":
        return np.zeros((0, 5), np.float32)
    if kind == "random":
        return random_rois(B, H, W, scale, 24, seed=22)
    if kind == "mixed":
        return np.concatenate([pool_rois(k, B, H, W, scale) for k in ("rounding", "malformed", "outside", "random")])
    raise KeyError(kind)


class PoolCase(namedtuple("PoolCase", "rois B H W C PH PW scale feat")):
    @property
    def id(self):
        return f"{self.rois}-{self.H}x{self.W}x{self.C}-p{self.PH}x{self.PW}-{self.feat}"

    def make_rois(self):
        return pool_rois(self.rois, self.B, self.H, self.W, self.scale)

    def make_feat(self):
        shape = (self.B, self.H, self.W, self.C)
        rng = np.random.default_rng(_seed("pool_feat", *self))
        if self.feat == "const":       # every bin ties: argmax must be the bin's first pixel
            return np.full(shape, 0.75, np.float32)
        if self.feat == "neginf":
            return np.full(shape, -np.inf, np.float32)
        f = rng.standard_normal(shape).astype(np.float32)
        if self.feat == "nan":         # one NaN pixel (all channels), in the middle of the map
            f[:, self.H // 2, self.W // 2] = np.nan
        if self.feat == "ties":        # few distinct values: many ties inside a bin
            f = np.round(f)
        return f

    def make_grad(self, K):
        rng = np.random.default_rng(_seed("pool_grad", *self))
        return rng.standard_normal((K, self.PH, self.PW, self.C)).astype(np.float32)


def pool_case(rois="mixed", B=2, H=38, W=63, C=8, P=7, scale=0.0625, feat="normal"):
    PH, PW = (P, P) if isinstance(P, int) else P
    return PoolCase(rois, B, H, W, C, PH, PW, scale, feat)


POOL_CASES = [
    pool_case("lengths", P=7), pool_case("lengths", P=14),                               # the three discriminating rows
    pool_case("rounding"), pool_case("malformed"), pool_case("outside"), pool_case("one_image"), pool_case("empty"),
    pool_case(C=1), pool_case(C=3), pool_case(C=4), pool_case(C=5), pool_case(C=24), pool_case("random", C=256), pool_case("random", C=260),
    pool_case(P=(3, 5)), pool_case("random", H=20, W=30, C=12),
    pool_case(feat="const"), pool_case(feat="neginf"), pool_case(feat="nan"), pool_case(feat="ties", C=5),
]
assert len({c.id for c in POOL_CASES}) == len(POOL_CASES)


# ===================================================================================================================== PS-RoI pooling
def ps_cells(P, part, G):
    """(part cell, group cell) of every bin index along one axis, as the CUDA kernel computes them with scalar_t = float
    (deform_pool_kernel_cuda.cu:100-101,113-116): floor(float(ph) / P * part) and floor(float(ph) * G / P), op by op in float32"""
    ft = np.float32
    p = np.arange(P).astype(ft)
    return np.floor(p / ft(P) * ft(part)).astype(np.int64), np.clip(np.floor(p * ft(G) / ft(P)).astype(np.int64), 0, G - 1)


def ps_cells_exact(P, part, G):
    """the exact integers ph * part // P and ph * G // P: what the float32 expressions mean, and give for every (P, part, G) of the suites"""
    p = np.arange(P)
    return p * part // P, np.clip(p * G // P, 0, G - 1)


PsGeom = namedtuple("PsGeom", "b ncls rw rh w h ok near x1 x2 y1 y2 dx dy clamped on_boundary")


def ps_geometry(rois, trans, H, W, scale, P, part, spp, tstd, dtype=np.float64):
    """sample arrays [K, ncls, P (ph), P (pw), spp (ih), spp (iw)]; near [K, ncls, P, P]; rw, rh [K]"""
    ft = np.dtype(dtype).type
    r = np.asarray(rois).astype(ft)
    K, s = len(r), ft(np.float32(scale))
    x0, y0 = round_half_away(r[:, 1]) * s - ft(0.5), round_half_away(r[:, 2]) * s - ft(0.5)
    xe, ye = (round_half_away(r[:, 3]) + ft(1)) * s - ft(0.5), (round_half_away(r[:, 4]) + ft(1)) * s - ft(0.5)
    rw, rh = np.maximum(xe - x0, ft(0.1)), np.maximum(ye - y0, ft(0.1))
    bw, bh = rw / ft(P), rh / ft(P)
    sbw, sbh = bw / ft(spp), bh / ft(spp)
    pc, _ = ps_cells(P, part, 1)
    if trans is None:
        ncls = 1
        tx = ty = np.zeros((K, 1, P, P), ft)
    else:
        t = np.asarray(trans).astype(ft)
        ncls = t.shape[1] // 2
        tx = t[:, 0::2][:, :, pc[:, None], pc[None, :]] * ft(np.float32(tstd))
        ty = t[:, 1::2][:, :, pc[:, None], pc[None, :]] * ft(np.float32(tstd))
    p = np.arange(P).astype(ft)
    e4 = (slice(None), None, None, None)
    ws = p[None, None, None, :] * bw[e4] + x0[e4]
    ws = ws + tx * rw[e4]
    hs = p[None, None, :, None] * bh[e4] + y0[e4]
    hs = hs + ty * rh[e4]
    i = np.arange(spp).astype(ft)
    e6 = (slice(None), None, None, None, None, None)
    w = ws[..., None, None] + i[None, None, None, None, None, :] * sbw[e6]
    h = hs[..., None, None] + i[None, None, None, None, :, None] * sbh[e6]
    w, h = np.broadcast_arrays(w, h)
    assert w.dtype == h.dtype == np.dtype(dtype)
    lo, wx, hx = ft(-0.5), ft(W - 0.5), ft(H - 0.5)
    ok = ~((w < lo) | (w > wx) | (h < lo) | (h > hx))
    dist = np.minimum(np.minimum(np.abs(w - lo), np.abs(w - wx)), np.minimum(np.abs(h - lo), np.abs(h - hx)))
    wc, hc = np.clip(w, ft(0), ft(W - 1)), np.clip(h, ft(0), ft(H - 1))
    x1, x2, y1, y2 = np.floor(wc), np.ceil(wc), np.floor(hc), np.ceil(hc)
    return PsGeom(np.asarray(rois)[:, 0].astype(np.int64), ncls, rw, rh, w, h, ok, (dist < NEAR).any((-1, -2)), x1.astype(np.int64),
                  x2.astype(np.int64), y1.astype(np.int64), y2.astype(np.int64), wc - x1, hc - y1, ok & ((wc != w) | (hc != h)), dist == 0)


def _sum_last(v, order):
    """sum over the last axis: numpy's float64 sum, or dtype-preserving sequential / pairwise sums"""
    if order == "seq":
        acc = np.zeros(v.shape[:-1], v.dtype)
        for j in range(v.shape[-1]):
            acc = acc + v[..., j]
        return acc
    if order == "pair":
        while v.shape[-1] > 1:
            if v.shape[-1] % 2:
                v = np.concatenate([v, np.zeros(v.shape[:-1] + (1,), v.dtype)], -1)
            v = v[..., 0::2] + v[..., 1::2]
        return v[..., 0]
    raise KeyError(order)


def _ps_taps(F, g, cls, src):
    """the four taps of every sample of class `cls` for the channels src [P, P, n]: each [K, P, P, spp, spp, n]"""
    b = g.b[:, None, None, None, None, None]
    c = src[None, :, :, None, None, :]
    y1, y2, x1, x2 = (a[:, cls][..., None] for a in (g.y1, g.y2, g.x1, g.x2))
    return F[b, y1, x1, c], F[b, y2, x1, c], F[b, y1, x2, c], F[b, y2, x2, c]   # v11, v12 = (y2, x1), v21 = (y1, x2), v22


def _sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


PsOut = namedtuple("PsOut", "out count S n near raw Sraw")


def psroi_forward(feat, rois, trans, mask_logits, scale, OD, G, P, part, spp, tstd, dtype=np.float64, order="seq", geom_dtype=np.float64):
    """feat [B, H, W, C], rois [K, 5], trans [K, 2 ncls, part, part] or None, mask_logits [K, P, P] or None -> PsOut of [K, P, P, OD] arrays.
    dtype float32: the fractions rounded to float32, then weights, products and sums (`order`: 'seq' or 'pair') in float32 -- over float64
    sample coordinates, as the kernels compute them, unless geom_dtype says float32 too"""
    ft = np.dtype(dtype).type
    B, H, W, C = feat.shape
    g = ps_geometry(rois, trans, H, W, scale, P, part, spp, tstd, geom_dtype)
    K, cec = len(g.b), OD // g.ncls
    _, gc = ps_cells(P, part, G)
    F = np.asarray(feat).astype(ft)
    ctop = np.arange(OD)
    src_all = (ctop[None, None, :] * G + gc[:, None, None]) * G + gc[None, :, None]
    raw, Sraw = np.zeros((K, P, P, OD), ft), np.zeros((K, P, P, OD), np.float64)
    count, near = np.zeros((K, P, P, OD), np.float64), np.zeros((K, P, P, OD), bool)
    one = ft(1)
    for cls in range(g.ncls):
        sel = np.arange(cls * cec, (cls + 1) * cec)
        v11, v12, v21, v22 = _ps_taps(F, g, cls, src_all[:, :, sel])
        dx, dy, ok = g.dx[:, cls][..., None], g.dy[:, cls][..., None], g.ok[:, cls][..., None]
        w11, w12, w21, w22 = (((1 - dx) * (1 - dy)).astype(ft), ((1 - dx) * dy).astype(ft), (dx * (1 - dy)).astype(ft), (dx * dy).astype(ft))
        val = np.where(ok, w11 * v11 + w12 * v12 + w21 * v21 + w22 * v22, ft(0))
        aval = np.where(ok, (w11 * np.abs(v11) + w12 * np.abs(v12) + w21 * np.abs(v21) + w22 * np.abs(v22)).astype(np.float64), 0.0)
        cnt = g.ok[:, cls].sum((-1, -2))[..., None]                                       # [K, P, P, 1]
        tot = _sum_last(np.moveaxis(val.reshape(K, P, P, spp * spp, cec), 3, -1), order)
        with np.errstate(invalid="ignore", divide="ignore"):
            raw[..., sel] = np.where(cnt > 0, tot / cnt.astype(ft), ft(0))
            Sraw[..., sel] = np.where(cnt > 0, aval.sum((3, 4)) / cnt, 0.0)
        count[..., sel] = cnt
        near[..., sel] = g.near[:, cls][..., None]
    sig = one if mask_logits is None else _sigmoid(np.asarray(mask_logits).astype(np.float64)).astype(ft)[..., None]   # formed in double, rounded once
    return PsOut(raw * sig, count, Sraw * np.asarray(sig, np.float64), 4 * count, near, raw, Sraw)


PsGrads = namedtuple("PsGrads", "gfeat Sfeat nfeat gtrans Strans ntrans glogits Slogits nlogits")


def psroi_backward(gout, feat, rois, trans, mask_logits, scale, OD, G, P, part, spp, tstd, dtype=np.float64):
    """the exact transpose of psroi_forward in `feat`, and the CUDA kernel's analytic gradients of the offsets (:254-257) and of the mask logits
    (sigma (1 - sigma) sum_c g raw); each with S = sum of |addends| and n = their number"""
    ft = np.dtype(dtype).type
    B, H, W, C = feat.shape
    g = ps_geometry(rois, trans, H, W, scale, P, part, spp, tstd)
    fwd = psroi_forward(feat, rois, trans, None, scale, OD, G, P, part, spp, tstd, dtype)
    K, cec = len(g.b), OD // g.ncls
    pc, gc = ps_cells(P, part, G)
    F = np.asarray(feat).astype(ft)
    go = np.asarray(gout).astype(ft)
    ctop = np.arange(OD)
    src_all = (ctop[None, None, :] * G + gc[:, None, None]) * G + gc[None, :, None]
    one = ft(1)
    sig = 1.0 if mask_logits is None else _sigmoid(np.asarray(mask_logits).astype(np.float64))[..., None]       # float64 in every dtype
    gfeat, Sfeat, nfeat = np.zeros((B, H, W, C), ft), np.zeros((B, H, W, C), np.float64), np.zeros((B, H, W, C), np.int64)
    gtrans = Strans = ntrans = None
    if trans is not None:
        gtrans, Strans, ntrans = np.zeros(np.shape(trans), ft), np.zeros(np.shape(trans), np.float64), np.zeros(np.shape(trans), np.int64)
    m, Sm, nm = np.zeros((K, P, P), ft), np.zeros((K, P, P), np.float64), np.zeros((K, P, P), np.int64)
    kk = np.arange(K)[:, None, None]
    cell = (kk + 0 * pc[None, :, None] + 0 * pc[None, None, :], pc[None, :, None] + 0 * kk + 0 * pc[None, None, :],
            pc[None, None, :] + 0 * kk + 0 * pc[None, :, None])
    for cls in range(g.ncls):
        sel = np.arange(cls * cec, (cls + 1) * cec)
        src = src_all[:, :, sel]
        v11, v12, v21, v22 = _ps_taps(F, g, cls, src)
        dx, dy, ok = g.dx[:, cls][..., None], g.dy[:, cls][..., None], g.ok[:, cls][..., None]
        weights64 = ((1 - dx) * (1 - dy), (1 - dx) * dy, dx * (1 - dy), dx * dy)
        weights = tuple(w.astype(ft) for w in weights64)
        dx, dy, ex, ey = dx.astype(ft), dy.astype(ft), (1 - dx).astype(ft), (1 - dy).astype(ft)
        cnt = g.ok[:, cls].sum((-1, -2))[..., None]
        with np.errstate(invalid="ignore", divide="ignore"):
            # g sigma / count formed in double and rounded once to `dtype`                                [K, P, P, 1, 1, cec]
            dv = np.where(cnt > 0, (go[..., sel].astype(np.float64) * sig / cnt).astype(ft), ft(0))[:, :, :, None, None, :]
        b = np.broadcast_to(g.b[:, None, None, None, None, None], v11.shape)
        c = np.broadcast_to(src[None, :, :, None, None, :], v11.shape)
        okb = np.broadcast_to(ok, v11.shape)
        # float64: every tap of every sample is an addend (they also define S and n).  The restatement (another dtype) adds what the
        # kernel adds: per bin and pixel ONE addend, the bin's weights on that pixel summed in double and rounded once, times dv
        per_pixel = np.zeros((K, P, P, H, W), np.float64) if ft is not np.float64 else None
        ok5 = g.ok[:, cls]
        k5, ph5, pw5 = (np.broadcast_to(a, ok5.shape) for a in (np.arange(K)[:, None, None, None, None], np.arange(P)[None, :, None, None, None],
                                                                 np.arange(P)[None, None, :, None, None]))
        for q64, q, yy, xx in zip(weights64, weights, (g.y1, g.y2, g.y1, g.y2), (g.x1, g.x1, g.x2, g.x2)):
            add = np.where(okb, q * dv, ft(0))
            at = (b[okb], np.broadcast_to(yy[:, cls][..., None], v11.shape)[okb], np.broadcast_to(xx[:, cls][..., None], v11.shape)[okb], c[okb])
            if per_pixel is None:
                np.add.at(gfeat, at, add[okb])
            else:
                np.add.at(per_pixel, (k5[ok5], ph5[ok5], pw5[ok5], yy[:, cls][ok5], xx[:, cls][ok5]), q64[..., 0][ok5])
            np.add.at(Sfeat, at, np.abs(add[okb]).astype(np.float64))
            np.add.at(nfeat, at, 1)
        if per_pixel is not None:
            k_, ph_, pw_, y_, x_ = np.nonzero(per_pixel)
            add = per_pixel[k_, ph_, pw_, y_, x_].astype(ft)[:, None] * dv[k_, ph_, pw_, 0, 0, :]
            np.add.at(gfeat, (g.b[k_][:, None], y_[:, None], x_[:, None], src[ph_, pw_, :]), add)
        if trans is not None:
            rw, rh = g.rw.astype(ft)[:, None, None, None, None, None], g.rh.astype(ft)[:, None, None, None, None, None]
            ts = ft(np.float32(tstd))
            ddx = np.where(okb, (v22 * dy + v21 * ey - v12 * dy - v11 * ey) * ts * dv * rw, ft(0))
            ddy = np.where(okb, (v22 * dx + v12 * ex - v21 * dx - v11 * ex) * ts * dv * rh, ft(0))
            adx = np.where(okb, (np.abs(v22) * dy + np.abs(v21) * ey + np.abs(v12) * dy + np.abs(v11) * ey) * ts * np.abs(dv) * rw, 0.0)
            ady = np.where(okb, (np.abs(v22) * dx + np.abs(v12) * ex + np.abs(v21) * dx + np.abs(v11) * ex) * ts * np.abs(dv) * rh, 0.0)
            nadd = (4 * cnt[..., 0] * cec).astype(np.int64)
            for xy, d, a in ((0, ddx, adx), (1, ddy, ady)):
                np.add.at(gtrans[:, 2 * cls + xy], cell, d.sum((3, 4, 5)))
                np.add.at(Strans[:, 2 * cls + xy], cell, a.astype(np.float64).sum((3, 4, 5)))
                np.add.at(ntrans[:, 2 * cls + xy], cell, nadd)
        m += (go[..., sel] * fwd.raw[..., sel]).sum(-1)
        Sm += (np.abs(go[..., sel]).astype(np.float64) * fwd.Sraw[..., sel]).sum(-1)
        nm += ((4 * cnt[..., 0] + 1) * cec).astype(np.int64)
    glogits = Slogits = nlogits = None
    if mask_logits is not None:
        s1 = sig[..., 0]
        glogits, Slogits, nlogits = (s1 * (1.0 - s1)).astype(ft) * m, s1 * (1.0 - s1) * Sm, nm
    return PsGrads(gfeat, Sfeat, nfeat, gtrans, Strans, ntrans, glogits, Slogits, nlogits)


class PsCase(namedtuple("PsCase", "family B H W OD G P spp part tstd ncls mask seed")):
    """one deformable PS-RoI pooling call.  family 'random': random_rois-style boxes (24 per image), offsets uniform in [-1, 1];
    family 'dyadic': every coordinate a short dyadic rational, so that float32 and float64 evaluate the same sample coordinates"""

    scale = 0.0625

    @property
    def id(self):
        t = "notrans" if self.ncls == 0 else f"cls{self.ncls}"
        return f"{self.family}-{self.H}x{self.W}-od{self.OD}-g{self.G}-p{self.P}s{self.spp}q{self.part}-t{self.tstd}-{t}{'-mask' if self.mask else ''}"

    @property
    def C(self):
        return self.OD * self.G * self.G

    def rng(self, what):
        return np.random.default_rng(_seed("ps", what, *self))

    def make_rois(self):
        if self.family == "random":
            return random_rois(self.B, self.H, self.W, self.scale, 24, seed=self.seed)
        rng = self.rng("rois")
        rows = []
        for b in range(self.B):
            for _ in range(10):
                x1, y1 = 16 * rng.integers(-1, self.W), 16 * rng.integers(-1, self.H)
                sw, sh = 16 * 2 ** rng.integers(0, 4), 16 * 2 ** rng.integers(0, 4)
                rows.append([b, x1, y1, x1 + sw - 1, y1 + sh - 1])
        return np.array(rows, np.float32)

    def make_feat(self):
        return self.rng("feat").standard_normal((self.B, self.H, self.W, self.C)).astype(np.float32)

    def make_trans(self, K):
        if self.ncls == 0:
            return None
        shape = (K, 2 * self.ncls, self.part, self.part)
        if self.family == "dyadic":
            return (self.rng("trans").integers(-8, 9, shape) / 8.0).astype(np.float32)
        return self.rng("trans").uniform(-1, 1, shape).astype(np.float32)

    def make_logits(self, K):
        return self.rng("logits").standard_normal((K, self.P, self.P)).astype(np.float32) if self.mask else None

    def make_grad(self, K):
        return self.rng("grad").standard_normal((K, self.P, self.P, self.OD)).astype(np.float32)

    def inputs(self):
        rois = self.make_rois()
        K = len(rois)
        return self.make_feat(), rois, self.make_trans(K), self.make_logits(K), self.make_grad(K)

    @property
    def args(self):
        return (self.scale, self.OD, self.G, self.P, self.part, self.spp, self.tstd)

    def excluded(self, near):
        """the outputs a float32 implementation is not held to: those flagged `near` in a random case; none in the dyadic family, whose
        coordinates are the same in every precision (its samples ON a boundary are what it is for)"""
        return np.zeros_like(near) if self.family == "dyadic" else near


def ps_case(family, H, W, P, spp, part, tstd, OD=8, G=1, ncls=1, mask=False, B=2, seed=0):
    return PsCase(family, B, H, W, OD, G, P, spp, part, tstd, ncls, mask, seed)


# (P, spp, part, trans_std) of the dyadic family: the issue's four
_DY = [(4, 2, 4, 0.25), (2, 4, 2, 0.5), (8, 2, 4, 0.125), (4, 4, 2, 0.25)]
DYADIC_CASES = [
    ps_case("dyadic", 6, 8, *_DY[0], ncls=0), ps_case("dyadic", 6, 8, *_DY[0]), ps_case("dyadic", 6, 8, *_DY[1], OD=16, ncls=2),
    ps_case("dyadic", 6, 8, *_DY[2], mask=True), ps_case("dyadic", 6, 8, *_DY[3], G=2), ps_case("dyadic", 6, 8, *_DY[1], OD=16, G=2, ncls=2, mask=True),
    ps_case("dyadic", 6, 8, *_DY[2], ncls=0, mask=True), ps_case("dyadic", 6, 8, *_DY[3], OD=16),
]
# P / spp / part of the random cases: 7/4/7, 7/2/7, 3/4/3, 8/4/4 on the two maps
RANDOM_CASES = [
    ps_case("random", 20, 30, 7, 4, 7, 0.1), ps_case("random", 38, 63, 7, 4, 7, 0.3, mask=True), ps_case("random", 20, 30, 7, 2, 7, 0.5, ncls=0),
    ps_case("random", 38, 63, 7, 2, 7, 0.2, OD=16, ncls=2), ps_case("random", 20, 30, 3, 4, 3, 0.4, G=2, mask=True),
    ps_case("random", 38, 63, 3, 4, 3, 0.1, OD=12), ps_case("random", 20, 30, 8, 4, 4, 0.25, OD=16, ncls=2, mask=True),
    ps_case("random", 38, 63, 8, 4, 4, 0.5, G=2),
]
PS_CASES = DYADIC_CASES + RANDOM_CASES
assert len({c.id for c in PS_CASES}) == len(PS_CASES)

"""Deformable PS-RoI pooling (abr_iod_amd/csrc/roi_pool.hip) against the float64 reference of tests/roi_pool_ref.py: `ops` (NHWC), `_C` (NCHW),
and the layers built on them.

Bound, per element: |got - want| <= max(TOL, (n + 8) 2^-24) * S with n the element's addend count and S the sum of their magnitudes, through
roi_align_ref.check (exactly 0 where nothing lands).  tests/test_roi_pool_ref.py shows on the CPU what meets it: float64 sample coordinates
(the kernels compute them in double), float32 after that.

  * the DYADIC family evaluates to the same coordinates in any precision, 1459 of its samples exactly on an accept boundary: top_count is
    equal everywhere, without exclusions;
  * the RANDOM cases: outputs the reference flags `near` (a sample within 1e-4 of an accept boundary, at most 0.07 % of a case) need only be
    finite; all others have equal top_count and values within the bound (worst measured: 0.19 of it forward, 0.15 for grad_feat);
  * backward on the same cases, flagged outputs' out_grad zeroed on both sides: grad_feat, grad_trans and grad_mask_logits within the bound,
    the latter two bit-equal across runs;
  * module level: DeformRoIPoolingPack and ModulatedDeformRoIPoolingPack (P 3, C 8, deform_fc_channels 16, K 6), stage by stage against float64
    with every stage fed what the GPU run fed it.  The FC stacks' bound is the contraction's own admitted one -- 32 ulp of sum |x||w| per
    contraction (tests/test_gpu_f16x3_admission.py: "within max(2 x the fp32 MFMA kernel's, 8 ulp) and below 32 ulp") --
    propagated through the stack on magnitudes (e' <= e |W|^T + 32 ulp |a| |W|^T), forward and backward.
"""
import functools

import numpy as np
import pytest
import torch

import roi_align_ref as R
import roi_pool_ref as P
from roi_align_ref import check
from roi_pool_ref import DYADIC_CASES, PS_CASES

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -24
FC_ULPS = 32.0


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return None if t is None else t.detach().cpu().numpy()


def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def nhwc(a):
    return np.ascontiguousarray(np.transpose(a, (0, 2, 3, 1)))


@functools.lru_cache(maxsize=None)
def fwd_ref(c):
    feat, rois, trans, logits, grad = c.inputs()
    return feat, rois, trans, logits, grad, P.psroi_forward(feat, rois, trans, logits, *c.args)


@functools.lru_cache(maxsize=None)
def bwd_ref(c):
    feat, rois, trans, logits, grad, want = fwd_ref(c)
    grad = np.where(c.excluded(want.near), 0, grad).astype(np.float32)          # flagged outputs contribute to neither side
    return grad, P.psroi_backward(grad, feat, rois, trans, logits, *c.args)


def fwd_check(out, count, c, what):
    want = fwd_ref(c)[5]
    out, count = np.asarray(out), np.asarray(count)
    assert np.isfinite(out).all(), f"{what} {c.id}: non-finite output"
    keep = ~c.excluded(want.near)
    bad = keep & (count != want.count)
    assert not bad.any(), f"{what} {c.id}: top_count differs at (k,ph,pw,c) = {np.argwhere(bad)[0]}: {count[bad][0]} vs {want.count[bad][0]}"
    got = np.where(keep, out, want.out)
    S = P.scaled(want.S, want.n)
    print(f"RATIO psroi fwd {what} {c.id} {R.worst_ratio(got, want.out, S) / R.TOL:.3f} of the bound ({int((~keep).sum())} outputs near a boundary)")
    check(got, want.out, S, f"{what} forward {c.id}")


@pytest.mark.parametrize("c", PS_CASES, ids=[c.id for c in PS_CASES])
def test_forward(c):
    from abr_iod_amd import _C, ops
    feat, rois, trans, logits = fwd_ref(c)[:4]
    out, count = ops.deform_psroi_forward(T(feat), T(rois), T(trans), *c.args, mask_logits=T(logits))
    fwd_check(N(out), N(count), c, "nhwc")
    if not c.mask:     # the reference's entry point has no mask operand
        K = len(rois)
        out = torch.full((K, c.OD, c.P, c.P), 7.0, device="cuda")
        count = torch.full((K, c.OD, c.P, c.P), 7.0, device="cuda")
        t = T(trans) if trans is not None else out.new_empty(0)
        _C.deform_psroi_pooling_forward(T(nchw(feat)), T(rois), t, out, count, trans is None, *c.args)
        fwd_check(nhwc(N(out)), nhwc(N(count)), c, "nchw")


def bwd_check(got, want, S, n, c, what, axes):
    got = np.asarray(got)
    S = P.scaled(S, n)
    print(f"RATIO psroi bwd {what} {c.id} {R.worst_ratio(got, want, S) / R.TOL:.3f} of the bound")
    check(got, want, S, f"{what} backward {c.id}", axes=axes)


@pytest.mark.parametrize("c", PS_CASES, ids=[c.id for c in PS_CASES])
def test_backward(c):
    from abr_iod_amd import _C, ops
    feat, rois, trans, logits = fwd_ref(c)[:4]
    grad, want = bwd_ref(c)
    tf, tr, tt, tl, tg = T(feat), T(rois), T(trans), T(logits), T(grad)
    _, count = ops.deform_psroi_forward(tf, tr, tt, *c.args, mask_logits=tl)
    runs = [ops.deform_psroi_backward(tg, tf, tr, tt, count, *c.args, mask_logits=tl) for _ in range(2)]
    gfeat, gtrans, glogits = runs[0]
    bwd_check(N(gfeat), want.gfeat, want.Sfeat, want.nfeat, c, "grad_feat", "b,y,x,c")
    assert (gtrans is None) == (trans is None) and (glogits is None) == (logits is None)
    if trans is not None:
        bwd_check(N(gtrans), want.gtrans, want.Strans, want.ntrans, c, "grad_trans", "k,c,py,px")
        assert torch.equal(gtrans, runs[1][1]), "grad_trans differs between two runs"
    if logits is not None:
        bwd_check(N(glogits), want.glogits, want.Slogits, want.nlogits, c, "grad_mask_logits", "k,ph,pw")
        assert torch.equal(glogits, runs[1][2]), "grad_mask_logits differs between two runs"
    if not c.mask:
        # _C: ADDS into a non-zero input_grad, writes trans_grad over whatever it held
        base = np.random.default_rng(4).standard_normal((c.B, c.C, c.H, c.W)).astype(np.float32)
        gin = T(base)
        t = tt if trans is not None else tf.new_empty(0)
        gt = torch.full_like(t, 9.0)
        cnt = T(nchw(N(count)))
        _C.deform_psroi_pooling_backward(T(nchw(grad)), T(nchw(feat)), tr, t, cnt, gin, gt, trans is None, *c.args)
        b64 = nhwc(base).astype(np.float64)
        bwd_check(nhwc(N(gin)), want.gfeat + b64, want.Sfeat + np.abs(b64), want.nfeat + 1, c, "_C input_grad", "b,y,x,c")
        if trans is not None:
            bwd_check(N(gt), want.gtrans, want.Strans, want.ntrans, c, "_C trans_grad", "k,c,py,px")


@pytest.mark.parametrize("c", [DYADIC_CASES[1], DYADIC_CASES[3]], ids=lambda c: c.id)
def test_autograd_function(c):
    from abr_iod_amd import layers
    feat, rois, trans, logits = fwd_ref(c)[:4]
    grad, want = bwd_ref(c)
    x, t = T(nchw(feat)).requires_grad_(True), T(trans).requires_grad_(True)
    m = None if logits is None else T(logits).requires_grad_(True)
    out = layers.deform_roi_pooling(x, T(rois), t, c.scale, c.P, c.OD, False, c.G, c.part, c.spp, c.tstd, m)
    assert tuple(out.shape) == (len(rois), c.OD, c.P, c.P)
    out.backward(T(nchw(grad)))
    bwd_check(nhwc(N(x.grad)), want.gfeat, want.Sfeat, want.nfeat, c, "autograd grad_feat", "b,y,x,c")
    bwd_check(N(t.grad), want.gtrans, want.Strans, want.ntrans, c, "autograd grad_trans", "k,c,py,px")
    if m is not None:
        bwd_check(N(m.grad), want.glogits, want.Slogits, want.nlogits, c, "autograd grad_mask_logits", "k,ph,pw")


# --------------------------------------------------------------------------------------------------------------------------- module level
def _fc64(x, layers_wb):
    """float64 FC stack on x [K, n] -> (output, its error bound in units of FC_ULPS ulp, per layer (input a_l, bound of a_l, ReLU mask of a_l)).
    Bound: e_{l+1} <= e_l |W|^T + ulps (|a_l| |W|^T + |b|) (ReLU is 1-Lipschitz); a hidden unit whose sign the bound cannot tell is refused."""
    a, e, per_layer = x, np.zeros_like(x), []
    for i, (w, b) in enumerate(layers_wb):
        per_layer.append((a, e))
        e = e @ np.abs(w).T + (np.abs(a) @ np.abs(w).T + np.abs(b))
        a = a @ w.T + b
        if i < len(layers_wb) - 1:
            assert (np.abs(a) > FC_ULPS * ULP * e).all(), "a hidden pre-activation within the bound of 0: its ReLU mask is not determined"
            a = np.maximum(a, 0)
    return a, e, per_layer


def _fc64_backward(g, per_layer, layers_wb):
    """float64 backward of the stack from g = dL/d output (taken as exact) -> (g_x, bound of g_x, [(dW, db)], [(bound dW, bound db)]), bounds
    in units of FC_ULPS ulp: dW = g^T a carries ulps |g|^T |a| + e_g^T |a| + |g|^T e_a, the chain g W likewise"""
    grads, bounds = [], []
    eg = np.zeros_like(g)
    for i in range(len(layers_wb) - 1, -1, -1):
        w, _ = layers_wb[i]
        a, ea = per_layer[i]
        grads.append((g.T @ a, g.sum(0)))
        bounds.append(((np.abs(g) + eg).T @ np.abs(a) + np.abs(g).T @ ea, (np.abs(g) + eg).sum(0)))
        eg = (np.abs(g) + eg) @ np.abs(w)
        g = g @ w
        if i > 0:
            g, eg = g * (a > 0), eg * (a > 0)
    return g, eg, grads[::-1], bounds[::-1]


@pytest.mark.parametrize("modulated", [False, True], ids=["DeformRoIPoolingPack", "ModulatedDeformRoIPoolingPack"])
@pytest.mark.parametrize("init", ["zero_last", "random_last"])
def test_pack_modules(modulated, init):
    from abr_iod_amd import layers
    Pn, C, FC, K, B, H, W, scale, spp, tstd = 3, 8, 16, 6, 2, 12, 16, 0.0625, 2, 0.1
    rng = np.random.default_rng(R._seed("pack", modulated, init))
    feat = rng.standard_normal((B, H, W, C)).astype(np.float32)
    rois = np.array([[k % B, 16 * rng.integers(1, 6), 16 * rng.integers(1, 4), 0, 0] for k in range(K)], np.float32)
    rois[:, 3] = rois[:, 1] + rng.integers(40, 140, K)
    rois[:, 4] = rois[:, 2] + rng.integers(40, 110, K)
    gout = rng.standard_normal((K, Pn, Pn, C)).astype(np.float32)
    cls = layers.ModulatedDeformRoIPoolingPack if modulated else layers.DeformRoIPoolingPack
    torch.manual_seed(7)
    mod = cls(scale, Pn, C, False, sample_per_part=spp, trans_std=tstd, deform_fc_channels=FC)
    if init == "random_last":          # the zero-initialised last layers make every offset 0 and every mask 1/2: also run away from there
        sd = mod.state_dict()
        for k in sd:
            if k.startswith("offset_fc.4") or k.startswith("mask_fc.2"):
                sd[k] = torch.from_numpy(rng.uniform(-0.5, 0.5, tuple(sd[k].shape)).astype(np.float32))
        mod.load_state_dict(sd, strict=True)          # a reference-keyed state dict loads strictly
    mod = mod.cuda()
    args = (scale, C, 1, Pn, Pn, spp, tstd)

    seen = {}
    stacks = [("offset", mod.offset_fc)] + ([("mask", mod.mask_fc)] if modulated else [])
    for name, st in stacks:
        def hook(m, inp, out, name=name):
            out.retain_grad()
            inp[0].retain_grad()
            seen[name] = (inp[0], out)
        st.register_forward_hook(hook)
    x_in = T(nchw(feat)).requires_grad_(True)
    out = mod(x_in, T(rois))
    out.backward(T(nchw(gout)))
    torch.cuda.synchronize()

    # ---- forward, stage by stage
    x_gpu = seen["offset"][0]
    x_np = nhwc(N(x_gpu))                                                               # [K, P, P, C]
    w1 = P.psroi_forward(feat, rois, None, None, *args)
    assert not w1.near.any()
    check(x_np, w1.out, P.scaled(w1.S, w1.n), "first pass")
    flat = nchw(x_np).reshape(K, -1).astype(np.float64)                                  # (c, ph, pw): the reference's x.view(n, -1)
    sd = {k: N(v).astype(np.float64) for k, v in mod.state_dict().items()}
    outs = {}
    for name, st in stacks:
        key = name + "_fc"
        wb = [(sd[f"{key}.{2 * i}.weight"], sd[f"{key}.{2 * i}.bias"]) for i in range(st.n)]
        y, mag, acts = _fc64(flat, wb)
        got = N(seen[name][1]).astype(np.float64)
        print(f"RATIO pack {name}_fc forward {np.abs(got - y).max() / max((FC_ULPS * ULP * mag).max(), 1e-300):.3f} of the bound")
        assert (np.abs(got - y) <= FC_ULPS * ULP * mag).all(), name
        outs[name] = (got, wb, acts)
    offset = N(seen["offset"][1]).reshape(K, 2, Pn, Pn)
    logits = N(seen["mask"][1]).reshape(K, Pn, Pn) if modulated else None
    if init == "zero_last":
        assert (offset == 0).all() and (logits is None or (logits == 0).all())
    w2 = P.psroi_forward(feat, rois, offset, logits, *args)
    assert not w2.near.any()
    check(nhwc(N(out)), w2.out, P.scaled(w2.S, w2.n), "second pass")

    # ---- backward, stage by stage: the second pass
    g2 = P.psroi_backward(gout, feat, rois, offset, logits, *args)
    check(N(seen["offset"][1].grad).reshape(K, 2, Pn, Pn), g2.gtrans, P.scaled(g2.Strans, g2.ntrans), "second pass grad_trans", axes="k,c,py,px")
    if modulated:
        check(N(seen["mask"][1].grad).reshape(K, Pn, Pn), g2.glogits, P.scaled(g2.Slogits, g2.nlogits), "second pass grad_mask_logits", axes="k,ph,pw")
    # the FC stacks, fed the GPU's own output gradients
    gx, gx_mag = np.zeros((K, flat.shape[1])), np.zeros((K, flat.shape[1]))
    params = dict(mod.named_parameters())
    for name, st in stacks:
        got_y, wb, acts = outs[name]
        g = N(seen[name][1].grad).astype(np.float64)
        gxi, mg, grads, mags = _fc64_backward(g, acts, wb)
        gx, gx_mag = gx + gxi, gx_mag + mg
        for i, ((dw, db), (mw, mb)) in enumerate(zip(grads, mags)):
            for what, want, mag in ((f"{name}_fc.{2 * i}.weight", dw, mw), (f"{name}_fc.{2 * i}.bias", db, mb)):
                got = N(params[what].grad).astype(np.float64)
                bound = FC_ULPS * ULP * mag
                print(f"RATIO pack grad {what} {np.abs(got - want).max() / max(bound.max(), 1e-300):.3f} of the bound")
                assert got.shape == want.shape and (np.abs(got - want) <= bound).all(), what
    got_gx = nchw(nhwc(N(x_gpu.grad))).reshape(K, -1).astype(np.float64)
    bound = FC_ULPS * ULP * gx_mag
    print(f"RATIO pack grad of the first pass's output {np.abs(got_gx - gx).max() / max(bound.max(), 1e-300):.3f} of the bound")
    assert (np.abs(got_gx - gx) <= bound).all()
    # the first pass, fed the GPU's own gradient, plus the second pass's share of the map's gradient
    g1 = P.psroi_backward(nhwc(N(x_gpu.grad)), feat, rois, None, None, *args)
    check(nhwc(N(x_in.grad)), g1.gfeat + g2.gfeat, P.scaled(g1.Sfeat + g2.Sfeat, g1.nfeat + g2.nfeat), "grad of data", axes="b,y,x,c")


def test_pack_output_carries_the_maps_amax():
    from abr_iod_amd import layers, ops
    from abr_iod_amd.layers._layout import from_nhwc
    rng = np.random.default_rng(8)
    x = ops.amax_compute(T(rng.standard_normal((2, 12, 16, 8)).astype(np.float32)))
    rois = T(np.array([[0, 10, 10, 100, 90], [1, 30, 20, 200, 150]], np.float32))
    for cls in (layers.DeformRoIPoolingPack, layers.ModulatedDeformRoIPoolingPack):
        mod = cls(0.0625, 3, 8, False, sample_per_part=2, trans_std=0.1, deform_fc_channels=16).cuda()
        out = mod(from_nhwc(x), rois)
        assert ops.amax_of(x)[0] is not None and ops.amax_of(out) == ops.amax_of(x)

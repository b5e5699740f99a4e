"""GPU: the FPN neck.  csrc/fpn.hip's kernels bit for bit against tests/fpn_ref.py; modeling/backbone/fpn.py stage by stage (every conv against
float64 of the GPU's own input to it under the conv sweep's fp32 rule, every top-down stage bit for bit), end to end against the reference's
own FPN (tests/golden/fpn.npz), its autograd plumbing and optimiser hook-up; the R-50-FPN body; and the composition
build_backbone -> RPNModule.eval() -> Pooler over a real pyramid.

End to end against the golden (fp32 convs, MATH_F32), worst |got - expected| / max |expected| per tensor as measured on the MI355X: see
MEASUREMENTS.md, "FPN neck"."""
import os

import numpy as np
import pytest
import torch
from torch import nn

import conv_ref as CR
import fpn_ref as R
from abr_iod_amd import ops

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fpn.npz")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want):
    return got.shape == want.shape and bool((bits(got) == bits(want)).all())


class no_sync(object):
    """torch's sync debug mode at "error": any host synchronisation inside raises"""

    def __enter__(self):
        self.before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")

    def __exit__(self, *a):
        torch.cuda.set_sync_debug_mode(self.before)


# ------------------------------------------------------------------------------------------------------------------ 1. kernels
CASES = [(1, 1, 4, (3, 5)), (1, 3, 260, (2, 2)), (2, 3, 8, (1, 1)), (2, 1, 260, (5, 7)), (4, 1, 260, (3, 5)), (4, 3, 8, (2, 3)), (4, 1, 4, (1, 1)),
         (5, 1, 4, (1, 2)), (5, 3, 260, (1, 1)), (5, 1, 8, (2, 1))]


@pytest.fixture(scope="module", autouse=True)
def _warm():
    ops.fpn_topdown_forward([torch.zeros((1, 2, 2, 4), device="cuda"), torch.zeros((1, 1, 1, 4), device="cuda")])   # library load
    torch.cuda.synchronize()


@pytest.mark.parametrize("L, B, C, top", CASES)
def test_topdown_forward_is_bit_equal(L, B, C, top):
    lats = R.pyramid(B, C, top, L, np.random.default_rng(100 + L + C))
    dev = [T(a) for a in lats]
    torch.cuda.synchronize()
    with no_sync():
        got = ops.fpn_topdown_forward(dev)
    assert len(got) == L and got[-1] is dev[-1]                      # the top level is aliased, not copied
    for l, (g, w) in enumerate(zip(got, R.topdown_forward(lats))):
        assert same(N(g), w), l
    for d, a in zip(dev, lats):                                      # the laterals are untouched
        assert same(N(d), a)


@pytest.mark.parametrize("L, B, C, top", CASES)
def test_topdown_backward_is_bit_equal(L, B, C, top):
    gs = R.pyramid(B, C, top, L, np.random.default_rng(200 + L + C))
    want = R.topdown_backward(gs)
    dev = [T(a) for a in gs]
    torch.cuda.synchronize()
    with no_sync():
        got = ops.fpn_topdown_backward(dev)
    assert got[0] is dev[0]
    for l in range(L):
        assert same(N(got[l]), want[l]), l
        assert same(N(dev[l]), gs[l]), l                             # out of place: the gradients are untouched
    with no_sync():
        got = ops.fpn_topdown_backward(dev, inplace=True)            # T_l written over g_l
    for l in range(L):
        assert got[l] is dev[l] and same(N(dev[l]), want[l]), l
    # the raw entry point copies level 0 when asked for a separate output
    if L > 1:
        import ctypes as C_
        outs = [torch.empty_like(d) for d in dev]
        src = [T(a) for a in gs]
        n = L
        ops.L.check(ops.L.lib().abr_fpn_topdown_backward((C_.c_void_p * n)(*[t.data_ptr() for t in src]), (C_.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                                         (C_.c_int * n)(*[a.shape[1] for a in gs]), (C_.c_int * n)(*[a.shape[2] for a in gs]), n, B, C,
                                                         ops.L.stream()), "fpn_topdown_backward")
        for l in range(L):
            assert same(N(outs[l]), want[l]), l


def test_topdown_backward_without_some_gradients():
    gs = R.pyramid(3, 8, (2, 3), 4, np.random.default_rng(7))
    for holes in ([0, None, 2, None], [0, 1, None, 3], [0, None, None, None]):
        sel = [None if h is None else gs[h] for h in holes]
        want = R.topdown_backward(sel)
        dev = [None if a is None else T(a) for a in sel]
        with no_sync():
            got = ops.fpn_topdown_backward(dev)
        for l in range(4):
            assert same(N(got[l]), want[l]), (holes, l)
    with pytest.raises(ValueError, match="finest"):
        ops.fpn_topdown_backward([None, T(gs[1])])


@pytest.mark.parametrize("B, H, W, C", [(1, 1, 1, 4), (3, 3, 5, 8), (1, 4, 6, 260), (2, 7, 2, 4), (1, 25, 42, 8)])
def test_subsample2_both_ways_is_bit_equal(B, H, W, C):
    rng = np.random.default_rng(H * 100 + W)
    x = rng.standard_normal((B, H, W, C)).astype(np.float32)
    g = rng.standard_normal((B, (H - 1) // 2 + 1, (W - 1) // 2 + 1, C)).astype(np.float32)
    g_in = rng.standard_normal(x.shape).astype(np.float32)
    xd, gd, gid = T(x), T(g), T(g_in)
    torch.cuda.synchronize()
    with no_sync():
        y = ops.fpn_subsample2(xd)
        a = ops.fpn_subsample2_backward(gd, x.shape)
        b = ops.fpn_subsample2_backward(gd, x.shape, gid)
    assert same(N(y), R.subsample2(x))
    assert same(N(a), R.subsample2_backward(g, x.shape))
    assert same(N(b), R.subsample2_backward(g, x.shape, g_in)) and same(N(gid), g_in)
    with no_sync():
        c = ops.fpn_subsample2_backward(gd, x.shape, gid, inplace=True)
    assert c is gid and same(N(gid), R.subsample2_backward(g, x.shape, g_in))
    with pytest.raises(ValueError, match="subsampled shape"):
        ops.fpn_subsample2_backward(gd, (B, H + 2, W, C))


def test_nan_and_inf_pass_through():
    rng = np.random.default_rng(5)
    for fn, ref in ((ops.fpn_topdown_forward, R.topdown_forward), (ops.fpn_topdown_backward, R.topdown_backward)):
        maps = R.pyramid(2, 8, (2, 3), 4, rng)
        for l, a in enumerate(maps):
            flat = a.reshape(-1)
            flat[3 + l], flat[11 + l], flat[17 + l] = np.nan, np.inf, -np.inf
        with np.errstate(invalid="ignore"):
            want = ref(maps)
        got = [N(t) for t in fn([T(a) for a in maps])]
        for l in range(4):
            nan = np.isnan(want[l])
            assert nan.any() and np.isinf(want[l]).any()
            assert (np.isnan(got[l]) == nan).all() and (bits(got[l])[~nan] == bits(want[l])[~nan]).all(), l
    x = rng.standard_normal((1, 3, 3, 4)).astype(np.float32)
    x[0, 0, 0, 0], x[0, 2, 2, 1], x[0, 0, 2, 3] = np.nan, np.inf, -np.inf
    y = N(ops.fpn_subsample2(T(x)))
    assert np.isnan(y[0, 0, 0, 0]) and y[0, 1, 1, 1] == np.inf and y[0, 0, 1, 3] == -np.inf


def test_mismatched_levels_raise_before_any_launch(monkeypatch):
    z = lambda h, w, c=8, b=2: torch.zeros((b, h, w, c), device="cuda")     # noqa: E731

    def boom():
        raise AssertionError("the library was called")

    monkeypatch.setattr(ops.L, "lib", boom)
    for fn in (ops.fpn_topdown_forward, ops.fpn_topdown_backward):
        for maps in ([z(8, 8), z(4, 4), z(2, 3)], [z(9, 8), z(4, 4)], [z(8, 8), z(4, 3)], [z(4, 4), z(8, 8)]):
            with pytest.raises(ValueError, match="not twice level"):
                fn(maps)
        with pytest.raises(ValueError, match="multiple of 4"):
            fn([z(4, 4, c=6), z(2, 2, c=6)])
    monkeypatch.undo()
    # the library refuses the same by itself, before any launch: a status and a message
    import ctypes as C_
    a, b = z(8, 8), z(4, 3)
    o = torch.empty_like(a)
    rc = ops.L.lib().abr_fpn_topdown_forward((C_.c_void_p * 2)(a.data_ptr(), b.data_ptr()), (C_.c_void_p * 2)(o.data_ptr(), 0), (C_.c_int * 2)(8, 4),
                                             (C_.c_int * 2)(8, 3), 2, 2, 8, ops.L.stream())
    assert rc == -1 and b"not twice" in ops.L.lib().abr_last_error()


# ------------------------------------------------------------------------------------------------------------------ 2. module
def _golden_fpn(g, requires_grad=True):
    from abr_iod_amd.modeling.backbone.fpn import FPN, LastLevelMaxPool
    from abr_iod_amd.utils.checkpoint import load_state_dict
    f = FPN(list(R.GOLDEN_IN), R.GOLDEN_OUT, LastLevelMaxPool())
    sd = {}
    for name, (w, b) in R.golden_params(g).items():
        sd[name + ".weight"], sd[name + ".bias"] = torch.from_numpy(w), torch.from_numpy(b)
    load_state_dict(f, sd)
    f = f.cuda()
    f.math = ops.MATH_F32
    for p in f.parameters():
        p.requires_grad_(requires_grad)
    return f


@pytest.fixture(scope="module")
def gold_run():
    """one forward and backward of the golden's FPN on the GPU with every intermediate kept: shared, never modified"""
    g = np.load(GOLD)
    xs_np, rs_np = R.golden_inputs(int(g["seed"]))
    f = _golden_fpn(g)
    xs = [T(x).requires_grad_(True) for x in xs_np]
    nhwc = [T(x.transpose(0, 2, 3, 1)) for x in xs_np]
    with torch.no_grad():
        laterals, inners, results = f._run(nhwc)
    staged = dict(laterals=[N(t) for t in laterals], inners=[N(t) for t in inners], results=[N(t) for t in results])
    rec = {}
    real = ops.fpn_topdown_backward

    def spy(grads, inplace=False):
        rec["g_inner"] = [None if t is None else N(t) for t in grads]
        out = real(grads, inplace=inplace)
        rec["d_lat"] = [N(t) for t in out]
        return out

    ops.fpn_topdown_backward = spy
    try:
        ps = f(xs)
        loss = sum((p * T(r)).sum() for p, r in zip(ps, rs_np))
        loss.backward()
        torch.cuda.synchronize()
    finally:
        ops.fpn_topdown_backward = real
    return dict(g=g, f=f, xs_np=xs_np, rs_np=rs_np, ps=[N(p) for p in ps], gx=[N(x.grad) for x in xs], staged=staged, rec=rec,
                grads={n: N(p.grad) for n, p in f.named_parameters()}, params={n: N(p) for n, p in f.named_parameters()})


def _rule(got, want, tol, what):
    ok, err, lim = R.conv_rule_ok(got, want, tol)
    print("%-28s err %.3e  limit %.3e  rel-to-max %.3e" % (what, err, lim, err / max(np.abs(want).max(), 1e-300)))
    assert ok, (what, err, lim)


def _d(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _wt64(w):
    """the dgrad copy of an OHWI weight in float64: [Cin,R,S,Cout], taps flipped"""
    return _d(w).flip(1, 2).permute(3, 1, 2, 0).contiguous()


def test_module_forward_stage_by_stage(gold_run):
    s, prm, xs_np = gold_run["staged"], gold_run["params"], gold_run["xs_np"]
    for l in range(4):
        w, b = prm["fpn_inner%d.weight" % (l + 1)], prm["fpn_inner%d.bias" % (l + 1)]
        want = CR.conv64(_d(xs_np[l].transpose(0, 2, 3, 1)), _d(w), 1, 0) + _d(b)
        _rule(s["laterals"][l], want.numpy(), R.CONV_TOL_FWD, "lateral %d" % l)
        w, b = prm["fpn_layer%d.weight" % (l + 1)], prm["fpn_layer%d.bias" % (l + 1)]
        want = CR.conv64(_d(s["inners"][l]), _d(w), 1, 1) + _d(b)
        _rule(s["results"][l], want.numpy(), R.CONV_TOL_FWD, "output %d" % l)
    for l, want in enumerate(R.topdown_forward(s["laterals"])):
        assert same(s["inners"][l], want), l
    assert same(s["results"][4], R.subsample2(s["results"][3])) and s["results"][4].shape == (2, 2, 3, 8)
    # the autograd path computes the same values as the plain forward
    for l in range(5):
        assert same(gold_run["ps"][l].transpose(0, 2, 3, 1), s["results"][l]), l


def test_module_backward_stage_by_stage(gold_run):
    s, prm, rec, grads = gold_run["staged"], gold_run["params"], gold_run["rec"], gold_run["grads"]
    rs = [r.transpose(0, 2, 3, 1) for r in gold_run["rs_np"]]
    gP = list(rs[:4])
    gP[3] = R.subsample2_backward(np.ascontiguousarray(rs[4]), rs[3].shape, np.ascontiguousarray(rs[3]))     # P6's gradient joins P5's
    for l in range(4):
        name = "fpn_layer%d" % (l + 1)
        _rule(rec["g_inner"][l], CR.conv64(_d(gP[l]), _wt64(prm[name + ".weight"]), 1, 1).numpy(), R.CONV_TOL_GRAD, "d inner %d" % l)
        _rule(grads[name + ".weight"], CR.wgrad64(_d(s["inners"][l]), _d(gP[l]), 3, 1, 1).numpy(), R.CONV_TOL_GRAD, "d " + name + ".weight")
        _rule(grads[name + ".bias"], gP[l].astype(np.float64).sum((0, 1, 2)), R.CONV_TOL_GRAD, "d " + name + ".bias")
    want = R.topdown_backward(rec["g_inner"])
    for l in range(4):
        assert same(rec["d_lat"][l], want[l]), l
    for l in range(4):
        name = "fpn_inner%d" % (l + 1)
        t = rec["d_lat"][l]
        x = gold_run["xs_np"][l].transpose(0, 2, 3, 1)
        _rule(grads[name + ".weight"], CR.wgrad64(_d(x), _d(t), 1, 1, 0).numpy(), R.CONV_TOL_GRAD, "d " + name + ".weight")
        _rule(grads[name + ".bias"], t.astype(np.float64).sum((0, 1, 2)), R.CONV_TOL_GRAD, "d " + name + ".bias")
        _rule(gold_run["gx"][l].transpose(0, 2, 3, 1), CR.conv64(_d(t), _wt64(prm[name + ".weight"]), 1, 0).numpy(), R.CONV_TOL_GRAD, "d C%d" % (l + 2))


def test_against_the_reference_golden(gold_run):
    """outputs and every gradient against the reference's own FPN, at the conv rule's bound for a chain of two convs"""
    g = gold_run["g"]
    for i in range(5):
        _rule(gold_run["ps"][i], g["p_%d" % i].astype(np.float64), R.CHAIN_TOL_FWD, "golden P%d" % (i + 2))
    for i in range(4):
        _rule(gold_run["gx"][i], g["gx_%d" % i].astype(np.float64), R.CHAIN_TOL_GRAD, "golden d C%d" % (i + 2))
    for name in sorted(R.golden_params(g)):
        gw = gold_run["grads"][name + ".weight"].transpose(0, 3, 1, 2)      # OHWI -> OIHW
        _rule(gw, g["gw_" + name].astype(np.float64), R.CHAIN_TOL_GRAD, "golden d " + name + ".weight")
        _rule(gold_run["grads"][name + ".bias"], g["gb_" + name].astype(np.float64), R.CHAIN_TOL_GRAD, "golden d " + name + ".bias")


# ------------------------------------------------------------------------------------------------------------------ 3. autograd plumbing
class _Count(object):
    """counts the calls of the ops the neck's backward makes"""
    NAMES = ("conv_backward", "conv_forward", "bias_grad", "fpn_topdown_backward", "fpn_subsample2_backward")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        self.dgrads = 0
        for name in self.NAMES:
            monkeypatch.setattr(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, fn):
        def call(*a, **k):
            self.n[name] += 1
            if name == "conv_backward" and k.get("dgrad", True):
                self.dgrads += 1
            return fn(*a, **k)
        return call


def _run_partial(g, monkeypatch, keep, requires_grad=True, x_grad=(True, True, True, True)):
    """loss over the outputs in `keep` only -> (fpn, inputs, call counts during backward, float64 expectation)"""
    xs_np, rs_np = R.golden_inputs(int(g["seed"]))
    f = _golden_fpn(g, requires_grad)
    xs = [T(x).requires_grad_(rg) for x, rg in zip(xs_np, x_grad)]
    ps = f(xs)
    loss = sum((ps[i] * T(rs_np[i])).sum() for i in keep)
    cnt = _Count(monkeypatch)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    rs = [r if i in keep else np.zeros_like(r) for i, r in enumerate(rs_np)]
    return f, xs, cnt, R.fpn64(xs_np, R.golden_params(g), rs)


def test_outputs_left_out_of_the_loss_cost_nothing(monkeypatch):
    g = np.load(GOLD)
    f, xs, cnt, (_, gx64, gp64) = _run_partial(g, monkeypatch, keep=(0, 2, 3))          # P3 and P6 unused
    assert cnt.n["fpn_subsample2_backward"] == 0 and cnt.n["fpn_topdown_backward"] == 1
    assert cnt.n["conv_backward"] == 3 + 4 and cnt.n["bias_grad"] == 3 + 4 and cnt.n["conv_forward"] == 0
    assert f.fpn_layer2.weight.grad is None and f.fpn_layer2.bias.grad is None
    for l in range(4):
        _rule(N(xs[l].grad), gx64[l], R.CHAIN_TOL_GRAD, "P3, P6 unused: d C%d" % (l + 2))
    for name, (gw, gb) in gp64.items():
        if name == "fpn_layer2":
            continue
        _rule(N(getattr(f, name).weight.grad).transpose(0, 3, 1, 2), gw, R.CHAIN_TOL_GRAD, "P3, P6 unused: d " + name + ".weight")
        _rule(N(getattr(f, name).bias.grad), gb, R.CHAIN_TOL_GRAD, "P3, P6 unused: d " + name + ".bias")
    # only the coarsest output: the finer levels' laterals and inputs see no gradient at all
    f, xs, cnt, (_, gx64, gp64) = _run_partial(g, monkeypatch, keep=(4,))
    assert cnt.n["fpn_subsample2_backward"] == 1 and cnt.n["conv_backward"] == 2 and cnt.n["bias_grad"] == 2
    assert all(xs[l].grad is None for l in range(3)) and f.fpn_inner1.weight.grad is None
    _rule(N(xs[3].grad), gx64[3], R.CHAIN_TOL_GRAD, "P6 only: d C5")


def test_frozen_fpn_still_passes_input_gradients(monkeypatch):
    g = np.load(GOLD)
    f, xs, cnt, (_, gx64, _) = _run_partial(g, monkeypatch, keep=(0, 1, 2, 3, 4), requires_grad=False)
    assert all(p.grad is None for p in f.parameters())
    assert cnt.n["conv_backward"] == 0 and cnt.n["bias_grad"] == 0 and cnt.n["conv_forward"] == 8
    for l in range(4):
        _rule(N(xs[l].grad), gx64[l], R.CHAIN_TOL_GRAD, "frozen FPN: d C%d" % (l + 2))
    # nothing requires a gradient: the plain forward, no autograd node
    with torch.enable_grad():
        ps = f([x.detach() for x in xs])
    assert all(p.grad_fn is None and not p.requires_grad for p in ps)


def test_an_input_without_requires_grad_gets_no_gradient(monkeypatch):
    g = np.load(GOLD)
    f, xs, cnt, (_, gx64, gp64) = _run_partial(g, monkeypatch, keep=(0, 1, 2, 3, 4), x_grad=(True, False, True, False))
    assert xs[1].grad is None and xs[3].grad is None
    assert cnt.n["conv_backward"] == 8 and cnt.dgrads == 4 + 2           # every 3x3's input gradient, two of the four 1x1's
    for l in (0, 2):
        _rule(N(xs[l].grad), gx64[l], R.CHAIN_TOL_GRAD, "d C%d" % (l + 2))
    _rule(N(f.fpn_inner2.weight.grad).transpose(0, 3, 1, 2), gp64["fpn_inner2"][0], R.CHAIN_TOL_GRAD, "d fpn_inner2.weight")


# ------------------------------------------------------------------------------------------------------------------ 4. optimiser
class _TinyModel(nn.Module):
    """the golden's FPN as a model FusedSGD can own: flat parameter storage like GeneralizedRCNN's"""

    def __init__(self, fpn):
        super().__init__()
        self.fpn = fpn
        self.flat = None

    def flatten_parameters(self):
        from abr_iod_amd.modeling._flat import flatten_parameters
        from abr_iod_amd.modeling.backbone.resnet import bump_param_version
        self.flat = flatten_parameters(self)
        bump_param_version()
        return self.flat


def test_fused_sgd_moves_the_fpn_and_refreshes_its_dgrad_copies():
    from abr_iod_amd.modeling.backbone import resnet
    from abr_iod_amd.solver.build import FusedSGD
    g = np.load(GOLD)
    xs_np, rs_np = R.golden_inputs(int(g["seed"]))
    model = _TinyModel(_golden_fpn(g))
    opt = FusedSGD(model, 0.001, 0.9, 1e-4, 2.0, 0.0)
    convs = [m for m in model.modules() if isinstance(m, resnet.Conv2d)]
    assert len(convs) == 8 and all(c._optimised for c in convs)
    assert {n for n, _, _, _ in model.flat.segments} == {n for n, _ in model.named_parameters()}
    assert all(p.data_ptr() >= model.flat.params.data_ptr() and p.grad is not None for p in model.parameters())
    before = {n: N(p).copy() for n, p in model.named_parameters()}

    def backward():
        xs = [T(x).requires_grad_(True) for x in xs_np]
        ps = model.fpn(xs)
        sum((p * T(r)).sum() for p, r in zip(ps, rs_np)).backward()
        return xs

    opt.zero_grad()
    backward()
    opt.step()
    torch.cuda.synchronize()
    after = {n: N(p) for n, p in model.named_parameters()}
    assert all(np.isfinite(after[n]).all() and (after[n] != before[n]).any() for n in before)
    assert all(c._wt_version == resnet._PARAM_VERSION[0] for c in convs)              # rebuilt by the step's batched preparation
    opt.zero_grad()
    xs = backward()
    torch.cuda.synchronize()
    params = {}
    for c_name in sorted({n.rsplit(".", 1)[0] for n in after}):
        params[c_name.split(".")[-1]] = (after[c_name + ".weight"].transpose(0, 3, 1, 2), after[c_name + ".bias"])
    _, gx64, _ = R.fpn64(xs_np, params, rs_np)
    for l in range(4):
        _rule(N(xs[l].grad), gx64[l], R.CHAIN_TOL_GRAD, "after a step: d C%d" % (l + 2))


# ------------------------------------------------------------------------------------------------------------------ 5. body and composition
@pytest.fixture(scope="module")
def r50_fpn():
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.backbone.backbone import build_backbone
    c = cfg.clone()
    c.MODEL.BACKBONE.CONV_BODY = "R-50-FPN"
    c.MODEL.RESNETS.BACKBONE_OUT_CHANNELS = 256
    c.MODEL.RPN.USE_FPN = True
    c.MODEL.RPN.ANCHOR_STRIDE, c.MODEL.RPN.ANCHOR_SIZES = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512)
    c.MODEL.RPN.PRE_NMS_TOP_N_TEST, c.MODEL.RPN.POST_NMS_TOP_N_TEST, c.MODEL.RPN.FPN_POST_NMS_TOP_N_TEST = 200, 50, 100
    c.MODEL.ROI_HEADS.USE_FPN = True
    c.MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION = 7
    c.MODEL.ROI_BOX_HEAD.POOLER_SCALES = (0.25, 0.125, 0.0625, 0.03125)
    c.MODEL.ROI_BOX_HEAD.POOLER_SAMPLING_RATIO = 2
    torch.manual_seed(0)
    model = build_backbone(c).cuda()
    image = torch.randn(2, 3, 64, 96, device="cuda")
    return c, model, image


def test_r50_fpn_body(r50_fpn):
    c, model, image = r50_fpn
    assert model.out_channels == 256 and c.MODEL.BACKBONE.FREEZE_CONV_BODY_AT == 2
    with torch.no_grad():
        feats, bfeats = model(image)
        prefix = model.frozen_prefix(image)
        feats2, bfeats2 = model(image, prefix=prefix)
    assert [tuple(f.shape) for f in feats] == [(2, 256, 16, 24), (2, 256, 8, 12), (2, 256, 4, 6), (2, 256, 2, 3), (2, 256, 1, 2)]
    assert [tuple(f.shape) for f in bfeats] == [(2, 256, 16, 24), (2, 512, 8, 12), (2, 1024, 4, 6), (2, 2048, 2, 3)]
    assert all(bool(torch.isfinite(f).all()) for f in feats)
    assert prefix is not None and len(prefix[1]) == 1
    for a, b in zip(list(feats) + list(bfeats), list(feats2) + list(bfeats2)):
        assert torch.equal(a, b)
    model.zero_grad()
    feats, _ = model(image)
    sum(f.sum() for f in feats).backward()
    torch.cuda.synchronize()
    body = model.body
    assert all(p.grad is None for p in list(body.stem.parameters()) + list(body.layer1.parameters()))
    for stage in (body.layer2, body.layer3, body.layer4):
        for blk in (stage[0], stage[-1]):
            for conv in (blk.conv1, blk.conv2, blk.conv3):
                gw = conv.weight.grad
                assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0 for p in model.fpn.parameters())
    model.zero_grad(set_to_none=True)


def test_backbone_rpn_pooler_compose(r50_fpn):
    """build_backbone -> RPNModule.eval() over five strides -> the multi-level Pooler over P2..P5, on real features"""
    from abr_iod_amd.modeling.poolers import make_pooler
    from abr_iod_amd.modeling.rpn.rpn import RPNModule
    from abr_iod_amd.structures.image_list import ImageList
    c, model, image = r50_fpn
    torch.manual_seed(1)
    rpn = RPNModule(c, model.out_channels).cuda().eval()
    with torch.no_grad():
        for conv in (rpn.head.cls_logits, rpn.head.bbox_pred):
            conv.weight.mul_(20)
    sizes = [(64, 96), (60, 90)]
    images = ImageList(image, sizes)
    with torch.no_grad():
        feats, _ = model(image)
        (boxes, losses), anchors, (obj, reg) = rpn(images, list(feats))
    assert losses == {} and len(obj) == 5 and len(boxes) == 2
    for b, (h, w) in zip(boxes, sizes):
        bb = b.bbox.cpu().numpy()
        assert 0 < len(bb) <= 100 and np.isfinite(bb).all()
        assert (bb[:, 0] >= 0).all() and (bb[:, 1] >= 0).all() and (bb[:, 2] <= w - 1).all() and (bb[:, 3] <= h - 1).all()
        assert (bb[:, 0] <= w - 1).all() and (bb[:, 1] <= h - 1).all() and (bb[:, 2] >= 0).all() and (bb[:, 3] >= 0).all()
    pooler = make_pooler(c, "ROI_BOX_HEAD")
    with torch.no_grad():
        pooled = pooler(list(feats[:4]), boxes)
    K = sum(len(b) for b in boxes)
    assert tuple(pooled.shape) == (K, 256, 7, 7) and bool(torch.isfinite(pooled).all()) and float(pooled.abs().max()) > 0

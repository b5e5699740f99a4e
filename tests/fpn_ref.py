"""numpy restatements of csrc/fpn.hip's four kernels on NHWC arrays, in the kernels' own order of fp32 additions (the forward's is the
reference's: modeling/backbone/fpn.py:51-65; the backward's is the one include/abr_iod_hip.h prescribes), plus float64 forms and the inputs of
tests/golden/fpn.npz.  Shared by tests/test_fpn_ref.py (CPU), tests/test_gpu_fpn.py and tests/golden/make_golden_fpn.py."""
import numpy as np

# the golden's geometry (tests/golden/make_golden_fpn.py)
GOLDEN_B = 2
GOLDEN_IN = (8, 16, 32, 64)
GOLDEN_OUT = 8
GOLDEN_MAPS = ((24, 40), (12, 20), (6, 10), (3, 5))     # P6 is then 2 x 3: an odd top size
GOLDEN_SEED = 20260


def golden_inputs(seed=GOLDEN_SEED):
    """(C2..C5 as NCHW float32, R_2..R_6 as NCHW float32): the maps fed to the FPN and the seeded weights of the loss sum_l <P_l, R_l>"""
    rng = np.random.default_rng(seed)
    xs = [rng.standard_normal((GOLDEN_B, c, h, w)).astype(np.float32) for c, (h, w) in zip(GOLDEN_IN, GOLDEN_MAPS)]
    hw = list(GOLDEN_MAPS) + [((GOLDEN_MAPS[-1][0] - 1) // 2 + 1, (GOLDEN_MAPS[-1][1] - 1) // 2 + 1)]
    rs = [rng.standard_normal((GOLDEN_B, GOLDEN_OUT, h, w)).astype(np.float32) for h, w in hw]
    return xs, rs


def up2(a):
    """nearest-neighbour 2x upsampling of an NHWC array"""
    return a.repeat(2, axis=1).repeat(2, axis=2)


def topdown_forward(lats):
    """lats: NHWC arrays, finest first -> inners; inner_l = lat_l + up2(inner_{l+1}), the top inner is the top lateral"""
    inners = [None] * len(lats)
    inners[-1] = lats[-1]
    for l in range(len(lats) - 2, -1, -1):
        inners[l] = lats[l] + up2(inners[l + 1])
    return inners


def topdown_backward(gs):
    """gs: gradients at inner_0 .. inner_{L-1} (None past level 0: none) -> T_l with T_0 = g_0 and
    T_l = g_l + ((T(2y,2x) + T(2y,2x+1)) + (T(2y+1,2x) + T(2y+1,2x+1))) of T_{l-1}, in the arrays' dtype (float32: the kernel's roundings)"""
    out = [gs[0]]
    for l in range(1, len(gs)):
        t = out[-1]
        s = (t[:, 0::2, 0::2] + t[:, 0::2, 1::2]) + (t[:, 1::2, 0::2] + t[:, 1::2, 1::2])
        out.append(s if gs[l] is None else gs[l] + s)
    return out


def topdown_backward_abs(gs):
    """sum |addends| behind every element of topdown_backward's result, in float64: the scale of its rounding bound"""
    return topdown_backward([None if g is None else np.abs(g.astype(np.float64)) for g in gs])


def subsample2(x):
    return np.ascontiguousarray(x[:, 0::2, 0::2])


def subsample2_backward(g_out, shape, g_in=None):
    g = np.zeros(shape, g_out.dtype) if g_in is None else g_in.copy()
    if g_in is None:
        g[:, 0::2, 0::2] = g_out
    else:
        g[:, 0::2, 0::2] = g_in[:, 0::2, 0::2] + g_out
    return g


def pyramid(B, C, top_hw, L, rng, scale=1.0):
    """L random NHWC float32 maps, finest first, each twice the next, the coarsest top_hw"""
    h, w = top_hw
    return [(scale * rng.standard_normal((B, h << (L - 1 - l), w << (L - 1 - l), C))).astype(np.float32) for l in range(L)]


# The conv sweep's rule for an fp32 conv (tools/conv_fuzz.py, `check` and MODES): |got - float64| <= tol * max(1, max |float64|) with
# tol = 1e-4 for a forward result and 2e-4 for a gradient.  Every FPN output and every gradient passes through two convs (1x1 and 3x3), each of
# which may spend the rule's allowance once at the scale of the final tensor; the top-down adds between them are exact to 2^-24 per add.
CONV_TOL_FWD, CONV_TOL_GRAD = 1e-4, 2e-4
CHAIN_TOL_FWD, CHAIN_TOL_GRAD = 2 * CONV_TOL_FWD, 2 * CONV_TOL_GRAD


def conv_rule_ok(got, want, tol):
    """the sweep's comparison -> (passes, error, limit); got / want: numpy arrays, want in float64"""
    err = float(np.abs(got.astype(np.float64) - want).max())
    lim = tol * max(1.0, float(np.abs(want).max()))
    return bool(np.isfinite(got).all()) and err <= lim, err, lim


def fpn64(xs, params, rs):
    """The reference's FPN.forward with LastLevelMaxPool and the loss sum_l <P_l, R_l> in float64 (torch on the CPU).  xs / rs: NCHW numpy arrays,
    params: {"fpn_inner1": (w OIHW, b), ..} -> (P list, gx list, {name: (gw, gb)}) as float64 numpy arrays"""
    import torch
    import torch.nn.functional as F
    n = len(xs)
    xt = [torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True) for x in xs]
    pt = {k: tuple(torch.from_numpy(np.asarray(v, np.float64)).requires_grad_(True) for v in wb) for k, wb in params.items()}
    inner = lambda i, t: F.conv2d(t, *pt["fpn_inner%d" % (i + 1)])                # noqa: E731
    layer = lambda i, t: F.conv2d(t, *pt["fpn_layer%d" % (i + 1)], padding=1)     # noqa: E731
    last = inner(n - 1, xt[-1])
    ps = [layer(n - 1, last)]
    for i in range(n - 2, -1, -1):
        last = inner(i, xt[i]) + F.interpolate(last, scale_factor=2, mode="nearest")
        ps.insert(0, layer(i, last))
    ps.append(F.max_pool2d(ps[-1], 1, 2, 0))
    sum((p * torch.from_numpy(np.asarray(r, np.float64))).sum() for p, r in zip(ps, rs)).backward()
    return ([p.detach().numpy() for p in ps], [x.grad.numpy() for x in xt], {k: (w.grad.numpy(), b.grad.numpy()) for k, (w, b) in pt.items()})


def golden_params(g):
    """{"fpn_inner1": (w OIHW, b), ..} of a loaded tests/golden/fpn.npz"""
    return {k[2:]: (g[k], g["b_" + k[2:]]) for k in g.files if k.startswith("w_")}

#!/usr/bin/env python3
"""Random-shape sweep of the conv engine against float64, stratified by the route the library takes (abr::conv_route, asked through
ops.conv_route_info -- never restated here).

Stratum `any` is the blind draw: forward (with a random choice of the fused epilogue: BN scale / bias / residual / ReLU), input gradient and
weight gradient, in the arithmetics, at shapes the model never uses (odd extents, channel counts that are not tile multiples, 1-pixel maps,
strides).  The other strata are drawn TOWARDS a route and then confirmed with the library; a drawn case whose confirmed route is not the
stratum's fails the run:
  wino             wide 3x3 stride 1 pad 1: Winograd forward (scale / bias / ReLU / mask), input gradient, weight gradient self-contained and from
                   the forward's kept V (x overwritten by NaN); every H % 4 and W % 4, maps smaller than a tile, batches of 40..96 one-tile images
  wino_wgrad_only  the same convs pushed off the forward route one way each (residual; Cout % 32 != 0 under the split arithmetics; Cout % 4 != 0;
                   Cin % 32 != 0): forward direct, weight gradient Winograd, nothing kept
  f16              ABR_MATH_F16 against the mode's definition (tests/conv_ref.py), with tests/test_gpu_f16_math.py's bound
  bf16_fallback    ABR_MATH_BF16 at channel counts that are no multiple of 64: runs in fp32 and must meet fp32's tolerance
  tail64           the fused bottleneck tail, bit-equal to the two convs it replaces, and both against float64
  dgrad_fused      the input gradient with the ReLU mask and / or a residual fused into its epilogue
A configuration the library does not support must raise (counted, listed), never return wrong values.
Every forward and input-gradient call asks for the output's amax word (emit_amax=True, in all arithmetics); where the result carries the
tag, the word must hold exactly the bits of max |result| (the definition tests/amax_words.py::expect checks, restated below: the tool needs
nothing from tests/ but conv_ref.py, so it also runs beside an older tests/ directory): counted as amax_checks per stratum and mode.
GPU box: python tools/conv_fuzz.py [--cases 300] [--per-stratum 40] [--seed 0] [--strata any,wino,...]; --plan draws, asks the library for
the routes and prints the counts without touching a device."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from abr_iod_amd import ops  # noqa: E402

STRATA = ["any", "wino", "wino_wgrad_only", "f16", "bf16_fallback", "tail64", "dgrad_fused"]
ap = argparse.ArgumentParser()
ap.add_argument("--cases", type=int, default=300, help="cases of stratum `any`")
ap.add_argument("--per-stratum", type=int, default=None, help="cases of every other stratum (given without --strata: all strata run)")
ap.add_argument("--seed", type=int, default=0)
ap.add_argument("--strata", default=None, help="comma-separated subset of: " + ",".join(STRATA) + " (default: any)")
ap.add_argument("--plan", action="store_true", help="draw and ask the library for the routes only: no device, no comparison")
a = ap.parse_args()
strata = a.strata.split(",") if a.strata else (STRATA if a.per_stratum else ["any"])
assert all(s in STRATA for s in strata), strata
if a.per_stratum is None:
    a.per_stratum = 40
MODES = [("f32", ops.MATH_F32, 1e-4), ("bf16x6", ops.MATH_BF16X6, 1e-4), ("f16x3", ops.MATH_F16X3, 1e-4), ("bf16", ops.MATH_BF16, 3e-2)]
FULL = MODES[:3]        # the full-precision arithmetics: the ones that may take Winograd
MATH_NAME = {ops.MATH_F32: "f32", ops.MATH_BF16: "bf16", ops.MATH_BF16X6: "bf16x6", ops.MATH_F16X3: "f16x3", ops.MATH_F16: "f16"}
CH = [4, 8, 12, 16, 20, 32, 36, 48, 64, 76, 96, 100, 128, 160, 192, 256, 320, 512]
WIDE_IN, WIDE_OUT = [128, 160, 192, 256, 320, 512], [128, 160, 192, 256, 512]
EPS = 2.0 ** -24
PTR = torch.zeros(4)     # stands for "a residual is given" in a route query (the route looks at the pointer only)
fails, refused, ran = [], {}, 0
cov = {}                 # stratum -> {"cases", "comparisons", "misrouted", "routes": {mode: {"op/route": n}}, "features": {...}, "reasons": {...},
#                                       "fwd_dgrad": {mode: forward / input-gradient comparisons that ran}, "amax_checks": {mode: n}}
cur = [None]             # the stratum being drawn


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().float().cuda()


_hip = []


def expect(word, epoch, t, what):
    """the amax word at device address `word` carries `epoch` and exactly the bits of max |t| (integer order on magnitudes, read from the
    tensor copied back from the device): tests/amax_words.py::expect"""
    import ctypes
    if not _hip:
        hip = ctypes.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
        _hip.append(hip)
    host = ctypes.c_uint64(0)
    torch.cuda.synchronize()
    assert _hip[0].hipMemcpy(ctypes.byref(host), ctypes.c_void_p(word), 8, 2) == 0   # hipMemcpyDeviceToHost
    got = (int(host.value) >> 32, int(host.value) & 0xFFFFFFFF)
    want = (int(epoch) & 0xFFFFFFFF, int((t.detach().cpu().contiguous().view(torch.int32) & 0x7FFFFFFF).max()) if t.numel() else 0)
    assert got == want, "%s amax word: epoch %d, bits 0x%08x; want epoch %d, bits 0x%08x = max |result|" % ((what,) + got + want)


def check_amax(tag, case, src):
    """src: the tensor a forward / input-gradient call returned (not a view of it: a view loses the tag), asked with emit_amax=True.  Its amax
    word must hold exactly the bits of max |src|; a result without a tag is a failure (nothing is skipped silently)."""
    mode = "bf16x6" if tag.startswith("tail64") else tag.split("/", 1)[1]
    word, epoch = ops.amax_of(src)
    if word is None:
        fails.append((tag, case, "the result carries no amax tag"))
        return
    try:
        expect(word, epoch, src, tag)
    except AssertionError as e:
        fails.append((tag, case, str(e)))
    if cur[0]:
        d = cov[cur[0]]["amax_checks"]
        d[mode] = d.get(mode, 0) + 1


def count(tag):
    """one comparison of the current stratum; those of a forward / input-gradient result also per mode (fwd_dgrad)"""
    global ran
    ran += 1
    if cur[0]:
        cov[cur[0]]["comparisons"] += 1
        op, _, mode = tag.partition("/")
        if op in ("fwd", "fwd_keep_v", "dgrad"):
            d = cov[cur[0]]["fwd_dgrad"]
            d[mode] = d.get(mode, 0) + 1


def check(tag, case, got, want, tol, src=None):
    count(tag)
    err = (got.detach().cpu().double() - want).abs().max().item()
    lim = tol * max(1.0, want.abs().max().item())
    if not (err <= lim) or not bool(torch.isfinite(got).all()):
        fails.append((tag, case, err, lim))
    if src is not None:
        check_amax(tag, case, src)


def attempt(tag, case, fn):
    try:
        return fn()
    except RuntimeError as e:
        refused.setdefault((tag, str(e)[:90]), []).append(case)
        # the targeted strata: only the backward kernels' documented vector width (a Cout that is no multiple of 4) may be refused
        Cout = case[4]
        if cur[0] != "any" and not (("multiple of 4" in str(e) or "multiples of 4" in str(e)) and Cout % 4 != 0 and tag.split("/")[0] in ("wgrad", "dgrad")):
            fails.append(("refused in stratum " + cur[0], tag, case, str(e)[:90]))
        return None


def route_fwd(case, m, residual=False):
    B, Cin, H, W, Cout, k, s, p = case
    return ops.conv_route_info((B, H, W, Cin), (Cout, k, k, Cin), s, p, residual=PTR if residual else None, math=m)


def route_dgrad(case, m, residual=False):
    """the input gradient is a forward call: conv(gy, wt) with stride 1, pad k-1-p (scattered into [H, W] for a strided 1x1)"""
    B, Cin, H, W, Cout, k, s, p = case
    Ho, Wo = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    kw = dict(out_hw=(H, W), out_stride=(s, s)) if s > 1 else {}
    return ops.conv_route_info((B, Ho, Wo, Cout), (Cin, k, k, Cout), 1, (k - 1 - p) if s == 1 else 0, residual=PTR if residual else None, math=m, **kw)


def step(op, mode, got, expect=None, feats=(), reason=None):
    """one planned comparison (or group of them) of the current stratum: counted by the route the LIBRARY confirmed; `expect` (None: either)
    is the route the stratum was drawn for.  Returns whether to run it (not under --plan, and not misrouted)."""
    c = cov[cur[0]]
    r = "wino" if got else "direct"
    key = op + "/" + r
    c["routes"].setdefault(mode, {}).setdefault(key, 0)
    c["routes"][mode][key] += 1
    if expect is not None and r != expect:
        c["misrouted"] += 1
        fails.append(("misrouted in stratum " + cur[0], op, mode, "drawn for " + expect + ", the library takes " + r))
        return False
    for f in feats:
        d = c["features"].setdefault(mode, {}).setdefault(op, {})
        d[f] = d.get(f, 0) + 1
    if reason:
        d = c["reasons"].setdefault(reason, {})
        d[mode] = d.get(mode, 0) + 1
    return not a.plan


def misrouted(what):
    cov[cur[0]]["misrouted"] += 1
    fails.append(("misrouted in stratum " + cur[0], what))


class Data(object):
    """operands, epilogue tensors and the float64 reference of one conv case (the draw order is the sweep's since its first version)"""

    def __init__(self, case, gseed):
        B, Cin, H, W, Cout, k, s, p = case
        g = torch.Generator().manual_seed(gseed)
        self.x = torch.randn(B, Cin, H, W, generator=g).float().double().requires_grad_(True)
        self.w = (torch.randn(Cout, Cin, k, k, generator=g) / (Cin * k * k) ** 0.5).float().double().requires_grad_(True)
        self.scale = (torch.rand(Cout, generator=g) + 0.5).float()
        self.bias = (torch.randn(Cout, generator=g) * 0.1).float()
        y = F.conv2d(self.x, self.w, stride=s, padding=p)
        self.res = torch.randn(y.shape, generator=g).float()
        self.gy = torch.randn(y.shape, generator=g).float().double()
        (y * self.scale.double().view(1, -1, 1, 1)).backward(self.gy)
        self.y = y.detach()
        self.mask = torch.randn(y.shape, generator=g).float()          # ReLU mask of a forward output
        self.xmask = torch.randn(self.x.shape, generator=g).float()    # ... and of an input gradient
        self.xres = torch.randn(self.x.shape, generator=g).float()
        self.xg, self.wg, self.gyg = nhwc(self.x.detach()), nhwc(self.w.detach()), nhwc(self.gy)

    def epilogue(self, use):
        yr = self.y
        if use.get("scale"):
            yr = yr * self.scale.double().view(1, -1, 1, 1)
        if use.get("bias"):
            yr = yr + self.bias.double().view(1, -1, 1, 1)
        if use.get("residual"):
            yr = yr + self.res.double()
        if use.get("relu"):
            yr = torch.relu(yr)
        if use.get("mask"):
            yr = torch.where(self.mask.double() > 0, yr, torch.zeros_like(yr))
        return yr

    def kw(self, use):
        return dict(scale=self.scale.cuda() if use.get("scale") else None, bias=self.bias.cuda() if use.get("bias") else None,
                    residual=nhwc(self.res) if use.get("residual") else None, mask=nhwc(self.mask) if use.get("mask") else None,
                    relu=bool(use.get("relu")))


def used(use):
    return (tuple(sorted(k_ for k_, v in use.items() if v)),)


def run_dgrad(D, case, m, **kw):
    B, Cin, H, W, Cout, k, s, p = case
    wt = ops.conv_dgrad_weights(D.wg, D.scale.cuda())
    if s == 1:
        return ops.conv_forward(D.gyg, wt, 1, k - 1 - p, math=m, emit_amax=True, **kw)
    return ops.conv_forward(D.gyg, wt, 1, 0, out_hw=(H, W), out_stride=(s, s), math=m, emit_amax=True, **kw)


def draw_any(rng):
    k = rng.choice([1, 1, 3, 3, 7])
    Cin = 4 if k == 7 else rng.choice(CH)
    Cout = rng.choice(CH + [1, 3, 5, 21, 33, 108])
    s = rng.choice([1, 1, 2])
    p = rng.choice([0, (k - 1) // 2]) if k > 1 else 0
    B = rng.randint(1, 5)
    H, W = rng.randint(max(1, k - 2 * p), 41), rng.randint(max(1, k - 2 * p), 41)
    if (Cin * k * k * Cout * H * W * B) > 6e9:      # keep the float64 CPU reference in seconds
        B, H, W = 1, min(H, 16), min(W, 16)
        H, W = max(H, k - 2 * p), max(W, k - 2 * p)
    return (B, Cin, H, W, Cout, k, s, p)


def stratum_any(n, seed):
    rng = random.Random(seed)
    for ci in range(n):
        case = draw_any(rng)
        B, Cin, H, W, Cout, k, s, p = case
        cov["any"]["cases"] += 1
        use = dict(scale=rng.random() < 0.7, bias=rng.random() < 0.5, residual=rng.random() < 0.4, relu=rng.random() < 0.6)
        D = None if a.plan else Data(case, seed * 100003 + ci)
        for name, m, tol in MODES:
            if m != ops.MATH_F32 and k == 7:
                continue
            if Cin % 4 == 0 and step("fwd", name, route_fwd(case, m, use["residual"])[1]):
                got = attempt("fwd/" + name, case, lambda: ops.conv_forward(D.xg, D.wg, s, p, math=m, emit_amax=True, **D.kw(use)))
                if got is not None:
                    check("fwd/" + name, case + used(use), got.permute(0, 3, 1, 2), D.epilogue(use), tol, src=got)
            if k == 7:
                continue      # the stem is frozen: no backward on the path
            if step("wgrad", name, route_fwd(case, m)[2]):
                dw = torch.zeros_like(D.wg)
                if attempt("wgrad/" + name, case, lambda: (ops.conv_wgrad(D.xg, D.gyg, dw, s, p, scale=D.scale.cuda(), math=m), True)[1]):
                    check("wgrad/" + name, case, dw.permute(0, 3, 1, 2), D.w.grad, tol * 2)
            if (s == 1 or k == 1) and step("dgrad", name, route_dgrad(case, m)[1]):
                dx = attempt("dgrad/" + name, case, lambda: run_dgrad(D, case, m))
                if dx is not None:
                    check("dgrad/" + name, case, dx.permute(0, 3, 1, 2), D.x.grad, tol * 2, src=dx)
        if (ci + 1) % 50 == 0:
            print("%d cases, %d comparisons, %d failures, %d refusals" % (ci + 1, ran, len(fails), sum(len(v) for v in refused.values())), flush=True)


def draw_wide(rng, Cin=None, Cout=None):
    """a wide 3x3 stride-1 pad-1 conv: H and W over every residue mod 4, the sizes below a tile and just above it; one case in five a
    batch of 40..96 images of at most one tile"""
    Cin, Cout = Cin or rng.choice(WIDE_IN), Cout or rng.choice(WIDE_OUT)
    if rng.random() < 0.2:
        B, H, W = rng.randint(40, 96), rng.randint(1, 4), rng.randint(1, 4)
    else:
        B = rng.randint(1, 5)
        H, W = (rng.choice([1, 2, 3, 5]) if rng.random() < 0.35 else rng.randint(4, 23) for _ in range(2))
    while Cin * 9 * Cout * H * W * B > 6e9:     # keep the float64 CPU reference in seconds, and the residues
        if B > 1:
            B = 1
        elif H >= W:
            H -= 4
        else:
            W -= 4
    return (B, Cin, H, W, Cout, 3, 1, 1)


def wide_feats(case):
    B, _, H, W = case[:4]
    f = ["H%%4=%d" % (H % 4), "W%%4=%d" % (W % 4)]
    if H <= 3 and W <= 3:
        f.append("below_one_tile")
    if B >= 40 and H <= 4 and W <= 4:
        f.append("batch40_one_tile")
    return f


def stratum_wino(n, seed):
    rng = random.Random("%d/wino" % seed)
    for ci in range(n):
        case = draw_wide(rng)
        B, Cin, H, W, Cout, k, s, p = case
        cov["wino"]["cases"] += 1
        use = dict(scale=rng.random() < 0.7, bias=rng.random() < 0.5, relu=rng.random() < 0.5, mask=rng.random() < 0.5)
        feats = wide_feats(case)
        D = None if a.plan else Data(case, seed * 100003 + 1000003 + ci)
        for name, m, tol in FULL:
            _, fw, ww, _ = route_fwd(case, m)
            if step("fwd", name, fw, "wino", feats):
                got = attempt("fwd/" + name, case, lambda: ops.conv_forward(D.xg, D.wg, 1, 1, math=m, emit_amax=True, **D.kw(use)))
                if got is not None:
                    check("fwd/" + name, case + used(use), got.permute(0, 3, 1, 2), D.epilogue(use), tol, src=got)
            if step("dgrad", name, route_dgrad(case, m)[1], "wino", feats):
                dx = attempt("dgrad/" + name, case, lambda: run_dgrad(D, case, m))
                if dx is not None:
                    check("dgrad/" + name, case, dx.permute(0, 3, 1, 2), D.x.grad, tol * 2, src=dx)
            dw_ref = None
            if step("wgrad", name, ww, "wino", feats):
                dw_ref = torch.zeros_like(D.wg)
                if attempt("wgrad/" + name, case, lambda: (ops.conv_wgrad(D.xg, D.gyg, dw_ref, 1, 1, scale=D.scale.cuda(), math=m), True)[1]):
                    check("wgrad/" + name, case, dw_ref.permute(0, 3, 1, 2), D.w.grad, tol * 2)
            # what the training step runs: the forward keeps its Winograd-domain input V, the weight gradient reads V and never touches x
            if step("wgrad_kept_v", name, fw and ww, "wino", feats):
                v = ops.wino_v_alloc(D.xg, D.wg, 1, 1, m)
                if v is None or v.numel() != 36 * B * ((H + 3) // 4) * ((W + 3) // 4) * Cin:
                    misrouted("wino_v_alloc %s %s" % (name, case))
                    continue
                v.fill_(float("nan"))
                got = attempt("fwd_keep_v/" + name, case, lambda: ops.conv_forward(D.xg, D.wg, 1, 1, math=m, wino_v=v, emit_amax=True, **D.kw(use)))
                if got is None:
                    continue
                check("fwd_keep_v/" + name, case + used(use), got.permute(0, 3, 1, 2), D.epilogue(use), tol, src=got)
                dw = torch.zeros_like(D.wg)
                if attempt("wgrad_kept_v/" + name, case, lambda: (ops.conv_wgrad(torch.full_like(D.xg, float("nan")), D.gyg, dw, 1, 1, scale=D.scale.cuda(),
                                                                                  math=m, wino_v=v), True)[1]):
                    check("wgrad_kept_v/" + name, case, dw.permute(0, 3, 1, 2), D.w.grad, tol * 2)
                    if dw_ref is not None:      # against the self-contained call: 1e-5 max(1, max|dw|)
                        check("wgrad_kept_v=self/" + name, case, dw, dw_ref.cpu().double(), 1e-5)
        if (ci + 1) % 10 == 0:
            print("wino: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


REASONS = ["residual", "cout_not_32_split", "cout_not_4", "cin_not_32"]


def stratum_wino_wgrad_only(n, seed):
    rng = random.Random("%d/wino_wgrad_only" % seed)
    for ci in range(n):
        reason = REASONS[ci % len(REASONS)]       # one way off the forward route each, in turn
        if reason == "cout_not_32_split":
            case, modes = draw_wide(rng, Cout=rng.choice([132, 136, 200])), FULL[1:]     # (fp32 Winograd takes any Cout % 4 == 0)
        elif reason == "cout_not_4":
            case, modes = draw_wide(rng, Cout=rng.choice([129, 131, 133])), FULL
        elif reason == "cin_not_32":
            case, modes = draw_wide(rng, Cin=rng.choice([132, 136])), FULL
        else:
            case, modes = draw_wide(rng), FULL
        B, Cin, H, W, Cout, k, s, p = case
        cov["wino_wgrad_only"]["cases"] += 1
        use = dict(scale=rng.random() < 0.7, bias=rng.random() < 0.5, relu=rng.random() < 0.5, residual=reason == "residual")
        D = None if a.plan else Data(case, seed * 100003 + 2000003 + ci)
        for name, m, tol in modes:
            _, fw, ww, _ = ops.conv_route_info((B, H, W, Cin), (Cout, 3, 3, Cin), 1, 1, residual=PTR if use["residual"] else None, math=m)
            run_f = step("fwd", name, fw, "direct")
            run_w = step("wgrad", name, route_fwd(case, m)[2], "wino", reason=None if fw or not ww else reason)
            if run_f:
                got = attempt("fwd/" + name, case, lambda: ops.conv_forward(D.xg, D.wg, 1, 1, math=m, emit_amax=True, **D.kw(use)))
                if got is not None:
                    check("fwd/" + name, case + used(use), got.permute(0, 3, 1, 2), D.epilogue(use), tol, src=got)
            if run_w:
                # nothing is kept for a conv whose forward is direct (the residual is no part of the weight gradient's descriptor, so that
                # reason is asked with it) ...
                if reason != "residual" and ops.wino_v_alloc(D.xg, D.wg, 1, 1, m) is not None:
                    misrouted("wino_v_alloc is not None: %s %s" % (name, case))
                # ... and a wino_v handed to the weight gradient anyway is not read
                v = None if reason == "residual" else torch.full((36 * B * ((H + 3) // 4) * ((W + 3) // 4) * Cin,), float("nan"), device="cuda")
                dw = torch.zeros_like(D.wg)
                if attempt("wgrad/" + name, case, lambda: (ops.conv_wgrad(D.xg, D.gyg, dw, 1, 1, scale=D.scale.cuda(), math=m, wino_v=v), True)[1]):
                    check("wgrad/" + name, case, dw.permute(0, 3, 1, 2), D.w.grad, tol * 2)
        if (ci + 1) % 10 == 0:
            print("wino_wgrad_only: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


def ulp_err(y, y64, scale):
    ok = scale > 0
    return float(((y.detach().double().cpu() - y64).abs()[ok] / scale[ok]).max()) if bool(ok.any()) else 0.0


def check_f16(tag, case, e16, e32, src=None):
    """tests/test_gpu_f16_math.py's criterion: the error against float64 ON THE MODE'S ROUNDED OPERANDS is fp32 accumulation only: within
    max(2 x the fp32 kernel's on the same operands, 8 ulp) and below 32 ulp of sum |q(x)||q(w)|"""
    count(tag)
    if not (e16 <= max(2.0 * e32, 8 * EPS)) or not (e16 <= 32 * EPS):
        fails.append((tag, case, "f16 %.1f ulp, f32 on the same operands %.1f ulp of sum|q(x)||q(w)|" % (e16 / EPS, e32 / EPS)))
    if src is not None:
        check_amax(tag, case, src)


def stratum_f16(n, seed):
    from conv_ref import conv64, q16, wgrad64      # tests/conv_ref.py: the restatement tests/test_gpu_f16_math.py uses (only this stratum needs it)
    rng = random.Random("%d/f16" % seed)
    m, f32 = ops.MATH_F16, ops.MATH_F32
    for ci in range(n):
        if ci % 4 == 3:
            case = draw_wide(rng)
        else:
            while True:
                case = draw_any(rng)
                if case[1] % 32 == 0:
                    break
        B, Cin, H, W, Cout, k, s, p = case
        cov["f16"]["cases"] += 1
        use = dict(scale=rng.random() < 0.7, bias=rng.random() < 0.5, residual=rng.random() < 0.4, relu=rng.random() < 0.6)
        wide = ["wide3x3"] if (k == 3 and s == 1 and p == 1 and Cin >= 128 and Cout >= 128) else []
        D = None if a.plan else Data(case, seed * 100003 + 3000003 + ci)
        if D is not None:
            sc, bi, rs = D.scale.double(), D.bias.double(), D.res.double().permute(0, 2, 3, 1)
            qx, qw, qg = q16(D.xg), q16(D.wg, per_row=True), q16(D.gyg)
        # forward: the route must keep the arithmetic (Cin % 32 == 0) and never take Winograd
        rm, fw, _, wm = route_fwd(case, m, use["residual"])
        if rm != m:
            misrouted("forward of %s runs in %s" % (case, MATH_NAME[rm]))
        elif step("fwd", "f16", fw, "direct", wide):
            y64, s64 = conv64(qx, qw, s, p), conv64(qx.abs(), qw.abs(), s, p)
            if use["scale"]:
                y64, s64 = y64 * sc, s64 * sc.abs()
            if use["bias"]:
                y64, s64 = y64 + bi, s64 + bi.abs()
            if use["residual"]:
                y64, s64 = y64 + rs, s64 + rs.abs()
            if use["relu"]:
                y64 = torch.relu(y64)
            y16 = attempt("fwd/f16", case, lambda: ops.conv_forward(D.xg, D.wg, s, p, math=m, emit_amax=True, **D.kw(use)))
            if y16 is not None:
                y32 = ops.conv_forward(qx.float().cuda(), qw.float().cuda(), s, p, math=f32, **D.kw(use))
                check_f16("fwd/f16", case + used(use), ulp_err(y16, y64, s64), ulp_err(y32, y64, s64), src=y16)
        # weight gradient: any Cin % 4 == 0 stays in the mode
        if wm != m:
            misrouted("weight gradient of %s runs in %s" % (case, MATH_NAME[wm]))
        elif step("wgrad", "f16", route_fwd(case, m)[2], "direct", wide):
            dw16 = torch.zeros_like(D.wg)
            if attempt("wgrad/f16", case, lambda: (ops.conv_wgrad(D.xg, D.gyg, dw16, s, p, scale=D.scale.cuda(), math=m), True)[1]):
                sc4 = sc.view(-1, 1, 1, 1)
                d64, s64 = wgrad64(qx, qg, k, s, p) * sc4, wgrad64(qx.abs(), qg.abs(), k, s, p) * sc4.abs()
                dw32 = torch.zeros_like(D.wg)
                ops.conv_wgrad(qx.float().cuda(), qg.float().cuda(), dw32, s, p, scale=D.scale.cuda(), math=f32)
                check_f16("wgrad/f16", case, ulp_err(dw16, d64, s64), ulp_err(dw32, d64, s64))
        # input gradient: a forward call whose contraction runs over Cout -- in the mode when Cout % 32 == 0, else in fp32 (the library says which)
        if s == 1 or k == 1:
            rm, dwino, _, _ = route_dgrad(case, m)
            if rm == m and step("dgrad", "f16", dwino, "direct", wide):
                wt = attempt("dgrad/f16", case, lambda: ops.conv_dgrad_weights(D.wg, D.scale.cuda()))
                g16 = attempt("dgrad/f16", case, lambda: run_dgrad(D, case, m))
                if g16 is not None:
                    qwt = q16(wt, per_row=True)
                    pp = (k - 1 - p) if s == 1 else 0
                    y64, s64 = conv64(qg, qwt, 1, pp), conv64(qg.abs(), qwt.abs(), 1, pp)
                    kw = dict(out_hw=(H, W), out_stride=(s, s)) if s > 1 else {}
                    g32 = ops.conv_forward(qg.float().cuda(), qwt.float().cuda(), 1, pp, math=f32, **kw)
                    if s > 1:     # rows land on every s-th pixel of a zeroed tensor
                        z64, zs = torch.zeros(B, H, W, Cin, dtype=torch.float64), torch.zeros(B, H, W, Cin, dtype=torch.float64)
                        z64[:, ::s, ::s], zs[:, ::s, ::s] = y64, s64
                        y64, s64 = z64, zs
                    check_f16("dgrad/f16", case, ulp_err(g16, y64, s64), ulp_err(g32, y64, s64), src=g16)
            elif rm == f32 and step("dgrad", "f16->f32", dwino):
                dx = attempt("dgrad/f16->f32", case, lambda: run_dgrad(D, case, m))
                if dx is not None:
                    check("dgrad/f16->f32", case, dx.permute(0, 3, 1, 2), D.x.grad, 2e-4, src=dx)
        if (ci + 1) % 10 == 0:
            print("f16: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


def stratum_bf16_fallback(n, seed):
    rng = random.Random("%d/bf16_fallback" % seed)
    m, tol = ops.MATH_BF16, 1e-4          # the tolerance of the arithmetic the library says it runs in: fp32
    off64 = [c for c in CH + [108] if c % 64 != 0]
    for ci in range(n):
        while True:
            case = draw_any(rng)
            if case[5] != 7:
                break
        B, Cin, H, W, Cout, k, s, p = case
        if ci % 4 == 3:
            k, s, p, Cin, Cout = 3, 1, 1, rng.choice([160, 224]), rng.choice([160, 200])     # wide: fp32 may take Winograd here
        else:
            Cin, Cout = rng.choice(off64), rng.choice(off64)
        H, W = max(H, k - 2 * p), max(W, k - 2 * p)
        if Cin * k * k * Cout * H * W * B > 6e9:
            B, H, W = 1, min(H, 16), min(W, 16)
        case = (B, Cin, H, W, Cout, k, s, p)
        cov["bf16_fallback"]["cases"] += 1
        use = dict(scale=rng.random() < 0.7, bias=rng.random() < 0.5, residual=rng.random() < 0.4, relu=rng.random() < 0.6)
        D = None if a.plan else Data(case, seed * 100003 + 4000003 + ci)
        rm, fw, ww, wm = route_fwd(case, m, use["residual"])
        if rm != ops.MATH_F32 or wm != ops.MATH_F32:
            misrouted("%s runs in %s / %s" % (case, MATH_NAME[rm], MATH_NAME[wm]))
            continue
        if step("fwd", "bf16->f32", fw):
            got = attempt("fwd/bf16->f32", case, lambda: ops.conv_forward(D.xg, D.wg, s, p, math=m, emit_amax=True, **D.kw(use)))
            if got is not None:
                check("fwd/bf16->f32", case + used(use), got.permute(0, 3, 1, 2), D.epilogue(use), tol, src=got)
        if step("wgrad", "bf16->f32", route_fwd(case, m)[2]):
            dw = torch.zeros_like(D.wg)
            if attempt("wgrad/bf16->f32", case, lambda: (ops.conv_wgrad(D.xg, D.gyg, dw, s, p, scale=D.scale.cuda(), math=m), True)[1]):
                check("wgrad/bf16->f32", case, dw.permute(0, 3, 1, 2), D.w.grad, tol * 2)
        if s == 1 or k == 1:
            rm, dwino, _, _ = route_dgrad(case, m)
            if rm != ops.MATH_F32:
                misrouted("input gradient of %s runs in %s" % (case, MATH_NAME[rm]))
            elif step("dgrad", "bf16->f32", dwino):
                dx = attempt("dgrad/bf16->f32", case, lambda: run_dgrad(D, case, m))
                if dx is not None:
                    check("dgrad/bf16->f32", case, dx.permute(0, 3, 1, 2), D.x.grad, tol * 2, src=dx)
        if (ci + 1) % 10 == 0:
            print("bf16_fallback: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


def stratum_tail64(n, seed):
    rng = random.Random("%d/tail64" % seed)
    m = ops.MATH_BF16X6
    for ci in range(n):
        B = rng.randint(1, 4)
        H, W = (1 if rng.random() < 0.15 else rng.randint(1, 45) for _ in range(2))
        case = (B, 64, H, W, 256, 3, 1, 1)
        cov["tail64"]["cases"] += 1
        feats = (["one_pixel_row_or_column"] if H == 1 or W == 1 else []) + (["ragged_last_tile"] if (B * H * W) % 128 else [])
        fw2 = ops.conv_route_info((B, H, W, 64), (64, 3, 3, 64), 1, 1, math=m)
        fw3 = ops.conv_route_info((B, H, W, 64), (256, 1, 1, 64), 1, 0, residual=PTR, math=m)
        if fw2[0] != m or fw3[0] != m:
            misrouted("tail64 %s does not run in bf16x6" % (case,))
            continue
        if not step("tail64", "bf16x6", fw2[1] or fw3[1], "direct", feats):
            continue
        g = torch.Generator().manual_seed(seed * 100003 + 5000003 + ci)
        o1 = torch.relu(torch.randn(B, H, W, 64, generator=g))
        w2, w3 = torch.randn(64, 3, 3, 64, generator=g) * 0.06, torch.randn(256, 1, 1, 64, generator=g) * 0.15
        s2, b2 = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
        s3, b3 = torch.rand(256, generator=g) + 0.5, torch.randn(256, generator=g) * 0.2
        idt = torch.randn(B, H, W, 256, generator=g)
        x64 = o1.double().permute(0, 3, 1, 2)
        r2 = torch.relu(F.conv2d(x64, w2.double().permute(0, 3, 1, 2), padding=1) * s2.double().view(1, -1, 1, 1) + b2.double().view(1, -1, 1, 1))
        r3 = torch.relu(F.conv2d(r2, w3.double().permute(0, 3, 1, 2)) * s3.double().view(1, -1, 1, 1) + b3.double().view(1, -1, 1, 1)
                        + idt.double().permute(0, 3, 1, 2))
        o1, w2, w3, s2, b2, s3, b3, idt = (t.cuda() for t in (o1, w2, w3, s2, b2, s3, b3, idt))
        ops.conv_cache_clear()      # the library caches packed planes per (weight ADDRESS, w_version): fresh tensors may reuse an address
        ver = 500000 + ci
        if not ops.bottleneck_tail64_applies(o1, w2, w3, m):
            misrouted("bottleneck_tail64_applies refuses %s" % (case,))
            continue
        o2 = attempt("tail64/two calls", case, lambda: ops.conv_forward(o1, w2, 1, 1, scale=s2, bias=b2, relu=True, math=m, w_version=ver, emit_amax=True))
        want = attempt("tail64/two calls", case, lambda: ops.conv_forward(o2, w3, 1, 0, scale=s3, bias=b3, residual=idt, relu=True, math=m, w_version=ver, emit_amax=True))
        got = attempt("tail64/fused", case, lambda: ops.bottleneck_tail64(o1, w2, w3, s2, b2, s3, b3, idt, ver, ver))
        if want is None or got is None:
            continue
        check("tail64/fused bit-equal to two calls", case, got, want.cpu().double(), 0.0)
        check("tail64/fused", case, got.permute(0, 3, 1, 2), r3, 1e-4)
        check("tail64/two calls", case, want.permute(0, 3, 1, 2), r3, 1e-4, src=want)
        if (ci + 1) % 10 == 0:
            print("tail64: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


def stratum_dgrad_fused(n, seed):
    """the input gradient as the backward pass issues it: conv(gy, wt) with the producer's ReLU mask and / or the gradient of the other
    branch fused into the epilogue, y = (acc + residual) * (mask > 0) (include/abr_iod_hip.h)"""
    rng = random.Random("%d/dgrad_fused" % seed)
    KINDS = [dict(mask=True), dict(residual=True), dict(mask=True, residual=True)]
    for ci in range(n):
        while True:
            case = draw_any(rng)
            B, Cin, H, W, Cout, k, s, p = case
            if k != 7 and (s == 1 or k == 1) and Cout % 4 == 0:
                break
        cov["dgrad_fused"]["cases"] += 1
        kind = KINDS[ci % 3]
        feat = ["+".join(sorted(kind)) + (" scattered" if s > 1 else "")]
        D = None if a.plan else Data(case, seed * 100003 + 6000003 + ci)
        for name, m, tol in MODES:
            if not step("dgrad", name, route_dgrad(case, m, bool(kind.get("residual")))[1], None, feat):
                continue
            want = D.x.grad
            rs, mk = D.xres.double(), D.xmask.double()
            if s > 1:      # only the pixels the scatter writes exist
                z = torch.zeros_like(rs); z[:, :, ::s, ::s] = rs[:, :, ::s, ::s]; rs = z
            if kind.get("residual"):
                want = want + rs
            if kind.get("mask"):
                want = torch.where(mk > 0, want, torch.zeros_like(want))
            kw = dict(mask=nhwc(D.xmask) if kind.get("mask") else None, residual=nhwc(D.xres) if kind.get("residual") else None)
            dx = attempt("dgrad/" + name, case, lambda: run_dgrad(D, case, m, **kw))
            if dx is not None:
                check("dgrad/" + name, case + (feat[0],), dx.permute(0, 3, 1, 2), want, tol * 2, src=dx)
        if (ci + 1) % 10 == 0:
            print("dgrad_fused: %d cases, %d comparisons so far, %d failures" % (ci + 1, ran, len(fails)), flush=True)


RUN = dict(any=stratum_any, wino=stratum_wino, wino_wgrad_only=stratum_wino_wgrad_only, f16=stratum_f16, bf16_fallback=stratum_bf16_fallback,
           tail64=stratum_tail64, dgrad_fused=stratum_dgrad_fused)
for st in strata:
    cur[0] = st
    cov[st] = dict(cases=0, comparisons=0, misrouted=0, routes={}, features={}, reasons={}, fwd_dgrad={}, amax_checks={})
    RUN[st](a.cases if st == "any" else a.per_stratum, a.seed)
cur[0] = None

n_cases = sum(c["cases"] for c in cov.values())
print("\n%d cases (B, Cin, H, W, Cout, k, stride, pad), %d comparisons against float64; tolerances: f32 / bf16x6 1e-4 (2e-4 gradients), bf16 3e-2 of the output scale" % (n_cases, ran))
for st in strata:
    c = cov[st]
    print("stratum %s: cases %d, comparisons %d, misrouted %d%s" % (st, c["cases"], c["comparisons"], c["misrouted"], "  (planned, nothing run)" if a.plan else ""))
    for mode in sorted(c["routes"]):
        print("    %-10s %s" % (mode, "  ".join("%s %d" % kv for kv in sorted(c["routes"][mode].items()))))
    for reason in sorted(c["reasons"]):
        print("    off the forward route by %-18s %s" % (reason, "  ".join("%s %d" % kv for kv in sorted(c["reasons"][reason].items()))))
    if c["amax_checks"]:
        print("    amax words equal to max |result|: %s" % "  ".join("%s %d" % kv for kv in sorted(c["amax_checks"].items())))
print("COVERAGE " + json.dumps(cov, sort_keys=True))
print("refused (RuntimeError) configurations:")
for (tag, msg), cs in sorted(refused.items()):
    print("  %-14s %4d x  %s   e.g. %s" % (tag, len(cs), msg, cs[0]))
print("FAILURES: %d" % len(fails))
for f in fails[:40]:
    print("  ", f)
sys.exit(1 if fails else 0)

"""GPU: one deformable bottleneck (conv1 -> DFConv2d -> conv3 + identity) forward and backward -- o3, dx, dW1..3, dW_off, db_off -- under
f32 and f16x3 against a float64 restatement, and the zero-offset identities: with the offset conv zeroed, v1 is the plain bottleneck with
the same weights, v2 the plain bottleneck with conv2's weight halved (sigmoid(0) = 1/2)."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_dcn_kernels import deform_cols_ref

pytestmark = pytest.mark.gpu


def _randomize(blk, seed):
    from abr_iod_amd.layers import FrozenBatchNorm2d
    g = torch.Generator().manual_seed(seed)
    for m in blk.modules():
        if isinstance(m, FrozenBatchNorm2d):
            n = m.weight.numel()
            m.weight.copy_(torch.rand(n, generator=g) + 0.5)
            m.bias.copy_(torch.randn(n, generator=g) * 0.1)
            m.running_mean.copy_(torch.randn(n, generator=g) * 0.1)
            m.running_var.copy_(torch.rand(n, generator=g) + 0.5)
            m.invalidate()


def _block(cin, c, cout, stride, dcn, math, seed=0):
    from abr_iod_amd.modeling.backbone.resnet import Bottleneck
    torch.manual_seed(seed)
    blk = Bottleneck(cin, c, cout, stride, dcn=dcn)
    _randomize(blk, seed + 1)
    if dcn is not None:
        with torch.no_grad():   # offsets of a few pixels: a non-trivial sampling pattern
            blk.conv2.offset.weight.mul_(4.0)
            blk.conv2.offset.bias[: blk.conv2.offset.out_channels].uniform_(-1.5, 1.5)
    blk = blk.cuda()
    blk.math = math
    # fresh weights, possibly at the address of an earlier test's: nothing the library derived from those may be reused
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    bump_param_version()
    return blk


def _run(blk, x_nhwc, R):
    from abr_iod_amd.layers._layout import from_nhwc, as_nhwc
    from abr_iod_amd.modeling.backbone.resnet import run_stage
    for p in blk.parameters():
        p.grad = None
    x = from_nhwc(x_nhwc.clone()).requires_grad_(True)
    out = run_stage(x, [blk])
    loss = (as_nhwc(out) * R).sum()
    loss.backward()
    torch.cuda.synchronize()
    return as_nhwc(out).detach(), x.grad.permute(0, 2, 3, 1).contiguous(), loss.item()


def _ref(blk, x_nhwc, R):
    """float64 restatement of the block; returns (o3, dx, {param name: grad}) in this package's storage layouts"""
    d = lambda t: t.detach().double()
    sb = lambda bn: (d(bn.scale_bias()[0]).view(1, -1, 1, 1), d(bn.scale_bias()[1]).view(1, -1, 1, 1))
    x = d(x_nhwc).permute(0, 3, 1, 2).requires_grad_(True)
    w1 = blk.conv1.oihw().double().requires_grad_(True)
    w3 = blk.conv3.oihw().double().requires_grad_(True)
    off, dc = blk.conv2.offset, blk.conv2.conv
    C = dc.out_channels
    woff = off.oihw().double().requires_grad_(True)
    boff = d(off.bias)[: off.out_channels].requires_grad_(True)
    w2 = d(dc.weight).view(C, 9 * C).requires_grad_(True)
    s1, b1 = sb(blk.bn1)
    s2, b2 = sb(blk.bn2)
    s3, b3 = sb(blk.bn3)
    o1 = torch.relu(F.conv2d(x, w1, stride=blk.stride) * s1 + b1)
    om = F.conv2d(o1, woff, boff, padding=1).permute(0, 2, 3, 1)
    cols = deform_cols_ref(o1.permute(0, 2, 3, 1), om, blk.conv2.deformable_groups, blk.conv2.modulated)
    o2 = torch.relu((cols @ w2.t()).permute(0, 3, 1, 2) * s2 + b2)
    idt = x
    params = [x, w1, woff, boff, w2, w3]
    if blk.downsample is not None:
        wd = blk.downsample[0].oihw().double().requires_grad_(True)
        sd, bd = sb(blk.downsample[1])
        idt = F.conv2d(x, wd, stride=blk.stride) * sd + bd
        params.append(wd)
    o3 = torch.relu(F.conv2d(o2, w3) * s3 + b3 + idt)
    loss = (o3 * d(R).permute(0, 3, 1, 2)).sum()
    grads = torch.autograd.grad(loss, params)
    g = dict(zip(["x", "conv1", "offset.w", "offset.b", "conv2", "conv3", "ds"], grads))
    return o3.detach().permute(0, 2, 3, 1), g


def _close(got, want, tol, name):
    want = want.to(got.device)
    err = (got.double() - want).abs().max().item()
    scale = want.abs().max().item()
    print("{}: error/bound {:.3f}".format(name, err / (tol * scale + 1e-30)))
    assert err <= tol * scale + 1e-30, "{}: max error {:.3g} against max |ref| {:.3g}".format(name, err, scale)


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("modulated,dg", [(False, 1), (False, 2), (True, 1), (False, 4), (False, 16)])
def test_block_vs_float64(math, modulated, dg):
    from abr_iod_amd import ops
    m = {"f32": ops.MATH_F32, "f16x3": ops.MATH_F16X3}[math]
    # dg = 4, 16 at bottleneck width 64: 16 and 4 channels per deformable group, the offset conv's output padded 72 -> 96 and 288 -> 288
    width = 64 if dg >= 4 else 128
    blk = _block(256, width, 512, 2, (modulated, dg), m, seed=3)
    torch.manual_seed(9)
    x = torch.relu(torch.randn(2, 14, 18, 256, device="cuda"))
    R = torch.randn(2, 7, 9, 512, device="cuda")
    o3, dx, _ = _run(blk, x, R)
    ro3, g = _ref(blk, x, R)
    tol = 2e-5 if math == "f32" else 1e-4
    _close(o3, ro3, tol, "o3")
    _close(dx, g["x"].permute(0, 2, 3, 1), tol, "dx")
    _close(blk.conv1.ref_layout(blk.conv1.weight.grad), g["conv1"], tol, "dW1")
    _close(blk.conv2.conv.weight.grad.view(width, 9 * width), g["conv2"], tol, "dW2")
    _close(blk.conv3.ref_layout(blk.conv3.weight.grad), g["conv3"], tol, "dW3")
    _close(blk.downsample[0].ref_layout(blk.downsample[0].weight.grad), g["ds"], tol, "dWds")
    off = blk.conv2.offset
    _close(off.ref_layout(off.weight.grad), g["offset.w"], tol, "dW_off")
    _close(off.bias.grad[: off.out_channels], g["offset.b"], tol, "db_off")
    # the padding rows of the offset conv get exactly zero gradient
    assert torch.count_nonzero(off.weight.grad[off.out_channels:]) == 0 and torch.count_nonzero(off.bias.grad[off.out_channels:]) == 0


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("modulated", [False, True])
def test_zero_offsets_equal_plain_block(math, modulated):
    from abr_iod_amd import ops
    m = {"f32": ops.MATH_F32, "f16x3": ops.MATH_F16X3}[math]
    D = _block(256, 64, 256, 1, (modulated, 1), m, seed=5)
    P = _block(256, 64, 256, 1, None, m, seed=5)
    with torch.no_grad():
        D.conv2.offset.weight.zero_()
        D.conv2.offset.bias.zero_()
        for a, b in ((P.conv1, D.conv1), (P.conv3, D.conv3)):
            a.weight.copy_(b.weight)
        # v1: the same 3x3 weight; v2: the mask is sigmoid(0) = 1/2 everywhere, so the plain block's conv2 is halved (exact)
        P.conv2.weight.copy_(D.conv2.conv.weight.view(P.conv2.weight.shape) * (0.5 if modulated else 1.0))
        for a, b in zip(P.buffers(), D.buffers()):
            a.copy_(b)
    for mod in (P, D):
        for bn in mod.modules():
            if hasattr(bn, "invalidate"):
                bn.invalidate()
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    bump_param_version()
    torch.manual_seed(4)
    x = torch.relu(torch.randn(2, 13, 17, 256, device="cuda"))
    R = torch.randn(2, 13, 17, 256, device="cuda")
    po, pdx, pl = _run(P, x, R)
    do, ddx, dl = _run(D, x, R)
    assert abs(dl - pl) <= 1e-5 * max(1.0, abs(pl)), (dl, pl)
    tol = 2e-5 if math == "f32" else 1e-4
    _close(do, po.double(), tol, "o3")
    _close(ddx, pdx.double(), tol, "dx")
    _close(D.conv1.weight.grad, P.conv1.weight.grad.double(), tol, "dW1")
    _close(D.conv3.weight.grad, P.conv3.weight.grad.double(), tol, "dW3")
    f = 0.5 if modulated else 1.0
    _close(D.conv2.conv.weight.grad.view(P.conv2.weight.shape) * (1 / f), P.conv2.weight.grad.double() * 1.0, tol, "dW2")
    # the offset conv still learns: its gradient is non-zero and is the restatement's
    off = D.conv2.offset
    assert torch.count_nonzero(off.weight.grad) > 0
    _, g = _ref(D, x, R)
    _close(off.ref_layout(off.weight.grad), g["offset.w"], tol, "dW_off")
    _close(off.bias.grad[: off.out_channels], g["offset.b"], tol, "db_off")

"""The mask loss against float64 BCE, with the tolerances both GPU mask test files hold it to (tests/test_gpu_mask_head.py on the recorded
fixture, tests/test_gpu_mask_kernels.py at the kernel's edges)."""
import torch

EPS = 2.0 ** -24
MEASURED = {"loss rel to addends": 0.0, "grad of its bound": 0.0}     # the worst seen in this process, for the record tests print


def check_loss(logits_nchw, labels, targets, n_pos=None, tag="", gscale=1.0, ldk=None):
    """logits [P,K,M,M] fp32 (CPU), labels [P] (outside (0, K): skipped), targets [P,M,M] against float64 BCE; tolerances of
    test_gpu_loss_kernels.py: 1e-6 relative to the sum of |addends| for the loss, a few ulps of the largest term for each gradient element.
    ldk: the row stride of the device logits (None: K rounded up to 4); gscale multiplies the gradient and leaves the loss alone;
    want_grad=False must give the same loss bits."""
    from abr_iod_amd import ops
    P, K, M, _ = logits_nchw.shape
    ld = (K + 3) // 4 * 4 if ldk is None else ldk
    z = torch.zeros(P, M, M, ld)
    z[..., :K] = logits_nchw.permute(0, 2, 3, 1)
    args = (z.cuda(), K, labels.cuda(), targets.cuda())
    nd = None if n_pos is None else torch.tensor([n_pos], dtype=torch.int32, device="cuda")
    loss, grad = ops.mask_loss(*args, n_pos=nd, gscale=gscale, want_grad=True)
    loss2, grad2 = ops.mask_loss(*args, n_pos=nd, gscale=gscale, want_grad=True)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2), tag + ": two runs differ"
    loss3, grad3 = ops.mask_loss(*args, n_pos=nd, gscale=gscale, want_grad=False)
    assert grad3 is None and torch.equal(loss3, loss), tag + ": want_grad=False changes the loss"
    pos = ((labels > 0) & (labels < K)).nonzero().flatten()
    n = P if n_pos is None else n_pos          # (ops.mask_loss: without a device count the mean is over all P rows, skipped ones included)
    x64 = logits_nchw.double()
    if n == 0 or len(pos) == 0:
        assert float(loss) == 0.0 and not bool(grad.any()), tag
        return float(loss)
    sel = x64[pos, labels[pos]]
    t64 = targets.double()[pos]
    terms = sel.clamp(min=0) - sel * t64 + torch.log1p(torch.exp(-sel.abs()))
    want = terms.sum() / (n * M * M)
    # (the analytic gradient: autograd through max(x, 0) and |x| takes a one-sided derivative at x == 0, where the loss is smooth)
    want_grad = torch.zeros_like(x64)
    want_grad[pos, labels[pos]] = (torch.sigmoid(sel) - t64) / (n * M * M) * gscale
    addends = float(terms.abs().sum() / (n * M * M))
    rel = abs(float(loss) - float(want)) / max(addends, 1e-300)
    print(tag, "loss", float(loss), "float64", float(want), "rel to addends", rel)
    assert abs(float(loss) - float(want)) <= 1e-6 * addends + 1e-30, tag
    got = grad.cpu()[..., :K].permute(0, 3, 1, 2).double()
    gtol = 8 * EPS / (n * M * M)
    gerr = float((got - want_grad).abs().max())
    assert gerr <= gtol, (tag, gerr, gtol)
    assert not bool(grad.cpu()[..., K:].any())
    MEASURED["loss rel to addends"] = max(MEASURED["loss rel to addends"], rel)
    MEASURED["grad of its bound"] = max(MEASURED["grad of its bound"], gerr / gtol)
    return float(loss)

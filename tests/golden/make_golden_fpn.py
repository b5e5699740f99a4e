#!/usr/bin/env python3
"""FPN golden FROM THE REFERENCE (in-container only): the reference's own modeling/backbone/fpn.py `FPN` with
conv_with_kaiming_uniform(False, False) and `LastLevelMaxPool`, run on the CPU in float32 over the maps of tests/fpn_ref.py: B = 2,
in-channels (8, 16, 32, 64), out-channels 8, maps 24 x 40, 12 x 20, 6 x 10 and 3 x 5 (P6 is then 2 x 3, an odd top size).

The weights are the reference's kaiming_uniform_(a=1) draw under torch.manual_seed(seed); the biases, which the reference initialises to zero,
are redrawn from U(-0.5, 0.5) so that their path is exercised.  The loss is sum_l <P_l, R_l> over P2..P6 with the seeded R_l of fpn_ref.

Stored as tests/golden/fpn.npz (data only): seed; w_<name> / b_<name> per conv in the reference's OIHW layout; p_0 .. p_4 (NCHW);
gx_0 .. gx_3 (the gradients of C2..C5); gw_<name> / gb_<name>.  The inputs are NOT stored: fpn_ref.golden_inputs(seed) regenerates them."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_harness as rh  # noqa: E402
import fpn_ref as F  # noqa: E402


def main():
    rh.setup()
    from maskrcnn_benchmark.modeling.backbone.fpn import FPN, LastLevelMaxPool
    from maskrcnn_benchmark.modeling.make_layers import conv_with_kaiming_uniform
    seed = F.GOLDEN_SEED
    torch.manual_seed(seed)
    fpn = FPN(list(F.GOLDEN_IN), F.GOLDEN_OUT, conv_with_kaiming_uniform(False, False), LastLevelMaxPool())
    with torch.no_grad():
        for name, p in fpn.named_parameters():
            if name.endswith(".bias"):
                p.uniform_(-0.5, 0.5)
    xs_np, rs_np = F.golden_inputs(seed)
    xs = [torch.from_numpy(x).requires_grad_(True) for x in xs_np]
    ps = fpn(xs)
    assert len(ps) == len(rs_np)
    loss = sum((p * torch.from_numpy(r)).sum() for p, r in zip(ps, rs_np))
    loss.backward()
    out = dict(seed=np.int64(seed))
    for i, p in enumerate(ps):
        out["p_%d" % i] = p.detach().numpy()
    for i, x in enumerate(xs):
        out["gx_%d" % i] = x.grad.numpy()
    for name, p in fpn.named_parameters():
        mod, kind = name.rsplit(".", 1)
        out[("w_" if kind == "weight" else "b_") + mod] = p.detach().numpy()
        out[("gw_" if kind == "weight" else "gb_") + mod] = p.grad.numpy()
    path = os.path.join(HERE, "fpn.npz")
    np.savez_compressed(path, **out)
    print("seed", seed, "keys", len(out), "bytes", os.path.getsize(path), "P shapes", [tuple(p.shape) for p in ps])


if __name__ == "__main__":
    main()

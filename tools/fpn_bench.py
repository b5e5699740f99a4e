"""Per-call time of the FPN neck's fused top-down launches (abr_fpn_topdown_forward / _backward: one launch each) and of the whole neck
(modeling/backbone/fpn.py: forward, and forward + backward) at an FPN-shaped call, next to the reference's per-level procedure built from
torch ops in the same process.

Shape: B = 2, an 800 x 1344 image, C = 256, maps 200 x 336 (P2), 100 x 168, 50 x 84, 25 x 42 (P5), NHWC; the neck's inputs C2..C5 carry
256, 512, 1024 and 2048 channels.

The yardstick is modeling/backbone/fpn.py:59-64 as the reference runs it: per level F.interpolate(last_inner, scale_factor=2, mode="nearest")
and an add (2 launches per level below the top, 6 for four levels), and autograd's backward of that chain (per level
upsample_nearest2d_backward and an add: 6 launches), on channels-last tensors.  "neck" rows run the same FPN module twice: as built, and with
the two fused launches swapped for those per-level procedures (the convs are this library's in both).

Bytes are algorithmic: forward = every lateral read once, every inner below the top written once; backward = every gradient read once, every
lateral gradient above the finest written once (the finest is aliased).  `hbm` is bytes / time over the 8 TB/s peak.  Device events around
--reps back-to-back calls.  Prints the table, then one JSON line.

    python tools/fpn_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

B, C = 2, 256
MAPS = [(200, 336), (100, 168), (50, 84), (25, 42)]
IN_CHANNELS = (256, 512, 1024, 2048)
HBM_PEAK_GBS = 8000.0


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3   # us


def torch_topdown_forward(lats):
    """the reference's chain on NHWC tensors (seen as channels-last NCHW)"""
    last = lats[-1].permute(0, 3, 1, 2)
    out = [lats[-1]]
    for lat in lats[-2::-1]:
        last = lat.permute(0, 3, 1, 2) + F.interpolate(last, scale_factor=2, mode="nearest")
        out.insert(0, last.permute(0, 2, 3, 1))
    return out


def torch_topdown_backward(grads, inplace=False):
    """what autograd runs for that chain: per level upsample_nearest2d_backward of the finer level's gradient, and an add"""
    out = [grads[0]]
    t = grads[0].permute(0, 3, 1, 2)
    for g in grads[1:]:
        Bn, H, W, Cn = g.shape
        t = g.permute(0, 3, 1, 2) + torch.ops.aten.upsample_nearest2d_backward(t, [2 * H, 2 * W], [Bn, Cn, H, W], 2.0, 2.0)
        out.append(t.permute(0, 2, 3, 1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import ctypes
    from abr_iod_amd import _lib as L
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.fpn import FPN, LastLevelMaxPool
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    lats = [torch.randn(B, H, W, C, device="cuda", generator=g) for H, W in MAPS]
    grads = [torch.randn(B, H, W, C, device="cuda", generator=g) for H, W in MAPS]
    n = len(MAPS)
    nbytes = [4 * t.numel() for t in lats]
    fwd_b = sum(nbytes) + sum(nbytes[:-1])
    bwd_b = sum(nbytes) + sum(nbytes[1:])
    Hs, Ws = (ctypes.c_int * n)(*[h for h, _ in MAPS]), (ctypes.c_int * n)(*[w for _, w in MAPS])
    outs = [torch.empty_like(t) for t in lats]

    def fused_forward_kept():      # into caller-kept buffers: the launch alone, without the allocator
        L.check(L.lib().abr_fpn_topdown_forward((ctypes.c_void_p * n)(*[t.data_ptr() for t in lats]), (ctypes.c_void_p * n)(*[t.data_ptr() for t in outs]),
                                                Hs, Ws, n, B, C, L.stream()), "fpn_topdown_forward")

    def fused_backward_kept():
        L.check(L.lib().abr_fpn_topdown_backward((ctypes.c_void_p * n)(*[t.data_ptr() for t in grads]),
                                                 (ctypes.c_void_p * n)(*([grads[0].data_ptr()] + [t.data_ptr() for t in outs[1:]])),
                                                 Hs, Ws, n, B, C, L.stream()), "fpn_topdown_backward")

    # the two procedures agree before they are timed: forward bit for bit, backward to rounding (autograd's kernel sums in another order)
    for x, y in zip(ops.fpn_topdown_forward(lats), torch_topdown_forward(lats)):
        assert torch.equal(x, y)
    for x, y in zip(ops.fpn_topdown_backward(grads), torch_topdown_backward(grads)):
        assert float((x - y).abs().max()) <= 1e-5 * float(y.abs().max())

    rows = []

    def row(name, us, bytes_=None, launches=None):
        r = {"call": name, "us": round(us, 1), "launches": launches}
        if bytes_ is not None:
            r.update(bytes=int(bytes_), GBs=round(bytes_ / us / 1e3, 1), hbm=round(bytes_ / us / 1e3 / HBM_PEAK_GBS, 3))
        rows.append(r)

    row("top-down forward, fused", timed(fused_forward_kept, a.reps), fwd_b, 1)
    row("top-down forward, fused (ops, allocating)", timed(lambda: ops.fpn_topdown_forward(lats), a.reps), fwd_b, 1)
    row("top-down forward, per level (torch)", timed(lambda: torch_topdown_forward(lats), a.reps), fwd_b, 2 * (n - 1))
    row("top-down backward, fused", timed(fused_backward_kept, a.reps), bwd_b, 1)
    row("top-down backward, fused (ops, allocating)", timed(lambda: ops.fpn_topdown_backward(grads), a.reps), bwd_b, 1)
    row("top-down backward, per level (torch)", timed(lambda: torch_topdown_backward(grads), a.reps), bwd_b, 2 * (n - 1))

    # the whole neck in the library's default arithmetic
    torch.manual_seed(0)
    fpn = FPN(list(IN_CHANNELS), C, LastLevelMaxPool()).cuda()
    fpn.math = ops.default_conv_math()
    xs = [torch.randn(B, c, H, W, device="cuda", generator=g).contiguous(memory_format=torch.channels_last).requires_grad_(True)
          for c, (H, W) in zip(IN_CHANNELS, MAPS)]
    gouts = [torch.randn(B, C, H, W, device="cuda", generator=g).contiguous(memory_format=torch.channels_last)
             for H, W in MAPS + [((MAPS[-1][0] - 1) // 2 + 1, (MAPS[-1][1] - 1) // 2 + 1)]]

    def neck_forward():
        with torch.no_grad():
            return fpn(xs)

    def neck_both():
        for p in fpn.parameters():
            p.grad = None if p.grad is None else p.grad.zero_()
        for x in xs:
            x.grad = None
        torch.autograd.backward(fpn(xs), gouts)
        ops.join_side_stream()

    fused = (ops.fpn_topdown_forward, ops.fpn_topdown_backward)
    for name, fns in (("fused", fused), ("per level (torch)", (torch_topdown_forward, torch_topdown_backward))):
        ops.fpn_topdown_forward, ops.fpn_topdown_backward = fns
        try:
            row("neck forward, top-down " + name, timed(neck_forward, a.reps))
            row("neck forward + backward, top-down " + name, timed(neck_both, a.reps))
        finally:
            ops.fpn_topdown_forward, ops.fpn_topdown_backward = fused

    print(f"maps {MAPS} x {C} (B = {B}); neck inputs {IN_CHANNELS} channels, arithmetic {fpn.math}")
    print(f"{'call':46s} {'us':>9s} {'launches':>9s} {'GB/s':>8s} {'of HBM':>7s}")
    for r in rows:
        print(f"{r['call']:46s} {r['us']:9.1f} {str(r['launches'] or '-'):>9s} {r.get('GBs', float('nan')):8.1f} {r.get('hbm', float('nan')):7.3f}")
    print(json.dumps({"maps": MAPS, "B": B, "C": C, "in_channels": IN_CHANNELS, "hbm_peak_GBs": HBM_PEAK_GBS, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()

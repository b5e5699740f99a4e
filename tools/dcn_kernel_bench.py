"""Per-launch time of the two deformable-conv kernels (abr_deform_im2col, abr_deform_col2im_coord) at the body's shapes for B = 4, 600x1000:
layer1 (150000 pixels x 64 channels), layer2 (37500 x 128), layer3 (9576 x 256), DCNv2 with offsets of about a pixel.  Device events around
--reps back-to-back launches.  Bytes are algorithmic: im2col reads x and the offset field once and writes the columns; col2im_coord reads the
column gradient, x and the offset field once, writes d_om, and adds 4 corners x 9 taps x C floats per pixel by atomics (reported apart).
Prints one JSON line.

    python tools/dcn_kernel_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {"layer1": (150, 250, 64), "layer2": (75, 125, 128), "layer3": (38, 63, 256)}
B, COM = 4, 32
HBM_PEAK_GBS, ATOMIC_GBS = 8000.0, 1300.0


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from abr_iod_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"B": B, "mode": "v2 (27 of 32 offset channels)", "hbm_peak_GBs": HBM_PEAK_GBS, "atomic_ref_GBs": ATOMIC_GBS}
    for name, (H, W, C) in SHAPES.items():
        P = B * H * W
        x = torch.relu(torch.randn(B, H, W, C, device="cuda", generator=g))
        om = torch.randn(B, H, W, COM, device="cuda", generator=g)
        dcol = torch.randn(B, H, W, 9 * C, device="cuda", generator=g)
        us_f = timed(lambda: ops.deform_im2col(x, om, 1, True), a.reps)
        us_b = timed(lambda: ops.deform_col2im_coord(dcol, x, om, 1, True), a.reps)
        by_f = 4 * P * (9 * C + C + COM)
        by_b = 4 * P * (9 * C + C + 2 * COM)
        by_at = 4 * P * 36 * C
        # (the backward's time includes zeroing dx: 4 P C bytes written by a fill kernel ahead of it)
        res[name] = {"pixels": P, "C": C,
                     "im2col": {"us": round(us_f, 1), "bytes": by_f, "GBs": round(by_f / us_f / 1e3, 1), "hbm_fraction": round(by_f / us_f / 1e3 / HBM_PEAK_GBS, 3)},
                     "col2im_coord": {"us": round(us_b, 1), "bytes": by_b, "atomic_bytes": by_at,
                                      "atomic_GBs": round(by_at / us_b / 1e3, 1), "atomic_fraction": round(by_at / us_b / 1e3 / ATOMIC_GBS, 3),
                                      "plain_GBs": round(by_b / us_b / 1e3, 1)}}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

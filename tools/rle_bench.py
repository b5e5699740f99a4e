"""Run-length codec on the device (csrc/rle.hip) at VOC-like sizes, beside the host codec.  Informational: nothing is asserted.

For each (h, w, instances) it reports the device time of ops.rle_decode (uint8 and packed) and ops.rle_encode (uint8 and packed input) --
whole calls, upload / read-back included, from a host clock around a synchronise, median over --iters after --warmup -- the algorithmic
bytes (compressed characters + 4 bytes per run end + the masks written or read once), those bytes over the HBM peak (8 TB/s spec,
MI355X; abr_device_info gives the CU count, it has no bandwidth field), and the time of the host codec on the same data.  One JSON line.

    python tools/rle_bench.py --iters 20 --warmup 5
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK = 8.0e12
CASES = [(375, 500, 8), (500, 375, 20), (600, 1000, 8), (375, 500, 100)]     # (h, w, instances): ground truth, and 100 detections


def ellipses(rng, n, H, W):
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((n, H, W), np.uint8)
    for i in range(n):
        cx, cy, rx, ry = rng.uniform(0.1, 0.9) * W, rng.uniform(0.1, 0.9) * H, rng.uniform(0.05, 0.3) * W, rng.uniform(0.05, 0.3) * H
        out[i] = ((xs - cx) / rx) ** 2 + ((ys - cy) / ry) ** 2 <= 1
    return out


def call_us(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    from abr_iod_amd import _lib as L
    from abr_iod_amd import ops
    from abr_iod_amd.structures import rle as R
    assert torch.cuda.is_available(), "rle_bench measures the device codec: it needs the GPU"
    info = (ctypes.c_int32 * 8)()
    L.check(L.lib().abr_device_info(info), "device_info")
    rng = np.random.default_rng(0)
    rows = []
    for h, w, n in CASES:
        masks = ellipses(rng, n, h, w)
        t0 = time.perf_counter()
        rles = R.encode(masks)
        host_encode = time.perf_counter() - t0
        t0 = time.perf_counter()
        back = R.decode(rles, (h, w))
        host_decode = time.perf_counter() - t0
        dev = torch.from_numpy(masks).cuda()
        bits = ops.mask_pack_bits(dev)
        chars = sum(len(r["counts"]) for r in rles)
        runs = sum(len(R.string_to_counts(r["counts"])) for r in rles)
        u8_bytes, packed_bytes = n * h * w, bits.numel() * 8
        ok = bool(np.array_equal(back, masks)) and ops.rle_encode(dev) == rles and bool(torch.equal(ops.rle_decode(rles, (h, w), "cuda"), dev))
        row = {"hw": [h, w], "instances": n, "characters": chars, "runs": runs, "device_equals_host": ok,
               "host_decode_us": host_decode * 1e6, "host_encode_us": host_encode * 1e6}
        for name, fn, moved in [("decode_u8", lambda: ops.rle_decode(rles, (h, w), "cuda"), chars + 4 * chars + u8_bytes),
                                ("decode_packed", lambda: ops.rle_decode(rles, (h, w), "cuda", packed=True), chars + 4 * chars + packed_bytes),
                                ("encode_u8", lambda: ops.rle_encode(dev), u8_bytes + 2 * n * ((h * w + 63) // 64) * 8 + 8 * runs + chars),
                                ("encode_packed", lambda: ops.rle_encode(bits, width=w), packed_bytes + 2 * n * ((h * w + 63) // 64) * 8 + 8 * runs + chars)]:
            us = call_us(fn, args.iters, args.warmup)
            row[name + "_us"] = us
            row[name + "_bytes"] = int(moved)
            row[name + "_hbm_frac"] = moved / (us * 1e-6) / HBM_PEAK
        rows.append(row)
    print(json.dumps({"tool": "rle_bench", "cus": int(info[0]), "hbm_peak_bytes_per_s": HBM_PEAK, "timing": "whole call, host clock around a synchronise",
                      "cases": rows}))


if __name__ == "__main__":
    main()

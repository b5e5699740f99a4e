"""Per-call time of the feature-pyramid pooler (abr_roi_align_pyramid_forward / _backward: one launch each) at an FPN-shaped call, next to the
reference's per-level procedure built from this library's single-level operators in the same process.

Shape: B = 2, an 800 x 1344 image, maps 200 x 336, 100 x 168, 50 x 84, 25 x 42 (NHWC, C = 256), 512 RoIs per image with log-uniform
sizes, sampling_ratio 2; pooled 7 x 7 (the box head's pooler) and 14 x 14 (the mask head's).

The yardstick is modeling/poolers.py:99-103 as the reference runs it: per level a `nonzero` (a blocking device-to-host copy of the count), a
row gather, ops.roi_align_forward, an indexed write into a zero-filled result; backward: per level a gather of the gradient rows and
ops.roi_align_backward(method="scatter").  `host_syncs` counts the blocking copies one call makes.

Bytes are algorithmic -- every map once, the rois and the pooled tensor once -- so GB/s is the rate a kernel that touched nothing twice would
show; `hbm` is that rate over the 8 TB/s peak.  For the backward, `atomic` is the rate of bytes ADDED by float atomics over the chip-wide
float-atomic rate of 1.3 TB/s (the constants of tools/roi_pool_bench.py); the fused backward adds float64 (8 bytes per add, into scratch it
zeroes first and rounds to the gradients in a second launch -- both inside its time), the per-level scatter float32 (4 bytes); the separable
kernel (7 x 7) issues one add per channel and footprint pixel of every RoI, the direct kernel (14 x 14) four per channel, bin and sample.  Device events around --reps back-to-back calls.
Prints the table, then one JSON line.

    python tools/pyramid_pool_bench.py --reps 20
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IMG_H, IMG_W, C, PER_IMG, SR = 2, 800, 1344, 256, 512, 2
MAPS = [(200, 336), (100, 168), (50, 84), (25, 42)]
SCALES = (0.25, 0.125, 0.0625, 0.03125)
K_MIN, K_MAX = 2.0, 5.0
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


def proposals(g):
    K = B * PER_IMG
    side = torch.exp(torch.empty(K, device="cuda").uniform_(math.log(16.0), math.log(1000.0), generator=g))
    ar = torch.exp(torch.empty(K, device="cuda").uniform_(math.log(0.5), math.log(2.0), generator=g))
    w, h = (side * ar.sqrt()).clamp(max=IMG_W - 1.0), (side / ar.sqrt()).clamp(max=IMG_H - 1.0)
    x1 = torch.rand(K, device="cuda", generator=g) * (IMG_W - 1.0 - w)
    y1 = torch.rand(K, device="cuda", generator=g) * (IMG_H - 1.0 - h)
    b = torch.arange(K, device="cuda").div(PER_IMG, rounding_mode="floor").float()
    return torch.stack([b, x1, y1, x1 + w, y1 + h], 1).contiguous()


def footprint_pixels(rois, levels):
    """pixels of its level's map that every RoI's samples can touch (rows x columns of the bilinear footprint)"""
    total = 0
    for l, ((H, W), s) in enumerate(zip(MAPS, SCALES)):
        r = rois[levels == l].double() * s
        nx = (r[:, 3].floor().clamp(max=W - 1) + 2).clamp(max=W) - r[:, 1].floor().clamp(min=0)
        ny = (r[:, 4].floor().clamp(max=H - 1) + 2).clamp(max=H) - r[:, 2].floor().clamp(min=0)
        total += int((nx.clamp(min=1) * ny.clamp(min=1)).sum().item())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from abr_iod_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    feats = [torch.randn(B, H, W, C, device="cuda", generator=g) for H, W in MAPS]
    shapes = [tuple(f.shape) for f in feats]
    rois = proposals(g)
    K = rois.shape[0]
    levels = ops.fpn_levels(rois, K_MIN, K_MAX)
    per_level = torch.bincount(levels.long(), minlength=len(MAPS)).tolist()
    maps_b = sum(4 * f.numel() for f in feats)
    fp = footprint_pixels(rois, levels)
    rows = []

    def row(name, P, us, bytes_, atomic_bytes=None, host_syncs=0):
        r = {"call": name, "pooled": P, "us": round(us, 1), "bytes": int(bytes_), "GBs": round(bytes_ / us / 1e3, 1),
             "hbm": round(bytes_ / us / 1e3 / HBM_PEAK_GBS, 3), "host_syncs": host_syncs}
        if atomic_bytes is not None:
            r["atomic_bytes"] = int(atomic_bytes)
            r["atomic_GBs"] = round(atomic_bytes / us / 1e3, 1)
            r["atomic"] = round(atomic_bytes / us / 1e3 / ATOMIC_GBS, 3)
        rows.append(r)

    for P in (7, 14):
        grad = torch.randn(K, P, P, C, device="cuda", generator=g)
        out_b = 4 * grad.numel() + 4 * rois.numel()
        adds = float(C) * fp if P <= 8 else float(C) * K * P * P * SR * SR * 4
        gbufs = [torch.empty(s, device="cuda") for s in shapes]
        syncs = [0]

        def per_level_forward():
            lv = ops.fpn_levels(rois, K_MIN, K_MAX)
            result = torch.zeros((K, P, P, C), device="cuda")
            idxs = []
            for l, (f, s) in enumerate(zip(feats, SCALES)):
                idx = torch.nonzero(lv == l).squeeze(1)      # the blocking copy
                syncs[0] += 1
                idxs.append(idx)
                result[idx] = ops.roi_align_forward(f, rois[idx], s, P, P, SR)
            return result, idxs

        _, idxs = per_level_forward()

        def per_level_backward():
            return [ops.roi_align_backward(grad[idx], rois[idx], s, P, P, SR, *shp[:3], C, method="scatter")
                    for idx, s, shp in zip(idxs, SCALES, shapes)]

        def fused_backward():      # into caller-kept buffers, zero-filled by the callee: what one autograd backward costs without the allocator
            from abr_iod_amd import _lib as L
            import ctypes
            n = len(gbufs)
            L.check(L.lib().abr_roi_align_pyramid_backward(
                L.ptr(grad), L.ptr(rois), K, B, C, (ctypes.c_int * n)(*[s[1] for s in shapes]), (ctypes.c_int * n)(*[s[2] for s in shapes]),
                (ctypes.c_float * n)(*SCALES), n, P, P, SR, K_MIN, K_MAX, 224.0, 4.0, 1e-6, 0, (ctypes.c_void_p * n)(*[t.data_ptr() for t in gbufs]),
                L.stream()), "roi_align_pyramid_backward")

        row("fused forward", P, timed(lambda: ops.roi_align_pyramid_forward(feats, rois, SCALES, P, P, SR, K_MIN, K_MAX), a.reps), maps_b + out_b)
        syncs[0] = 0
        us = timed(per_level_forward, a.reps)
        row("per-level forward", P, us, maps_b + out_b, host_syncs=syncs[0] // (a.reps + 1))
        row("fused backward", P, timed(fused_backward, a.reps), maps_b + out_b, 8 * adds)
        row("fused backward (ops, allocating)", P,
            timed(lambda: ops.roi_align_pyramid_backward(grad, rois, SCALES, P, P, SR, shapes, K_MIN, K_MAX), a.reps), maps_b + out_b, 8 * adds)
        row("per-level backward (scatter)", P, timed(per_level_backward, a.reps), maps_b + out_b, 4 * adds)

    print(f"maps {MAPS} x {C} (B = {B}), {K} RoIs, rows per level {per_level}, sampling_ratio {SR}, footprint pixels {fp}")
    print(f"{'call':36s} {'P':>3s} {'us':>9s} {'GB/s':>8s} {'of HBM':>7s} {'atomic GB/s':>12s} {'of 1.3 TB/s':>12s} {'host syncs':>11s}")
    for r in rows:
        print(f"{r['call']:36s} {r['pooled']:3d} {r['us']:9.1f} {r['GBs']:8.1f} {r['hbm']:7.3f} {r.get('atomic_GBs', float('nan')):12.1f} "
              f"{r.get('atomic', float('nan')):12.3f} {r['host_syncs']:11d}")
    print(json.dumps({"maps": MAPS, "B": B, "C": C, "rois": K, "rows_per_level": per_level, "sampling_ratio": SR, "footprint_pixels": fp,
                      "hbm_peak_GBs": HBM_PEAK_GBS, "atomic_ref_GBs": ATOMIC_GBS, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()

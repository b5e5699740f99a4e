"""Polygon masks on the device (csrc/poly.hip) at VOC-like sizes, beside the host codec and the bitmask route.  Informational: nothing is
asserted.

Whole images: for each (h, w, instances, vertices) the time of ops.poly_rasterize (uint8 and packed) -- whole calls from a host clock
around a synchronise, median over --iters after --warmup -- the algorithmic bytes (vertices read, one toggle plane per polygon written,
scanned in place and read once, the masks written once), those bytes over the HBM peak (8 TB/s spec, MI355X), and the time of the host
codec (structures/polygon.py) on the same polygons.

RoI targets: ops.poly_mask_targets against ops.mask_targets on the same instances pre-rasterised (the route MODEL.MASK_ON took before
polygons), at the RoI counts of the flagship configuration (4 images x 128 positives at most), for M = 14 and M = 8.  Both move a few
hundred kilobytes; they are bound by launch and per-RoI latency, so no share of the HBM peak is given for them.  One JSON line.

    python tools/poly_bench.py --iters 20 --warmup 5
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
CASES = [(375, 500, 1, 8), (375, 500, 8, 40), (375, 500, 32, 200), (600, 1000, 1, 8), (600, 1000, 8, 40), (600, 1000, 32, 200)]   # (h, w, instances, vertices)
ROI_IMAGES, ROI_POS_PER_IMAGE = 4, 128


def blobs(rng, n, h, w, k):
    """n star-shaped k-gons inside an h x w image"""
    out = []
    for _ in range(n):
        cx, cy = rng.uniform(0.15, 0.85) * w, rng.uniform(0.15, 0.85) * h
        r = rng.uniform(0.05, 0.3) * min(h, w) * rng.uniform(0.7, 1.3, k)
        a = np.sort(rng.uniform(0, 2 * np.pi, k))
        out.append([np.stack((cx + r * np.cos(a), cy + r * np.sin(a)), 1).astype(np.float32).reshape(-1).tolist()])
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
    from abr_iod_amd.structures.polygon import PolygonList
    assert torch.cuda.is_available(), "poly_bench measures the device kernels: it needs the GPU"
    info = (ctypes.c_int32 * 8)()
    L.check(L.lib().abr_device_info(info), "device_info")
    rng = np.random.default_rng(0)
    images = []
    for h, w, n, k in CASES:
        host = PolygonList(blobs(rng, n, h, w, k), (w, h))
        t0 = time.perf_counter()
        want = ops.poly_rasterize(host)
        host_us = (time.perf_counter() - t0) * 1e6
        dev = host.to("cuda")
        ok = bool(torch.equal(ops.poly_rasterize(dev).cpu(), want))
        plane = ((h * w + 64) // 64) * 8
        row = {"hw": [h, w], "instances": n, "vertices_per_instance": k, "device_equals_host": ok, "host_us": host_us}
        for name, fn, out_bytes in [("u8", lambda: ops.poly_rasterize(dev), n * h * w), ("packed", lambda: ops.poly_rasterize(dev, packed=True), n * h * ((w + 63) // 64) * 8)]:
            us = call_us(fn, args.iters, args.warmup)
            moved = n * k * 8 + n * plane * 4 + out_bytes      # plane: zeroed, scanned (read + write), read by the output pass
            row[name + "_us"] = us
            row[name + "_bytes"] = int(moved)
            row[name + "_hbm_frac"] = moved / (us * 1e-6) / HBM_PEAK
        row["host_over_device_u8"] = host_us / row["u8_us"]
        images.append(row)

    # RoI targets: 4 images of 600 x 1000 with 1..5 instances, 128 RoIs per image jittered around the ground truth
    h, w = 600, 1000
    polys, masks, gts, rois = [], [], [], []
    for img in range(ROI_IMAGES):
        n = 1 + img % 5
        pl = PolygonList(blobs(rng, n, h, w, 24), (w, h), device="cuda")
        gt = torch.stack([torch.cat((torch.cat(pl.polygons_of(i)).min(0)[0], torch.cat(pl.polygons_of(i)).max(0)[0])) for i in range(n)])
        polys.append(pl)
        masks.append(ops.poly_rasterize(pl))
        gts.append(gt)
        pick = torch.from_numpy(rng.integers(0, n, ROI_POS_PER_IMAGE)).cuda()
        jit = torch.from_numpy(rng.normal(0, 8, (ROI_POS_PER_IMAGE, 4))).float().cuda()
        b = gt[pick] + jit
        b = torch.stack((torch.minimum(b[:, 0], b[:, 2]), torch.minimum(b[:, 1], b[:, 3]), torch.maximum(b[:, 0], b[:, 2]), torch.maximum(b[:, 1], b[:, 3])), 1)
        rois.append(torch.cat((torch.full((ROI_POS_PER_IMAGE, 1), float(img), device="cuda"), b), 1))
    rois = torch.cat(rois)
    pos_rows = torch.arange(rois.shape[0], device="cuda")
    targets = []
    for M in (14, 8):
        poly_us = call_us(lambda: ops.poly_mask_targets(polys, gts, rois, pos_rows, M), args.iters, args.warmup)
        bit_us = call_us(lambda: ops.mask_targets(masks, gts, rois, pos_rows, M), args.iters, args.warmup)
        a, b = ops.poly_mask_targets(polys, gts, rois, pos_rows, M), ops.mask_targets(masks, gts, rois, pos_rows, M)
        targets.append({"M": M, "rois": int(rois.shape[0]), "poly_mask_targets_us": poly_us, "mask_targets_us": bit_us, "poly_over_bitmask": poly_us / bit_us,
                        "pixels_differing_between_routes": float((a != b).float().mean())})
    print(json.dumps({"tool": "poly_bench", "cus": int(info[0]), "hbm_peak_bytes_per_s": HBM_PEAK, "timing": "whole call, host clock around a synchronise",
                      "images": images, "roi_targets": targets}))


if __name__ == "__main__":
    main()

"""Per-launch time of the RoI poolers of csrc/roi_pool.hip alone, at the model's shape: map [4, 38, 63, 1024] (NHWC), 2048 RoIs (512 per
image, proposal-like: log-uniform sizes inside a 600 x 1000 image), 7 x 7 bins.  ROIPool forward / backward; deformable PS-RoI pooling
forward / backward with sample_per_part 4, group_size 1, without offsets (no_trans), with offsets, and with offsets and mask logits.
ops.roi_align_forward / ops.roi_align_backward (the training step's gather form and the atomic scatter form) run at the same shape in the
same process as the yardstick.  Device events around --reps back-to-back launches.

Bytes are algorithmic -- the map once, every other operand and result once -- so GB/s is the rate a kernel that touched nothing twice would
show; `hbm` is that rate over the 8 TB/s peak.  For the backward kernels `atomic` is the rate of bytes ADDED by float atomics over the
chip-wide float-atomic rate of 1.3 TB/s.  Prints the table, then one JSON line.

    python tools/roi_pool_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, H, W, C, K, P, SPP, SCALE = 4, 38, 63, 1024, 2048, 7, 4, 0.0625
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
    per = K // B
    w = torch.exp(torch.empty(K, device="cuda").uniform_(2.77, 6.4, generator=g))      # 16 .. 600 px
    h = torch.exp(torch.empty(K, device="cuda").uniform_(2.77, 6.0, generator=g))      # 16 .. 400 px
    x1 = torch.rand(K, device="cuda", generator=g) * (1000.0 - w).clamp(min=0)
    y1 = torch.rand(K, device="cuda", generator=g) * (600.0 - h).clamp(min=0)
    b = torch.arange(K, device="cuda").div(per, rounding_mode="floor").float()
    return torch.stack([b, x1, y1, (x1 + w).clamp(max=999.0), (y1 + h).clamp(max=599.0)], 1).contiguous()


def psroi_touched_pixels(rois, trans, tstd):
    """(bin, pixel) pairs the PS-RoI backward adds to, per channel: a bin's samples put their gradient on (distinct rows) x (distinct columns)"""
    r = rois.double()
    x0, y0 = torch.floor(r[:, 1] + 0.5) * SCALE - 0.5, torch.floor(r[:, 2] + 0.5) * SCALE - 0.5
    rw = ((torch.floor(r[:, 3] + 0.5) + 1) * SCALE - 0.5 - x0).clamp(min=0.1)
    rh = ((torch.floor(r[:, 4] + 0.5) + 1) * SCALE - 0.5 - y0).clamp(min=0.1)
    p = torch.arange(P, device="cuda", dtype=torch.float64)
    i = torch.arange(SPP, device="cuda", dtype=torch.float64)
    tx = trans[:, 0].double() * tstd if trans is not None else 0.0
    ty = trans[:, 1].double() * tstd if trans is not None else 0.0
    e = (slice(None), None, None)
    ws = p[None, None, :] * (rw / P)[e] + x0[e] + tx * rw[e]                 # [K, ph, pw]
    hs = p[None, :, None] * (rh / P)[e] + y0[e] + ty * rh[e]

    def distinct(start, step, L):
        v = start[..., None] + i * step[:, None, None, None]
        ok = ((v >= -0.5) & (v <= L - 0.5)).int()
        v = v.clamp(0, L - 1)
        m = torch.zeros(v.shape[:-1] + (L,), dtype=torch.int32, device="cuda")
        m.scatter_add_(-1, v.floor().long(), ok)
        m.scatter_add_(-1, v.ceil().long(), ok)
        return (m > 0).sum(-1)

    return int((distinct(ws, rw / P / SPP, W) * distinct(hs, rh / P / SPP, H)).sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from abr_iod_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    feat = torch.randn(B, H, W, C, device="cuda", generator=g)
    rois = proposals(g)
    grad = torch.randn(K, P, P, C, device="cuda", generator=g)
    trans = torch.empty(K, 2, P, P, device="cuda").uniform_(-1, 1, generator=g)
    logits = torch.randn(K, P, P, device="cuda", generator=g)
    gbuf = torch.zeros_like(feat)
    map_b, out_b = 4 * feat.numel(), 4 * grad.numel()
    rows = []

    def row(name, us, bytes_, atomic_bytes=None):
        r = {"kernel": name, "us": round(us, 1), "bytes": int(bytes_), "GBs": round(bytes_ / us / 1e3, 1), "hbm": round(bytes_ / us / 1e3 / HBM_PEAK_GBS, 3)}
        if atomic_bytes is not None:
            r["atomic_bytes"] = int(atomic_bytes)
            r["atomic_GBs"] = round(atomic_bytes / us / 1e3, 1)
            r["atomic"] = round(atomic_bytes / us / 1e3 / ATOMIC_GBS, 3)
        rows.append(r)

    # ---- the yardstick
    row("roi_align forward", timed(lambda: ops.roi_align_forward(feat, rois, SCALE, P, P, 0), a.reps), map_b + out_b)
    row("roi_align backward (gather)", timed(lambda: ops.roi_align_backward(grad, rois, SCALE, P, P, 0, B, H, W, C), a.reps), out_b + map_b)
    row("roi_align backward (scatter)", timed(lambda: ops.roi_align_backward(grad, rois, SCALE, P, P, 0, B, H, W, C, method="scatter"), a.reps),
        out_b + map_b)
    # ---- ROIPool: values and argmax out; backward reads both and adds one float per output with an argmax (into a buffer it zeroes first)
    out, am = ops.roi_pool_forward(feat, rois, SCALE, P, P)
    row("roi_pool forward", timed(lambda: ops.roi_pool_forward(feat, rois, SCALE, P, P), a.reps), map_b + 2 * out_b)
    live = int((am != -1).sum().item())
    row("roi_pool backward", timed(lambda: ops.roi_pool_backward(grad, rois, am, B, H, W), a.reps), 2 * out_b + map_b, 4 * live)
    # pixels a bin scans per output (what the forward reads through the caches): the RoI's footprint over its bins
    s = (rois[:, 1:] * SCALE).round()
    scanned = float((((s[:, 2] - s[:, 0] + 1).clamp(min=1) / P).ceil() * ((s[:, 3] - s[:, 1] + 1).clamp(min=1) / P).ceil()).mean().item())
    # ---- deformable PS-RoI pooling: out and top_count out; backward reads grad, top_count and the map and adds one float per touched pixel, bin and channel
    for name, t, m in (("no_trans", None, None), ("trans", trans, None), ("trans + mask", trans, logits)):
        o, cnt = ops.deform_psroi_forward(feat, rois, t, SCALE, C, 1, P, P, SPP, 0.1, mask_logits=m)
        row(f"deform_psroi forward ({name})", timed(lambda: ops.deform_psroi_forward(feat, rois, t, SCALE, C, 1, P, P, SPP, 0.1, mask_logits=m), a.reps),
            map_b + 2 * out_b)
        adds = 4.0 * C * psroi_touched_pixels(rois, t, 0.1)     # one float per channel and touched pixel of every bin
        row(f"deform_psroi backward ({name})",
            timed(lambda: ops.deform_psroi_backward(grad, feat, rois, t, cnt, SCALE, C, 1, P, P, SPP, 0.1, mask_logits=m, out=gbuf), a.reps),
            2 * out_b + 2 * map_b, adds)
    print(f"map [{B}, {H}, {W}, {C}], {K} RoIs, {P} x {P} bins, sample_per_part {SPP}; ROIPool scans {scanned:.1f} pixels per bin on average")
    print(f"{'kernel':44s} {'us':>9s} {'GB/s':>8s} {'of HBM':>7s} {'atomic GB/s':>12s} {'of 1.3 TB/s':>12s}")
    for r in rows:
        print(f"{r['kernel']:44s} {r['us']:9.1f} {r['GBs']:8.1f} {r['hbm']:7.3f} {r.get('atomic_GBs', float('nan')):12.1f} {r.get('atomic', float('nan')):12.3f}")
    print(json.dumps({"shape": [B, H, W, C], "rois": K, "bins": P, "sample_per_part": SPP, "roi_pool_pixels_per_bin": round(scanned, 2),
                      "hbm_peak_GBs": HBM_PEAK_GBS, "atomic_ref_GBs": ATOMIC_GBS, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()

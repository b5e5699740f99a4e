"""Per-launch time of the two general deformable-conv kernels (abr_deform_im2col_general, abr_deform_col2im_coord_general) alone, at layer2's
and layer3's B = 4 shapes (600x1000 images: 75 x 125 x 128 and 38 x 63 x 256) for 3x3 s1 p1, 3x3 s2 p1 and 3x3 d2 p2, with a mask and offsets
of about a pixel.  The specialised kernels (abr_deform_im2col, abr_deform_col2im_coord: 3x3 s1 p1 only, the mask as logits) run in the same
process at the shared geometry as the yardstick, and the general-to-specialised ratio is reported.  Device events around --reps back-to-back
launches.  Bytes are algorithmic: im2col reads x, the offsets and the mask once and writes the columns; col2im_coord reads the column
gradient, x, the offsets and the mask once, writes d_offset and d_mask, and adds 4 corners x K taps x C floats per output pixel by atomics
(reported apart, against the chip-wide float-atomic rate); its time includes zeroing dx.  Prints one JSON line.

    python tools/deform_conv_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

SHAPES = {"layer2": (75, 125, 128), "layer3": (38, 63, 256)}
GEOMETRIES = {"3x3_s1_p1": dict(kernel=(3, 3), stride=(1, 1), padding=(1, 1), dilation=(1, 1)),
              "3x3_s2_p1": dict(kernel=(3, 3), stride=(2, 2), padding=(1, 1), dilation=(1, 1)),
              "3x3_d2_p2": dict(kernel=(3, 3), stride=(1, 1), padding=(2, 2), dilation=(2, 2))}
B = 4
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


def entry(us_f, us_b, by_f, by_b, by_at):
    return {"im2col": {"us": round(us_f, 1), "bytes": by_f, "GBs": round(by_f / us_f / 1e3, 1), "hbm_fraction": round(by_f / us_f / 1e3 / HBM_PEAK_GBS, 3)},
            "col2im_coord": {"us": round(us_b, 1), "bytes": by_b, "atomic_bytes": by_at, "atomic_GBs": round(by_at / us_b / 1e3, 1),
                             "atomic_fraction": round(by_at / us_b / 1e3 / ATOMIC_GBS, 3), "plain_GBs": round(by_b / us_b / 1e3, 1)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    from abr_iod_amd import ops
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = {"B": B, "mode": "modulated, one deformable group, one conv group", "hbm_peak_GBs": HBM_PEAK_GBS, "atomic_ref_GBs": ATOMIC_GBS}
    for name, (H, W, C) in SHAPES.items():
        x = torch.relu(torch.randn(B, H, W, C, device="cuda", generator=g))
        res[name] = {"C": C}
        for gname, geo in GEOMETRIES.items():
            Ho, Wo = ops.deform_out_size(H, W, **geo)
            P = B * Ho * Wo
            offset = torch.randn(B, Ho, Wo, 18, device="cuda", generator=g)
            logits = torch.randn(B, Ho, Wo, 9, device="cuda", generator=g)
            mask = torch.sigmoid(logits)
            dcol = torch.randn(1, P, 9 * C, device="cuda", generator=g)
            us_f = timed(lambda: ops.deform_im2col_general(x, offset, mask, **geo), a.reps)
            us_b = timed(lambda: ops.deform_col2im_coord_general(dcol, x, offset, mask, **geo), a.reps)
            by_f = 4 * (P * (9 * C + 27) + B * H * W * C)
            by_b = 4 * (P * (9 * C + 2 * 27) + B * H * W * C)
            e = res[name][gname] = {"out_pixels": P, "general": entry(us_f, us_b, by_f, by_b, 4 * P * 36 * C)}
            if gname == "3x3_s1_p1":      # the specialised kernels' only geometry: the same offsets, the mask as its logits, the field padded to 32
                om = torch.cat([offset, logits, torch.zeros(B, H, W, 5, device="cuda")], -1)
                dcol_s = dcol.view(B, H, W, 9 * C)
                us_sf = timed(lambda: ops.deform_im2col(x, om, 1, True), a.reps)
                us_sb = timed(lambda: ops.deform_col2im_coord(dcol_s, x, om, 1, True), a.reps)
                e["specialised"] = entry(us_sf, us_sb, 4 * P * (9 * C + C + 32), 4 * P * (9 * C + C + 64), 4 * P * 36 * C)
                e["general_over_specialised"] = {"im2col": round(us_f / us_sf, 3), "col2im_coord": round(us_b / us_sb, 3)}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

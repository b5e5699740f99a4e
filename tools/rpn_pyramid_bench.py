"""Per-call time of the multi-level RPN proposal selection (RPNPostProcessor over a pyramid: abr_rpn_pyramid_topk / _decode,
abr_nms_sorted_batched over the N * L segments, abr_rpn_pyramid_select; one read-back of N counts) at an FPN-shaped call, next to the
reference's per-level procedure built from this library's single-level operators in the same process.

Shape: B = 2 (--images for more), an 800 x 1344 image, maps 200 x 336, 100 x 168, 50 x 84, 25 x 42, 13 x 21, A = 3 anchors per location in a
fused head output of ld = 16 columns, pre 2000, post 2000, fpn post 2000; both selection modes (per image = test, per batch = training).
Logits are normal, deltas normal * 0.5 (boxes of neighbouring locations overlap, so the NMS has work to do).

The yardstick is rpn/inference.py:120-176 as the reference runs it: per level ops.topk_sigmoid (torch sigmoid + topk where a level has more
keys than that operator admits: 196 608; the 200 x 336 level has 201 600), ops.rpn_decode_clip, ops.nms_sorted_batched over the N images and a
read-back of its counts to cut the lists; then torch for the cross-level step (per batch: cat, topk, mask scatter, a boolean index per image;
per image: topk and an index).  `host_syncs` counts the blocking device-to-host copies of one call, `launches` the device kernels and memsets
of one call as torch.profiler sees them (None where the profiler is unavailable).  Device events around --reps back-to-back calls.
Prints the table, then one JSON line.

    python tools/rpn_pyramid_bench.py --reps 20
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

IMG_H, IMG_W, A, LD = 800, 1344, 3, 16
MAPS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
STRIDES, SIZES, RATIOS = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)
PRE, POST, FPN_POST, NMS_THRESH = 2000, 2000, 2000, 0.7
TOPK_MAX_KEYS = 196608


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


def count_launches(fn):
    """device kernels + memsets + copies of one call, or None"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower())
        return n or None
    except Exception:
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.box_coder import BoxCoder
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator, RPNPostProcessor
    from abr_iod_amd.structures.image_list import ImageList
    torch.cuda.set_device(0)
    B = a.images
    g = torch.Generator(device="cuda").manual_seed(0)
    fused = []
    for H, W in MAPS:
        y = torch.randn(B, H, W, LD, device="cuda", generator=g)
        y[..., A:5 * A] *= 0.5
        fused.append(y.permute(0, 3, 1, 2))                       # logical [B,ld,H,W], channels-last memory
    yfs = [f.permute(0, 2, 3, 1).reshape(B, -1, LD) for f in fused]
    ag = AnchorGenerator(SIZES, RATIOS, STRIDES, 0).cuda()
    sizes = [(IMG_H, IMG_W)] * B
    anchors = ag(ImageList(torch.zeros(B, 3, IMG_H, IMG_W, device="cuda"), sizes), fused)
    grids = [anchors[0][l].bbox for l in range(len(MAPS))]
    img_hw = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    syncs = [0]
    rows = []

    def selector(per_batch):
        pp = RPNPostProcessor(PRE, POST, NMS_THRESH, 0, BoxCoder((1.0, 1.0, 1.0, 1.0)), FPN_POST, per_batch)
        pp.train(per_batch)
        return pp

    def one_pass(pp):
        pending = pp.launch(anchors, fused, A)
        n = pending["n_out"].tolist()                              # the only blocking copy
        syncs[0] += 1
        return [pending["rois"][i, :n[i]] for i in range(B)]

    def per_level(per_batch):
        boxes, scores = [[] for _ in range(B)], [[] for _ in range(B)]
        for yf, grid in zip(yfs, grids):
            n = yf.shape[1] * A
            k = min(PRE, n)
            if n <= TOPK_MAX_KEYS:
                sc, idx = ops.topk_sigmoid(yf, A, k)
            else:
                sc, idx = yf[:, :, :A].reshape(B, n).sigmoid().topk(k, dim=1, sorted=True)
            props = ops.rpn_decode_clip(yf, A, grid, idx, img_hw, (1.0, 1.0, 1.0, 1.0), A=A)
            keep, n_keep = ops.nms_sorted_batched(props, torch.full((B,), k, dtype=torch.int32, device="cuda"), NMS_THRESH, POST)
            nk = n_keep.tolist()                                   # blocking: the lists are cut on the host, level by level
            syncs[0] += 1
            for i in range(B):
                ki = keep[i, :nk[i]].long()
                boxes[i].append(props[i].index_select(0, ki))
                scores[i].append(sc[i].index_select(0, ki))
        boxes, scores = [torch.cat(b) for b in boxes], [torch.cat(s) for s in scores]
        if per_batch:                                              # inference.py:157-168
            obj = torch.cat(scores)
            top = torch.topk(obj, min(FPN_POST, obj.numel()), dim=0, sorted=True)[1]
            mask = torch.zeros_like(obj, dtype=torch.bool)
            mask[top] = True
            out = []
            for b, m in zip(boxes, mask.split([len(s) for s in scores])):
                out.append(b[m])                                   # a boolean index: nonzero, a blocking copy of the count
                syncs[0] += 1
            return out
        return [b[torch.topk(s, min(FPN_POST, s.numel()), dim=0, sorted=True)[1]] for b, s in zip(boxes, scores)]   # :169-176

    for per_batch in (False, True):
        mode = "per batch (training)" if per_batch else "per image (test)"
        pp = selector(per_batch)
        for name, fn in (("one pass over the pyramid", lambda: one_pass(pp)), ("per level + torch", lambda: per_level(per_batch))):
            out = fn()
            syncs[0] = 0
            us = timed(fn, a.reps)
            rows.append({"call": name, "mode": mode, "us": round(us, 1), "host_syncs": syncs[0] // (a.reps + 1),
                         "launches": None if a.no_launch_count else count_launches(fn), "proposals": [int(len(o)) for o in out]})

    print(f"maps {MAPS} x A = {A} (ld = {LD}), B = {B}, pre {PRE}, post {POST}, fpn post {FPN_POST}, NMS {NMS_THRESH}")
    print(f"{'call':28s} {'mode':22s} {'us':>10s} {'launches':>9s} {'host syncs':>11s}  proposals")
    for r in rows:
        print(f"{r['call']:28s} {r['mode']:22s} {r['us']:10.1f} {str(r['launches']):>9s} {r['host_syncs']:11d}  {r['proposals']}")
    print(json.dumps({"maps": MAPS, "B": B, "A": A, "ld": LD, "pre": PRE, "post": POST, "fpn_post": FPN_POST, "nms": NMS_THRESH, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()

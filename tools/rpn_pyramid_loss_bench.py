"""Per-call time of the RPN loss over a feature pyramid, forward plus backward, two ways in one process:

  (a) one pass: ops.rpn_pyramid_loss (abr_rpn_pyramid_loss: both losses in one launch, compact gradient records) and
      ops.rpn_pyramid_loss_backward (one memset over the levels' gradients, one scatter launch);
  (b) per level: the same result composed from the single-level operators -- per level the sampled indices translated to level-local ones
      (torch), ops.rpn_loss_indices, ops.bce_logits_gather, ops.smooth_l1_rows (each with a zero-filled dense gradient the size of the
      level's head output), the level losses added, and in backward ops.scale_, ops.scale_, ops.add_ per level.  A third row times (b)
      with the translated lists prepared outside the timed region: what remains is the library's single-level operators alone.

Shape: R-50-FPN's five maps for an 800 x 1344 image (200 x 336 .. 13 x 21), A = 3 anchors per location in a fused head output of Cf = 16
columns, B = 2 (--images for more), normal logits and deltas, four ground-truth boxes per image of 40 .. 500 pixels, targets from
ops.rpn_targets_batched over the concatenated anchors and one draw of the sampler (256 per image, half positive at most), shared by both.
Matching and sampling are outside the timed region: they are the same calls for both.

The candidates alternate in rounds (a, b, b', a, b, b', ...); per round device events around --reps back-to-back calls; the table gives the
median, the range over the rounds, and per call the device kernels, memsets and copies as torch.profiler sees them in a separate pass.
`zeroed` is the bytes of gradient storage each call zero-fills, computed from the shapes ((b): two dense buffers per level).
Prints the table, then one JSON line.

    python tools/rpn_pyramid_loss_bench.py --reps 50 --rounds 7
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

IMG_H, IMG_W, A, CF = 800, 1344, 3, 16
MAPS = [(200, 336), (100, 168), (50, 84), (25, 42), (13, 21)]
STRIDES, SIZES, RATIOS = (4, 8, 16, 32, 64), (32, 64, 128, 256, 512), (0.5, 1.0, 2.0)
BATCH, FRACTION, HI, LO = 256, 0.5, 0.7, 0.3


def timed(fn, reps):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3   # us


def count_device_events(fn):
    """(kernels, memsets, copies) of one call as torch.profiler sees them, or (None, None, None)"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name.lower() for e in prof.events() if getattr(e, "device_type", None) is not None and "cuda" in str(e.device_type).lower()]
        if not names:
            return None, None, None
        sets = sum("memset" in n for n in names)
        copies = sum("memcpy" in n for n in names)
        return len(names) - sets - copies, sets, copies
    except Exception:
        return None, None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--images", type=int, default=2)
    ap.add_argument("--no-launch-count", action="store_true")
    a = ap.parse_args()
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.rpn.rpn import AnchorGenerator
    torch.cuda.set_device(0)
    B, nL = a.images, len(MAPS)
    g = torch.Generator(device="cuda").manual_seed(0)
    ys = []
    for H, W in MAPS:
        y = torch.randn(B, H, W, CF, device="cuda", generator=g)
        y[..., A:5 * A] *= 0.5
        ys.append(y)
    ag = AnchorGenerator(SIZES, RATIOS, STRIDES, 0).cuda()
    boxes, vis, offs = ag.pyramid(MAPS, (IMG_H, IMG_W))
    n = offs[-1]
    cpu = torch.Generator().manual_seed(1)
    gts = []
    for _ in range(B):
        side = torch.tensor([40.0, 90.0, 200.0, 500.0]) * (0.8 + 0.4 * torch.rand(4, generator=cpu))
        x0, y0 = torch.rand(4, generator=cpu) * (IMG_W - side), torch.rand(4, generator=cpu) * (IMG_H - side)
        gts.append(torch.stack([x0, y0, x0 + side - 1, y0 + 0.8 * side - 1], 1).cuda())
    lab2d, tgt3d, _keep = ops.rpn_targets_batched(boxes, [vis] * B, gts, HI, LO, (1.0, 1.0, 1.0, 1.0))
    pos, neg, counts = ops.sample_pos_neg(lab2d, BATCH, int(BATCH * FRACTION), index_offset_per_image=n, seed=7)
    lab_flat, tgt_flat = lab2d.view(-1), tgt3d.view(-1, 4)
    pos_flat = pos.reshape(-1)
    samp_flat = torch.cat([pos_flat, neg.reshape(-1)])
    g_obj, g_box = torch.tensor(0.7, device="cuda"), torch.tensor(1.3, device="cuda")
    shapes = [tuple(y.shape) for y in ys]
    level_bytes = [y.numel() * 4 for y in ys]

    def one_pass():
        losses, rec = ops.rpn_pyramid_loss(ys, A, lab2d, tgt3d, pos, neg, counts, want_grad=True)
        grads = ops.rpn_pyramid_loss_backward(shapes, A, rec, pos.shape[1], neg.shape[1], g_obj, g_box, ys[0].device)
        return losses, grads

    def level_lists():
        """the sampled indices translated to level-local ones (-1 where the anchor lies on another level), per level"""
        i_p, i_n = torch.div(pos, n, rounding_mode="floor"), torch.div(neg, n, rounding_mode="floor")
        j_p, j_n = pos - i_p * n, neg - i_n * n
        out = []
        for l in range(nL):
            n_l = offs[l + 1] - offs[l]
            m_p = (pos >= 0) & (j_p >= offs[l]) & (j_p < offs[l + 1])
            m_n = (neg >= 0) & (j_n >= offs[l]) & (j_n < offs[l + 1])
            out.append((torch.where(m_p, i_p * n_l + (j_p - offs[l]), -1), torch.where(m_n, i_n * n_l + (j_n - offs[l]), -1)))
        return out

    given = level_lists()

    def per_level(lists=None):
        lists = level_lists() if lists is None else lists
        lo_l, lb_l, g_l = [], [], []
        for (pos_l, neg_l), y in zip(lists, ys):
            samp, obj_flat, prow, pcol, denom = ops.rpn_loss_indices(pos_l, neg_l, counts, A, CF)
            y2 = y.view(-1, CF)
            lo, go = ops.bce_logits_gather(y2, lab_flat, obj_flat, want_grad=True, yidx=samp_flat, denom_dev=denom)
            lb, gr = ops.smooth_l1_rows(y2, tgt_flat, prow, pcol, 1.0 / 9, scale=1.0, want_grad=True, trows=pos_flat, denom_dev=denom)
            lo_l.append(lo[0])
            lb_l.append(lb[0])
            g_l.append((go, gr))
        losses = torch.stack([torch.stack(lo_l).sum(), torch.stack(lb_l).sum()])
        grads = []
        for (go, gr), shp in zip(g_l, shapes):          # backward: the single-level route's three passes, per level
            ops.scale_(go, 1.0, g_obj)
            ops.scale_(gr, 1.0, g_box)
            ops.add_(go, gr)
            grads.append(go.view(shp))
        return losses, grads

    la, ga = one_pass()
    lb_, gb = per_level()
    torch.cuda.synchronize()
    diff_loss = (la - lb_).abs().max().item()
    diff_grad = max((x - y).abs().max().item() for x, y in zip(ga, gb))
    nonzero = sum(int((x != 0).sum()) for x in ga)
    assert diff_loss <= 1e-5 * la.abs().max().item() and diff_grad <= 1e-7, (la.tolist(), lb_.tolist(), diff_grad)
    cands = (("one pass (a)", one_pass, sum(level_bytes)), ("per level (b)", per_level, 2 * sum(level_bytes)),
             ("(b), lists given", lambda: per_level(given), 2 * sum(level_bytes)))
    times = {name: [] for name, _, _ in cands}
    for name, fn, _ in cands:        # warm-up of every shape
        for _ in range(5):
            fn()
    for _ in range(a.rounds):
        for name, fn, _ in cands:
            times[name].append(timed(fn, a.reps))
    rows = []
    for name, fn, zeroed in cands:
        k, s, c = (None, None, None) if a.no_launch_count else count_device_events(fn)
        t = times[name]
        rows.append({"call": name, "us_median": round(statistics.median(t), 1), "us_min": round(min(t), 1), "us_max": round(max(t), 1),
                     "kernels": k, "memsets": s, "copies": c, "zeroed_bytes": zeroed})
    print(f"maps {MAPS} x A = {A} (Cf = {CF}), B = {B}, {n} anchors per image; sampled {counts.tolist()} (pos, neg) per image; "
          f"{nonzero} gradient elements written of {sum(level_bytes) // 4}")
    print(f"losses (a) {la.tolist()} (b) {lb_.tolist()}; max |d loss| {diff_loss:.3e}, max |d gradient| {diff_grad:.3e}")
    print(f"{a.rounds} alternating rounds of {a.reps} calls, forward + backward, us per call")
    print(f"{'call':18s} {'median':>9s} {'min':>9s} {'max':>9s} {'kernels':>8s} {'memsets':>8s} {'copies':>7s} {'zeroed MB':>10s}")
    for r in rows:
        print(f"{r['call']:18s} {r['us_median']:9.1f} {r['us_min']:9.1f} {r['us_max']:9.1f} {str(r['kernels']):>8s} {str(r['memsets']):>8s} "
              f"{str(r['copies']):>7s} {r['zeroed_bytes'] / 1e6:10.2f}")
    print(json.dumps({"maps": MAPS, "B": B, "A": A, "Cf": CF, "reps": a.reps, "rounds": a.rounds, "sampled": counts.tolist(),
                      "max_abs_diff_loss": diff_loss, "max_abs_diff_grad": diff_grad, "rows": rows}), flush=True)


if __name__ == "__main__":
    main()

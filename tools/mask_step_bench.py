"""Training-step time and memory with MODEL.MASK_ON off (the default) and on, in ONE process, and the mask head's own kernels alone.

The workload is BASELINE.json configs[2] (task 15-5, ID + ARD, batch 4, 600x1000) on seeded synthetic batches with uint8 ellipse masks, as
bench.py builds it, in the default arithmetic.  Four legs: MASK_ON off and on at the Mask R-CNN C4 setting (ROI_BOX_HEAD.POOLER_RESOLUTION 14 -> layer4 7x7 ->
ROI_MASK_HEAD.RESOLUTION 14; an even pooler, so the trainer runs the detection and the distillation RoIs in two head passes), and off and on at
the voc YAMLs' pooler (7 -> 4x4 -> RESOLUTION 8, the joint head pass; the off leg is bench.py's workload).  All models are built first, each leg
is warmed up, then the legs alternate in rounds of --steps steps timed with device events.  The kernels of csrc/mask.hip are then timed alone
at both settings' shapes (P = 512 positives) with their algorithmic bytes over the HBM peak (8 TB/s).  Prints one JSON line.

    python tools/mask_step_bench.py --rounds 3 --steps 10 --warmup 5
"""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IH, IW = 4, 600, 1000
N_OLD, N_NEW = 15, 5
MIB = 1024.0 * 1024.0
HBM_PEAK = 8.0e12
LEGS = {"pooler14_mask_off": (14, False), "pooler14_mask_on": (14, True), "pooler7_mask_off": (7, False), "pooler7_mask_on": (7, True)}


def overrides(res, mask):
    o = ["MODEL.ROI_BOX_HEAD.POOLER_RESOLUTION", res]
    if mask:
        o += ["MODEL.MASK_ON", True, "MODEL.ROI_MASK_HEAD.POOLER_RESOLUTION", res, "MODEL.ROI_MASK_HEAD.POOLER_SCALES", (0.0625,),
              "MODEL.ROI_MASK_HEAD.RESOLUTION", 2 * ((res - 1) // 2 + 1)]
    return o


def build_leg(name, batches, warmup):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=B, overrides=overrides(*LEGS[name]))
    random.seed(0)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    opt = make_optimizer(cfg_t, mt)
    leg = {"name": name, "ms": ms, "mt": mt, "opt": opt, "sch": make_lr_scheduler(cfg_t, opt), "cfg": cfg_t, "step": 0, "times": [], "peaks": []}
    run(leg, batches, warmup)
    torch.cuda.synchronize()
    leg["resident"] = torch.cuda.memory_allocated() - mem0
    return leg


def run(leg, batches, n):
    from abr_iod_amd.engine import train_step
    ld = None
    for _ in range(n):
        im, tg = batches[leg["step"] % len(batches)]
        nxt = batches[(leg["step"] + 1) % len(batches)][0]
        ld, _ = train_step(leg["ms"], leg["mt"], im, tg, leg["opt"], leg["sch"], leg["cfg"], next_images=nxt)
        leg["step"] += 1
    return ld


def _time(fn, reps=20):
    for _ in range(3):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e-3 / reps


def kernel_times(targets, h):
    """each new kernel alone at the step's shapes (layer4 output h x h, M = 2h): seconds and algorithmic bytes / (seconds * HBM peak)"""
    from abr_iod_amd import ops
    P, K, C, Cm, M, Kc, ld = 512, 2048, 2048, 256, 2 * h, 21, 24
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.randn(K, h, h, C, device=dev, generator=g)
    labels = torch.zeros(K, dtype=torch.int64, device=dev)
    labels[torch.randperm(K, device=dev, generator=g)[:P]] = 3
    rows, plab, inv, n_pos = ops.mask_compact_pos(labels, P)
    xg = ops.mask_gather_rows(x, rows)
    y = torch.randn(P, h, h, 4 * Cm, device=dev, generator=g)
    bias = torch.randn(Cm, device=dev, generator=g)
    t = ops.mask_d2s_bias_relu(y, bias)
    gt = torch.randn_like(t)
    z = torch.randn(P, M, M, ld, device=dev, generator=g)
    tg = torch.rand(P, M, M, device=dev, generator=g)
    rois = torch.cat([torch.cat((torch.full((K // B, 1), float(i), device=dev), tt.bbox[:1].repeat(K // B, 1)), 1) for i, tt in enumerate(targets)])
    masks = [tt.get_field("masks").masks for tt in targets]
    gts = [tt.bbox for tt in targets]
    prob = torch.rand(100, 1, M, M, device=dev, generator=g)
    boxes = targets[0].bbox[:1].repeat(100, 1)
    cases = {
        "mask_compact_pos": (lambda: ops.mask_compact_pos(labels, P), K * 16 + P * 16),
        "mask_gather_rows (forward)": (lambda: ops.mask_gather_rows(x, rows), 2 * xg.numel() * 4),
        "mask_gather_rows (backward)": (lambda: ops.mask_gather_rows(xg, inv), (xg.numel() + x.numel()) * 4),
        "mask_targets": (lambda: ops.mask_targets(masks, gts, rois, rows, M), P * M * M * 4 * 2),
        "mask_d2s_bias_relu": (lambda: ops.mask_d2s_bias_relu(y, bias), 2 * y.numel() * 4),
        "mask_d2s_bias_relu_backward": (lambda: ops.mask_d2s_bias_relu_backward(gt, t), 3 * y.numel() * 4),
        "mask_loss (+ gradient)": (lambda: ops.mask_loss(z, Kc, plab, tg, n_pos=n_pos, want_grad=True), (2 * z.numel() + tg.numel()) * 4),
        "mask_select_sigmoid": (lambda: ops.mask_select_sigmoid(z[:100], Kc, plab[:100].clamp(min=0)), 100 * M * M * 8),
        "mask_paste (100 detections, 600x1000)": (lambda: ops.mask_paste(prob, boxes, IH, IW), 100 * IH * IW),
    }
    out = {}
    for name, (fn, nbytes) in cases.items():
        s = _time(fn)
        out[name] = {"us": round(s * 1e6, 1), "algorithmic_mb": round(nbytes / 1e6, 2), "fraction_of_hbm_peak": round(nbytes / s / HBM_PEAK, 4)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg (the legs alternate)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg before the first round")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    from abr_iod_amd.engine.synthetic import synthetic_batch
    batches = [synthetic_batch(B, IH, IW, seed=42 + 1009 * j, label_range=(N_OLD + 1, N_OLD + N_NEW + 1), max_boxes=mb, masks="ellipse")
               for j, mb in enumerate((5, 3, 8, 12))]
    legs = [build_leg(n, batches, a.warmup) for n in LEGS]
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for leg in legs:
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ld = run(leg, batches, a.steps)
            t1.record()
            t1.synchronize()
            leg["times"].append(t0.elapsed_time(t1) / a.steps)
            leg["peaks"].append(torch.cuda.max_memory_allocated() - base)
            leg["losses"] = {k: round(float(v.detach()), 5) for k, v in ld.items()}
    res = {"workload": "configs[2]: 15-5, ID + ARD, B = 4, 600x1000, uint8 ellipse masks", "rounds": a.rounds, "steps_per_round": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for leg in legs:
        ms = sorted(leg["times"])
        med = ms[len(ms) // 2]
        res[leg["name"]] = {"trainable_tensors": sum(p.requires_grad for p in leg["mt"].parameters()), "trainable_floats": leg["mt"].flat.n_trainable,
                            "ms_per_step": [round(t, 3) for t in leg["times"]], "ms_per_step_median": round(med, 3),
                            "img_per_s_median": round(1e3 * B / med, 2), "resident_mib": round(leg["resident"] / MIB, 1),
                            "peak_mib": round((leg["resident"] + max(leg["peaks"])) / MIB, 1), "last_losses": leg["losses"]}
    for r in (14, 7):
        on, off = res["pooler%d_mask_on" % r]["ms_per_step_median"], res["pooler%d_mask_off" % r]["ms_per_step_median"]
        res["pooler%d_delta_mask_ms" % r], res["pooler%d_ratio_on_over_off" % r] = round(on - off, 3), round(on / off, 4)
    del legs
    torch.cuda.empty_cache()
    res["kernels_alone_pooler14_M14"] = kernel_times(batches[0][1], 7)
    res["kernels_alone_pooler7_M8"] = kernel_times(batches[0][1], 4)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""Training-step time and memory with MODEL.KEYPOINT_ON off (the default) and on, in ONE process, and the keypoint head's own kernels alone.

The workload is BASELINE.json configs[2] (task 15-5, ID + ARD, batch 4, 600x1000) on seeded synthetic batches with 17 keypoints per instance,
as bench.py builds it, in the default arithmetic; the off leg is bench.py's workload.  The on leg is upstream's keypoint setting: its own
extractor (SHARE_BOX_FEATURE_EXTRACTOR False), POOLER_RESOLUTION 14, eight conv3x3 layers of 512 channels, RESOLUTION 56, 17 keypoints --
128 positives per image at most, so 512 (RoI) rows through the conv stack, -1 padding included.  Both models are built first, each leg is
warmed up, then the legs alternate in rounds of --steps steps timed with device events.  The kernels of csrc/keypoint.hip are then timed
alone at the step's shapes (P = 512 rows, 14 x 14 pooled, 28 x 28 low-resolution planes, 56 x 56 heat maps; the decode on 100 detections)
with their algorithmic bytes over the HBM peak (8 TB/s).  Last, the on leg is rebuilt twice from the same seed and run --revisit-steps
steps each: whether the two runs' losses agree bit for bit is reported for the upstream pooler (14: ROIAlign's backward takes its per-RoI
atomics beyond 8 bins per axis) and for a pooler of 8 (its atomic-free gather form).  Reports only, asserts nothing.  Prints one JSON line.

    python tools/keypoint_step_bench.py --rounds 3 --steps 10 --warmup 5
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
K = 17
MIB = 1024.0 * 1024.0
HBM_PEAK = 8.0e12
LEGS = {"keypoint_off": None, "keypoint_on": 14}


def overrides(pooler):
    if pooler is None:
        return []
    return ["MODEL.KEYPOINT_ON", True, "MODEL.ROI_KEYPOINT_HEAD.SHARE_BOX_FEATURE_EXTRACTOR", False, "MODEL.ROI_KEYPOINT_HEAD.POOLER_RESOLUTION", pooler,
            "MODEL.ROI_KEYPOINT_HEAD.RESOLUTION", 4 * pooler, "MODEL.ROI_KEYPOINT_HEAD.POOLER_SCALES", (0.0625,), "MODEL.ROI_KEYPOINT_HEAD.NUM_CLASSES", K]


def build_leg(name, pooler, batches, warmup):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    torch.cuda.synchronize()
    mem0 = torch.cuda.memory_allocated()
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=B, overrides=overrides(pooler))
    random.seed(0)
    torch.manual_seed(0)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    opt = make_optimizer(cfg_t, mt)
    leg = {"name": name, "ms": ms, "mt": mt, "opt": opt, "sch": make_lr_scheduler(cfg_t, opt), "cfg": cfg_t, "step": 0, "times": [], "peaks": []}
    run(leg, batches, warmup)
    torch.cuda.synchronize()
    leg["resident"] = torch.cuda.memory_allocated() - mem0
    return leg


def run(leg, batches, n, record=None):
    from abr_iod_amd.engine import train_step
    ld = None
    for _ in range(n):
        im, tg = batches[leg["step"] % len(batches)]
        nxt = batches[(leg["step"] + 1) % len(batches)][0]
        ld, _ = train_step(leg["ms"], leg["mt"], im, tg, leg["opt"], leg["sch"], leg["cfg"], next_images=nxt)
        leg["step"] += 1
        if record is not None:
            record.append({k: float(v.detach()) for k, v in ld.items()})
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


def kernel_times(targets, r=14):
    """each new kernel alone at the step's shapes: seconds and algorithmic bytes / (seconds * HBM peak)"""
    from abr_iod_amd import ops
    P, R, D, Kp, h, M = 512, 2048, 100, ops.kp_pad(K), 2 * r, 4 * r
    dev = "cuda"
    g = torch.Generator(device=dev).manual_seed(0)
    # the sampled set: every fourth row a positive that sits on a ground-truth box of its image
    rois = torch.cat([torch.cat((torch.full((R // B, 1), float(i), device=dev), tt.bbox[torch.arange(R // B, device=dev) % len(tt)]), 1)
                      for i, tt in enumerate(targets)])
    labels = (torch.arange(R, device=dev) % 4 == 0).to(torch.int64)
    gts = [tt.bbox for tt in targets]
    kps = [tt.get_field("keypoints").keypoints for tt in targets]
    sel = ops.kp_select_targets(rois, labels, gts, kps, M, P)
    y = torch.randn(P, r, r, 16 * Kp, device=dev, generator=g)
    bias = torch.randn(K, device=dev, generator=g)
    low = ops.kp_deconv_fold(y, bias)
    glow = torch.randn_like(low)
    hi = ops.kp_upsample2x(low[:D], K)
    boxes = torch.tensor([[100.0, 80.0, 220.0, 380.0]], device=dev).repeat(D, 1)
    cases = {
        "kp_select_targets (2048 sampled rows)": (lambda: ops.kp_select_targets(rois, labels, gts, kps, M, P), R * 28 + R * 8 + P * (8 + K * 9)),
        "kp_deconv_fold": (lambda: ops.kp_deconv_fold(y, bias), (y.numel() + low.numel()) * 4),
        "kp_deconv_unfold": (lambda: ops.kp_deconv_unfold(glow, K), (y.numel() + low.numel()) * 4),
        "kp_loss (+ gradient)": (lambda: ops.kp_loss(low, K, sel["targets"], sel["valid"], sel["n_valid"], want_grad=True), 2 * low.numel() * 4),
        "kp_loss (forward only)": (lambda: ops.kp_loss(low, K, sel["targets"], sel["valid"], sel["n_valid"]), low.numel() * 4),
        "kp_upsample2x (100 detections)": (lambda: ops.kp_upsample2x(low[:D], K), (D * Kp * h * h + hi.numel()) * 4),
        "kp_decode (100 detections, 120 x 300 boxes)": (lambda: ops.kp_decode(hi, boxes), hi.numel() * 4 + D * K * 16),
    }
    out = {"valid_rows_of_the_loss": int(sel["n_valid"].item()), "positives": int(sel["n_pos"].item())}
    for name, (fn, nbytes) in cases.items():
        s = _time(fn)
        out[name] = {"us": round(s * 1e6, 1), "algorithmic_mb": round(nbytes / 1e6, 2), "fraction_of_hbm_peak": round(nbytes / s / HBM_PEAK, 4)}
    return out


def revisit(pooler, batches, steps):
    """the on leg built twice from the same seed: do the losses of `steps` steps agree bit for bit?"""
    runs = []
    for _ in range(2):
        rec = []
        leg = build_leg("revisit", pooler, batches, 0)
        run(leg, batches, steps, record=rec)
        torch.cuda.synchronize()
        runs.append(rec)
        del leg
        torch.cuda.empty_cache()
    first = next((i for i, (a, b) in enumerate(zip(*runs)) if a != b), None)
    return {"steps": steps, "losses_bit_identical": first is None, "first_step_that_differs": first,
            "loss_kp": [[r["loss_kp"] for r in rec] for rec in runs]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg (the legs alternate)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg before the first round")
    ap.add_argument("--revisit-steps", type=int, default=3, help="steps of each of the two same-seed runs (0: skip)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    from abr_iod_amd.engine.synthetic import synthetic_batch
    batches = [synthetic_batch(B, IH, IW, seed=42 + 1009 * j, label_range=(N_OLD + 1, N_OLD + N_NEW + 1), max_boxes=mb, keypoints=K)
               for j, mb in enumerate((5, 3, 8, 12))]
    legs = [build_leg(n, p, batches, a.warmup) for n, p in LEGS.items()]
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
    res = {"workload": "configs[2]: 15-5, ID + ARD, B = 4, 600x1000, 17 synthetic keypoints per instance", "rounds": a.rounds,
           "steps_per_round": a.steps, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    for leg in legs:
        ms = sorted(leg["times"])
        med = ms[len(ms) // 2] if ms else float("nan")
        res[leg["name"]] = {"trainable_tensors": sum(p.requires_grad for p in leg["mt"].parameters()), "trainable_floats": leg["mt"].flat.n_trainable,
                            "ms_per_step": [round(t, 3) for t in leg["times"]], "ms_per_step_median": round(med, 3),
                            "img_per_s_median": round(1e3 * B / med, 2), "resident_mib": round(leg["resident"] / MIB, 1),
                            "peak_mib": round((leg["resident"] + max(leg["peaks"] or [0])) / MIB, 1), "last_losses": leg.get("losses")}
    on, off = res["keypoint_on"]["ms_per_step_median"], res["keypoint_off"]["ms_per_step_median"]
    res["delta_keypoint_ms"], res["ratio_on_over_off"] = round(on - off, 3), round(on / off, 4)
    del legs
    torch.cuda.empty_cache()
    res["kernels_alone_pooler14_M56"] = kernel_times(batches[0][1])
    if a.revisit_steps > 0:
        res["revisit_pooler14"] = revisit(14, batches, a.revisit_steps)
        res["revisit_pooler8"] = revisit(8, batches, a.revisit_steps)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

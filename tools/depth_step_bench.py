"""Training-step time and memory of the R-50-C4 body (the default) against the R-101-C4 body (MODEL.BACKBONE.CONV_BODY, 23 layer3 blocks
instead of 6), in ONE process.

The workload is BASELINE.json configs[2] (task 15-5, ID + ARD, batch 4, 600x1000) on seeded synthetic batches, as bench.py builds it, in the
default arithmetic.  bench.py runs R-50-C4 only, so this tool times the two bodies side by side: both pairs of models are built first, each
leg is warmed up, then the legs alternate in rounds of --steps steps, timed with device events on the current stream.  Prints one JSON line.

Memory, per leg: `resident_mib` = what building and warming up the leg left allocated (both models' weights, the flat gradient and momentum
buffers, cached dgrad copies); `step_peak_above_resident_mib` = the largest torch.cuda.max_memory_allocated() of a timed round above what was
allocated when the round began (the step's activations and temporaries); `peak_mib` = their sum, what the leg alone would peak at.  These are
the torch caching allocator's bytes; the library's own derived-weight cache (Winograd-domain weights, packed planes) is reported separately as
`library_cache_mib`, the growth of ops.conv_cache_bytes() while the leg was built and warmed up.

--exchange: the data-parallel gradient exchange on a ONE-rank RCCL group (forced, as tests/test_gpu_dist.py does), with the per-bucket issue
point and main-stream wait of the last step (GradReducer.describe).  One rank only: an all-reduce over one GPU moves no data between GPUs, so
this shows WHEN each bucket is issued and whether the main stream waits for it, not what an N-GPU exchange costs.

    python tools/depth_step_bench.py --rounds 3 --steps 10 --warmup 5
"""
import argparse
import json
import os
import random
import socket
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, IH, IW = 4, 600, 1000
N_OLD, N_NEW = 15, 5
LEGS = ("R-50-C4", "R-101-C4")
MIB = 1024.0 * 1024.0


def build_leg(name, batches, warmup, exchange):
    from abr_iod_amd import ops
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    torch.cuda.synchronize()
    mem0, cache0 = torch.cuda.memory_allocated(), ops.conv_cache_bytes()
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=B,
                             overrides=["MODEL.BACKBONE.CONV_BODY", name])
    random.seed(0)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    opt = make_optimizer(cfg_t, mt)
    if exchange:
        opt.force_all_reduce = True
        opt.reducer.measure = True
    sch = make_lr_scheduler(cfg_t, opt)
    leg = {"name": name, "ms": ms, "mt": mt, "opt": opt, "sch": sch, "cfg": cfg_t, "step": 0, "times": [], "peaks": []}
    run(leg, batches, warmup)
    torch.cuda.synchronize()
    leg["resident"] = torch.cuda.memory_allocated() - mem0
    leg["cache"] = ops.conv_cache_bytes() - cache0
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


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg (the legs alternate)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg before the first round")
    ap.add_argument("--only", choices=LEGS, help="time one leg alone (a kernel trace of that step)")
    ap.add_argument("--exchange", action="store_true", help="gradient exchange on a one-rank RCCL group (see the module docstring)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    if a.exchange:
        import torch.distributed as dist
        dist.init_process_group(backend="nccl", init_method="tcp://127.0.0.1:{}".format(_free_port()), rank=0, world_size=1)
    from abr_iod_amd.engine.synthetic import synthetic_batch
    batches = [synthetic_batch(B, IH, IW, seed=42 + 1009 * j, label_range=(N_OLD + 1, N_OLD + N_NEW + 1), max_boxes=mb)
               for j, mb in enumerate((5, 3, 8, 12))]
    legs = [build_leg(n, batches, a.warmup, a.exchange) for n in ((a.only,) if a.only is not None else LEGS)]
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
    res = {"workload": "configs[2]: 15-5, ID + ARD, B = 4, 600x1000", "rounds": a.rounds, "steps_per_round": a.steps, "warmup": a.warmup,
           "device": torch.cuda.get_device_name(0)}
    for leg in legs:
        ms = sorted(leg["times"])
        med = ms[len(ms) // 2]
        step_peak = max(leg["peaks"])
        row = {"layer3_blocks": len(leg["mt"].backbone.body.layer3), "trainable_tensors": sum(p.requires_grad for p in leg["mt"].parameters()),
               "optimizer_segments": len(leg["opt"].param_groups), "trainable_floats": leg["mt"].flat.n_trainable,
               "ms_per_step": [round(t, 3) for t in leg["times"]], "ms_per_step_median": round(med, 3),
               "img_per_s_median": round(1e3 * B / med, 2), "resident_mib": round(leg["resident"] / MIB, 1),
               "step_peak_above_resident_mib": round(step_peak / MIB, 1), "peak_mib": round((leg["resident"] + step_peak) / MIB, 1),
               "library_cache_mib": round(leg["cache"] / MIB, 1), "last_losses": leg["losses"]}
        if a.exchange:
            row["gradient_exchange_one_rank"] = leg["opt"].reducer.describe()
        res[leg["name"]] = row
    if a.only is None:
        res["ratio_r101_over_r50"] = round(res["R-101-C4"]["ms_per_step_median"] / res["R-50-C4"]["ms_per_step_median"], 4)
        res["delta_r101_ms"] = round(res["R-101-C4"]["ms_per_step_median"] - res["R-50-C4"]["ms_per_step_median"], 3)
    print(json.dumps(res), flush=True)
    if a.exchange:
        for leg in legs:
            leg["opt"].reducer.close()
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()

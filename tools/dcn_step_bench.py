"""Training-step time of the plain body (the default), of MODEL.RESNETS.STAGE_WITH_DCN (F, T, T, F) with DCNv1 and of the same with DCNv2
(WITH_MODULATED_DCN: offsets and mask), in ONE process.

The workload is BASELINE.json configs[2] (task 15-5, ID + ARD, batch 4, 600x1000) on seeded synthetic batches, as bench.py builds it, in the
default arithmetic.  bench.py runs the plain body only, so this tool times the three legs side by side: every pair of models is built first,
each leg is warmed up, then the legs alternate in rounds of --steps steps, timed with device events on the current stream.  Prints one JSON line.

    python tools/dcn_step_bench.py --rounds 3 --steps 10 --warmup 5
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
LEGS = ("default", "v1", "v2")
DCN = ["MODEL.RESNETS.STAGE_WITH_DCN", "(False, True, True, False)"]
OVERRIDES = {"default": [], "v1": DCN, "v2": DCN + ["MODEL.RESNETS.WITH_MODULATED_DCN", True]}


def build_leg(name, batches):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=B, overrides=OVERRIDES[name])
    random.seed(0)
    ms, mt = build_models(cfg_s, cfg_t, seed=0)
    opt = make_optimizer(cfg_t, mt)
    sch = make_lr_scheduler(cfg_t, opt)
    return {"name": name, "ms": ms, "mt": mt, "opt": opt, "sch": sch, "cfg": cfg_t, "step": 0, "times": []}


def run(leg, batches, n):
    from abr_iod_amd.engine import train_step
    for _ in range(n):
        im, tg = batches[leg["step"] % len(batches)]
        nxt = batches[(leg["step"] + 1) % len(batches)][0]
        ld, _ = train_step(leg["ms"], leg["mt"], im, tg, leg["opt"], leg["sch"], leg["cfg"], next_images=nxt)
        leg["step"] += 1
    return ld


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3, help="timed rounds per leg (the legs alternate)")
    ap.add_argument("--steps", type=int, default=10, help="steps per timed round")
    ap.add_argument("--warmup", type=int, default=5, help="untimed steps per leg before the first round")
    ap.add_argument("--only", choices=LEGS, help="time one leg alone (a kernel trace of that step)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    torch.cuda.set_device(0)
    from abr_iod_amd.engine.synthetic import synthetic_batch
    batches = [synthetic_batch(B, IH, IW, seed=42 + 1009 * j, label_range=(N_OLD + 1, N_OLD + N_NEW + 1), max_boxes=mb)
               for j, mb in enumerate((5, 3, 8, 12))]
    legs = [build_leg(n, batches) for n in ((a.only,) if a.only is not None else LEGS)]
    for leg in legs:
        run(leg, batches, a.warmup)
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for leg in legs:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ld = run(leg, batches, a.steps)
            t1.record()
            t1.synchronize()
            leg["times"].append(t0.elapsed_time(t1) / a.steps)
            leg["losses"] = {k: round(float(v.detach()), 5) for k, v in ld.items()}
    res = {"workload": "configs[2]: 15-5, ID + ARD, B = 4, 600x1000", "rounds": a.rounds, "steps_per_round": a.steps, "warmup": a.warmup}
    for leg in legs:
        ms = sorted(leg["times"])
        med = ms[len(ms) // 2]
        res[leg["name"]] = {"optimizer_segments": len(leg["opt"].param_groups), "ms_per_step": [round(t, 3) for t in leg["times"]], "ms_per_step_median": round(med, 3),
                             "img_per_s_median": round(1e3 * B / med, 2), "last_losses": leg["losses"]}
    if a.only is None:
        for n in ("v1", "v2"):
            res["ratio_%s_over_default" % n] = round(res[n]["ms_per_step_median"] / res["default"]["ms_per_step_median"], 4)
            res["delta_%s_ms" % n] = round(res[n]["ms_per_step_median"] - res["default"]["ms_per_step_median"], 3)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

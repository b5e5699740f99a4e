"""GPU: the deformable body in the training loop at the BASELINE.json configs[2] shape (15-5, ID + ARD, B = 4, 600x1000): STAGE_WITH_DCN
(F, T, T, F) with WITH_MODULATED_DCN trains (finite losses, the offset convs move), a deformable layer1 under the default
FREEZE_CONV_BODY_AT 2 stays put, the eval forward returns detections under the range guard, and the columns cost no amax reduction."""
import math
import random

import pytest
import torch

pytestmark = pytest.mark.gpu

B, IH, IW = 4, 600, 1000


def _leg(stages, modulated=True, seed=0):
    from abr_iod_amd.engine.synthetic import build_models, make_cfgs
    from abr_iod_amd.solver.build import make_lr_scheduler, make_optimizer
    over = ["MODEL.RESNETS.STAGE_WITH_DCN", str(tuple(stages)), "MODEL.RESNETS.WITH_MODULATED_DCN", modulated] if stages else []
    cfg_s, cfg_t = make_cfgs("15-5", dist_type="id", feat="ard", alpha=0.5, beta=1.0, ims_per_batch=B, overrides=over)
    random.seed(seed)
    ms, mt = build_models(cfg_s, cfg_t, seed=seed)
    opt = make_optimizer(cfg_t, mt)
    sch = make_lr_scheduler(cfg_t, opt)
    return cfg_t, ms, mt, opt, sch


def _batches():
    from abr_iod_amd.engine.synthetic import synthetic_batch
    return [synthetic_batch(B, IH, IW, seed=42 + 1009 * j, label_range=(16, 21), max_boxes=mb) for j, mb in enumerate((5, 3))]


def _steps(leg, batches, n):
    from abr_iod_amd.engine import train_step
    cfg, ms, mt, opt, sch = leg
    out = []
    for i in range(n):
        im, tg = batches[i % len(batches)]
        ld, _ = train_step(ms, mt, im, tg, opt, sch, cfg, next_images=batches[(i + 1) % len(batches)][0])
        out.append({k: float(v.detach()) for k, v in ld.items()})
    torch.cuda.synchronize()
    return out


def test_train_v2_layer2_layer3_moves_offsets_and_evaluates():
    from abr_iod_amd.engine.inference import EvalRangeGuard
    leg = _leg((False, True, True, False))
    mt = leg[2]
    batches = _batches()
    offs = {n: p.detach().clone() for n, p in mt.named_parameters() if ".conv2.offset." in n}
    assert len(offs) == 2 * (4 + 6) and all(mt.get_parameter(n).requires_grad for n in offs)
    losses = _steps(leg, batches, 3)
    for ld in losses:
        assert all(math.isfinite(v) for v in ld.values()), ld
    moved = [n for n, v in offs.items() if not torch.equal(mt.get_parameter(n).detach(), v)]
    assert sorted(moved) == sorted(offs)
    # the padding rows / entries of the offset conv stay exactly zero
    for m in mt.modules():
        if hasattr(m, "offset") and hasattr(m, "modulated"):
            assert torch.count_nonzero(m.offset.weight[m.offset.out_channels:]) == 0
            assert torch.count_nonzero(m.offset.bias[m.offset.out_channels:]) == 0
    mt.eval()
    with torch.no_grad():
        out = EvalRangeGuard(mt).forward(batches[0][0])
    dets = out[0]
    assert len(dets) == B and all(len(d) >= 0 for d in dets)
    assert sum(len(d) for d in dets) > 0
    mt.train()


def test_dcn_layer1_stays_frozen_under_default_freeze():
    leg = _leg((True, True, True, False), modulated=False)
    mt = leg[2]
    l1 = {n: p.detach().clone() for n, p in mt.named_parameters() if n.startswith("backbone.body.layer1.") and ".offset." in n}
    assert len(l1) == 6 and not any(mt.get_parameter(n).requires_grad for n in l1)
    l2 = {n: p.detach().clone() for n, p in mt.named_parameters() if n.startswith("backbone.body.layer2.") and ".offset." in n}
    _steps(leg, _batches(), 2)
    for n, v in l1.items():
        assert torch.equal(mt.get_parameter(n).detach(), v), n
    assert any(not torch.equal(mt.get_parameter(n).detach(), v) for n, v in l2.items())


def test_columns_add_no_amax_reduction():
    """under the default ABR_H3_TAGS=1 f16x3 step, cols inherit o1's amax word and d_om carries its own: the per-step count of amax
    reductions is the plain model's"""
    from abr_iod_amd import ops
    batches = _batches()
    counts = []
    for stages in (None, (False, True, True, False)):
        leg = _leg(stages)
        _steps(leg, batches, 2)
        n0 = ops.amax_reductions[0]
        _steps(leg, batches, 2)
        counts.append(ops.amax_reductions[0] - n0)
        del leg
        torch.cuda.empty_cache()
    assert counts[1] == counts[0], counts

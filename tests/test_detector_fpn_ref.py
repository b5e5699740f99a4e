"""CPU: the float64 model of the FPN detector (tests/detector_fpn_ref.py) pinned to the reference's own forward (tests/golden/e2e_fpn_tiny.npz,
written by tests/golden/make_golden_e2e_fpn.py from the reference's code), its hand-written adjoints checked by gradcheck, and the fixture's
ability to SEE the composition bugs the whole-detector GPU test (tests/test_gpu_e2e_fpn.py) exists for.

Tolerances of the pin: 1e-4 of each tensor's max |value|, 1e-4 * max(1, |loss|) -- what tests/test_gpu_e2e_golden.py allows fp32 against fp32."""
import numpy as np
import pytest
import torch

import detector_fpn_ref as D
import e2e_fpn_common as E
import pooler_ref as P
import rpn_fpn_loss_ref as LR

LOSSES = ("loss_classifier", "loss_box_reg", "loss_objectness", "loss_rpn_box_reg")


def fixture_inputs(g):
    """the float64 model's `step` arguments from the fixture's draws -> (kwargs, per-image extras)"""
    labels, targets, pos, samp, rois, dlab, dreg = [], [], [], [], [], [], []
    n = None
    for i in range(2):
        _, boxes, vis, offs = E.anchors_np(E.IMAGE_SIZES[i])
        n = len(boxes)
        t = LR.prepare_targets(boxes, vis, g[f"gt{i}"])
        labels.append(t["labels"]); targets.append(t["targets"])
        pos.append(i * n + g[f"rpn_pos{i}"].astype(np.int64))
        samp.append(i * n + np.concatenate([g[f"rpn_pos{i}"], g[f"rpn_neg{i}"]]).astype(np.int64))
        sel = g[f"head_sel{i}"].astype(np.int64)
        rois.append(np.concatenate([np.full((len(sel), 1), i, np.float32), g[f"props{i}"][sel]], 1))
        dlab.append(g[f"det_labels{i}"].astype(np.int64)); dreg.append(g[f"det_reg_targets{i}"])
    return dict(rpn_labels=np.stack(labels), rpn_targets=np.stack(targets), pos_idx=np.concatenate(pos), samp_idx=np.concatenate(samp),
                det_rois=np.concatenate(rois), det_labels=np.concatenate(dlab), det_reg_targets=np.concatenate(dreg))


@pytest.fixture(scope="module")
def run(gold):
    g = gold("e2e_fpn_tiny")
    assert int(g["image_seed"]) == E.IMAGE_SEED and int(g["enrich_seed"]) == E.ENRICH_SEED and int(g["straddle"]) == E.STRADDLE, \
        "e2e_fpn_tiny.npz was written for other inputs: regenerate it"
    torch.manual_seed(0)
    _, _, _, _, _, sd_t = E.build("cpu", need_source=False)
    kw = fixture_inputs(g)
    model = D.DetectorFPNRef(sd_t)
    out = D.step(model, E.make_images(), **kw)
    return g, sd_t, kw, model, out


def _near(got, want, absmax, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print("%-22s err %.3e  limit %.3e" % (what, err, 1e-4 * absmax))
    assert err <= 1e-4 * absmax, (what, err, absmax)


def test_trainable_set_counts_72():
    """the rule of the float64 model on the reference's own key list (tests/golden/box_head_fpn_state_dict_shapes.json)"""
    keys = D.trainable_keys(E.shapes_json()["shapes"])
    assert len(keys) == 72
    assert not any(k.startswith(D.FROZEN_PREFIXES) or ".bn" in k or "downsample.1" in k or "anchor_generator" in k for k in keys)
    assert sum(k.startswith("backbone.body.layer4") for k in keys) == 10 and sum(k.startswith("backbone.fpn") for k in keys) == 16


def test_fixture_conditions(run):
    g, _, kw, _, out = run
    for c in ("cond_roi_levels", "cond_pos_and_neg", "cond_rpn_levels", "cond_gt_positive_anchor"):
        assert bool(g[c]), c
    assert (np.bincount(P.levels(kw["det_rois"]), minlength=4) >= 4).all()            # every pooled level holds at least 4 sampled RoIs
    assert (kw["det_labels"] > 0).any() and (kw["det_labels"] == 0).any() and (kw["det_labels"] >= 0).all()
    for i in range(2):
        _, boxes, vis, offs = E.anchors_np(E.IMAGE_SIZES[i])
        samp = np.concatenate([g[f"rpn_pos{i}"], g[f"rpn_neg{i}"]])
        assert (np.bincount(np.searchsorted(offs, samp, side="right") - 1, minlength=5) >= 1).all()     # every RPN level is sampled
        t = LR.prepare_targets(boxes, vis, g[f"gt{i}"])
        assert all(((t["matches"] == k) & (t["labels"] == 1)).any() for k in range(4))               # every ground truth has a positive anchor
        assert (t["labels"][g[f"rpn_pos{i}"]] == 1).all() and (t["labels"][g[f"rpn_neg{i}"]] == 0).all()   # the reference drew what these labels allow
        lab, tgt, _ = E.box_targets(g[f"gt{i}"], g[f"gt_labels{i}"], g[f"props{i}"])
        sel = g[f"head_sel{i}"]
        assert np.array_equal(lab[sel], g[f"det_labels{i}"])
        np.testing.assert_allclose(tgt[sel], g[f"det_reg_targets{i}"], rtol=1e-5, atol=1e-6)
    assert not np.array_equal(E.anchors_np(E.IMAGE_SIZES[0])[2], E.anchors_np(E.IMAGE_SIZES[1])[2])   # the two images' visibility differs


def test_model_reproduces_the_reference_forward(run):
    g, _, _, _, out = run
    for l in range(5):
        _near(E.spot(out["ps"][l].detach(), l).numpy(), g[f"p{l + 2}_spot"], float(g[f"p{l + 2}_absmax"]), "P%d" % (l + 2))
        st = max(1, 8 >> l)
        _near(out["objs"][l].detach()[:, :, ::st, ::st].numpy(), g[f"rpn_obj{l}_spot"], float(g[f"rpn_obj{l}_absmax"]), "RPN logits %d" % l)
    _near(out["logits"].detach().numpy(), g["det_logits"], float(np.abs(g["det_logits"]).max()), "class logits")
    _near(out["boxreg"].detach().numpy(), g["det_boxreg"], float(np.abs(g["det_boxreg"]).max()), "box regression")
    for k in LOSSES:
        got, want = out["losses"][k], float(g[k])
        print(k, got, want)
        assert abs(got - want) <= 1e-4 * max(1.0, abs(want)), (k, got, want)


def test_every_trainable_tensor_has_a_gradient(run):
    _, sd_t, _, model, _ = run
    grads = model.grads()
    assert sorted(grads) == sorted(D.trainable_keys(sd_t)) and len(grads) == 72
    for k, gr in grads.items():
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k


def test_pooler_function_is_its_own_adjoint():
    rng = np.random.default_rng(5)
    maps = [torch.from_numpy(rng.standard_normal((2, 2, h, w))).requires_grad_(True) for h, w in ((16, 24), (8, 12), (4, 6), (2, 3))]
    rows = [[0, 3.0, 5.0, 30.0, 40.0], [1, 10.0, 2.0, 90.0, 60.0], [0, -4.0, 1.0, 70.0, 63.0], [1, 0.0, 0.0, 95.0, 63.0],      # P2
            [0, 1.0, 1.0, 95.0, 63.0], [1, 0.0, 0.0, 200.0, 120.0], [0, 0.0, 0.0, 300.0, 400.0], [1, -50.0, -20.0, 700.0, 500.0]]
    rois = np.array(rows, np.float32)
    lv = P.levels(rois)
    assert set(lv.tolist()) == {0, 1, 2, 3}
    assert torch.autograd.gradcheck(lambda *m: D._Pool.apply(rois, lv, 3, 2, *m), maps, eps=1e-6, atol=1e-7, rtol=1e-6)


def test_neck_gradcheck_at_a_toy_size():
    g = torch.Generator().manual_seed(3)
    cs = [torch.randn(1, c, h, w, generator=g, dtype=torch.float64, requires_grad=True) for c, (h, w) in zip((2, 3, 4, 5), ((24, 16), (12, 8), (6, 4), (3, 2)))]
    flat = []
    for i, c in enumerate((2, 3, 4, 5), 1):
        flat += [torch.randn(2, c, 1, 1, generator=g, dtype=torch.float64, requires_grad=True), torch.randn(2, generator=g, dtype=torch.float64, requires_grad=True),
                 torch.randn(2, 2, 3, 3, generator=g, dtype=torch.float64, requires_grad=True), torch.randn(2, generator=g, dtype=torch.float64, requires_grad=True)]

    def f(*a):
        params = {}
        for i in range(4):
            params["fpn_inner%d" % (i + 1)], params["fpn_layer%d" % (i + 1)] = (a[4 + 4 * i], a[5 + 4 * i]), (a[6 + 4 * i], a[7 + 4 * i])
        return tuple(D.neck(list(a[:4]), params))
    out = f(*cs, *flat)
    assert [tuple(o.shape[-2:]) for o in out] == [(24, 16), (12, 8), (6, 4), (3, 2), (2, 1)]      # (an odd top: P6 is 2 x 1)
    assert torch.autograd.gradcheck(f, cs + flat, eps=1e-6, atol=1e-7, rtol=1e-6)


@pytest.mark.parametrize("mutation", D.MUTATIONS)
def test_fixture_sees_composition_bugs(run, mutation):
    """each deliberate composition bug moves at least one parameter gradient by more than 10 x the GPU test's bound, relative to its max |g|"""
    _, sd_t, kw, model, _ = run
    base = model.grads()
    bad = D.DetectorFPNRef(sd_t)
    D.step(bad, E.make_images(), mutate=mutation, **kw)
    moved = {k: float((v - base[k]).abs().max() / base[k].abs().max()) for k, v in bad.grads().items()}
    name = max(moved, key=moved.get)
    print(mutation, "moves", name, "by", moved[name], "; tensors over the limit:", sum(v > 10 * E.GRAD_MAX_REL for v in moved.values()))
    assert moved[name] > 10 * E.GRAD_MAX_REL, (mutation, name, moved[name])

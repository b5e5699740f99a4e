"""CPU: the float64 model of the RetinaNet detector (tests/detector_retinanet_ref.py) pinned to the reference's own forward
(tests/golden/e2e_retinanet_tiny.npz, written by tests/golden/make_golden_e2e_retinanet.py from the reference's code) in both
MODEL.RETINANET.USE_C5 variants, its loss pinned to tests/retinanet_loss_ref.py, and the fixture's ability to SEE the composition bugs the
whole-detector GPU test (tests/test_gpu_e2e_retinanet.py) exists for.

Tolerances of the pin: 1e-4 of each tensor's max |value|, 1e-4 * max(1, |loss|) -- what tests/test_detector_fpn_ref.py allows a float32
reference.  The loss against its numpy restatement: 1e-12 relative, values and every element of the gradient."""
import os

import numpy as np
import pytest
import torch

import detector_retinanet_ref as D
import e2e_retinanet_common as E
import retinanet_loss_ref as RL
import retinanet_ref as R

N_TRAINABLE = 70      # layer2..layer4: 4 + 6 + 3 blocks x 3 convs + 3 downsample convs = 42; the neck 2 x (3 x 2 + 2) = 16; the head 2 x 6 = 12


@pytest.fixture(scope="module", params=(True, False), ids=("use_c5", "use_p5"))
def run(request, gold):
    use_c5 = request.param
    g = gold("e2e_retinanet_tiny")
    assert int(g["image_seed"]) == E.IMAGE_SEED and int(g["enrich_seed"]) == E.ENRICH_SEED and tuple(g["anchor_sizes"].tolist()) == E.ANCHOR_SIZES, \
        "e2e_retinanet_tiny.npz was written for other inputs: regenerate it"
    torch.manual_seed(0)
    _, _, sd = E.build("cpu", use_c5)
    tg = E.batch_targets()
    model = D.DetectorRetinaNetRef(sd)
    out = D.step(model, E.make_images(), tg["labels"], tg["targets"], not use_c5)
    return dict(use_c5=use_c5, v=E.variant(use_c5), g=g, sd=sd, tg=tg, model=model, out=out)


def _near(got, want, absmax, what):
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)).max())
    print("%-22s err %.3e  limit %.3e" % (what, err, 1e-4 * absmax))
    assert err <= 1e-4 * absmax, (what, err, absmax)


def test_trainable_set_counts_70():
    """the rule of the float64 model on the reference's own key lists (tests/golden/retinanet_state_dict_shapes.json): the same keys in
    both variants, only p6's input width differs"""
    shapes = E.shapes_json()["shapes"]
    assert list(shapes["c5"]) == list(shapes["p5"])
    assert [k for k in shapes["c5"] if shapes["c5"][k] != shapes["p5"][k]] == ["backbone.fpn.top_blocks.p6.weight"]
    assert shapes["c5"]["backbone.fpn.top_blocks.p6.weight"] == [16, 256, 3, 3] and shapes["p5"]["backbone.fpn.top_blocks.p6.weight"] == [16, 16, 3, 3]
    keys = D.trainable_keys(shapes["c5"])
    assert len(keys) == N_TRAINABLE == 70
    frozen = [k for k in shapes["c5"] if k not in keys]
    assert all(k.startswith(("backbone.body.stem", "backbone.body.layer1")) or ".bn" in k or "downsample.1" in k or "anchor_generator" in k
               for k in frozen)
    assert not any(k.startswith(("backbone.body.stem", "backbone.body.layer1")) or ".bn" in k or "downsample.1" in k or "anchor_generator" in k
                   for k in keys)
    assert sum(k.startswith("backbone.body.layer") for k in keys) == 42 and sum(k.startswith("backbone.fpn.") for k in keys) == 16
    assert sum(k.startswith("rpn.head.") for k in keys) == 12 and not any("fpn_inner1" in k or "fpn_layer1" in k for k in shapes["c5"])
    new_biases = ["rpn.head.cls_tower.0.bias", "rpn.head.cls_tower.2.bias", "rpn.head.bbox_tower.0.bias", "rpn.head.bbox_tower.2.bias",
                  "rpn.head.cls_logits.bias", "rpn.head.bbox_pred.bias", "backbone.fpn.top_blocks.p6.bias", "backbone.fpn.top_blocks.p7.bias"]
    assert all(k in keys for k in new_biases)
    assert shapes["c5"]["rpn.head.cls_logits.weight"] == [E.A * E.C, 16, 3, 3]      # the reference stores no pad row


def test_fixture_conditions(run):
    g, tg, out, v = run["g"], run["tg"], run["out"], run["v"]
    margin = RL.threshold_margin(tg["per_image"])
    print("threshold margin %.3e" % margin)
    assert margin >= 1e-4                                                      # labels compare exactly
    hist = E.level_histogram(tg["labels"])
    assert np.array_equal(hist, g[v + "_label_hist"]) and out["n_pos"] == int(g[v + "_n_pos"]) == tg["n_pos"]      # the reference drew these labels
    assert (hist[:, 2:].sum(1) >= 1).all(), hist.tolist()                      # every level holds a positive anchor
    assert hist[:, 0].sum() >= 1                                               # an ignored anchor
    assert all((lab > 0).any() for lab in tg["labels"]) and all(len(b) > 0 for b in E.gt_arrays()[0])      # both images have ground truth
    assert set(np.unique(tg["labels"]).tolist()) == {-1, 0, 1, 2, 3}
    assert [tuple(p.shape[-2:]) for p in out["ps"]] == list(E.MAPS) == [(16, 24), (8, 12), (4, 6), (2, 3), (1, 2)]
    assert len(out["pre"]) == 5 * 2 * E.NUM_CONVS
    near = min(float(t.detach().abs().min()) for t in out["pre"])
    print("closest tower ReLU input to zero %.3e, closest P6 element %.3e" % (near, float(out["ps"][3].detach().abs().min())))
    assert near > E.NEAR_ZERO and float(out["ps"][3].detach().abs().min()) > E.NEAR_ZERO      # no sign the three arithmetics could flip
    # ... and none after the optimiser step of the GPU test, whose second backward pass is compared as well
    sd2, lr = E.stepped_sd(run["sd"], run["model"].grads())
    out2 = D.step(D.DetectorRetinaNetRef(sd2, trainable=False), E.make_images(), tg["labels"], tg["targets"], not run["use_c5"], backward=False)
    near2, p6_2 = min(float(t.abs().min()) for t in out2["pre"]), float(out2["ps"][3].abs().min())
    print("after the step (lr %.4g, total %.3f -> %.3f): closest tower ReLU input %.3e, closest P6 element %.3e" % (lr, out["total"], out2["total"], near2, p6_2))
    assert near2 > E.NEAR_ZERO_STEPPED and p6_2 > E.NEAR_ZERO_STEPPED and np.isfinite(out2["total"])
    d = np.concatenate([x.detach().permute(0, 2, 3, 1).reshape(2, -1, 4).numpy() for x in out["deltas"]], 1)
    e = np.abs(d - tg["targets"])[tg["labels"] > 0]
    assert (e > RL.BETA).any() and (e < RL.BETA).any()                         # both branches of smooth-L1 occur among the positives


def test_model_reproduces_the_reference_forward(run):
    g, out, v = run["g"], run["out"], run["v"]
    for l in range(5):
        for name, t in (("p", out["ps"][l]), ("cls", out["logits"][l]), ("reg", out["deltas"][l])):
            key = "%s_%s%d" % (v, name, l)
            _near(E.spot(t.detach(), l, E.CSTEP[name]).numpy(), g[key + "_spot"], float(g[key + "_absmax"]), key)
    for k, want in zip(("loss_retina_cls", "loss_retina_reg"), g[v + "_losses"]):
        got = out["losses"][k]
        print(k, got, float(want))
        assert abs(got - float(want)) <= 1e-4 * max(1.0, abs(float(want))), (k, got, float(want))


def test_every_trainable_tensor_has_a_gradient(run):
    grads = run["model"].grads()
    assert sorted(grads) == sorted(D.trainable_keys(run["sd"])) == sorted(D.trainable_keys(E.shapes_json()["shapes"][run["v"]]))
    assert len(grads) == N_TRAINABLE
    for k, gr in grads.items():
        assert bool(torch.isfinite(gr).all()) and float(gr.abs().max()) > 0, k
    assert not any(t.requires_grad for k, t in run["model"].p.items() if not D.is_trainable(k))


@pytest.mark.parametrize("mutation", D.MUTATIONS)
def test_fixture_sees_composition_bugs(run, mutation):
    """each deliberate composition bug moves at least one parameter gradient by more than 10 x the GPU test's bound, relative to its max |g|,
    and leaves every forward value alone"""
    base = run["model"].grads()
    bad = D.DetectorRetinaNetRef(run["sd"])
    out = D.step(bad, E.make_images(), run["tg"]["labels"], run["tg"]["targets"], not run["use_c5"], mutate=mutation)
    for a, b in zip(out["ps"] + out["logits"] + out["deltas"], run["out"]["ps"] + run["out"]["logits"] + run["out"]["deltas"]):
        assert torch.equal(a.detach(), b.detach())
    moved = {k: float((v - base[k]).abs().max() / base[k].abs().max()) for k, v in bad.grads().items()}
    name = max(moved, key=moved.get)
    print(mutation, run["v"], "moves", name, "by", moved[name], "; tensors over the limit:", sum(v > 10 * E.GRAD_MAX_REL for v in moved.values()))
    assert moved[name] > 10 * E.GRAD_MAX_REL, (mutation, name, moved[name])


def test_torch_loss_agrees_with_the_restatement():
    """detector_retinanet_ref.loss on retinanet_loss_ref.golden_inputs (logits from -6 to 3, deltas on both sides of beta, ignored anchors,
    five levels): the values equal retinanet_loss_ref.losses', autograd's gradient with respect to the head outputs its closed forms"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retinanet_loss.npz"))
    gt_boxes, gt_labels, cls_code, reg_code = RL.golden_inputs(int(g["seed"]))
    cls, reg = RL.golden_arrays(cls_code, reg_code)
    tg = RL.batch_targets(np.concatenate(R.pyramid_anchors()), gt_boxes, gt_labels)
    assert (tg["labels"] < 0).any() and tg["n_pos"] > 0
    N = len(R.IMAGE_SIZES)
    for g_cls, g_reg in ((1.0, 1.0), (0.7, -2.0)):
        want = RL.losses(cls, reg, R.A, R.C, tg["labels"], tg["targets"], g_cls=g_cls, g_reg=g_reg)
        nchw = lambda t, hw: torch.tensor(t.astype(np.float64).reshape(N, hw[0], hw[1], -1).transpose(0, 3, 1, 2).copy(), requires_grad=True)   # noqa: E731
        logits = [nchw(c, hw) for c, hw in zip(cls, R.MAPS)]
        deltas = [nchw(r, hw) for r, hw in zip(reg, R.MAPS)]
        lc, lr, n_pos = D.loss(logits, deltas, tg["labels"], tg["targets"])
        assert n_pos == want["n_pos"]
        assert abs(float(lc.detach()) - want["cls"]) <= 1e-12 * abs(want["cls"]) and abs(float(lr.detach()) - want["reg"]) <= 1e-12 * abs(want["reg"])
        (g_cls * lc + g_reg * lr).backward()
        for l in range(len(R.MAPS)):
            got_c = logits[l].grad.permute(0, 2, 3, 1).reshape(want["d_cls"][l].shape).numpy()
            got_r = deltas[l].grad.permute(0, 2, 3, 1).reshape(want["d_reg"][l].shape).numpy()
            np.testing.assert_allclose(got_c, want["d_cls"][l], rtol=1e-12, atol=0, err_msg="d_cls level %d" % l)
            np.testing.assert_allclose(got_r, want["d_reg"][l], rtol=1e-12, atol=0, err_msg="d_reg level %d" % l)
            assert want["d_cls"][l].any()
        assert any(w.any() for w in want["d_reg"])

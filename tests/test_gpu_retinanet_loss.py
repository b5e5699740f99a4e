"""GPU: RetinaNet's training half.  csrc/retinanet_loss.hip (abr_retina_targets, abr_retina_loss, abr_retina_loss_backward) against the float64
restatement of tests/retinanet_loss_ref.py; RetinaNetHead.forward_train (one autograd node) against float64 gradients of the golden head; the
tiny R-50-FPN-RETINANET detector through model(images, targets), loss.backward() and FusedSGD.step.

Tolerances.  Labels, n_pos and every "exactly zero" are exact: the boxes lie on an integer grid and a case is redrawn until no anchor's best IoU
lies within 1e-5 of a threshold and no two different IoUs that decide a match lie within 1e-6 of each other.  Regression targets: 4 fp32 ulps of
the magnitude of each output's addends (rpn_fpn_loss_ref.encode64, the bound tests/test_gpu_rpn_targets.py gives abr_rpn_targets_batched).
Losses: TOL * sum |addends| / denominator (tests/test_gpu_loss_kernels.py's rule).  d_cls: the bits of _C.sigmoid_focalloss_backward on the same
logits gathered into rows -- it is the same element code.  d_reg: rpn_fpn_loss_ref.check_grads' smooth-L1 bound.  The head: FR.conv_rule_ok at
one CONV_TOL_GRAD per contraction between an output gradient and the compared tensor (three)."""
import ctypes as C

import numpy as np
import pytest
import torch

import fpn_ref as FR
import retinanet_loss_ref as RL
import retinanet_ref as R

pytestmark = pytest.mark.gpu

EPS = RL.EPS


def cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def N(t):
    return t.detach().cpu().numpy()


def _rule(got, want, tol, what):
    ok, err, lim = FR.conv_rule_ok(np.asarray(got), np.asarray(want, np.float64), tol)
    assert ok, "%s: max error %.3e > %.3e" % (what, err, lim)


# ================================================================================================================= targets
def _separated(iou):
    """no two DIFFERENT IoUs that decide a match lie within 1e-6 of each other (fp32 could tie what float64 tells apart): per anchor its two
    largest, per ground truth its largest and the next different one"""
    if iou.shape[0] == 0:
        return True
    if iou.shape[0] > 1:
        top = np.sort(iou, 0)[-2:]
        d = top[1] - top[0]
        if np.any((d > 0) & (d < 1e-6)):
            return False
    for row in iou:
        rest = row[row < row.max()]
        if rest.size and row.max() - rest.max() < 1e-6:
            return False
    return True


def _int_boxes(rng, G, w, h, lo=10, hi=120):
    out = []
    for _ in range(G):
        bw, bh = int(rng.integers(lo, min(hi, w - 2))), int(rng.integers(lo, min(hi, h - 2)))
        x1, y1 = int(rng.integers(0, w - bw)), int(rng.integers(0, h - bh))
        out.append([x1, y1, x1 + bw, y1 + bh])
    return np.asarray(out, np.float32).reshape(-1, 4)


def _targets_case(name):
    """-> (anchors [n,4], list of gt boxes, list of gt labels, the restatement's targets), redrawn until the exact comparisons are safe"""
    pyr = R.pyramid_anchors()
    h, w = R.IMAGE_SIZES[0]
    for seed in range(100):
        rng = np.random.default_rng(1000 + seed)
        if name == "five levels":            # an image without ground truth next to one with g_max of them and one with a single one
            anchors = np.concatenate(pyr)
            gts = [np.zeros((0, 4), np.float32), _int_boxes(rng, 5, w, h), _int_boxes(rng, 1, w, h)]
            labs = [np.zeros(0, np.int64), np.array([1, R.C, 2, R.C, 1], np.int64), np.array([R.C], np.int64)]
        elif name == "four levels":          # n = 1152: no multiple of 256
            anchors = np.concatenate(pyr[1:])
            gts = [_int_boxes(rng, 3, w, h, 20, 150), _int_boxes(rng, 2, w, h, 20, 150)]
            labs = [rng.integers(1, R.C + 1, size=3).astype(np.int64), rng.integers(1, R.C + 1, size=2).astype(np.int64)]
        else:                                # one level of synthetic integer anchors (n = 300) with the ties built in
            anchors = _int_boxes(rng, 300, w, h, 8, 60)
            anchors[21] = anchors[20]        # two anchors reach every ground truth's maximum together
            anchors[41] = anchors[40]
            far = np.array([[150, 90, 189, 125]], np.float32)
            twin = anchors[40] + np.array([3, 2, 9, 7], np.float32)      # overlaps anchors 40 and 41 by less than half: low-quality positives
            gts = [np.stack([anchors[7], anchors[20], anchors[20], twin]), far]
            labs = [np.array([2, 1, R.C, 3], np.int64), np.array([R.C], np.int64)]     # the two equal ground truths tie everywhere: the first wins
        tg = RL.batch_targets(anchors, gts, labs)
        ok = RL.threshold_margin(tg["per_image"]) >= 1e-5 and all(_separated(p["iou"]) for p in tg["per_image"])
        if ok and name == "one level with ties":      # ... and the built-in cases are what they are meant to be
            p0, p1 = tg["per_image"]
            ok = p0["lq"][40] and p0["lq"][41] and p0["matches"][7] == 0 and p0["matches"][20] == 1 and p1["lq"].any() and \
                not np.array_equal(anchors[7], anchors[20])
        if ok:
            return anchors, gts, labs, tg
    raise AssertionError("no draw keeps the IoUs clear of the thresholds")


@pytest.mark.parametrize("name", ["five levels", "four levels", "one level with ties"])
def test_targets_against_the_restatement(name):
    from abr_iod_amd import ops
    anchors, gts, labs, tg = _targets_case(name)
    n = anchors.shape[0]
    labels, tgt, n_pos = ops.retina_targets(cuda(anchors), [cuda(b) for b in gts], [cuda(l) for l in labs], RL.HI, RL.LO, RL.WEIGHTS)
    torch.cuda.synchronize()
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (len(gts), n) and tuple(tgt.shape) == (len(gts), n, 4)
    assert n_pos.dtype == torch.int32 and tuple(n_pos.shape) == (1,)
    got_l, got_t = N(labels).astype(np.int64), N(tgt).astype(np.float64)
    print(name, "n", n, "positives", tg["n_pos"], "ignored", int((tg["labels"] < 0).sum()), "per image", [int((l > 0).sum()) for l in tg["labels"]])
    bad = np.argwhere(got_l != tg["labels"])
    assert bad.size == 0, (name, bad[:5].tolist(), got_l[tuple(bad[0])], tg["labels"][tuple(bad[0])])
    assert int(n_pos.item()) == int((got_l > 0).sum()) == tg["n_pos"] > 0
    err = np.abs(got_t - tg["targets"])
    assert np.all(err <= tg["target_bound"]), (name, float((err - tg["target_bound"]).max()))
    for i, b in enumerate(gts):
        if len(b) == 0:        # no ground truth: all background, zero targets
            assert not got_l[i].any() and not got_t[i].any()
    if name == "five levels":
        assert n % 256 == 0 and {1, R.C} <= set(np.unique(got_l).tolist()) and (got_l == -1).any()
        assert (got_l[2] > 0).any()                                    # the single ground truth finds its anchor
    if name == "four levels":
        assert n % 256 != 0
    if name == "one level with ties":
        assert n % 256 != 0
        p = tg["per_image"][0]
        assert got_l[0, 7] == 2 and p["best"][7] == 1.0                 # a ground truth equal to an anchor
        assert got_l[0, 20] == 1 and got_l[0, 21] == 1                  # the tie goes to the first ground truth, on both anchors that reach it
        assert got_l[0, 40] == 3 and got_l[0, 41] == 3 and p["lq"][40] and p["lq"][41] and p["best"][40] < RL.HI
        assert tg["per_image"][1]["lq"].any()                           # image 1's only box overlaps nothing by half: low quality only


def test_targets_without_any_ground_truth_and_without_images():
    from abr_iod_amd import ops
    anchors = cuda(np.concatenate(R.pyramid_anchors()[2:]))
    none = [torch.zeros((0, 4), device="cuda"), torch.zeros((0, 4), device="cuda")]
    labels, tgt, n_pos = ops.retina_targets(anchors, none, [torch.zeros((0,), dtype=torch.int64, device="cuda")] * 2, RL.HI, RL.LO)
    assert not labels.any() and not tgt.any() and int(n_pos.item()) == 0
    labels, tgt, n_pos = ops.retina_targets(anchors, [], [], RL.HI, RL.LO)
    assert tuple(labels.shape) == (0, anchors.shape[0]) and int(n_pos.item()) == 0


# ================================================================================================================= losses
MAPSETS = {1: ((3, 5),), 2: ((4, 6), (1, 1)), 5: ((8, 12), (4, 6), (2, 3), (1, 2), (1, 1))}
SHAPES = [(1, 1, 5), (9, 1, 2), (9, 3, 1), (9, 4, 5), (3, 80, 2)]          # (A, C, L): ld = 4, 12, 28, 36, 240
DIFFS = np.array([0.0, 0.05, -0.05, 0.109, -0.109, 0.111, -0.111, 0.5, -0.7, 3.0], np.float32)      # both sides of beta = 0.11


def _loss_case(A, Cn, L, seed=0, all_ignored=False):
    rng = np.random.default_rng(seed + 31 * A + Cn)
    maps = MAPSETS[L]
    Nimg = 2
    ldc, ldr = (A * Cn + 3) // 4 * 4, 4 * A
    nlocs = [h * w for h, w in maps]
    n = A * sum(nlocs)
    labels = np.zeros((Nimg, n), np.int64)
    draw = rng.random(n)
    labels[0][draw < 0.25] = rng.integers(1, Cn + 1, size=int((draw < 0.25).sum()))       # image 1 keeps no positive
    labels[0][draw > 0.85] = -1
    labels[1][rng.random(n) > 0.8] = -1
    labels[0, 0], labels[0, n - 1] = 1, Cn                                                # label values 1 and C, first and last anchor
    if all_ignored:
        labels[:] = -1
    targets = rng.standard_normal((Nimg, n, 4)).astype(np.float32)
    cls, reg, o = [], [], 0
    for nloc in nlocs:
        c = (rng.standard_normal((Nimg, nloc, ldc)) * 3).astype(np.float32)
        r = np.full((Nimg, nloc, ldr), np.nan, np.float32)
        r[:, :, :4 * A] = targets[:, o:o + nloc * A].reshape(Nimg, nloc, 4 * A) + rng.choice(DIFFS, size=(Nimg, nloc, 4 * A))
        c[:, :, A * Cn:] = np.nan                                                          # pad columns are never read
        cls.append(c)
        reg.append(r)
        o += nloc * A
    # logits of +-80 at a labelled class, at unlabelled classes, and under an ignored anchor
    x0 = cls[0]
    x0[0, 0, 0] = 80.0                              # anchor 0 has label 1: its own class
    x0[0, 0, Cn - 1] = -80.0 if Cn > 1 else 80.0
    flat = cls[-1]
    flat[0, -1, A * Cn - 1] = -80.0                 # the last anchor has label C: its own class at -80
    flat[1, -1, 0] = 80.0
    flat[1, 0, A * Cn - 1] = -80.0
    return dict(A=A, C=Cn, L=L, N=Nimg, n=n, ldc=ldc, ldr=ldr, nlocs=nlocs, labels=labels, targets=targets, cls=cls, reg=reg)


def _run_loss(case, upstream=((1.0, 1.0),), sentinel=None):
    from abr_iod_amd import ops
    cls, reg = [cuda(c) for c in case["cls"]], [cuda(r) for r in case["reg"]]
    labels, tgt = cuda(case["labels"].astype(np.int32)), cuda(case["targets"])
    n_pos = torch.tensor([int((case["labels"] > 0).sum())], dtype=torch.int32).cuda()
    nums = (case["A"], case["C"], labels, tgt, n_pos, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)
    losses = ops.retina_loss(cls, reg, *nums)
    grads = []
    for gc, gr in upstream:
        d = ops.retina_loss_backward(cls, reg, *nums, torch.tensor([gc], dtype=torch.float32).cuda(), torch.tensor([gr], dtype=torch.float32).cuda())
        grads.append(d)
    torch.cuda.synchronize()
    return losses, grads, dict(cls=cls, reg=reg, labels=labels, tgt=tgt, n_pos=n_pos)


@pytest.mark.parametrize("A,Cn,L", SHAPES)
def test_losses_and_gradients_against_float64(A, Cn, L):
    from abr_iod_amd import _C
    case = _loss_case(A, Cn, L)
    assert case["ldc"] in (4, 12, 28, 36, 240) and (case["labels"][1] <= 0).all() and (case["labels"][0] > 0).any()
    upstream = ((1.0, 1.0), (0.7, -2.0))
    losses, grads, dev = _run_loss(case, upstream)
    ref = RL.losses(case["cls"], case["reg"], A, Cn, case["labels"], case["targets"])
    RL.check_losses(float(losses[0]), float(losses[1]), ref, "A %d C %d L %d" % (A, Cn, L))
    lab = case["labels"]
    rows = torch.cat([c[:, :, :A * Cn].reshape(case["N"], -1, Cn) for c in dev["cls"]], 1).reshape(-1, Cn).contiguous()
    assert not torch.isnan(rows).any() and rows.shape[0] == case["N"] * case["n"]
    for (gc, gr), (d_cls, d_reg) in zip(upstream, grads):
        want = RL.losses(case["cls"], case["reg"], A, Cn, lab, case["targets"], g_cls=gc, g_reg=gr)
        # one allocation each, the levels back to back
        for d in (d_cls, d_reg):
            for l in range(L):
                assert d[l].is_contiguous() and d[l].data_ptr() == d[0].data_ptr() + 4 * sum(t.numel() for t in d[:l]), l
                assert d[l].untyped_storage().data_ptr() == d[0].untyped_storage().data_ptr()
        assert [tuple(t.shape) for t in d_cls] == [tuple(t.shape) for t in dev["cls"]] and [tuple(t.shape) for t in d_reg] == [tuple(t.shape) for t in dev["reg"]]
        # d_cls: the bits of the focal backward entry point on the gathered rows, with d_losses = s = g_cls / float(n_pos + N) formed in fp32
        s = torch.tensor([gc], dtype=torch.float32).cuda() / torch.tensor([float(ref["n_pos"] + case["N"])], dtype=torch.float32).cuda()
        exp = _C.sigmoid_focalloss_backward(rows, dev["labels"].reshape(-1), s.expand(rows.shape).contiguous(), Cn, RL.GAMMA, RL.ALPHA)
        got = torch.cat([d[:, :, :A * Cn].reshape(case["N"], -1, Cn) for d in d_cls], 1).reshape(-1, Cn)
        live = (dev["labels"].reshape(-1) >= 0)
        assert torch.equal(got[live], exp[live]), "d_cls differs from sigmoid_focalloss_backward's bits (upstream %s)" % (gc,)
        assert not got[~live].any(), "an ignored anchor has a gradient"
        for d in d_cls:
            assert not d[:, :, A * Cn:].any() and bool(torch.isfinite(d).all()), "pad columns must be exactly 0"
        # and near float64.  The element rounds p = sigmoid(x) to fp32 before it forms 1 - p: half an ulp of 1, which the factor gamma |x| of
        # the derivative multiplies; four more ulps for its products and transcendentals.
        for l in range(L):
            e = np.abs(N(d_cls[l]).astype(np.float64) - want["d_cls"][l])
            lim = (0.5 * RL.GAMMA * np.abs(np.nan_to_num(case["cls"][l].astype(np.float64))) + 4) * EPS * want["cls_scale"]
            assert np.all(e <= lim), (l, float((e - lim).max()))
        RL.check_d_reg([N(d) for d in d_reg], want, "A %d C %d L %d upstream %s" % (A, Cn, L, gr))
        assert any(N(d).any() for d in d_reg)


def test_every_anchor_ignored_gives_exact_zeros():
    case = _loss_case(9, 4, 2, all_ignored=True)
    losses, grads, _ = _run_loss(case, ((0.7, -2.0),))
    assert losses.tolist() == [0.0, 0.0]
    for d in grads[0][0] + grads[0][1]:
        assert not d.any() and bool(torch.isfinite(d).all())


def test_same_bits_from_run_to_run_and_after_a_larger_pyramid():
    small, large = _loss_case(9, 4, 2, seed=3), _loss_case(9, 4, 5, seed=4)
    first = _run_loss(small, ((0.7, -2.0),))
    again = _run_loss(small, ((0.7, -2.0),))
    _run_loss(large, ((1.0, 1.0),))
    third = _run_loss(small, ((0.7, -2.0),))
    for other in (again, third):
        assert torch.equal(first[0], other[0])
        for a, b in zip(first[1][0][0] + first[1][0][1], other[1][0][0] + other[1][0][1]):
            assert torch.equal(a, b)
    # through the autograd node: the losses do not depend on whether a gradient is wanted
    from abr_iod_amd.modeling.rpn.retinanet import _RetinaLossFn
    nums = (9, 4, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)
    dev = first[2]
    with torch.no_grad():
        plain = _RetinaLossFn.apply(nums, 2, dev["labels"], dev["tgt"], dev["n_pos"], *dev["cls"], *dev["reg"])
    leaves = [t.clone().requires_grad_(True) for t in dev["cls"] + dev["reg"]]
    lc, lr = _RetinaLossFn.apply(nums, 2, dev["labels"], dev["tgt"], dev["n_pos"], *leaves)
    assert torch.equal(plain[0], lc) and torch.equal(plain[1], lr) and torch.equal(lc, first[0][0]) and torch.equal(lr, first[0][1])
    (0.7 * lc - 2.0 * lr).backward()
    for t, want in zip(leaves, first[1][0][0] + first[1][0][1]):
        assert torch.equal(t.grad, want)


def test_argument_errors_come_before_any_launch():
    from abr_iod_amd import _lib as L
    from abr_iod_amd import ops
    lib = L.lib()
    case = _loss_case(9, 4, 2)
    A, Cn, Nimg, n = 9, 4, case["N"], case["n"]
    cls, reg = [cuda(c) for c in case["cls"]], [cuda(r) for r in case["reg"]]
    labels, tgt = cuda(case["labels"].astype(np.int32)), cuda(case["targets"])
    n_pos = torch.tensor([3], dtype=torch.int32).cuda()
    losses = torch.full((2,), 7.0, device="cuda")
    d_cls = torch.full((sum(c.numel() for c in cls),), 7.0, device="cuda")
    d_reg = torch.full((sum(r.numel() for r in reg),), 7.0, device="cuda")
    one = torch.ones(1, device="cuda")
    vp, ci = C.c_void_p * 2, C.c_int * 2
    good = dict(cls=vp(*[t.data_ptr() for t in cls]), ldc=ci(36, 36), reg=vp(*[t.data_ptr() for t in reg]), ldr=ci(36, 36), nloc=ci(*case["nlocs"]),
                L=2, N=Nimg, A=A, C=Cn)

    def call(**kw):
        a = dict(good, **kw)
        head = (a["cls"], a["ldc"], a["reg"], a["ldr"], a["nloc"], a["L"], a["N"], a["A"], a["C"], L.ptr(labels), L.ptr(tgt), L.ptr(n_pos),
                RL.GAMMA, RL.ALPHA, a.get("beta", RL.BETA), RL.NORM)
        rc_f = lib.abr_retina_loss(*head, L.ptr(losses), L.stream())
        msg_f = lib.abr_last_error().decode()
        rc_b = lib.abr_retina_loss_backward(*head, L.ptr(one), L.ptr(one), L.ptr(d_cls), L.ptr(d_reg), L.stream())
        msg_b = lib.abr_last_error().decode()
        return rc_f, msg_f, rc_b, msg_b

    bad = [dict(L=0), dict(L=ops.MAX_PYRAMID_LEVELS + 1), dict(A=0), dict(C=0), dict(A=10), dict(C=5), dict(ldc=ci(36, 32)), dict(ldr=ci(32, 36)),
           dict(ldc=ci(38, 36)), dict(ldr=ci(36, 38)), dict(nloc=ci(0, 1)), dict(nloc=ci(1 << 29, 1), N=4), dict(N=-1), dict(cls=None), dict(nloc=None),
           dict(ldr=None), dict(cls=vp(cls[0].data_ptr(), None)), dict(beta=0.0), dict(nloc=ci(1 << 27, 1), N=2, A=9)]
    for kw in bad:
        rc_f, msg_f, rc_b, msg_b = call(**kw)
        assert rc_f != 0 and msg_f.startswith("retina_loss:"), (kw, rc_f, msg_f)
        assert rc_b != 0 and msg_b.startswith("retina_loss_backward:"), (kw, rc_b, msg_b)
    # targets: N * n past int32, too many images, misaligned outputs
    anchors = cuda(np.concatenate(R.pyramid_anchors()[3:]))
    lab_out = torch.full((2, anchors.shape[0]), 7, dtype=torch.int32, device="cuda")
    tgt_out = torch.full((2, anchors.shape[0], 4), 7.0, device="cuda")
    np_out = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    tab = torch.zeros(2, dtype=torch.int64, device="cuda")
    ngt = torch.zeros(2, dtype=torch.int32, device="cuda")
    for n_, N_, a_ptr in ((1 << 30, 4, L.ptr(anchors)), (8, 70000, L.ptr(anchors)), (-1, 2, L.ptr(anchors)), (8, 2, None), (8, 2, L.ptr(anchors) + 4)):
        rc = lib.abr_retina_targets(a_ptr, n_, N_, L.ptr(tab), L.ptr(tab), L.ptr(ngt), 0, RL.HI, RL.LO, 10.0, 10.0, 5.0, 5.0, L.ptr(lab_out),
                                    L.ptr(tgt_out), L.ptr(np_out), L.stream())
        assert rc != 0 and lib.abr_last_error().decode().startswith("retina_targets:"), (n_, N_)
    torch.cuda.synchronize()
    assert bool((losses == 7).all()) and bool((d_cls == 7).all()) and bool((d_reg == 7).all())          # the sentinels stand
    assert bool((lab_out == 7).all()) and bool((tgt_out == 7).all()) and int(np_out.item()) == 7
    # N == 0 launches nothing and is no error
    assert lib.abr_retina_loss(good["cls"], good["ldc"], good["reg"], good["ldr"], good["nloc"], 2, 0, A, Cn, None, None, None, RL.GAMMA, RL.ALPHA,
                               RL.BETA, RL.NORM, L.ptr(losses), L.stream()) == 0
    torch.cuda.synchronize()
    assert bool((losses == 7).all())
    # the wrappers say what is wrong with a tensor before the library is asked
    with pytest.raises(RuntimeError, match="labels"):
        ops.retina_loss(cls, reg, A, Cn, labels.to(torch.int64), tgt, n_pos, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)
    with pytest.raises(RuntimeError, match="levels"):
        ops.retina_loss([], [], A, Cn, labels, tgt, n_pos, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)
    with pytest.raises(RuntimeError, match="ldc"):
        ops.retina_loss([c[:, :, :34].contiguous() for c in cls], reg, A, Cn, labels, tgt, n_pos, RL.GAMMA, RL.ALPHA, RL.BETA, RL.NORM)


# ================================================================================================================= the head node
GOLD = __import__("os").path.join(__import__("os").path.dirname(__import__("os").path.abspath(__file__)), "golden", "retinanet.npz")


@pytest.fixture(scope="module")
def g():
    return np.load(GOLD)


def _head(g, num_classes=R.C + 1):
    """tests/test_gpu_retinanet.py's construction: the golden's head weights in a NUM_CONVS 2, 16-channel head"""
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.rpn.retinanet import RetinaNetHead
    c = cfg.clone()
    c.merge_from_list(["MODEL.RETINANET.NUM_CLASSES", num_classes, "MODEL.RETINANET.NUM_CONVS", 2])
    head = RetinaNetHead(c, 16).cuda()
    sd = {str(k)[len("head_"):]: g[k] for k in g.files if k.startswith("head_") and k.endswith(("weight", "bias"))}
    with torch.no_grad():
        for name, conv in [("cls_tower.0", head.cls_tower[0]), ("cls_tower.2", head.cls_tower[2]), ("bbox_tower.0", head.bbox_tower[0]),
                           ("bbox_tower.2", head.bbox_tower[2]), ("cls_logits", head.cls_logits), ("bbox_pred", head.bbox_pred)]:
            w, b = sd[name + ".weight"], sd[name + ".bias"]
            if name == "cls_logits":
                w, b = w[: conv.out_channels], b[: conv.out_channels]
            conv.weight[: conv.out_channels].copy_(cuda(w).permute(0, 2, 3, 1))
            conv.bias[: conv.out_channels].copy_(cuda(b))
    bump_param_version()
    return head, sd


CONVS = ("cls_tower.0", "cls_tower.2", "bbox_tower.0", "bbox_tower.2", "cls_logits", "bbox_pred")


def _head_run(g, math, num_classes=R.C + 1):
    """the node on the golden's two levels with fixed random output gradients (zero in the pad column) -> dict of numpy results in the
    reference's layouts, and the float64 model's"""
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.resnet import set_conv_math
    head, sd = _head(g, num_classes)
    set_conv_math(head, math)
    n_cls = head.num_anchors * head.num_classes
    sd = dict(sd)
    sd["cls_logits.weight"], sd["cls_logits.bias"] = sd["cls_logits.weight"][:n_cls], sd["cls_logits.bias"][:n_cls]
    xs = [g["head_x_%d" % l] for l in range(2)]
    rng = np.random.default_rng(23)
    g_cls = [rng.standard_normal((x.shape[0], n_cls) + x.shape[2:]).astype(np.float32) for x in xs]
    g_reg = [rng.standard_normal((x.shape[0], 36) + x.shape[2:]).astype(np.float32) for x in xs]
    xt = [cuda(x).requires_grad_(True) for x in xs]
    head.zero_grad()
    cls, reg = head.forward_train(xt)
    assert [tuple(c.shape) for c in cls] == [(x.shape[0], x.shape[2], x.shape[3], head.ld_cls) for x in xs]
    total = 0.0
    for l in range(2):
        gc = np.zeros(tuple(cls[l].shape), np.float32)
        gc[..., :n_cls] = g_cls[l].transpose(0, 2, 3, 1)
        total = total + (cls[l] * cuda(gc)).sum() + (reg[l] * cuda(np.ascontiguousarray(g_reg[l].transpose(0, 2, 3, 1)))).sum()
    total.backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    got = dict(logits=[N(c.permute(0, 3, 1, 2)[:, :n_cls]) for c in cls], deltas=[N(r.permute(0, 3, 1, 2)) for r in reg], gx=[N(x.grad) for x in xt])
    for name in CONVS:
        conv = head.get_submodule(name)
        got["gw_" + name] = N(conv.weight.grad[: conv.out_channels].permute(0, 3, 1, 2))
        got["gb_" + name] = N(conv.bias.grad[: conv.out_channels])
    want_l, want_d, gp, gx = RL.head_ref_grads(sd, xs, 2, g_cls, g_reg)
    want = dict(logits=want_l, deltas=want_d, gx=gx)
    for name in CONVS:
        want["gw_" + name], want["gb_" + name] = gp[name + ".weight"], gp[name + ".bias"]
    return head, got, want


def _head_errors(got, want):
    out = {}
    for k, w in want.items():
        for l, (a, b) in enumerate(zip(got[k], w) if isinstance(w, list) else [(got[k], w)]):
            scale = max(float(np.abs(b).max()), 1e-30)
            out["%s[%d]" % (k, l)] = float(np.abs(np.asarray(a, np.float64) - b).max()) / scale
    return out


def test_head_node_on_two_levels_against_float64(g):
    from abr_iod_amd import ops
    head, got, want = _head_run(g, ops.MATH_F32)
    depth = 3 * FR.CONV_TOL_GRAD        # three contractions between an output gradient and anything compared (the output conv, the tower's two)
    for l in range(2):
        _rule(got["logits"][l], want["logits"][l], 3 * FR.CONV_TOL_FWD, "logits %d" % l)
        _rule(got["deltas"][l], want["deltas"][l], 3 * FR.CONV_TOL_FWD, "deltas %d" % l)
        _rule(got["gx"][l], want["gx"][l], depth, "d x %d (the two towers' input gradients add)" % l)
    for name in CONVS:      # the float64 gradients are the sums over both levels: the levels' gradients add in the flat buffer
        _rule(got["gw_" + name], want["gw_" + name], depth, "d %s.weight" % name)
        _rule(got["gb_" + name], want["gb_" + name], depth, "d %s.bias" % name)
    # one level alone gives something else: the second level really arrives
    xs1 = [cuda(g["head_x_0"]).requires_grad_(True)]
    head.zero_grad()
    c1, r1 = head.forward_train(xs1)
    (c1[0].sum() + r1[0].sum()).backward()
    ops.join_side_stream()
    assert head.cls_logits.weight.grad.any() and xs1[0].grad.any()
    # the reference signature still refuses autograd
    with pytest.raises(NotImplementedError, match="backward is not built"):
        head([cuda(g["head_x_0"])])


def test_head_node_pad_row_gets_exactly_zero(g):
    from abr_iod_amd import ops
    head, got, want = _head_run(g, ops.MATH_F32, num_classes=4)
    assert head.ld_cls == 28 and tuple(head.cls_logits.weight.grad.shape) == (28, 3, 3, 16)
    assert not head.cls_logits.weight.grad[27].any() and not head.cls_logits.bias.grad[27].any()
    assert head.cls_logits.weight.grad[:27].any()
    depth = 3 * FR.CONV_TOL_GRAD
    _rule(got["gw_cls_logits"], want["gw_cls_logits"], depth, "d cls_logits.weight (27 rows)")
    _rule(got["gw_cls_tower.0"], want["gw_cls_tower.0"], depth, "d cls_tower.0.weight (27 classes)")
    for l in range(2):
        _rule(got["gx"][l], want["gx"][l], depth, "d x %d (27 classes)" % l)


def test_head_node_under_f16x3(g):
    """the admitted bound of the split arithmetics (tests/test_gpu_mask_head_fpn.py's form): every compared tensor within max(2 x the fp32
    route's own error on the same inputs, 8 eps) of float64, relative to max |expected|; the pad row stays exactly zero"""
    from abr_iod_amd import ops
    ops.x6_range_flags(reset=True)
    _, got32, want = _head_run(g, ops.MATH_F32, num_classes=4)
    head, got, _ = _head_run(g, ops.MATH_F16X3, num_classes=4)
    assert head.math == ops.MATH_F16X3 and ops.x6_range_flags(reset=True) == 0
    e32, eo = _head_errors(got32, want), _head_errors(got, want)
    for k in sorted(eo):
        print("%-28s f32 %.2f eps   f16x3 %.2f eps" % (k, e32[k] / EPS, eo[k] / EPS))
        assert eo[k] <= max(2.0 * e32[k], 8 * EPS), (k, eo[k], e32[k])
    assert not head.cls_logits.weight.grad[27].any() and not head.cls_logits.bias.grad[27].any()


# ================================================================================================================= the tiny detector
C_T = 3                 # 27 logits in rows of 28: the pad row exists
LR, STEPS = 0.002, 8    # chosen by running it: the total goes 2.1756, 2.1738, 2.1704, 2.1660, 2.1610, 2.1551, 2.1486, 2.1413 (momentum 0.9)


def _tiny():
    """tests/test_gpu_retinanet.py's tiny config, with 3 foreground classes so that cls_logits carries a pad row, and a fresh head"""
    from abr_iod_amd.config import cfg
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.structures.bounding_box import BoxList
    from abr_iod_amd.structures.image_list import to_image_list
    c = cfg.clone()
    c.merge_from_list(["MODEL.RETINANET_ON", True, "MODEL.BACKBONE.CONV_BODY", "R-50-FPN-RETINANET", "MODEL.RESNETS.STEM_OUT_CHANNELS", 16,
                       "MODEL.RESNETS.RES2_OUT_CHANNELS", 32, "MODEL.RESNETS.WIDTH_PER_GROUP", 8, "MODEL.RESNETS.BACKBONE_OUT_CHANNELS", 16,
                       "MODEL.RETINANET.NUM_CLASSES", C_T + 1, "MODEL.RETINANET.NUM_CONVS", 2, "MODEL.RETINANET.ANCHOR_SIZES", R.SIZES,
                       "MODEL.RETINANET.PRE_NMS_TOP_N", 60, "TEST.DETECTIONS_PER_IMG", 40])
    torch.manual_seed(0)
    model = build_detection_model(c)
    gen = torch.Generator().manual_seed(3)
    images = [torch.randn(3, 128, 192, generator=gen).cuda() * 40, torch.randn(3, 112, 160, generator=gen).cuda() * 40]
    batch = to_image_list(images, 64)
    # (integer boxes whose IoUs with the pyramid's anchors stay 3.8e-4 clear of both thresholds: the labels compare exactly)
    boxes = [np.array([[9, 13, 72, 91], [101, 31, 133, 60], [38, 57, 161, 119], [149, 6, 167, 43]], np.float32),
             np.array([[19, 22, 50, 85], [79, 39, 149, 103]], np.float32)]
    labs = [np.array([1, 2, 3, 2], np.int64), np.array([3, 1], np.int64)]
    targets = []
    for (h, w), b, l in zip(R.IMAGE_SIZES, boxes, labs):
        t = BoxList(cuda(b), (w, h), mode="xyxy")
        t.add_field("labels", cuda(l))
        targets.append(t)
    return c, model, batch, targets


def _rows(ts, width):
    return [N(t.permute(0, 2, 3, 1)).reshape(t.shape[0], -1, width) for t in ts]


def test_tiny_detector_trains():
    from abr_iod_amd import ops
    from abr_iod_amd.modeling.backbone.resnet import bump_param_version
    from abr_iod_amd.modeling.detector.generalized_rcnn import build_detection_model
    from abr_iod_amd.solver.build import FusedSGD
    c, model, batch, targets = _tiny()
    head, ev = model.rpn.head, model.rpn.loss_evaluator
    assert head.ld_cls == 28 and head.num_classes == C_T
    opt = FusedSGD(model, LR, 0.9, 1e-4, 2.0, 0.0)
    model.train()
    opt.zero_grad()
    out = model(batch, targets)
    assert len(out) == 8 and out[5] is None and out[6] is None and out[7] is None
    losses, feats, anchors, (box_cls, box_reg) = out[0], out[1], out[3], out[4]
    assert set(losses) == {"loss_retina_cls", "loss_retina_reg"} and len(feats) == 5 and len(anchors) == 2
    # the losses are the restatement's on the model's own head outputs and the targets it drew
    labels, reg_targets = ev.last_targets
    lab = np.stack([N(l) for l in labels]).astype(np.int64)
    tgt = np.stack([N(t) for t in reg_targets])
    ref = RL.losses(_rows(box_cls, 9 * C_T), _rows(box_reg, 36), 9, C_T, lab, tgt)
    assert int(ev.last_n_pos.item()) == ref["n_pos"] > 0 and (lab == -1).any()
    RL.check_losses(float(losses["loss_retina_cls"]), float(losses["loss_retina_reg"]), ref, "tiny detector")
    want_t = RL.batch_targets(np.concatenate([N(a.bbox) for a in anchors[0]]), [N(t.bbox) for t in targets], [N(t.get_field("labels")) for t in targets])
    assert np.array_equal(lab, want_t["labels"]) and np.all(np.abs(tgt - want_t["targets"]) <= want_t["target_bound"])
    arrived = {}
    for l, f in enumerate(feats):
        f.register_hook(lambda gr, l=l: arrived.__setitem__(l, gr.detach().clone()))
    sum(losses.values()).backward()
    ops.join_side_stream()
    torch.cuda.synchronize()
    for name, p in model.named_parameters():
        if p.requires_grad:
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
            if "cls_logits" not in name or p.dim() == 4:
                assert p.grad.any(), name + " has no gradient"
        else:
            assert p.grad is None or not p.grad.any(), name + " is frozen"
    assert any(not p.requires_grad for p in model.parameters())
    assert not head.cls_logits.weight.grad[27].any() and not head.cls_logits.bias.grad[27].any()
    # the gradient arriving at each of P3..P7 is the head node's input gradient: the node alone on the same maps, same targets
    assert sorted(arrived) == [0, 1, 2, 3, 4]
    leaves = [f.detach().clone().requires_grad_(True) for f in feats]
    cls2, reg2 = head.forward_train(leaves)
    lc, lr = ev.call_nhwc(anchors, cls2, reg2, targets, head.num_anchors, head.num_classes)
    assert torch.equal(lc, losses["loss_retina_cls"]) and torch.equal(lr, losses["loss_retina_reg"])
    keep = model.flat.grads.clone()
    (lc + lr).backward()
    ops.join_side_stream()
    for l in range(5):
        assert torch.equal(leaves[l].grad, arrived[l]), "P%d" % (l + 3)
    model.flat.grads.copy_(keep)          # (the second backward added the head's parameter gradients once more)
    # one step; the derived-weight caches follow the weights: a fresh model loaded with the stepped state dict computes the same bits
    before = head.cls_logits.weight.detach().clone()
    opt.step()
    torch.cuda.synchronize()
    assert not torch.equal(before, head.cls_logits.weight.detach()) and not head.cls_logits.weight[27].any() and not head.cls_logits.bias[27].any()
    model.eval()
    fresh = build_detection_model(c)
    fresh.load_state_dict(model.state_dict())
    bump_param_version()
    fresh.eval()
    with torch.no_grad():
        _, f1, _ = model(batch)
        _, _, (c1, r1) = model.rpn(batch, f1)
        _, f2, _ = fresh(batch)
        _, _, (c2, r2) = fresh.rpn(batch, f2)
    for a, b in zip(list(f1) + list(c1) + list(r1), list(f2) + list(c2) + list(r2)):
        assert torch.equal(a, b)


def test_tiny_detector_short_run_lowers_the_loss():
    """STEPS steps of momentum SGD at LR on one batch: the total loss at the end is below the one it began with (the run printed
    below is how LR and STEPS were chosen); the pad row of cls_logits is still exactly zero"""
    from abr_iod_amd.solver.build import FusedSGD
    c, model, batch, targets = _tiny()
    opt = FusedSGD(model, LR, 0.9, 1e-4, 2.0, 0.0)
    model.train()
    seen = []
    for step in range(STEPS):
        opt.zero_grad()
        losses = model(batch, targets)[0]
        total = sum(losses.values())
        total.backward()
        opt.step()
        seen.append(float(total))
    print("total loss per step", ["%.4f" % v for v in seen])
    assert all(np.isfinite(seen)) and seen[-1] < seen[0], seen
    head = model.rpn.head
    assert not head.cls_logits.weight[27].any() and not head.cls_logits.bias[27].any()

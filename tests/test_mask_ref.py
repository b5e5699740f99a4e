"""CPU: the plain restatements of tests/mask_ref.py, pinned to what the reference recorded in tests/golden/mask_head.npz and to torch, so that
tests/test_gpu_mask_kernels.py can hold the kernels of csrc/mask.hip to them at shapes the fixture does not have.  Also the two conditions
on that file's INPUTS that need no GPU: every paste case keeps its excused pixels within the cap, and torch's CPU resize really changes its
operation order beyond M = 64."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mask_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24
W, H = 97, 61


def _gold():
    return np.load(os.path.join(GOLD, "mask_head.npz"))


# ------------------------------------------------------------------------------------------------ pinned to the fixture
@pytest.mark.parametrize("tag", ["u8", "f32"])
@pytest.mark.parametrize("M", [8, 14, 28])
def test_targets_ref_reproduces_the_recorded_targets(tag, M):
    g = _gold()
    boxes, inst, want = g["t_boxes"], torch.from_numpy(g["t_masks_" + tag]), g["t_%s_M%d" % (tag, M)]
    n = len(boxes)
    rois = np.concatenate((np.arange(n, dtype=np.float32)[:, None], boxes), 1)
    got, matched = R.targets_ref([inst[i:i + 1] for i in range(n)], [boxes[i:i + 1] for i in range(n)], rois, np.arange(n), M)
    assert matched == [0] * n
    if tag == "u8":
        assert np.array_equal(got.numpy(), want)
    else:
        assert np.abs(got.numpy().astype(np.float64) - want).max() <= 1e-6


def test_compact_and_targets_ref_reproduce_the_recorded_loss_targets():
    g = _gold()
    labels = g["l_labels"]
    props = [g["l_props0"], g["l_props1"]]
    rois = np.concatenate([np.concatenate((np.full((len(p), 1), i, np.float32), p), 1) for i, p in enumerate(props)])
    P = int((labels > 0).sum())
    rows, plab, inv, n_pos = R.compact_ref(labels, P + 3)
    assert n_pos == P == len(g["l_targets"]) and (rows[P:] == -1).all() and (plab[P:] == -1).all()
    assert np.array_equal(rows[:P], np.nonzero(labels > 0)[0]) and np.array_equal(plab[:P], labels[labels > 0])
    assert np.array_equal(inv[rows[:P]], np.arange(P)) and (inv[labels <= 0] == -1).all()
    got, _ = R.targets_ref([torch.from_numpy(g["l_masks0"]), torch.from_numpy(g["l_masks1"])], [g["l_gt0"], g["l_gt1"]], rois, rows, 14)
    assert np.array_equal(got[:P].numpy(), g["l_targets"]) and not bool(got[P:].any())
    # the cut list
    rows, plab, inv, n_pos = R.compact_ref(labels, 3)
    assert n_pos == 3 and np.array_equal(rows, np.nonzero(labels > 0)[0][:3]) and int((inv >= 0).sum()) == 3


def test_select_sigmoid_ref_reproduces_the_recorded_probabilities():
    g = _gold()
    x = torch.from_numpy(g["e_logits"])
    got = R.select_sigmoid_ref(x.permute(0, 2, 3, 1), x.shape[1], g["e_labels"])
    assert got.shape == g["e_prob"].shape
    assert float((got - torch.from_numpy(g["e_prob"]).double()).abs().max()) <= 4 * EPS
    assert not bool(R.select_sigmoid_ref(x.permute(0, 2, 3, 1), x.shape[1], [-1, x.shape[1]] * 4 + [-7]).any())


def test_paste_f64_reproduces_the_recorded_paste():
    g = _gold()
    prob, boxes, want = torch.from_numpy(g["e_prob"]), torch.from_numpy(g["e_boxes"]), torch.from_numpy(g["e_pasted"])
    excused = 0
    for d in range(len(boxes)):
        vals, written = R.paste_f64(prob[d, 0], boxes[d], H, W)
        exp, near = R.paste_expected(vals, written, 0.5)
        excused += int(near.sum())
        assert not bool(((exp != want[d, 0]) & ~near).any()), d
    assert bool(want.any()) and excused <= 1e-3 * want.numel()


def test_gather_and_depth_to_space_refs_against_torch():
    """gather_ref is indexing with zeros outside the source; d2s_ref / d2s_backward_ref are ConvTranspose2d(k = 2, s = 2) + bias + ReLU and
    its autograd on the GEMM's columns -- on small integers, where every sum is exact, with h != w"""
    gen = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (3, 5, 2, 3), generator=gen).float()            # [P,C,h,w]
    w5 = torch.randint(-3, 4, (5, 4, 2, 2), generator=gen).float()            # [C,Cm,2,2]
    b5 = torch.randint(-6, 7, (4,), generator=gen).float()
    y = torch.einsum("pchw,cmyx->phwyxm", x, w5).reshape(3, 2, 3, 16).requires_grad_(True)
    want = F.relu(F.conv_transpose2d(x, w5, b5, stride=2)).permute(0, 2, 3, 1)
    got = R.d2s_ref(y.detach(), b5)
    assert torch.equal(got, want) and bool((got == 0).any()) and bool((got > 0).any())
    g = torch.randint(-5, 6, got.shape, generator=gen).float()
    yy = y.view(3, 2, 3, 2, 2, 4).permute(0, 1, 3, 2, 4, 5).reshape(3, 4, 6, 4)
    torch.where(yy + b5 > 0, yy + b5, torch.zeros(())).backward(g)
    assert torch.equal(R.d2s_backward_ref(g, got), y.grad)
    src = np.arange(24, dtype=np.float32).reshape(3, 2, 4) + 1
    out = R.gather_ref(src, np.array([2, -1, 0, 3, 2, -(2 ** 40)]))
    assert np.array_equal(out[[0, 2, 4]], src[[2, 0, 2]]) and not out[[1, 3, 5]].any()


# ------------------------------------------------------------------------------------------------ conditions on the GPU tests' inputs
def test_every_paste_case_keeps_its_excused_pixels_within_the_cap():
    """per case and threshold: the pixels whose float64 value lies within 1e-6 of the threshold are at most 1e-3 of the case's pixels (on a
    canvas of fewer than 1000 pixels: none).  Also that the cases are what they claim: D H W % 4 takes 0, 1, 2 and 3, the boxes wholly
    outside write nothing, the one-row / one-column boxes write exactly that, and every threshold separates something."""
    cases = R.paste_cases()
    assert {c.D * c.H * c.W % 4 for c in cases} == {0, 1, 2, 3}
    assert {(c.H, c.W) for c in cases} == set(R.PASTE_CANVASES) and {c.M for c in cases} == {1, 7, 14, 28}
    for c in cases:
        vals, written = R.paste_reference(c.name)
        line = []
        for t in R.PASTE_THRESHOLDS:
            want, near = R.paste_expected(vals, written, t)
            line.append(int(near.sum()))
            assert int(near.sum()) <= 1e-3 * want.numel(), (c.name, t, int(near.sum()), want.numel())
        print("paste case", c.name, "pixels", written.numel(), "written", int(written.sum()), "excused per threshold", line)
        for d, kind in enumerate(c.kinds):
            if kind.startswith("outside") or kind.startswith("reversed"):
                assert not bool(written[d].any()), (c.name, kind)
            if kind.startswith("one column"):
                assert bool(written[d, :, 0].all()) and not bool(written[d, :, 1:].any()), (c.name, kind)
            if kind.startswith("one row"):
                assert bool(written[d, c.H - 1].all()) and not bool(written[d, :c.H - 1].any()), (c.name, kind)
            if kind.startswith("corners in") or kind.startswith("huge"):
                assert bool(written[d, 0, 0]), (c.name, kind)
    big = R.paste_reference("M14-33x64-D56")
    counts = [int(R.paste_expected(big[0], big[1], t)[0].sum()) for t in R.PASTE_THRESHOLDS]
    assert counts[0] > counts[1] > counts[2] > counts[3] > 0, counts


def test_torch_resize_changes_its_operation_order_beyond_64():
    """csrc/mask_bilinear.h records that torch's CPU bilinear resize runs the four-weight sum only while out_h + out_w <= 128 and a separable
    form beyond.  Found here (torch 2.10, 1 and 8 threads alike): on masks of ones with a few holes the uint8 targets of the CPU reference
    equal the four-weight restatement at every pixel for M = 28 and 64, and differ from it for M = 65 and 96 (over the 3 x 4 and 37 x 53 crops below at
    225 and 244 pixels: four set taps whose rounded weights sum to 1 - 2^-24 truncate to 0 in one order and give 1 in the other); at M = 256
    the weights are exact and the two forms agree again.  So mask targets for 64 < M <= 256 need the separable form."""
    from abr_iod_amd.structures.segmentation_mask import SegmentationMask
    rng = np.random.default_rng(1)
    diffs = {}
    for M in (28, 64, 65, 96, 256):
        diffs[M] = 0
        for h, w in ((3, 4), (37, 53)):
            m = np.ones((h, w), np.uint8)
            m[rng.random((h, w)) < 0.02] = 0
            ref = SegmentationMask(torch.from_numpy(m), (w, h)).resize((M, M)).get_mask_tensor().numpy()
            four = R.resize_four_weight(m, M).astype(np.int64).astype(np.uint8)
            diffs[M] += int((four != ref).sum())
    print("uint8 pixels where torch's CPU resize differs from the four-weight form:", diffs)
    assert diffs[28] == 0 and diffs[64] == 0
    assert diffs[65] > 0 and diffs[96] > 0

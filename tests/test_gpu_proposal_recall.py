"""GPU: ops.proposal_cover (csrc/proposal_recall.hip) against the host restatement (coco_eval_host): the overlaps bit for bit, the counts
exactly -- proposal and ground-truth counts around the wave width and at the caps in one launch, integer boxes with frequent exact ties
and fractional ones, every hand case of tests/test_proposal_recall_host.py, the fallback for an image over the ground-truth cap, the
smallest and the widest launch, and do_coco_evaluation(box_only=True) on both devices."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from coco_eval_common import tiny  # noqa: E402
from proposal_recall_common import HAND, bits, random_image  # noqa: E402

from abr_iod_amd.data.datasets.evaluation.coco import coco_eval_host as H  # noqa: E402

pytestmark = pytest.mark.gpu

LIMITS = (100, 1000)
RANGES = np.asarray(H.PROPOSAL_AREA_RNG[:4], np.float32)
P_SIZES = (0, 1, 63, 64, 65, 100, 101, 999, 1000)
G_SIZES = (0, 1, 2, 63, 64, 65, 127, 128)


def _flat(images, max_limit):
    """images -> (prop [P_total,4], gt [G_total,4], gt_area [G_total], proposal counts, ground-truth counts) as ops.proposal_cover takes them"""
    props, gts, areas = [], [], []
    for im in images:
        props.append(im["boxes"].reshape(-1, 4)[H.proposal_rank(im["objectness"], max_limit)])
        g, a = H.proposal_ground_truth(im["gt_boxes"], im["gt_area"], im["gt_crowd"])
        gts.append(g)
        areas.append(a)
    return (torch.cat(props).reshape(-1, 4), torch.cat(gts).reshape(-1, 4), torch.cat(areas).reshape(-1), [len(p) for p in props],
            [len(g) for g in gts])


def _host(prop, gt, area, pc, gc, ranges, limits, thrs):
    """what ops.proposal_cover documents, from the host restatement alone"""
    ranges = np.asarray(ranges, np.float32).reshape(-1, 2)
    thrs = torch.as_tensor(thrs, dtype=torch.float32)
    L, A, T, Gt = len(limits), len(ranges), len(thrs), int(sum(gc))
    overlaps = np.full((L, A, Gt), -1, np.float32)
    hits = np.zeros((L, A, T), np.int32)
    num_pos = np.zeros((A,), np.int32)
    po, go = np.concatenate(([0], np.cumsum(pc))), np.concatenate(([0], np.cumsum(gc)))
    for k in range(len(pc)):
        p, g, ar = prop[po[k]: po[k + 1]], gt[go[k]: go[k + 1]], area[go[k]: go[k + 1]]
        for a in range(A):
            valid = (ar >= float(ranges[a, 0])) & (ar <= float(ranges[a, 1]))
            n_valid = int(valid.sum())
            num_pos[a] += n_valid
            for li, lim in enumerate(limits):
                if n_valid == 0 or len(p) == 0:
                    continue
                vec = H.proposal_cover(p[:lim], g[valid])
                overlaps[li, a, go[k]: go[k] + n_valid] = vec.numpy()
                hits[li, a] += (vec[None, :] >= thrs[:, None]).sum(1).to(torch.int32).numpy()
    return {"overlaps": overlaps, "hits": hits, "num_pos": num_pos}


def _check(images, limits=LIMITS, ranges=RANGES, thrs=None, n_fallback=0):
    from abr_iod_amd import ops
    thrs = H.proposal_thresholds() if thrs is None else thrs
    flat = _flat(images, max(limits))
    got = ops.proposal_cover(*flat, ranges, limits, thrs)
    want = _host(*flat, ranges, limits, thrs)
    assert got["overlaps"].dtype == np.float32 and got["overlaps"].shape == want["overlaps"].shape
    assert np.array_equal(bits(got["overlaps"]), bits(want["overlaps"]))
    assert np.array_equal(got["hits"], want["hits"]) and got["hits"].dtype == np.int32
    assert np.array_equal(got["num_pos"], want["num_pos"])
    assert got["n_fallback"] == n_fallback
    return got, flat


def _mixed_images(fractional=False, seed=0):
    rng = np.random.default_rng(seed)
    pairs = [(P, G) for i, P in enumerate(P_SIZES) for G in G_SIZES[i % 2::2]]
    pairs += [(1000, 128), (999, 127), (0, 0), (0, 128), (1, 1), (64, 64)]
    return [random_image(rng, P, G, fractional=fractional) for P, G in pairs]


def test_mixed_sizes_in_one_launch_integer_boxes():
    images = _mixed_images()
    assert 36 <= len(images) <= 44
    got, flat = _check(images)
    # every named count reaches the kernel: the crowd annotations of random_image come on top of G and are dropped again
    assert set(flat[3]) == set(P_SIZES) and set(flat[4]) == set(G_SIZES)
    assert any(any(im["gt_crowd"]) for im in images)
    assert (got["num_pos"] > 0).all() and got["hits"][1, 0, 0] > 0
    # two runs: the integer atomics make the counts reproducible
    from abr_iod_amd import ops
    again = ops.proposal_cover(*flat, RANGES, LIMITS, H.proposal_thresholds())
    assert np.array_equal(again["hits"], got["hits"]) and np.array_equal(again["num_pos"], got["num_pos"])
    assert np.array_equal(bits(again["overlaps"]), bits(got["overlaps"]))


def test_full_caps_without_crowds():
    """exactly 128 ground truths and 1000 proposals in one image, 127 / 999 and 65 / 101 beside it"""
    rng = np.random.default_rng(5)
    images = []
    for P, G in ((1000, 128), (999, 127), (101, 65)):
        images.append(random_image(rng, P, G, crowds=False))
    got, flat = _check(images)
    assert flat[4] == [128, 127, 65] and flat[3] == [1000, 999, 101]


def test_fractional_coordinates():
    pairs = ((0, 3), (1, 2), (63, 65), (65, 63), (100, 1), (101, 64), (999, 2), (1000, 127), (64, 128))
    rng = np.random.default_rng(2)
    got, flat = _check([random_image(rng, P, G, fractional=True) for P, G in pairs])
    assert flat[4] == [G for _, G in pairs]


def test_mixed_sizes_with_fractional_coordinates():
    got, flat = _check(_mixed_images(fractional=True, seed=1))
    assert set(flat[3]) == set(P_SIZES) and set(flat[4]) == set(G_SIZES)


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_cases(name):
    got, flat = _check(HAND[name])
    if name == "iou_exactly_half":
        assert got["overlaps"][:, 0, 0].tolist() == [0.5, 0.5] and got["hits"][0, 0].tolist() == [1] + [0] * 9
    if name == "tie_between_ground_truths":
        assert got["overlaps"][1, 0].tolist() == [0.5, 0.0]
    if name == "duplicates":
        assert got["overlaps"][1, 0].tolist() == [1.0, 1.0, 0.5]
    if name == "empty_range":
        assert got["num_pos"].tolist() == [1, 1, 0, 0] and (got["overlaps"][:, 2:] == -1).all()


def test_limit_and_rank_hand_cases_at_small_limits():
    for name in ("limit_cuts_before_the_cover", "unsorted_objectness"):
        got, _ = _check(HAND[name], limits=(1, 2))
        assert got["overlaps"][:, 0, 0].tolist() == [0.0, 1.0], name


def test_an_image_over_the_ground_truth_cap_goes_to_the_host():
    from abr_iod_amd import ops
    assert ops.COCO_MATCH_MAX_GT == 128 and ops.PROPOSAL_COVER_MAX_PROP >= 1000
    rng = np.random.default_rng(9)
    images = [random_image(rng, P, G) for P, G in ((100, 5), (65, 64), (200, 129), (63, 2), (1000, 7))]
    got, flat = _check(images, n_fallback=1)
    assert flat[4] == [5, 64, 129, 2, 7]
    # its neighbours' numbers are those of a launch without it
    alone, flat2 = _check(images[:2] + images[3:])
    go = np.concatenate(([0], np.cumsum(flat[4])))
    keep = np.concatenate([np.arange(go[k], go[k + 1]) for k in (0, 1, 3, 4)])
    assert np.array_equal(bits(got["overlaps"][:, :, keep]), bits(alone["overlaps"]))


def test_smallest_and_widest_launch():
    rng = np.random.default_rng(4)
    images = [random_image(rng, P, G) for P, G in ((65, 3), (1, 64), (100, 65), (0, 2))]
    _check(images, limits=(50,), ranges=RANGES[:1], thrs=torch.tensor([0.5]))
    _check(images, limits=(10, 64, 100, 1000), ranges=np.asarray(H.PROPOSAL_AREA_RNG, np.float32),
           thrs=torch.arange(0.0, 1.0 + 1e-5, 1.0 / 15, dtype=torch.float32))


def test_nothing_to_launch():
    from abr_iod_amd import ops
    thr = H.proposal_thresholds()
    z4, z1 = torch.zeros((0, 4)), torch.zeros((0,))
    out = ops.proposal_cover(z4, z4, z1, [], [], RANGES, LIMITS, thr)
    assert out["overlaps"].shape == (2, 4, 0) and not out["hits"].any() and not out["num_pos"].any() and out["n_fallback"] == 0
    out = ops.proposal_cover(torch.ones((3, 4)), z4, z1, [3, 0], [0, 0], RANGES, LIMITS, thr)
    assert out["overlaps"].shape == (2, 4, 0) and not out["num_pos"].any()
    # and through the evaluator's core: no image at all is every range empty
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import score_proposals
    cells, n_fallback = score_proposals([], LIMITS, RANGES.tolist())
    assert n_fallback == 0 and all(math.isnan(c["ar"].item()) and c["num_pos"] == 0 and c["gt_overlaps"].numel() == 0 for row in cells for c in row)


def test_arguments_are_validated():
    from abr_iod_amd import ops
    thr = H.proposal_thresholds()
    p, g, a = torch.zeros((2, 4)), torch.zeros((1, 4)), torch.ones((1,))
    with pytest.raises(RuntimeError, match="runs on the device"):
        ops.proposal_cover(p, g, a, [2], [1], RANGES, LIMITS, thr, device="cpu")
    with pytest.raises(RuntimeError, match="float32"):
        ops.proposal_cover(p.double(), g, a, [2], [1], RANGES, LIMITS, thr)
    with pytest.raises(RuntimeError, match="float32"):
        ops.proposal_cover(p, g, a, [2], [1], RANGES, LIMITS, thr.double())
    with pytest.raises(RuntimeError, match="counts"):
        ops.proposal_cover(p, g, a, [3], [1], RANGES, LIMITS, thr)
    with pytest.raises(RuntimeError, match="limits"):
        ops.proposal_cover(p, g, a, [2], [1], RANGES, (0,), thr)
    with pytest.raises(RuntimeError, match="area ranges"):
        ops.proposal_cover(p, g, a, [2], [1], np.zeros((9, 2), np.float32), LIMITS, thr)


def test_box_only_gives_the_same_numbers_on_both_devices():
    from test_proposal_recall_host import KEYS, _fixture_predictions
    from abr_iod_amd.data.datasets.evaluation.coco.coco_eval import do_coco_evaluation, evaluate_box_proposals
    for remove in (True, False):          # (False: also the two images without valid annotations)
        ds = tiny(remove)
        for shifted in (False, True):
            preds = _fixture_predictions(ds, shifted)
            cpu, _ = do_coco_evaluation(ds, preds, True, None, ("bbox",), (), 4, device="cpu")
            dev, second = do_coco_evaluation(ds, preds, True, None, ("bbox",), (), 4, device="cuda")
            assert second is None
            for key in KEYS:
                a, b = cpu.results["box_proposal"][key], dev.results["box_proposal"][key]
                assert (math.isnan(a) and math.isnan(b)) or a == b, (key, a, b)
    ds = tiny()
    preds = _fixture_predictions(ds, True)
    for area, limit in (("all", None), ("medium", 100), ("512-inf", 1000)):
        a = evaluate_box_proposals(preds, ds, area=area, limit=limit, device="cpu")
        b = evaluate_box_proposals(preds, ds, area=area, limit=limit, device="cuda")
        assert a["num_pos"] == b["num_pos"] and np.array_equal(bits(a["gt_overlaps"]), bits(b["gt_overlaps"]))
        assert np.array_equal(bits(a["recalls"]), bits(b["recalls"])) and np.array_equal(bits(a["ar"]), bits(b["ar"]))

"""GPU: the proposal ranking (csrc/topk.hip: `topk_sigmoid` and `abr_sort_scores_desc`) against the exact reference of tests/ranking_ref.py.

The contract is "descending score, equal scores by ascending index" -- the first k of that order, nothing else.  torch.topk cannot check it
(it leaves the members of a tie group open), so every case here asserts torch.equal(idx, reference idx) on logits whose order does not hang
on an expf rounding (multiples of 0.5 and the certain saturations: test_ranking_ref.py), and the scores against torch.sigmoid at the
project's rtol = 2e-7, atol = 0.  The cases sit where the five-kernel chain changes its path: the tie group cut by k, k == n (no selection),
the slice / chunk sizes, more ties of the k-th key than the 16384-word sort holds (zero-padded batches do that), one level-1 bin holding
everything, zero keys next to the zero padding, the largest admitted image, and the per-stream scratch across such calls.

What catches what (one-line changes to topk.hip tried on the MI355X, not kept): candidates `> thr` instead of `>= thr` fails the tie-cut,
k / n edge, one-bin, saturation, largest-image and scratch tests; survivors `bin >= b1` instead of `bin > b1` fails four of the five
overflow cases, the one-bin, largest-image and scratch tests; `j` instead of `~j` in the word fails every index comparison of the file.
Without the tie selection over the index bits, overflow cases 1-4 and the scratch test fail (case 0, k = 100, happened to pass: the
order in which workgroups win their atomics is usually, not always, the slice order) and nothing else does."""
import numpy as np
import pytest
import torch

import ranking_ref as R

pytestmark = pytest.mark.gpu

KMAX = 15360          # largest admitted k (and n of the score sort): CAP - 1024
NMAX = 196608         # largest admitted image


def topk_exact(y_np, A, k, tag=None, nan_heads=None):
    """one library call on y_np [N, nloc, ld], checked index for index (and score for score) against the reference; returns (scores, idx).
    nan_heads[i] = number of NaN logits of image i: they rank first, in any order among themselves (membership only)"""
    from abr_iod_amd import ops
    y = torch.from_numpy(y_np).cuda()
    N = y.shape[0]
    sc, idx = ops.topk_sigmoid(y, A, k)
    ref_i, _ = R.topk_ref(y_np, A, k)
    ref_i = torch.from_numpy(ref_i)
    got = idx.cpu()
    for i in range(N):
        h = 0 if nan_heads is None else nan_heads[i]
        assert sorted(got[i, :h].tolist()) == sorted(ref_i[i, :h].tolist()), (tag, i)
        if not torch.equal(got[i, h:], ref_i[i, h:]):
            bad = int((got[i, h:] != ref_i[i, h:]).nonzero()[0]) + h
            raise AssertionError("%s: image %d, first difference at rank %d of %d: got index %d, want %d (%d ranks differ)"
                                 % (tag, i, bad, k, int(got[i, bad]), int(ref_i[i, bad]), int((got[i] != ref_i[i]).sum())))
    want_s = torch.sigmoid(y[:, :, :A].reshape(N, -1)).gather(1, ref_i.cuda())
    assert torch.allclose(sc, want_s, rtol=2e-7, atol=0, equal_nan=True), tag
    return sc, idx


# ------------------------------------------------------------------------------------------------------------------------------------ A1
@pytest.mark.parametrize("A", [1, 3, 15])
def test_tie_group_cut_by_k_returns_its_lowest_indices(A):
    """values in {-1, 0, 1}, n = 3000: k = (number of +1) + m cuts one entry short of the zero group, exactly at it, one entry and half the
    group into it -- the zeros that are returned are the lowest-indexed ones, in every layout (A | ld, ld = A + 1, ld = 5A + 2)"""
    n, N = 3000, 2
    for ld in (A, A + 1, 5 * A + 2):
        rng = np.random.default_rng(100 * A + ld)
        flat = R.draw(rng, "three", (N, n))
        flat[1] = R.draw(rng, "three", n, p=[0.2, 0.5, 0.3])                    # another image, other group sizes
        y = R.embed(rng, flat, A, ld)
        for img in range(N):                                                    # k is per call: cut each image's zero group in turn
            ones, zeros = int((flat[img] == 1).sum()), int((flat[img] == 0).sum())
            for m in (-1, 0, 1, zeros // 2):
                topk_exact(y, A, ones + m, ("A1", A, ld, img, m))


# ------------------------------------------------------------------------------------------------------------------------------------ A2
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1023, 1024, 1025, KMAX])
def test_k_and_n_edges(n):
    """k in {1, n - 1, n} (k == n takes every key without a selection) around the slice (256 keys) and chunk (1024 words) sizes, one image
    and three images with different data"""
    for N, ld in ((1, 1), (3, 3)):
        rng = np.random.default_rng(n * 7 + N)
        y = R.embed(rng, R.draw(rng, "halves", (N, n)), 1, ld)
        for k in sorted({1, max(n - 1, 1), n}):
            topk_exact(y, 1, k, ("A2", n, N, k))


# ------------------------------------------------------------------------------------------------------------------------------------ A3
def overflow_cases():
    """(tag, logits [1, n, 1], k): more keys equal to the k-th key than the 16384-word sort holds"""
    rng = np.random.default_rng(3)
    two = np.zeros(39000, np.float32)
    two[rng.permutation(39000)[:9000]] = 2.0                                    # 9000 high, 30 000 tied low
    return [("const20000_k100", np.zeros((1, 20000, 1), np.float32), 100),
            ("const20000_k12000", np.zeros((1, 20000, 1), np.float32), 12000),
            ("const20000_k15360", np.zeros((1, 20000, 1), np.float32), KMAX),
            ("two39000_k15360", two.reshape(1, -1, 1), KMAX),
            ("const150000_k12000", np.zeros((1, 150000, 1), np.float32), 12000)]


@pytest.mark.parametrize("case", range(5))
def test_more_ties_than_the_sort_holds(case):
    """all-equal logits (the zero-padded interior of a batch): the result is idx = 0 .. k-1 exactly -- with two values, the high group
    followed by the lowest tied indices -- and a second identical call returns the identical tensors.  (Before the selection went on over
    the index bits, the ties that reached the sort were the ones whose workgroup had won an atomic.)"""
    tag, y, k = overflow_cases()[case]
    s1, i1 = topk_exact(y, 1, k, tag)
    if tag.startswith("const"):
        assert torch.equal(i1.cpu(), torch.arange(k).view(1, k))
    else:
        high = np.nonzero(y.reshape(-1) == 2.0)[0]
        low = np.nonzero(y.reshape(-1) == 0.0)[0]
        assert np.array_equal(i1.cpu().numpy()[0], np.concatenate([high, low[:k - len(high)]]))
    s2, i2 = topk_exact(y, 1, k, tag + " again")
    assert torch.equal(i1, i2) and torch.equal(s1, s2)


# ------------------------------------------------------------------------------------------------------------------------------------ A4
def test_everything_in_one_level1_bin():
    """logits 3.0 .. 8.0 in halves: every sigmoid shares the top 12 key bits, so the level-1 histogram decides nothing, all 60 000 keys are
    candidates and levels 2 and 3 carry the selection"""
    rng = np.random.default_rng(4)
    y = R.embed(rng, R.draw(rng, "one_bin", (2, 60000)), 3, 4)
    topk_exact(y, 3, 6000, "A4")


# ------------------------------------------------------------------------------------------------------------------------------------ A5
@pytest.mark.parametrize("with_nan", [False, True])
def test_saturated_and_special_logits(with_nan):
    """blocks of +30 / +inf (1.0f) and -200 / -inf (0.0f, key 0) among ordinary logits; k cuts inside the 1.0 group and inside the 0.0 group.
    Zero-score words come back in ascending index and are not taken for the zero padding of the sort.  A few NaN logits rank first, as
    with torch.topk (membership only)."""
    rng = np.random.default_rng(5 + with_nan)
    N, nloc, A, ld = 2, 1200, 3, 4
    n = nloc * A
    flat = R.draw(rng, "specials", (N, n), p=[0.3 / 33] * 33 + [0.15, 0.2, 0.2, 0.15])
    flat[0, 500:900] = 30.0; flat[0, 900:1000] = np.inf; flat[1, 2000:2600] = -200.0; flat[1, 2600:2700] = -np.inf
    heads = [0, 0]
    if with_nan:
        flat[0, [3, 1700, 3599]] = np.nan; flat[1, [0, 1, 2, 2650]] = np.nan
        heads = [3, 4]
    s = R.sigmoid32(flat)
    n_one, n_zero = (s == 1).sum(1), (s == 0).sum(1)
    assert n_one.min() > 600 and n_zero.min() > 600
    y = R.embed(rng, flat, A, ld)
    for k in (max(heads) + int(n_one.min()) // 2, n - int(n_zero.min()) // 2, n):
        sc, idx = topk_exact(y, A, k, ("A5", with_nan, k), nan_heads=heads)
        if k > n - int(n_zero.min()):
            assert float(sc[:, -1].max()) == 0.0                                # the cut really is inside the zero-score group


# ------------------------------------------------------------------------------------------------------------------------------------ A6
def test_largest_admitted_image_and_the_limits():
    """n = 196 608 keys of one image (the partition kernel's LDS limit) is ranked exactly; one key more, or k = 15 361, is refused by the
    library's argument checks -- both sit in front of every allocation and launch (abr_topk_sigmoid / topk_run) -- with a message that
    names the limit"""
    from abr_iod_amd import ops
    rng = np.random.default_rng(6)
    topk_exact(R.draw(rng, "halves", (1, NMAX, 1)), 1, 12000, "A6")
    with pytest.raises(RuntimeError, match="at most 196608"):
        ops.topk_sigmoid(torch.zeros(1, NMAX + 1, 1, device="cuda"), 1, 12000)
    with pytest.raises(RuntimeError, match="max 15360"):
        ops.topk_sigmoid(torch.zeros(1, 20000, 1, device="cuda"), 1, KMAX + 1)


# ------------------------------------------------------------------------------------------------------------------------------------ A7
def test_scratch_is_clean_after_an_overflowing_call():
    """the overflow cases interleaved with smaller and larger ordinary calls on one stream, each checked exactly: the counters and the
    histogram of the per-stream scratch are as clean after a call that took the tie selection as after any other"""
    rng = np.random.default_rng(7)
    ov = overflow_cases()

    def ordinary(N, nloc, A, ld, k):
        return R.embed(rng, R.draw(rng, "halves", (N, nloc * A)), A, ld), A, k

    seq = [ordinary(2, 700, 3, 4, 900), (ov[2][1], 1, ov[2][2]), ordinary(4, 38 * 63, 15, 16, 12000), (ov[3][1], 1, ov[3][2]),
           ordinary(1, 13 * 17, 3, 17, 300), (ov[4][1], 1, ov[4][2]), ordinary(3, 25000, 1, 2, 6000), (ov[0][1], 1, ov[0][2]),
           ordinary(5, 38 * 38, 15, 15, KMAX)]
    for step, (y, A, k) in enumerate(seq):
        topk_exact(y, A, k, ("A7", step))


# ------------------------------------------------------------------------------------------------------------------------------------ B
def lib_sort(scores_np):
    from abr_iod_amd import _lib as L
    s = torch.from_numpy(scores_np).cuda()
    n = s.shape[0]
    order = torch.empty(n, dtype=torch.int64, device="cuda")
    L.check(L.lib().abr_sort_scores_desc(L.ptr(s), n, L.ptr(order), L.stream()), "sort_scores_desc")
    return order.cpu().numpy()


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 4097, KMAX])
def test_score_sort_is_index_exact(n):
    """heavy duplicates, negatives, denormals, +-0.0, +-inf and NaNs of both signs: `order` is the reference's, index for index"""
    s = R.sort_zoo(np.random.default_rng(n), n)
    if n > 1000:
        assert np.isnan(s).any() and np.signbit(s[s == 0]).any() and not np.signbit(s[s == 0]).all()
    got, want = lib_sort(s), R.sort_desc_ref(s)
    assert np.array_equal(got, want), (n, int((got != want).sum()))


def test_score_sort_refuses_more_than_it_holds():
    """n = 15 361: the error code (the argument check is the first statement of abr_sort_scores_desc, before any launch)"""
    with pytest.raises(RuntimeError, match="at most 15360"):
        lib_sort(np.zeros(KMAX + 1, np.float32))


def test_nms_is_one_order_on_both_sides_of_the_hand_over():
    """_C.nms ranks n = 15 360 boxes with the library's sort and n = 15 361 with ATen's stable sort: the same boxes plus one, tied scores
    (no signed zeros, no NaNs), both index-exact against the oracle's nms (descending score, ties by ascending index)"""
    from abr_iod_amd import _C
    from oracle import ops as O
    rng = np.random.default_rng(8)
    n = KMAX + 1
    scores = R.sort_zoo(rng, n, specials=False)
    centers = rng.uniform([50, 50], [950, 550], (n // 20 + 1, 2)).repeat(20, 0)[:n]
    c = centers + rng.normal(0, 12, (n, 2))
    wh = np.exp(rng.normal(np.log(120), 0.5, (n, 2)))
    boxes = np.concatenate([c - wh / 2, c + wh / 2], 1).astype(np.float32)
    for m in (KMAX, KMAX + 1):
        want = O.nms(boxes[:m], scores[:m], 0.6)
        got = _C.nms(torch.from_numpy(boxes[:m]).cuda(), torch.from_numpy(scores[:m]).cuda(), 0.6).cpu().numpy()
        assert 1000 < len(want) < m - 1000      # (about the inputs, not the library: thousands kept, thousands suppressed -- the oracle keeps 4474)
        assert np.array_equal(got, want), (m, len(got), len(want))


def test_signed_zeros_are_the_one_place_the_two_sorts_differ():
    """The ONE known divergence between the two routes of _C.nms: scores -0.0 and +0.0.  The library's key is the bit pattern, so every
    +0.0 ranks before every -0.0; ATen's stable sort (n > 15 360) compares them equal and keeps them in index order.  Pinned here so that
    a change to either side shows up."""
    s = np.array([-0.0, 0.0, 1.0, -0.0, 0.0, -1.0], np.float32)
    assert lib_sort(s).tolist() == [2, 1, 4, 0, 3, 5]
    assert torch.sort(torch.from_numpy(s).cuda(), descending=True, stable=True)[1].tolist() == [2, 0, 1, 3, 4, 5]

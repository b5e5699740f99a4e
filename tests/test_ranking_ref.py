"""The exact ranking reference (tests/ranking_ref.py), checked on the CPU before the GPU tests lean on it.

  * every value set the GPU tests draw logits from has neighbouring distinct float32 sigmoids at least 64 ulps apart: no honest float32
    sigmoid (the kernel's is within 2 ulps, test_topk_sigmoid_matches_torch) can exchange two of them, so the reference order is the order;
    and the saturations the sets rely on are exact (+30, +inf -> 1.0f; -200, -inf -> 0.0f);
  * ONE_BIN really is one level-1 bin of the selection (the top 12 bits of the key);
  * `topk_ref` agrees with torch.sigmoid(...).topk on the scores, and with torch's indices wherever the order is strict;
  * `sort_desc_ref` agrees with torch.sort(stable=True, descending=True) index for index on inputs without signed zeros or NaNs, and puts
    the signed zeros and the NaNs where the library documents them."""
import numpy as np
import pytest
import torch

import ranking_ref as R


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32).astype(np.int64)


@pytest.mark.parametrize("name", sorted(R.VALUE_SETS))
def test_value_sets_leave_no_doubt_about_the_order(name):
    v = R.VALUE_SETS[name]
    s = np.unique(R.sigmoid32(v))                       # distinct float32 scores, ascending (non-negative: bit patterns order like values)
    gaps = np.diff(bits(s))
    assert (gaps >= 64).all(), (name, int(gaps.min()))
    # multiples of 0.5 in [-8, 8] or a certain saturation
    fin = v[np.isfinite(v) & (np.abs(v) <= 8)]
    assert np.array_equal(fin * 2, np.round(fin * 2))
    assert set(v[~(np.isfinite(v) & (np.abs(v) <= 8))].tolist()) <= {30.0, -200.0, -np.inf, np.inf}


def test_saturations_are_exact_in_float32():
    assert bits(R.sigmoid32(np.float32([30.0, np.inf]))).tolist() == [0x3F800000] * 2
    assert bits(R.sigmoid32(np.float32([-200.0, -np.inf]))).tolist() == [0, 0]
    # ... for any float32 evaluation of 1 / (1 + exp(-x)), not just the float64 one: exp(-30) is below half an ulp of 1, exp(200) overflows
    assert np.float32(1) + np.float32(np.exp(-30.0)) == np.float32(1)
    assert np.exp(200.0) > np.finfo(np.float32).max
    assert R.sigmoid32(np.float32(8.0)) < np.float32(1) and R.sigmoid32(np.float32(-8.0)) > np.float32(1e-4)


def test_one_bin_shares_the_top_12_key_bits():
    k = bits(R.sigmoid32(R.ONE_BIN))
    assert len(set((k >> 20).tolist())) == 1 and len(set(k.tolist())) == len(R.ONE_BIN)
    assert len(set((k >> 8).tolist())) > 1               # ... and not the next level: levels 2 and 3 have work to do


@pytest.mark.parametrize("name,N,nloc,A,ld,k", [("halves", 3, 500, 3, 5, 700), ("three", 2, 200, 15, 15, 1500), ("one_bin", 1, 4000, 1, 1, 400),
                                              ("specials", 2, 300, 3, 17, 900)])
def test_topk_ref_scores_match_torch(name, N, nloc, A, ld, k):
    rng = np.random.default_rng(len(name) + nloc)
    y = R.embed(rng, R.draw(rng, name, (N, nloc * A)), A, ld)
    idx, sc = R.topk_ref(y, A, k)
    s_all = torch.sigmoid(torch.from_numpy(y)[:, :, :A].reshape(N, -1))
    ref_s, ref_i = s_all.topk(k, dim=1, sorted=True)
    assert torch.allclose(torch.from_numpy(sc), ref_s, rtol=2e-7, atol=0)
    assert torch.allclose(s_all.gather(1, torch.from_numpy(idx)), ref_s, rtol=2e-7, atol=0)
    for i in range(N):
        assert len(set(idx[i].tolist())) == k
        eq = sc[i, 1:] == sc[i, :-1]
        assert (sc[i, 1:] <= sc[i, :-1]).all() and (idx[i, 1:][eq] > idx[i, :-1][eq]).all()      # ties by ascending index
        # and the members of the group cut by k are its lowest indices
        last = np.nonzero(R.sigmoid32(y[i, :, :A].reshape(-1)) == sc[i, -1])[0]
        took = idx[i][sc[i] == sc[i, -1]]
        assert np.array_equal(took, last[:len(took)])


def test_topk_ref_ranks_nan_first():
    y = np.float32([[[0.5], [np.nan], [8.0], [np.nan], [-1.0]]])
    idx, sc = R.topk_ref(y, 1, 4)
    assert idx.tolist() == [[1, 3, 2, 0]] and np.isnan(sc[0, :2]).all()


@pytest.mark.parametrize("n", [1, 2, 1025, 15360])
def test_sort_desc_ref_matches_torch_stable_sort(n):
    s = R.sort_zoo(np.random.default_rng(n), n, specials=False)
    assert not np.isnan(s).any() and not (s == 0).any()
    if n > 1000:
        assert np.isinf(s).any() and (np.abs(s[s != 0]) < 1e-38).any() and len(np.unique(s)) < n // 10
    want = torch.sort(torch.from_numpy(s), descending=True, stable=True)[1].numpy()
    assert np.array_equal(R.sort_desc_ref(s), want)


def test_sort_desc_ref_places_zeros_and_nans_as_documented():
    s = R.SORT_ZOO[[1, 0, 17, 16, 15, 18, 0, 1, 2, 19, 20]]      # -0 +0 +nan -inf +inf -nan +0 -0 1.0 +snan -nan(all ones)
    order = R.sort_desc_ref(s)
    # positive NaNs (larger payload first), +inf, 1.0, the +0.0s by index, the -0.0s by index, -inf, negative NaNs (larger payload last)
    assert order.tolist() == [2, 9, 4, 8, 1, 6, 0, 7, 3, 5, 10]
    full = R.sort_zoo(np.random.default_rng(0), 4097)
    o = R.sort_desc_ref(full)
    v = full[o]
    fin = ~np.isnan(v)
    assert (v[fin][1:] <= v[fin][:-1]).all()                      # float order on everything that has one
    assert sorted(o.tolist()) == list(range(4097))
    assert np.isnan(v[0]) and np.isnan(v[-1]) and not np.signbit(v[0]) and np.signbit(v[-1])

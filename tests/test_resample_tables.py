"""CPU: `abr_iod_amd/data/resample.py::coeff_table` -- the vectorised builder of the fixed-point filter tables the package hands to
`abr_img_resample_u8` -- against the oracle's loop restatement of Pillow's `precompute_coeffs` + `normalize_coeffs_8bpc`
(`oracle/abr_data_ref.py::precompute_coeffs`, itself pinned to Pillow by tests/test_oracle_data.py): bounds, tap count and every
coefficient, for both filters and every ordered pair of unequal sizes from 1..33 plus 63, 64, 65, 127, 500, 1333 (2964 tables).  And the
int32 accumulators of the resample kernels at the longest filters the data path can meet: 255 * max_row(sum |coeff|) + 2^21 < 2^31."""
import numpy as np
import pytest

from abr_iod_amd.data.resample import BICUBIC, BILINEAR, PRECISION_BITS, coeff_table
from oracle import abr_data_ref as R

SIZES = list(range(1, 34)) + [63, 64, 65, 127, 500, 1333]


@pytest.mark.parametrize("name", [BILINEAR, BICUBIC])
@pytest.mark.parametrize("a", SIZES)
def test_coeff_table_equals_pillow_restatement(a, name):
    """every table that reads an axis of `a` pixels"""
    n = 0
    for b in SIZES:
        if a == b:
            continue
        bounds, coeffs, ksize = coeff_table(a, b, name)
        rb, rk, rn = R.precompute_coeffs(a, b, name)
        assert ksize == rn, (a, b)
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and bounds.shape == (b, 2) and coeffs.shape == (b, ksize), (a, b)
        assert np.array_equal(bounds, rb), (a, b)
        assert int(bounds[:, 1].max()) <= ksize and int(bounds[:, 1].min()) >= 1 and int(bounds[:, 0].min()) >= 0, (a, b)
        assert int((bounds[:, 0] + bounds[:, 1]).max()) <= a, (a, b)          # (no tap outside the axis: the kernels index with these)
        live = np.arange(ksize)[None, :] < rb[:, 1:2]                         # coefficients up to each row's tap count
        assert np.array_equal(coeffs[live], rk[live]), (a, b, int((coeffs[live] != rk[live]).sum()))
        n += 1
    assert n == len(SIZES) - 1


@pytest.mark.parametrize("a,b,taps", [(2000, 3, 2669), (1333, 1, 5333), (4000, 7, 2287)])
def test_int32_accumulators_cannot_overflow_at_the_longest_filters(a, b, taps):
    """acc = 2^21 + sum_t u8 * k[t] with u8 <= 255: |acc| <= 2^21 + 255 * sum |k| must stay below 2^31 (bicubic has negative lobes, so the sum of
    magnitudes exceeds 2^22)"""
    bounds, coeffs, ksize = coeff_table(a, b, BICUBIC)
    rb, rk, rn = R.precompute_coeffs(a, b, BICUBIC)
    assert ksize == rn == taps
    assert np.array_equal(bounds, rb)
    live = np.arange(ksize)[None, :] < rb[:, 1:2]
    assert np.array_equal(coeffs[live], rk[live])
    mag = np.where(live, np.abs(coeffs.astype(np.int64)), 0).sum(1)
    assert 255 * int(mag.max()) + (1 << (PRECISION_BITS - 1)) < (1 << 31), int(mag.max())

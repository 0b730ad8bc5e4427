"""The check of tests/test_gpu_krylov_kernels.py discriminates (no GPU): krylov_sweep_ref.mgs_ratios passes a
correct float64 emulation of the one-pass MGS sweep and fails each of five wrong ones, at the smallest and the
largest n the GPU tests use.

Measured (this file prints them; i = 6): the correct emulation reaches at most 0.16 of the bound on the scalars
(n = 1; 1.7e-6 at n = 442 368, where the bound's n u is far above what pairwise sums lose) and 0.35 on w.  The
mutant that comes closest to the bound is `norm_early` at n = 442 368 (the norm formed before the last of six
updates): its norm misses by 1.3e3 times the bound.  One element of 442 368 missing from every sum (`drop_last`)
misses by 8.8e4 times on the scalars and 2.9e12 times on w; a skipped slot, a stale h and a partial counted twice
by 3.5e5 to 1.9e8 times.  At n = 1 every mutant misses by more than 1.6e5 times.  So the smallest mutant error is
three orders of magnitude outside the bound at the largest shape and more at every smaller one."""
import numpy as np
import pytest

import krylov_sweep_ref as R

N_SMALL = 1                 # the GPU tests' smallest n
N_LARGE = 12 * 9 * 4096     # their largest: k_mgs_wide<1024, 12> on 9 workgroups, every pass full


@pytest.fixture(scope="module", params=[N_SMALL, N_LARGE], ids=["n1", "n442368"])
def data(request):
    n = request.param
    i = 6
    w, V = R.make_inputs(4242, n, i, rows=1)
    return n, i, w, V


def test_correct_emulation_is_inside_the_bound(data):
    n, i, w, V = data
    h, wd = R.emulate_mgs(w, V, i)
    rh, rw = R.mgs_ratios(w, V, i, h, wd)
    print(f"n {n}: correct float64 sweep at {rh:.3g} of the bound (scalars), {rw:.3g} (w)")
    assert rh <= 1.0 and rw <= 1.0


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_mutant_is_outside_the_bound(data, mutant):
    n, i, w, V = data
    h, wd = R.emulate_mgs(w, V, i, mutant)
    rh, rw = R.mgs_ratios(w, V, i, h, wd)
    print(f"n {n}: {mutant} at {rh:.3g} times the bound (scalars), {rw:.3g} (w)")
    # the scalars alone must give it away: a kernel's w can be right while its reduction is wrong
    if mutant == "stale_h":
        # the update is what is wrong: w and every later scalar
        assert rh > 1.0 and rw > 1.0
    else:
        assert rh > 1.0


def test_nan_and_zero_bounds_fail():
    """a NaN from a read past n, or any error where the bound is zero, can never pass"""
    w, V = R.make_inputs(1, 64, 2, rows=1)
    h, wd = R.emulate_mgs(w, V, 2)
    hn = h.copy()
    hn[1] = np.nan
    assert R.mgs_ratios(w, V, 2, hn, wd)[0] == float("inf")
    wn = wd.copy()
    wn[5] = np.nan
    assert R.mgs_ratios(w, V, 2, h, wn)[1] == float("inf")
    assert R._ratio(np.array([1e-300]), np.array([0.0])) == float("inf")
    assert R._ratio(np.array([0.0]), np.array([0.0])) == 0.0

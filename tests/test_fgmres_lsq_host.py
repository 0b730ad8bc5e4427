"""FGMRES's least-squares recurrence on the host (no GPU): GivensLsq of csrc/fgmres_lsq.hpp, the one object all three
FGMRES drivers feed their Hessenberg columns to, through Nfft4GPAmdDebugGivensLsq, against numpy's lstsq.

The matrices: diagonal 4 + U(0, 1), above it U(-0.5, 0.5), subdiagonal U(0.5, 1), beta in U(0.5, 2); their condition
number is at most 3.  Bounds: 1e-13 relative for the solution, 1e-13 * beta absolute for every residual estimate (at
k = 40 the residual falls below lstsq's own noise, so a relative bound fails for the reference itself).  A numpy
restatement of the recurrence measured 4.9e-15 and 6.4e-15 on these matrices over 20 seeds: a margin of about 15."""
import ctypes as C

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

KS = (1, 2, 5, 40)
SEEDS = (0, 1, 2, 3, 4)
TOL = 1e-13


def hessenberg(k, seed):
    """(H, beta): H column-major (k + 1) x k upper Hessenberg"""
    rng = np.random.default_rng(1000 * k + seed)
    H = np.triu(rng.uniform(-0.5, 0.5, (k + 1, k)), 1)
    H[np.arange(k), np.arange(k)] = 4.0 + rng.uniform(0.0, 1.0, k)
    H[np.arange(1, k + 1), np.arange(k)] = rng.uniform(0.5, 1.0, k)
    return np.asfortranarray(H), float(rng.uniform(0.5, 2.0))


def givens_lsq(H, beta, prior=None):
    """(res, y, breakdown) of a cycle on (H, beta); prior = (H0, beta0): a cycle run on the same object before it"""
    k = H.shape[1]
    assert H.shape == (k + 1, k) and H.flags.f_contiguous
    res, y, brk = np.full(k, np.nan), np.full(k, np.nan), C.c_int(-2)
    H0, beta0 = prior if prior else (None, 0.0)
    rc = amd.lib().Nfft4GPAmdDebugGivensLsq(k, beta, H.ctypes.data, H0.shape[1] if prior else 0, beta0,
                                            H0.ctypes.data if prior else None, res.ctypes.data, y.ctypes.data,
                                            C.byref(brk))
    assert rc == 0
    return res, y, brk.value


def lstsq(H, beta, j):
    """(y, residual norm) of the leading (j + 1) x j problem min ||beta e1 - H y||"""
    rhs = np.zeros(j + 1)
    rhs[0] = beta
    y = np.linalg.lstsq(H[:j + 1, :j], rhs, rcond=None)[0]
    return y, np.linalg.norm(rhs - H[:j + 1, :j] @ y)


@pytest.mark.parametrize("k", KS)
def test_solution_and_residual_estimates(k):
    for seed in SEEDS:
        H, beta = hessenberg(k, seed)
        assert np.linalg.cond(H) <= 3.0
        res, y, brk = givens_lsq(H, beta)
        assert brk == -1
        y_ref, _ = lstsq(H, beta, k)
        ey = np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref)
        er = max(abs(res[j] - lstsq(H, beta, j + 1)[1]) for j in range(k)) / beta
        print(f"k {k} seed {seed}: solution {ey:.2e}, residual estimates {er:.2e} of beta (bound {TOL:.0e})")
        assert ey <= TOL
        assert er <= TOL


@pytest.mark.parametrize("at", (0, 2, 4))
def test_breakdown_leaves_the_earlier_columns(at):
    k = 5
    H, beta = hessenberg(k, 7)
    res_full, _, _ = givens_lsq(H, beta)
    H[:, at] = 0.0  # rotated, its last two entries are both zero
    res, y, brk = givens_lsq(H, beta)
    assert brk == at
    assert np.array_equal(res[:at], res_full[:at]) and np.all(res[at:] == 0.0) and np.all(y[at:] == 0.0)
    if at:
        y_ref, _ = lstsq(H, beta, at)
        assert np.linalg.norm(y[:at] - y_ref) <= TOL * np.linalg.norm(y_ref)


@pytest.mark.parametrize("k,k0", ((5, 40), (40, 5), (2, 2)))
def test_second_cycle_equals_a_fresh_object(k, k0):
    H, beta = hessenberg(k, 11)
    H0, beta0 = hessenberg(k0, 12)
    res, y, brk = givens_lsq(H, beta)
    res2, y2, brk2 = givens_lsq(H, beta, prior=(H0, beta0))
    assert brk == brk2 == -1
    assert np.array_equal(res, res2) and np.array_equal(y, y2)
    # and after a cycle that ended in breakdown
    H0[:, k0 // 2] = 0.0
    res3, y3, brk3 = givens_lsq(H, beta, prior=(H0, beta0))
    assert brk3 == -1 and np.array_equal(res, res3) and np.array_equal(y, y3)


def test_bad_arguments():
    H, beta = hessenberg(2, 0)
    out, brk = np.zeros(2), C.c_int()
    L = amd.lib()
    assert L.Nfft4GPAmdDebugGivensLsq(0, beta, H.ctypes.data, 0, 0.0, None, out.ctypes.data, out.ctypes.data,
                                      C.byref(brk)) == -1
    assert L.Nfft4GPAmdDebugGivensLsq(2, beta, None, 0, 0.0, None, out.ctypes.data, out.ctypes.data,
                                      C.byref(brk)) == -1
    assert L.Nfft4GPAmdDebugGivensLsq(2, beta, H.ctypes.data, 2, 1.0, None, out.ctypes.data, out.ctypes.data,
                                      C.byref(brk)) == -1

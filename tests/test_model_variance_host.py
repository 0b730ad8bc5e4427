"""The fitted model's variance, host side (no GPU): Nfft4GPAmdModelFeatureWeights, the map from the kernel's Fourier
coefficients b^ to the 33 weights of a window's features [cos 2 pi k xs, k = 0..16 | sin 2 pi k xs, k = 1..16],
against the oracle's own b^ and its exact-kernel operator."""
import ctypes as C

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from oracle import OracleAdditiveNFFT

CASES = {  # kernel, l, nw
    "gauss_l0.1_nw1": (amd.GAUSSIAN, 0.1, 1),
    "gauss_l0.3_nw1": (amd.GAUSSIAN, 0.3, 1),
    "gauss_l1_nw1": (amd.GAUSSIAN, 1.0, 1),
    "matern_l0.3_nw1": (amd.MATERN12, 0.3, 1),
    "gauss_l0.1_nw5": (amd.GAUSSIAN, 0.1, 5),
    "gauss_l0.3_nw5": (amd.GAUSSIAN, 0.3, 5),
    "gauss_l1_nw5": (amd.GAUSSIAN, 1.0, 5),
    "matern_l0.3_nw5": (amd.MATERN12, 0.3, 5),
}
N, F, MU = 60, 1.3, 0.01


def weights(kernel, l, scale, nw):
    w = np.full(33, np.nan)
    assert amd.lib().Nfft4GPAmdModelFeatureWeights(int(kernel), float(l), float(scale), int(nw), w.ctypes.data) == 0
    return w


def features(xs):
    """[cos 2 pi k xs, k = 0..16 | sin 2 pi k xs, k = 1..16] per row"""
    k = np.arange(17)
    a = 2.0 * np.pi * xs[:, None] * k[None, :]
    return np.concatenate([np.cos(a), np.sin(a[:, 1:])], axis=1)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request):
    kernel, l, nw = CASES[request.param]
    rng = np.random.default_rng(4321 + nw)
    X = rng.random((N, nw))
    orc = OracleAdditiveNFFT(X, np.arange(nw, dtype=np.int32), nw, 1)
    orc.setup(kernel, F, l, MU)
    return dict(kernel=kernel, l=l, nw=nw, orc=orc)


def test_weights_are_the_oracles_bhat(case):
    """w[cos 0] = b^_0 / nw; w[cos k] = w[sin k] = 2 b^_k / nw, k = 1..15; w[cos 16] = w[sin 16] = b^_-16 / nw, with
    b^ indexed k + 16: to 1e-14 absolute (b^ <= 1: a few ulps of the two libraries' own evaluations)."""
    nw = case["nw"]
    for c in range(nw):
        info = case["orc"].comp_info(c)
        bh = info["bhat"]
        want = np.empty(33)
        want[0] = bh[16] / nw
        want[1:16] = 2.0 * bh[17:32] / nw
        want[17:32] = 2.0 * bh[17:32] / nw
        want[16] = want[32] = bh[0] / nw
        got = weights(case["kernel"], case["l"], info["scale"], nw)
        err = np.max(np.abs(got - want))
        print(f"window {c}: max |w - w(oracle b^)| = {err:.2e}, min w = {got.min():.2e}")
        assert err <= 1e-14, err


def test_weights_reproduce_the_exact_operator(case):
    """f^2 (Z W Z^T + mu I) from the library's weights and the oracle's scaled coordinates is the oracle's exact-kernel
    operator, entry for entry, to 1e-13."""
    orc, nw = case["orc"], case["nw"]
    Z = np.concatenate([features(orc.comp_points(c)[:, 0]) for c in range(nw)], axis=1)
    w = np.concatenate([weights(case["kernel"], case["l"], orc.comp_info(c)["scale"], nw) for c in range(nw)])
    A = F * F * ((Z * w) @ Z.T + MU * np.eye(N))
    ref = np.stack([orc.matsymv(np.eye(N)[i], exact=True) for i in range(N)], axis=1)
    err = np.max(np.abs(A - ref))
    print(f"max |f^2 (Z W Z^T + mu I) - oracle exact| = {err:.2e}")
    assert err <= 1e-13, err


def test_host_lu_fallback():
    """The host LU that stands in when rocSOLVER cannot be loaded: against numpy's solve on nonsymmetric matrices
    that need row interchanges, of the shape of mu I + W G (a row-scaled Gram plus a small diagonal)."""
    L = amd.lib()
    rng = np.random.default_rng(3)
    for n, nrhs in ((1, 1), (2, 2), (7, 7), (165, 165), (300, 5)):
        Z = rng.standard_normal((n + 3, n))
        w = rng.standard_normal(n)  # both signs
        A = np.asfortranarray(MU * np.eye(n) + w[:, None] * (Z.T @ Z))
        B = np.asfortranarray(rng.standard_normal((n, nrhs)))
        X = B.copy(order="F")
        assert L.Nfft4GPAmdHostLuSolve(A.ctypes.data, n, X.ctypes.data, nrhs) == 0
        want = np.linalg.solve(A, B)
        err = np.max(np.abs(X - want)) / np.max(np.abs(want))
        bound = 64.0 * 2.0 ** -52 * np.linalg.cond(A)
        print(f"n {n}: host LU vs numpy {err:.2e}, bound {bound:.2e}")
        assert err <= bound, (n, err, bound)
    Zs = np.zeros((2, 2), order="F")
    assert L.Nfft4GPAmdHostLuSolve(Zs.ctypes.data, 2, np.ones(2).ctypes.data, 1) == 1


def test_bad_arguments():
    w = np.zeros(33)
    L = amd.lib()
    assert L.Nfft4GPAmdModelFeatureWeights(2, 0.3, 0.5, 1, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeights(0, 0.3, 0.5, 0, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeights(0, 0.3, 0.5, 1, None) == -1
    assert L.Nfft4GPAmdModelVarianceInfo(None, C.byref(C.c_int())) == -1

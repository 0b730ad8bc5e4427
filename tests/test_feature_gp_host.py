"""The feature-space GP, host side (no GPU): Nfft4GPAmdModelFeatureWeightsGrad, the map from the derivative kernel's
Fourier coefficients to dW/dl of a window's 33 features, against the oracle's own b^' and its exact-kernel gradient
operator; and the host LU's log|det| and sign (Nfft4GPAmdHostLuLogdet) against numpy's slogdet."""
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


def weights_grad(kernel, l, scale, nw):
    w = np.full(33, np.nan)
    assert amd.lib().Nfft4GPAmdModelFeatureWeightsGrad(int(kernel), float(l), float(scale), int(nw), w.ctypes.data) == 0
    return w


def weight_map(bh, nw):
    """the existing map (test_model_variance_host.py): b^ indexed k + 16 -> the 33 weights"""
    w = np.empty(33)
    w[0] = bh[16] / nw
    w[1:16] = 2.0 * bh[17:32] / nw
    w[17:32] = 2.0 * bh[17:32] / nw
    w[16] = w[32] = bh[0] / nw
    return w


def dscale(kernel, l, scale):
    """md_setup's / nfft_interface.c:536's factor of the derivative kernel"""
    sig = l * scale * np.sqrt(2.0) if kernel == amd.GAUSSIAN else l * scale
    return 2.0 * scale * np.sqrt(2.0) / sig if kernel == amd.GAUSSIAN else scale / sig


def features(xs):
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
    return dict(kernel=kernel, l=l, nw=nw, orc=orc, rng=rng)


def test_weight_gradients_are_the_oracles_bhat_d(case):
    """dw = map(b^' of the oracle) x dscale, to 1e-13 relative to max |dw|"""
    nw = case["nw"]
    for c in range(nw):
        info = case["orc"].comp_info(c)
        want = weight_map(info["bhat_d"], nw) * dscale(case["kernel"], case["l"], info["scale"])
        got = weights_grad(case["kernel"], case["l"], info["scale"], nw)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"window {c}: max |dw - dw(oracle)| / max |dw| = {err:.2e}, max |dw| = {np.max(np.abs(want)):.2e}")
        assert err <= 1e-13, err


def test_weight_gradients_reproduce_the_exact_gradient_operator(case):
    """f^2 (Z diag(dw) Z^T) x from the library's dw and the oracle's scaled coordinates is the l block of the oracle's
    exact-kernel gradient matvec for a standard normal x, to 1e-13 absolute (entries up to 62: a few ulps)"""
    orc, nw = case["orc"], case["nw"]
    Z = np.concatenate([features(orc.comp_points(c)[:, 0]) for c in range(nw)], axis=1)
    dw = np.concatenate([weights_grad(case["kernel"], case["l"], orc.comp_info(c)["scale"], nw) for c in range(nw)])
    x = case["rng"].standard_normal(N)
    got = F * F * (Z * dw) @ (Z.T @ x)
    ref = orc.gradmatsymv(x, exact=True)[N:2 * N]
    err = np.max(np.abs(got - ref))
    print(f"max |f^2 Z dW Z^T x - oracle exact| = {err:.2e} (max |ref| {np.max(np.abs(ref)):.2e})")
    assert err <= 1e-13, err


def test_host_lu_logdet():
    """log|det| and the sign from the host LU against numpy's slogdet, on the matrices of test_host_lu_fallback (both
    signs of weights: row-scaled Grams plus a small diagonal) -- the seed gives determinants of both signs.  Bound:
    the LU's backward error moves log|det| by at most about n eps cond."""
    L = amd.lib()
    rng = np.random.default_rng(3)
    signs = []
    for n in (1, 2, 7, 165, 300):
        Z = rng.standard_normal((n + 3, n))
        w = rng.standard_normal(n)
        A = np.asfortranarray(MU * np.eye(n) + w[:, None] * (Z.T @ Z))
        lad, sg = C.c_double(), C.c_int()
        assert L.Nfft4GPAmdHostLuLogdet(A.ctypes.data, n, C.byref(lad), C.byref(sg)) == 0
        s_np, l_np = np.linalg.slogdet(A)
        bound = 64.0 * 2.0 ** -52 * np.linalg.cond(A) * (1.0 + abs(l_np))
        print(f"n {n}: log|det| {lad.value:.12e} vs numpy {l_np:.12e} (|diff| {abs(lad.value - l_np):.2e}, bound "
              f"{bound:.2e}), sign {sg.value} vs {s_np:.0f}")
        assert sg.value == int(s_np) and abs(lad.value - l_np) <= bound
        signs.append(sg.value)
    assert -1 in signs and 1 in signs, signs
    # a negative determinant by construction: a row interchange of the identity
    P = np.asfortranarray(np.eye(4)[[1, 0, 2, 3]] * 2.0)
    lad, sg = C.c_double(), C.c_int()
    assert L.Nfft4GPAmdHostLuLogdet(P.ctypes.data, 4, C.byref(lad), C.byref(sg)) == 0
    assert sg.value == -1 and abs(lad.value - 4.0 * np.log(2.0)) <= 1e-15
    Zs = np.zeros((2, 2), order="F")
    assert L.Nfft4GPAmdHostLuLogdet(Zs.ctypes.data, 2, C.byref(lad), C.byref(sg)) == 1


def test_bad_arguments():
    w = np.zeros(33)
    L = amd.lib()
    assert L.Nfft4GPAmdModelFeatureWeightsGrad(2, 0.3, 0.5, 1, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeightsGrad(0, 0.0, 0.5, 1, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeightsGrad(0, 0.3, -1.0, 1, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeightsGrad(0, 0.3, 0.5, 0, w.ctypes.data) == -1
    assert L.Nfft4GPAmdModelFeatureWeightsGrad(0, 0.3, 0.5, 1, None) == -1
    lad, sg = C.c_double(), C.c_int()
    assert L.Nfft4GPAmdHostLuLogdet(None, 2, C.byref(lad), C.byref(sg)) == -1
    assert L.Nfft4GPAmdHostLuLogdet(w.ctypes.data, 0, C.byref(lad), C.byref(sg)) == -1
    assert L.Nfft4GPAmdFeatureGpLoss(None, w.ctypes.data, w.ctypes.data, w.ctypes.data) == -1
    assert L.Nfft4GPAmdFeatureGpSetOptions(None, 0, None) == -1
    assert L.Nfft4GPAmdFeatureGpInfo(None, None, None, None, None) == -1
    assert L.Nfft4GPAmdFeatureGpStatus(None, None, None) == -1
    assert L.Nfft4GPAmdFeatureGpMoments(None, None, None, None) == -1

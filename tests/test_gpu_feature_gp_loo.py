"""The exact leave-one-out loss, gradient and per-point predictions in feature space (Nfft4GPAmdFeatureGpLoo*,
k_fgp_loo in csrc/feature_gp.hip; FeatureGP.bind / loo / loo_predict, gp_fit(..., exact=True, objective="loo")).

Conventions of test_gpu_feature_gp.py: make_data, f = 1.3, mu = 0.01 (1e-4 in the last case), Z from the model's
quantised coordinate, W and W' from Nfft4GPAmdModelFeatureWeights[Grad].  The reference is dense numpy on the n x n
matrix: Ainv = inv(f^2 (Z W Z^T + mu I)), a = Ainv y; the loss, mean and variance from diag(Ainv); the gradient
analytic from d diag(A^{-1}) = -diag(A^{-1} dA A^{-1}) and da = -A^{-1} dA a.  No finite differences.

Bound everywhere: 64 2^-52 cond(mu I + W G) / min(1, min_i |mu m_i| of the reference), relative to 1 + |value|: the
project's LU bound times the amplification of the per-point division by m_i = [M^{-1}]_ii = f^2 [A^{-1}]_ii.

The measured errors are tabulated in DESIGN 3.18.
"""
import ctypes as C
import math
import types

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from test_gpu_feature_gp import (F, adam_by_hand, features, make_data, softplus_inverse, transform, weights,
                                 window_map)

pytestmark = pytest.mark.gpu

CASES = {  # n, nw, kernel, l, mu
    "n130_nw5_gauss": (130, 5, amd.GAUSSIAN, 0.1, 0.01),      # two workgroups and two column tiles, one ragged each
    "n1500_nw33_gauss": (1500, 33, amd.GAUSSIAN, 0.1, 0.01),  # R_p != R, nine column tiles
    "n1500_nw5_matern": (1500, 5, amd.MATERN12, 0.3, 0.01),
    "n200_nw3_gauss": (200, 3, amd.GAUSSIAN, 0.3, 0.01),      # 36 negative weights, all m_i > 0
    "n40_nw3_gauss": (40, 3, amd.GAUSSIAN, 0.3, 0.01),        # n < R
    "n2_nw1_gauss": (2, 1, amd.GAUSSIAN, 0.3, 0.01),          # the smallest data set the operator accepts
    "n40_nw3_indefinite": (40, 3, amd.GAUSSIAN, 1.0, 1e-4),   # m_i <= 0 at some points
}
INDEFINITE = "n40_nw3_indefinite"


def dense_loo(co, kernel, Z, y, x, kind):
    """the dense leave-one-out loss, its analytic gradient at x (before the transform `kind`), the per-point mean and
    variance, and the bound"""
    n = Z.shape[0]
    (f, l, mu), dt = transform(x, kind)
    w, dw = weights(co, kernel, l), weights(co, kernel, l, grad=True)
    M = (Z * w) @ Z.T + mu * np.eye(n)
    A = f * f * M
    Ainv = np.linalg.inv(A)
    a = Ainv @ y
    d = np.diag(Ainv).copy()
    loss = 0.5 / n * np.sum(np.log(1.0 / np.abs(d)) + a * a / d + math.log(2.0 * math.pi))
    grad = []
    for D in (2.0 * f * M, f * f * (Z * dw) @ Z.T, f * f * np.eye(n)):
        dd = -np.einsum("ij,ji->i", Ainv @ D, Ainv)
        da = -Ainv @ (D @ a)
        grad.append(0.5 / n * np.sum(-dd / d + 2.0 * a * da / d - a * a * dd / (d * d)))
    cond = np.linalg.cond(mu * np.eye(Z.shape[1]) + w[:, None] * (Z.T @ Z))
    mum = mu * f * f * d  # mu m_i
    bound = 64.0 * 2.0 ** -52 * cond / min(1.0, np.min(np.abs(mum)))
    return dict(loss=loss, grad=np.array(grad) * dt, mean=y - a / d, var=1.0 / d, nonpos=int(np.sum(d <= 0.0)),
                cond=cond, min_mum=np.min(np.abs(mum)), bound=bound, A=A, f=f, l=l, mu=mu)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request, torch_cuda):
    n, nw, kernel, l, mu = CASES[request.param]
    X, y, _, _, _ = make_data(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, mu) == 0
    co = window_map(op)
    fgp = amd.FeatureGP(op, X, y)
    fgp.bind(X, y)
    Z = features(co, X)
    ref = dense_loo(co, kernel, Z, y, (F, l, mu), 3)  # once per case; shared, never written
    out = dict(name=request.param, n=n, nw=nw, kernel=kernel, l=l, mu=mu, X=X, y=y, op=op, co=co, fgp=fgp, Z=Z, ref=ref,
               torch=torch_cuda)
    yield out
    fgp.free()
    op.free()


def check(name, got, want, bound):
    err = abs(got - want) / (1.0 + abs(want))
    print(f"{name}: got {got:.15e}, dense {want:.15e}, error {err:.2e}, bound {bound:.2e}")
    assert err <= bound, (name, err, bound)
    return err


def check_points(name, got, want, bound):
    """per point, relative to 1 + |value|; no point is left out"""
    assert got.shape == want.shape and np.all(np.isfinite(got)) and np.all(np.isfinite(want))
    err = np.abs(got - want) / (1.0 + np.abs(want))
    print(f"{name}: {err.size} points, max error {np.max(err):.2e}, bound {bound:.2e}")
    assert err.size == want.size and np.all(err <= bound), (name, np.max(err), bound)


def test_loss_and_gradient(case):
    """Check 1 (and 4's loss): the loss and the three gradient components against the dense reference, with the
    identity transform, the softplus and a mask."""
    fgp, co, ref = case["fgp"], case["co"], case["ref"]
    x3 = (F, case["l"], case["mu"])
    loss, grad = fgp.loo(x3, transform=3)
    print(f"{case['name']}: cond(mu I + W G) {ref['cond']:.2e}, min |mu m_i| {ref['min_mum']:.2e}, m_i <= 0 at "
          f"{fgp.n_nonpositive} points (dense {ref['nonpos']})")
    errs = [check("loss (identity)", loss, ref["loss"], ref["bound"])]
    for i, nm in enumerate("f l mu".split()):
        errs.append(check(f"dloss/d{nm} (identity)", grad[i], ref["grad"][i], ref["bound"]))
    assert fgp.n_nonpositive == ref["nonpos"]
    assert (ref["nonpos"] > 0) == (case["name"] == INDEFINITE)
    lm, gm = fgp.loo(x3, transform=3, mask=[1, 0, 1])
    assert lm == loss and gm[1] == 0.0 and gm[0] == grad[0] and gm[2] == grad[2]
    l2, g2 = fgp.loo(x3, transform=3)  # the mask does not stick
    assert l2 == loss and np.array_equal(g2, grad)
    x0 = [softplus_inverse(v) for v in x3]
    ref0 = dense_loo(co, case["kernel"], case["Z"], case["y"], x0, 0)
    loss0, grad0 = fgp.loo(x0)
    errs.append(check("loss (softplus)", loss0, ref0["loss"], ref0["bound"]))
    for i, nm in enumerate("f l mu".split()):
        errs.append(check(f"dloss/d{nm} (softplus)", grad0[i], ref0["grad"][i], ref0["bound"]))
    print(f"{case['name']}: table row: cond {ref['cond']:.1e}, min|mu m| {ref['min_mum']:.1e}, max error "
          f"{max(errs):.1e}, bound {ref['bound']:.1e}")


def test_predict(case):
    """Check 2 (and 4's variances): loo_predict's mean and variance per point against y_i - a_i / [A^{-1}]_ii and
    1 / [A^{-1}]_ii."""
    fgp, ref = case["fgp"], case["ref"]
    mean, var = fgp.loo_predict(F, case["l"], case["mu"])
    assert isinstance(mean, np.ndarray) and mean.shape == (case["n"],) and var.shape == (case["n"],)
    check_points(f"{case['name']}: mean", mean, ref["mean"], ref["bound"])
    check_points(f"{case['name']}: variance", var, ref["var"], ref["bound"])
    assert fgp.n_nonpositive == ref["nonpos"]
    assert np.array_equal(var < 0.0, ref["var"] < 0.0)  # negative exactly at the points with m_i <= 0
    assert int(np.sum(var < 0.0)) == ref["nonpos"]
    if case["name"] == INDEFINITE:
        assert ref["nonpos"] > 0
    k = C.c_longlong(-1)  # the count through the C call, with no per-point output
    assert amd.lib().Nfft4GPAmdFeatureGpLooPredict(fgp.h, F, case["l"], case["mu"], None, None, C.byref(k)) == 0
    assert k.value == ref["nonpos"]


@pytest.mark.parametrize("case", ["n40_nw3_gauss", INDEFINITE], indirect=True)
def test_brute_force(case):
    """Check 3: at n = 40, for five indices, the dense (n - 1)-point GP's predictive mean and variance at the deleted
    point (the full data set's Z rows and W) against loo_predict's entries."""
    fgp, ref, y, n = case["fgp"], case["ref"], case["y"], case["n"]
    mean, var = fgp.loo_predict(F, case["l"], case["mu"])
    A = ref["A"]
    for i in (0, 7, 19, 20, 39):
        keep = np.arange(n) != i
        k = A[i, keep]
        sol = np.linalg.solve(A[np.ix_(keep, keep)], np.stack([y[keep], k], axis=1))
        check(f"{case['name']}: point {i} mean", mean[i], k @ sol[:, 0], ref["bound"])
        check(f"{case['name']}: point {i} variance", var[i], A[i, i] - k @ sol[:, 1], ref["bound"])


def raw_loo(case, ldim):
    """loss and gradient through the C calls, X with a larger leading dimension (a second object: the fixture's
    binding stays)"""
    n, nw, X, y = case["n"], case["nw"], case["X"], case["y"]
    buf = np.zeros((nw, ldim))
    buf[:, :n] = X.T
    L = amd.lib()
    h = L.Nfft4GPAmdFeatureGpCreate(case["op"].h, buf.ctypes.data, n, ldim, nw, y.ctypes.data)
    assert h
    x = np.array([F, case["l"], case["mu"]])
    loss, grad = np.zeros(1), np.zeros(3)
    assert L.Nfft4GPAmdFeatureGpSetOptions(h, 3, None) == 0
    assert L.Nfft4GPAmdFeatureGpLooBind(h, buf.ctypes.data, n, ldim, nw, y.ctypes.data) == 0
    rc = L.Nfft4GPAmdFeatureGpLooLoss(h, x.ctypes.data, loss.ctypes.data, grad.ctypes.data)
    L.Nfft4GPAmdFeatureGpFree(h)
    return rc, loss[0], grad


def test_determinism(case):
    """Check 5: two calls, numpy against torch device tensors, and a larger leading dimension give the same bits."""
    fgp, torch = case["fgp"], case["torch"]
    x3 = (F, case["l"], case["mu"])
    loss, grad = fgp.loo(x3, transform=3)
    mean, var = fgp.loo_predict(*x3)
    l2, g2 = fgp.loo(x3, transform=3)
    m2, v2 = fgp.loo_predict(*x3)
    assert l2 == loss and np.array_equal(g2, grad) and np.array_equal(m2, mean) and np.array_equal(v2, var)
    rc, l3, g3 = raw_loo(case, case["n"] + 5)
    assert rc == 0 and l3 == loss and np.array_equal(g3, grad)
    Xd, yd = torch.tensor(case["X"], device="cuda"), torch.tensor(case["y"], device="cuda")
    dev = amd.FeatureGP(case["op"], Xd, yd)
    dev.bind(Xd, yd)
    l4, g4 = dev.loo(x3, transform=3)
    m4, v4 = dev.loo_predict(*x3)
    assert m4.is_cuda and v4.is_cuda
    assert l4 == loss and np.array_equal(g4, grad)
    assert np.array_equal(m4.cpu().numpy(), mean) and np.array_equal(v4.cpu().numpy(), var)
    dev.free()


def test_reversed_order(torch_cuda):
    """Check 5, last part: the 130 points in reversed order, on an object created over the reversed data, meet check
    2's bound point for point (the matrices differ in rounding, so no bitwise claim)."""
    n, nw, kernel, l, mu = CASES["n130_nw5_gauss"]
    X, y, _, _, _ = make_data(n, nw)
    Xr, yr = np.ascontiguousarray(X[::-1]), np.ascontiguousarray(y[::-1])
    op = amd.NFFTAdditiveKernel(Xr, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, mu) == 0
    co = window_map(op)
    ref = dense_loo(co, kernel, features(co, X), y, (F, l, mu), 3)
    fgp = amd.FeatureGP(op, Xr, yr)
    fgp.bind(Xr, yr)
    mean, var = fgp.loo_predict(F, l, mu)
    check_points("reversed: mean", mean[::-1], ref["mean"], ref["bound"])
    check_points("reversed: variance", var[::-1], ref["var"], ref["bound"])
    fgp.free()
    op.free()


def test_training(torch_cuda):
    """Check 6: gp_fit(..., exact=True, objective="loo") for 5 steps equals a hand-written Adam loop over
    FeatureGP.loo bit for bit; objective="mll" equals gp_fit(..., exact=True) bit for bit."""
    n, nw, kernel, l, mu = CASES["n1500_nw5_matern"]
    X, y, _, _, _ = make_data(n, nw)
    win = np.arange(nw, dtype=np.int32)
    x0 = np.array([0.5, -1.0, -3.0])
    hyper, loss, gnorm, flag = amd.gp_fit(X, win, nw, 1, y, x0, 5, lr=0.05, tol=1e-12, exact=True, objective="loo")
    assert flag == 1 and hyper.shape == (6, 3) and loss.shape == (5,)
    op = amd.NFFTAdditiveKernel(np.asfortranarray(X), win, nw, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 1.0, 0.1) == 0  # the moments do not depend on the setup's hyperparameters
    fgp = amd.FeatureGP(op, X, y)
    fgp.bind(X, y)
    hx, hl, hg = adam_by_hand(types.SimpleNamespace(loss=fgp.loo), x0, 5, 0.05, 0)
    print(f"leave-one-out losses {loss}, by hand {hl}")
    assert np.array_equal(hyper, hx) and np.array_equal(loss, hl) and np.array_equal(gnorm, hg)
    mll = amd.gp_fit(X, win, nw, 1, y, x0, 5, lr=0.05, tol=1e-12, exact=True, objective="mll", op=op)
    old = amd.gp_fit(X, win, nw, 1, y, x0, 5, lr=0.05, tol=1e-12, exact=True, op=op)
    for a, b in zip(mll[:3], old[:3]):
        assert np.array_equal(a, b)
    assert not np.array_equal(mll[1], loss)  # the two objectives are different functions
    fgp.free()
    op.free()


@pytest.mark.parametrize("case", ["n130_nw5_gauss"], indirect=True)
def test_refusals(case):
    """Check 7: no evaluation before a bind or after an unbind; a bind with the wrong n or d is refused;
    objective="loo" needs exact=True."""
    L = amd.lib()
    n, nw, X, y = case["n"], case["nw"], np.asfortranarray(case["X"]), case["y"]
    fgp = amd.FeatureGP(case["op"], X, y)
    x = np.array([F, case["l"], case["mu"]])
    loss, grad = np.zeros(1), np.zeros(3)
    k = C.c_longlong(0)

    def loo_loss():
        return L.Nfft4GPAmdFeatureGpLooLoss(fgp.h, x.ctypes.data, loss.ctypes.data, grad.ctypes.data)

    assert L.Nfft4GPAmdFeatureGpSetOptions(fgp.h, 3, None) == 0
    assert loo_loss() == -1  # nothing bound
    assert L.Nfft4GPAmdFeatureGpLooPredict(fgp.h, F, case["l"], case["mu"], None, None, C.byref(k)) == -1
    with pytest.raises(RuntimeError):
        fgp.loo(x, transform=3)
    with pytest.raises(RuntimeError):
        fgp.loo_predict(F, case["l"], case["mu"])
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, X.ctypes.data, n - 1, n, nw, y.ctypes.data) == -1  # a wrong n
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, X.ctypes.data, n, n, nw - 1, y.ctypes.data) == -1  # a wrong d
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, X.ctypes.data, n, n - 1, nw, y.ctypes.data) == -1  # ldim < n
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, X.ctypes.data, n, n, nw, None) == -1  # no y
    assert loo_loss() == -1  # a refused bind binds nothing
    with pytest.raises(ValueError):
        fgp.bind(X[:-1], y[:-1])
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, X.ctypes.data, n, n, nw, y.ctypes.data) == 0
    assert loo_loss() == 0 and loss[0] == fgp.loo(x, transform=3)[0]
    x[2] = 0.0  # what Nfft4GPAmdFeatureGpLoss refuses is refused here too
    assert loo_loss() == -1
    x[2] = case["mu"]
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, None, 0, 0, 0, None) == 0  # unbind
    assert loo_loss() == -1
    Xo = np.asfortranarray(X + 0.75)  # not the object's data: rows leave the domain -- refused with a message, no NaN
    fgp.bind(Xo, y)
    assert loo_loss() == -1
    with pytest.raises(RuntimeError):
        fgp.loo_predict(F, case["l"], case["mu"])
    fgp.bind(None, None)
    fgp.free()
    with pytest.raises(ValueError, match="exact=True"):
        amd.gp_fit(X, np.arange(nw, dtype=np.int32), nw, 1, y, x, 1, objective="loo")


def test_nothing_else_moved(torch_cuda):
    """Check 8: Nfft4GPAmdFeatureGpLoss at the first case gives the same bits before and after a loo call on the
    same object (the factor held in the object is shared)."""
    n, nw, kernel, l, mu = CASES["n130_nw5_gauss"]
    X, y, _, _, _ = make_data(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, mu) == 0
    fgp = amd.FeatureGP(op, X, y)
    before = fgp.loss((F, l, mu), transform=3)
    fresh = fgp.loss((F, 0.2, 0.02), transform=3)  # and at hyperparameters whose factor a loo call builds first
    fgp.bind(X, y)
    fgp.loo((F, l, mu), transform=3)
    after = fgp.loss((F, l, mu), transform=3)
    assert after[0] == before[0] and np.array_equal(after[1], before[1])
    fgp.loo((F, 0.2, 0.02), transform=3)
    again = fgp.loss((F, 0.2, 0.02), transform=3)
    assert again[0] == fresh[0] and np.array_equal(again[1], fresh[1])
    alpha = fgp.solve(X, y, F, l, mu)
    fgp.loo_predict(F, 0.2, 0.02)
    assert np.array_equal(fgp.solve(X, y, F, l, mu), alpha)
    fgp.free()
    op.free()

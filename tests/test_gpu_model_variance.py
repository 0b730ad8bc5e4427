"""The fitted model's predictive standard deviation (Nfft4GPAmdModelFitVariance / PredictStd, csrc/model_variance.hip;
FittedModel.fit_variance / predict_std): std = sqrt|f^2 (mu + phi^T S phi)|, S = mu (mu I + W G)^{-1} W.

Cases as in test_gpu_model.py: n = 1500, X ~ U[0,1)^nw with one 1-D window per feature, f = 1.3, mu = 0.01; 1000
new points uniform in the training set's per-feature [min, max], rows 0 and 1 the minimum and maximum.  R = 33 nw:
33 (less than one column tile of the serving kernel), 165 (a partial tile), 1089 (several tiles, n only just above
R); n = 200 with nw = 5 (n ~ R); and 64 windows (R = 2112, the size that must work) at n = 400 < R."""
import ctypes as C
import os

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from oracle import OracleAdditiveNFFT

pytestmark = pytest.mark.gpu

NNEW, F, MU = 1000, 1.3, 0.01
CASES = {  # n, nw, kernel, l
    "nw1_gauss": (1500, 1, amd.GAUSSIAN, 0.3),
    "nw5_gauss": (1500, 5, amd.GAUSSIAN, 0.1),
    "nw5_matern": (1500, 5, amd.MATERN12, 0.3),
    "nw33_gauss": (1500, 33, amd.GAUSSIAN, 0.1),
    "n200_nw5_gauss": (200, 5, amd.GAUSSIAN, 0.1),
    "n400_nw64_gauss": (400, 64, amd.GAUSSIAN, 0.1),
}


def make_points(n, nw):
    rng = np.random.default_rng(1234 + nw + n)
    X = rng.random((n, nw))
    alpha = rng.standard_normal(n)
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((NNEW, nw))
    Xnew[0], Xnew[1] = lo, hi
    return X, alpha, Xnew, lo, hi


def quantised(co, X, c):
    """the model's coordinate in window c (test_gpu_model.table_eval's q, as a signed fraction of the period)"""
    xs = (X[:, co["feature"][c]] - co["centre"][c]) * co["scale"][c]
    t = xs * 4294967296.0
    q = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64) % (1 << 32)
    return np.where(q >= (1 << 31), q - (1 << 32), q) / 4294967296.0


def features(co, X):
    """per window [cos 2 pi k xs, k = 0..16 | sin 2 pi k xs, k = 1..16], windows in order"""
    k = np.arange(17)
    out = []
    for c in range(len(co["centre"])):
        a = 2.0 * np.pi * quantised(co, X, c)[:, None] * k[None, :]
        out += [np.cos(a), np.sin(a[:, 1:])]
    return np.concatenate(out, axis=1)


def oracle_weights(X, nw, kernel, l):
    """W from the oracle's b^ (index k + 16): b^_0, 2 b^_k (k = 1..15) and b^_-16 for cos and sin, over nw"""
    orc = OracleAdditiveNFFT(X, np.arange(nw, dtype=np.int32), nw, 1)
    orc.setup(kernel, F, l, MU)
    w = np.empty((nw, 33))
    for c in range(nw):
        bh = orc.comp_info(c)["bhat"]
        w[c, 0] = bh[16]
        w[c, 1:16] = w[c, 17:32] = 2.0 * bh[17:32]
        w[c, 16] = w[c, 32] = bh[0]
    return (w / nw).ravel()


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request, torch_cuda):
    torch = torch_cuda
    n, nw, kernel, l = CASES[request.param]
    X, alpha, Xnew, lo, hi = make_points(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, MU) == 0
    model = amd.FittedModel.from_operator(op, torch.tensor(alpha, device="cuda"))
    assert not model.has_variance
    with pytest.raises(RuntimeError, match="fit_variance"):
        model.predict_std(Xnew)
    mean_before = model.predict(Xnew)
    assert model.fit_variance(X) is model and model.has_variance
    co = model.coefficients()
    # the restatement, once per case: dense A = f^2 (Z W Z^T + mu I) in the model's own coordinates
    Z, P = features(co, X), features(co, Xnew)
    w = oracle_weights(X, nw, kernel, l)
    A = F * F * ((Z * w) @ Z.T + MU * np.eye(n))
    cond = np.linalg.cond(MU * np.eye(33 * nw) + w[:, None] * (Z.T @ Z))

    def var_restated(Phi):
        ks = F * F * (Phi * w) @ Z.T  # rows k*^T
        return F * F * (MU + np.einsum("ij,j,ij->i", Phi, w, Phi)) - np.einsum("ij,ji->i", ks, np.linalg.solve(A, ks.T))

    out = dict(name=request.param, n=n, nw=nw, kernel=kernel, l=l, X=X, Xnew=Xnew, lo=lo, hi=hi, op=op, model=model,
               co=co, A=A, cond=cond, var_new=var_restated(P), var_train=var_restated(Z), mean_before=mean_before,
               full=model.predict_std(Xnew), n_outside_full=model.n_outside, torch=torch)
    yield out
    model.free()
    op.free()


def raw_std(model, X, ldim, device=None, noise=1):
    """Nfft4GPAmdModelPredictStd on a column-major buffer of leading dimension ldim; (status, std, n_outside)"""
    n_new, dd = X.shape
    buf = np.zeros((dd, ldim))
    buf[:, :n_new] = X.T
    nout = C.c_longlong(-1)
    L = amd.lib()
    if device is None:
        std = np.full(n_new, 7.0)
        rc = L.Nfft4GPAmdModelPredictStd(model.h, buf.ctypes.data, n_new, ldim, dd, std.ctypes.data, noise,
                                         C.byref(nout))
        return rc, std, nout.value
    bd = device.tensor(buf, device="cuda")
    sd = device.full((n_new,), 7.0, dtype=device.float64, device="cuda")
    rc = L.Nfft4GPAmdModelPredictStd(model.h, bd.data_ptr(), n_new, ldim, dd, sd.data_ptr(), noise, C.byref(nout))
    return rc, sd.cpu().numpy(), nout.value


def test_function_space_restatement(case):
    """Check 1: var = f^2 (mu + phi*^T W phi*) - k*^T A^{-1} k* with a dense solve of A = f^2 (Z W Z^T + mu I), Z and
    phi* from the model's quantised coordinates and W from the oracle's b^.  Bound: 64 2^-52 cond(mu I + W G)
    f^2 (1 + mu), LU's backward-error scale: 5.8e-10 .. 1.4e-7 over the cases (cond 2.4e4 .. 5.8e6); observed
    2.7e-15 .. 1.5e-14."""
    bound = 64.0 * 2.0 ** -52 * case["cond"] * F * F * (1.0 + MU)
    assert case["n_outside_full"] == 0 and np.all(np.isfinite(case["full"]))
    m = case["model"]
    for name, pts, want in (("new", case["Xnew"], case["var_new"]), ("train", case["X"], case["var_train"])):
        got = (case["full"] if name == "new" else m.predict_std(pts)) ** 2
        err = np.max(np.abs(got - want))
        print(f"{case['name']} ({name}): |var_model - var| {err:.2e}, bound {bound:.2e}, cond {case['cond']:.2e}, "
              f"var in [{want.min():.3e}, {want.max():.3e}]")
        assert err <= bound, (err, bound)


def test_against_the_operator(case):
    """Check 2: at 8 training points i, h = op.matsymv(e_i), k* = h - f^2 mu e_i, w = A^{-1} k* by the library's FGMRES
    on op to 1e-12 and var_i = h_i - k* . w.  Bound 2 (1 + |w|_1)^2 e_op, e_op the largest entry-wise distance of
    those 8 operator columns from the restatement's exact-feature columns."""
    torch, op, n = case["torch"], case["op"], case["n"]
    idx = np.linspace(0, n - 1, 8).astype(int)
    std = case["model"].predict_std(case["X"][idx])
    e_op, rows = 0.0, []
    for i in idx:
        e = torch.zeros(n, dtype=torch.float64, device="cuda")
        e[i] = 1.0
        h = op.matsymv(e)
        e_op = max(e_op, float(np.max(np.abs(h.cpu().numpy() - case["A"][:, i]))))
        ks = h - F * F * MU * e
        w = amd.fgmres(op, ks, kdim=min(n, 600), maxits=min(n, 600), tol=1e-12)[0]
        rows.append((float(h[i]) - float(ks @ w), float(w.abs().sum())))
    for j, (var, w1) in enumerate(rows):
        bound = 2.0 * (1.0 + w1) ** 2 * e_op
        err = abs(std[j] ** 2 - var)
        print(f"{case['name']} point {idx[j]}: |var_model - var_op| {err:.2e}, bound {bound:.2e} (e_op {e_op:.2e}, "
              f"|w|_1 {w1:.2e})")
        assert err <= bound, (err, bound)


def test_batching_and_reproducibility(case):
    """Check 4: batches of 1, 7 and 333 give the bits of the one call over all points; so do a second call, a larger
    leading dimension and device pointers; fitting twice gives the same S."""
    m, Xnew, full = case["model"], case["Xnew"], case["full"]
    assert np.array_equal(m.predict_std(Xnew), full)
    for k in (1, 7, 333):
        got = np.concatenate([m.predict_std(Xnew[i:i + k]) for i in range(0, NNEW, k)])
        assert np.array_equal(got, full), k
    rc, a, nout = raw_std(m, Xnew, NNEW + 3)
    assert rc == 0 and nout == 0 and np.array_equal(a, full)
    rc, b, nout = raw_std(m, Xnew, NNEW + 3, device=case["torch"])
    assert rc == 0 and nout == 0 and np.array_equal(b, full)
    t = m.predict_std(case["torch"].tensor(Xnew, device="cuda"))
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), full)
    S = case["co"]["S"]
    assert S.shape == (33 * case["nw"],) * 2 and np.array_equal(S, S.T)
    m.fit_variance(case["torch"].tensor(case["X"], device="cuda"))  # a device X this time
    assert np.array_equal(m.coefficients()["S"], S)
    assert np.array_equal(m.predict_std(Xnew), full)


def test_domain_and_conventions(case):
    """Check 5: outside points are NaN and counted and strict raises; n_new = 0; noise=False; the mean's bits are
    unchanged by the fit; a fit with an outside row fails and leaves S as it was."""
    m, nw, full = case["model"], case["nw"], case["full"]
    co = case["co"]
    X = case["Xnew"].copy()
    rows, cols = (10, 20, 30), (0, nw - 1, nw // 2)
    for r, c in zip(rows, cols):
        lo, hi = case["lo"][c], case["hi"][c]
        X[r, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    X[40, nw // 2] = np.nan
    got = m.predict_std(X, strict=False)
    assert m.n_outside == 4
    bad = np.zeros(NNEW, dtype=bool)
    bad[[10, 20, 30, 40]] = True
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], full[~bad])
    with pytest.raises(ValueError, match="4 of 1000"):
        m.predict_std(X)
    buf = np.asfortranarray(X)
    std = np.zeros(NNEW)
    assert amd.lib().Nfft4GPAmdModelPredictStd(m.h, buf.ctypes.data, NNEW, NNEW, nw, std.ctypes.data, 1, None) == 0
    assert np.array_equal(np.isnan(std), bad)
    nout = C.c_longlong(-1)
    assert amd.lib().Nfft4GPAmdModelPredictStd(m.h, None, 0, 0, nw, None, 1, C.byref(nout)) == 0 and nout.value == 0
    assert m.predict_std(np.zeros((0, nw))).shape == (0,)
    rc, _, _ = raw_std(m, case["Xnew"][:10, :max(nw - 1, 1)] if nw > 1 else np.zeros((10, 2)), 10)
    assert rc == -1
    quiet = m.predict_std(case["Xnew"], noise=False)
    assert np.max(np.abs(quiet - np.sqrt(np.abs(full ** 2 - F * F * MU)))) <= 1e-12
    assert np.array_equal(m.predict(case["Xnew"]), case["mean_before"])
    Xbad = case["X"].copy()
    Xbad[3, 0] = case["hi"][0] + (case["hi"][0] - case["lo"][0])
    with pytest.raises(ValueError, match="outside"):
        m.fit_variance(Xbad)
    assert amd.lib().Nfft4GPAmdModelFitVariance(m.h, np.asfortranarray(Xbad).ctypes.data, case["n"], case["n"],
                                                nw) == -2
    assert m.has_variance and np.array_equal(m.predict_std(case["Xnew"]), full)


def test_persistence(case, tmp_path):
    """Check 6: save -> load gives the same std bits; from_coefficients without S + fit_variance(X) equals the
    original; a model without variance saves and loads as before."""
    m, co, full = case["model"], case["co"], case["full"]
    path = os.path.join(tmp_path, "with_variance.npz")
    m.save(path)
    m2 = amd.FittedModel.load(path)
    assert m2.has_variance and np.array_equal(m2.predict_std(case["Xnew"]), full)
    assert np.array_equal(m2.predict(case["Xnew"]), case["mean_before"])
    m2.free()
    m3 = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                           co["hyper"])
    assert not m3.has_variance and "S" not in m3.coefficients()
    with pytest.raises(RuntimeError, match="fit_variance"):
        m3.predict_std(case["Xnew"])
    plain = os.path.join(tmp_path, "plain.npz")
    m3.save(plain)
    with np.load(plain) as z:
        assert sorted(z.files) == sorted(["H", "centre", "scale", "feature", "d", "kernel", "hyper"])
    m4 = amd.FittedModel.load(plain)
    assert not m4.has_variance and np.array_equal(m4.predict(case["Xnew"]), case["mean_before"])
    m4.free()
    m3.fit_variance(case["X"])
    assert np.array_equal(m3.coefficients()["S"], co["S"])
    assert np.array_equal(m3.predict_std(case["Xnew"]), full)
    m3.free()
    with pytest.raises(ValueError):
        amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                          co["hyper"], S=co["S"][:-1, :-1])


def test_reference_fixture(torch_cuda):
    """Check 3: the model over tests/golden/predict_synth.npz's X and hyperparameters (softplus), at the fixture's
    points inside the model's domain (39 of the 40), against the reference route's std.  The two routes scale
    differently -- the reference centres and scales a joint handle on [X; Xp], the model on X alone -- so they are
    two discretisations of the same kernel: 7.0e-4 relative was measured between them on the CPU from the
    reference-side quantities alone; the test allows twice that."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_synth.npz"))
    m = amd.gp_model(z["X"], z["windows"], 4, 1, z["y"], z["hyper"], tol=float(z["tol"]), maxits=int(z["maxits"]),
                     variance=True)
    assert m.has_variance
    std = m.predict_std(z["Xp"], strict=False)
    inside = ~np.isnan(std)
    assert inside.sum() == 39 and m.n_outside == 1
    err = np.max(np.abs(std[inside] - z["std"][inside]) / z["std"][inside])
    print(f"predict_synth: max relative distance from the reference's std {err:.2e}")
    np.testing.assert_allclose(std[inside], z["std"][inside], rtol=1.4e-3)
    m.free()


def test_32bit_mode_gives_the_same_variance(torch_cuda):
    """Check 7: the variance reads the model's centres, scales and hyperparameters, not H: the model of a 32-bit-mode
    operator holds the same S as its fp64 twin."""
    n, nw, kernel, l = CASES["nw5_gauss"]
    X, alpha, Xnew, _, _ = make_points(n, nw)
    S, std = [], []
    for bits in (64, 32):
        op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
        if bits == 32:
            op.set_precision(32)
        assert op.setup(kernel, F, l, MU) == 0
        m = amd.FittedModel.from_operator(op, alpha)
        m.fit_variance(X)
        S.append(m.coefficients()["S"])
        std.append(m.predict_std(Xnew))
        m.free()
        op.free()
    assert np.array_equal(S[0], S[1]) and np.array_equal(std[0], std[1])


def test_refusals(torch_cuda):
    """More than 128 windows: S would not be sensible to hold (170 MB at 128); bad arguments give -1."""
    nw = 129
    rng = np.random.default_rng(9)
    m = amd.FittedModel.from_coefficients(np.zeros((nw, 64, 8)), np.full(nw, 0.5), np.full(nw, 0.5),
                                          np.arange(nw, dtype=np.int32), nw, amd.GAUSSIAN, [F, 0.3, MU])
    with pytest.raises(RuntimeError):
        m.fit_variance(rng.random((50, nw)))
    assert not m.has_variance
    m.free()
    m = amd.FittedModel.from_coefficients(np.zeros((2, 64, 8)), np.full(2, 0.5), np.full(2, 0.5),
                                          np.arange(2, dtype=np.int32), 2, amd.GAUSSIAN, [F, 0.3, MU])
    X = np.asfortranarray(rng.random((50, 2)))
    L = amd.lib()
    assert L.Nfft4GPAmdModelFitVariance(m.h, X.ctypes.data, 50, 49, 2) == -1
    assert L.Nfft4GPAmdModelFitVariance(m.h, X.ctypes.data, 50, 50, 3) == -1
    assert L.Nfft4GPAmdModelFitVariance(m.h, None, 50, 50, 2) == -1
    assert L.Nfft4GPAmdModelSetVariance(m.h, X.ctypes.data, 65) == -1
    R = C.c_int(-1)
    assert L.Nfft4GPAmdModelVarianceInfo(m.h, C.byref(R)) == 0 and R.value == 0
    assert L.Nfft4GPAmdModelVariance(m.h, X.ctypes.data) == -3
    assert L.Nfft4GPAmdModelFitVariance(m.h, X.ctypes.data, 50, 50, 2) == 0
    assert L.Nfft4GPAmdModelVarianceInfo(m.h, C.byref(R)) == 0 and R.value == 66
    m.free()

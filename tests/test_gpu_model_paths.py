"""The fitted model's joint posterior sample paths (Nfft4GPAmdModelFitSampler / DrawPaths / EvalPaths, csrc/model_paths.hip
k_model_paths; FittedModel.fit_sampler / draw_paths / paths / sample / path_curve):
paths[i, s] = predict[i] + f sum_j phi_j(x_i) B[j, s], B = F xi, F F^T = S without its negative part.

Cases as in test_gpu_model_variance.py (its points and features are imported): n = 1500, f = 1.3, mu = 0.01 with nw = 1
(R = 33, less than one k step's tile, S indefinite), 5 (Gaussian and Matern-1/2; windows no multiple of 4), 33 (several
column groups) and n = 400 with 64 windows (n < R); 1000 new points (no multiple of a workgroup's 128).  With T the
kernel's sample tile the path counts are 1, T - 1, T + 1 and 2 T + 3.  One model per case is shared by the checks; every
check draws the paths it needs."""
import ctypes as C
import warnings

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd.model import PATHS_TILE as T
from test_gpu_model_variance import F, MU, NNEW, features, make_points, oracle_weights

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
CASES = {  # n, nw, kernel, l
    "nw1_gauss": (1500, 1, amd.GAUSSIAN, 0.3),
    "nw5_gauss": (1500, 5, amd.GAUSSIAN, 0.1),
    "nw5_matern": (1500, 5, amd.MATERN12, 0.3),
    "nw33_gauss": (1500, 33, amd.GAUSSIAN, 0.1),
    "n400_nw64_gauss": (400, 64, amd.GAUSSIAN, 0.1),
}
INDEFINITE = ("nw1_gauss",)
COUNTS = (1, T - 1, T + 1, 2 * T + 3)
SERVED = {"nw1_gauss": (0,), "nw5_gauss": (0, 1, 2, 3, 4), "nw5_matern": (0, 1, 2, 3, 4), "nw33_gauss": (0, 16, 32),
          "n400_nw64_gauss": tuple(range(64))}  # the effects tests' windows, and all 64 of the 64-window case
_built = {}


def quiet_fit(model):
    """fit_sampler with its warnings recorded, not shown"""
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        model.fit_sampler()
    return [w for w in rec if issubclass(w.category, RuntimeWarning)]


def build_case(name, torch):
    """one model per case; what the checks share is computed once and left unchanged"""
    if name in _built:
        return _built[name]
    n, nw, kernel, l = CASES[name]
    R = 33 * nw
    X, alpha, Xnew, lo, hi = make_points(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, MU) == 0
    model = amd.FittedModel.from_operator(op, torch.tensor(alpha, device="cuda"))
    model.fit_variance(X)
    co = model.coefficients()
    before = dict(mean=model.predict(Xnew), std=model.predict_std(Xnew), eff=model.predict_effects(Xnew),
                  S=co["S"].copy())  # before any of the new calls
    assert model.n_paths == 0 and model.sampler_defect is None
    warned = quiet_fit(model)
    lam, V = np.linalg.eigh(co["S"])
    Splus = (V * np.maximum(lam, 0.0)) @ V.T
    Fm = sampler_factor(model, R)
    rng = np.random.default_rng(77 + nw)
    xi = rng.standard_normal((R, COUNTS[-1]))
    _built[name] = dict(name=name, n=n, nw=nw, R=R, kernel=kernel, l=l, X=X, Xnew=Xnew, lo=lo, hi=hi, op=op, model=model,
                        co=co, before=before, warned=warned, lam=lam, Splus=Splus, Fm=Fm, xi=xi,
                        Phi=features(co, Xnew), quiet=model.predict_std(Xnew, noise=False), torch=torch)
    return _built[name]


@pytest.fixture(scope="module", autouse=True)
def _free_models():
    yield
    for c in _built.values():
        c["model"].free()
        c["op"].free()
    _built.clear()


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request, torch_cuda):
    return build_case(request.param, torch_cuda)


def sampler_factor(model, R):
    Fm = np.empty((R, R))
    assert amd.lib().Nfft4GPAmdModelSamplerFactor(model.h, Fm.ctypes.data) == 0
    return Fm


def path_weights(model, R):
    B = np.empty((R, model.n_paths), order="F")
    assert amd.lib().Nfft4GPAmdModelPathWeights(model.h, B.ctypes.data) == 0
    return B


def raw_paths(model, X, ldim, ldo, window=-1, device=None, d=None, n_new=None, ns=None):
    """Nfft4GPAmdModelEvalPaths on column-major buffers of leading dimensions ldim and ldo, the output filled with 7
    beforehand; (status, out ldo x ns in Fortran order, n_outside)"""
    rows, dd = X.shape
    n_new = rows if n_new is None else n_new
    ns = model.n_paths if ns is None else ns
    buf = np.zeros((dd, max(ldim, rows)))
    buf[:, :rows] = X.T
    shape = (max(ns, 1), max(ldo, 1))
    nout = C.c_longlong(-1)
    L = amd.lib()
    if device is None:
        o = np.full(shape, 7.0)
        rc = L.Nfft4GPAmdModelEvalPaths(model.h, buf.ctypes.data, n_new, ldim, dd if d is None else d, window,
                                        o.ctypes.data, ldo, C.byref(nout))
        return rc, o.T, nout.value
    bd = device.tensor(buf, device="cuda")
    o = device.full(shape, 7.0, dtype=device.float64, device="cuda")
    rc = L.Nfft4GPAmdModelEvalPaths(model.h, bd.data_ptr(), n_new, ldim, dd if d is None else d, window, o.data_ptr(),
                                    ldo, C.byref(nout))
    return rc, o.cpu().numpy().T, nout.value


def test_factor(case):
    """Check 1: max |F F^T - S+| <= 4 R eps lambda_max with S+ = V max(Lambda, 0) V^T from numpy's eigh of the model's S
    (numpy's own reconstruction sits at 0.005 .. 0.16 of R eps lambda_max on these cases; the 4 allows for another
    algorithm in rocSOLVER).  The defect is 0 exactly, without a warning and with lambda_min > 0, in the four positive
    definite cases; in nw1_gauss it is numpy's sum |lambda < 0| / sum |lambda| to 1e-8 relative, with the
    RuntimeWarning.  Two fits give the same F to the bit.
    Observed on an MI355X, max |F F^T - S+| / (R eps lambda_max): nw1 0.097, nw5 Gaussian 0.038, nw5 Matern 0.109,
    nw33 0.050, n400 nw64 0.152 (rocSOLVER's dsyevd; numpy's own range); nw1's defect 0.1205484."""
    m, R, lam = case["model"], case["R"], case["lam"]
    Fm = case["Fm"]
    err = np.max(np.abs(Fm @ Fm.T - case["Splus"]))
    scale = R * EPS * lam[-1]
    print(f"{case['name']}: max |F F^T - S+| = {err:.3e} = {err / scale:.4f} R eps lambda_max; defect "
          f"{m.sampler_defect:.6e}, lambda in [{m.sampler_eigen_range[0]:.3e}, {m.sampler_eigen_range[1]:.3e}]")
    assert err <= 4.0 * scale, err / scale
    want = np.abs(lam[lam < 0]).sum() / np.abs(lam).sum()
    if case["name"] in INDEFINITE:
        assert abs(m.sampler_defect - want) <= 1e-8 * want, (m.sampler_defect, want)
        assert len(case["warned"]) == 1 and "predict_std" in str(case["warned"][0].message)
        assert f"{m.sampler_defect:.3e}" in str(case["warned"][0].message)
        assert m.sampler_eigen_range[0] < 0.0
        again = quiet_fit(m)
        assert len(again) == 1
    else:
        assert m.sampler_defect == 0.0 and not case["warned"] and m.sampler_eigen_range[0] > 0.0
        assert not quiet_fit(m)
    assert np.array_equal(sampler_factor(m, R), Fm)
    info = (C.c_double * 3)()
    assert amd.lib().Nfft4GPAmdModelFitSampler(m.h, info) == 0
    assert info[0] == m.sampler_defect and (info[1], info[2]) == m.sampler_eigen_range
    ms = C.c_double(-1.0)
    assert amd.lib().Nfft4GPAmdModelSamplerFitTime(m.h, C.byref(ms)) == 0 and ms.value > 0.0


def test_weights(case):
    """Check 2: |B - F xi| <= 2 g (|F| |xi|) entrywise, g = R eps (the dot-product bound, doubled for numpy's own error);
    sample(seed=s) is draw_paths(xi=default_rng(s).standard_normal((R, ns))) followed by paths, to the bit."""
    m, R, Fm, Xnew = case["model"], case["R"], case["Fm"], case["Xnew"]
    for ns in COUNTS:
        xi = case["xi"][:, :ns]
        assert m.draw_paths(ns, xi=xi) is m and m.n_paths == ns
        B = path_weights(m, R)
        err = np.abs(B - Fm @ xi)
        bound = 2.0 * R * EPS * (np.abs(Fm) @ np.abs(xi))
        print(f"{case['name']} ns = {ns}: max |B - F xi| / bound = {np.max(err / bound):.4f}")
        assert np.all(err <= bound), float(np.max(err / bound))
    ns = T + 1
    a = m.sample(Xnew, ns, seed=31)
    assert a.shape == (NNEW, ns) and a.flags.f_contiguous and m.n_paths == ns
    b = m.draw_paths(ns, xi=np.random.default_rng(31).standard_normal((R, ns))).paths(Xnew)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, m.sample(Xnew, ns, seed=32))


def test_paths_against_the_restatement(case):
    """Check 3: with the library's own B and numpy's features of the model's quantised coordinates,
    |paths - predict - f Phi B| <= 2 g f (|Phi| |B|) + 4 eps |paths|, g = (R + 64) eps (the 64 covers the 16 rotations
    behind each feature), for every (point, path) and all four path counts."""
    m, R, Xnew, Phi = case["model"], case["R"], case["Xnew"], case["Phi"]
    mean = case["before"]["mean"]
    for ns in COUNTS:
        m.draw_paths(ns, xi=case["xi"][:, :ns])
        B = path_weights(m, R)
        got = m.paths(Xnew)
        assert got.shape == (NNEW, ns) and m.n_outside == 0 and np.all(np.isfinite(got))
        err = np.abs(got - mean[:, None] - F * (Phi @ B))
        bound = 2.0 * (R + 64) * EPS * F * (np.abs(Phi) @ np.abs(B)) + 4.0 * EPS * np.abs(got)
        print(f"{case['name']} ns = {ns}: max |paths - predict - f Phi B| / bound = {np.max(err / bound):.4f}")
        assert np.all(err <= bound), float(np.max(err / bound))


def test_mean_and_window_consistency(case):
    """Check 4: with xi = 0 every path is predict to the bit, and with window=c predict_effects(window=c) to the bit;
    with a random xi the windows' paths sum to paths() within nw eps sum_c |term_c| per entry."""
    m, nw, R, Xnew = case["model"], case["nw"], case["R"], case["Xnew"]
    ns = T + 1
    m.draw_paths(ns, xi=np.zeros((R, ns)))
    got = m.paths(Xnew)
    assert np.array_equal(got, np.repeat(case["before"]["mean"][:, None], ns, axis=1))
    for c in SERVED[case["name"]]:
        got = m.paths(Xnew, window=c)
        assert np.array_equal(got, np.repeat(case["before"]["eff"][:, c][:, None], ns, axis=1)), c
    m.draw_paths(ns, xi=case["xi"][:, :ns])
    total = m.paths(Xnew)
    terms = [m.paths(Xnew, window=c) for c in range(nw)]
    err = np.abs(sum(terms) - total)
    bound = nw * EPS * sum(np.abs(t) for t in terms)
    print(f"{case['name']}: max |sum_c paths(window=c) - paths()| / bound = {np.max(err / bound):.4f}")
    assert np.all(err <= bound), float(np.max(err / bound))
    feature = case["co"]["feature"]
    for c in sorted({0, nw - 1}):
        assert np.array_equal(m.path_curve(c, Xnew[:, feature[c]]), terms[c])
        t1 = m.path_curve(c, case["torch"].tensor(Xnew[:, feature[c]], device="cuda"))
        assert t1.is_cuda and np.array_equal(t1.cpu().numpy(), terms[c])


@pytest.mark.parametrize("name", ["nw1_gauss", "nw5_gauss", "nw5_matern", "nw33_gauss"])
def test_covariance_identity(name, torch_cuda):
    """Check 5: with xi = I (ns = R: several sample tiles) D = (paths - predict) / f has sum_s D^2 = phi^T F F^T phi.
    Positive definite cases: against (predict_std(noise=False) / f)^2.  nw1_gauss: against numpy's phi^T S+ phi, and
    it differs from predict_std^2 by more than the tolerance somewhere: the negative part the sampler drops."""
    case = build_case(name, torch_cuda)
    m, R, Xnew, Phi, lam = case["model"], case["R"], case["Xnew"], case["Phi"], case["lam"]
    m.draw_paths(R, xi=np.eye(R))
    got = m.paths(Xnew)
    D = (got - case["before"]["mean"][:, None]) / F
    q = (D * D).sum(axis=1)
    # The tolerance, per point.  (a) the factor: |phi^T (F F^T - S+) phi| <= |phi|_1^2 max |F F^T - S+|, the entrywise
    # bound of check 1, 4 R eps lambda_max.  (b) the evaluation: check 3 bounds each D_s's error by e_s = 2 g (|Phi||B|)_s
    # + 4 eps |paths_s| / f, so sum_s D_s^2 moves by at most sum_s (2 |D_s| e_s + e_s^2).  (c) positive definite cases
    # only: predict_std's own published tolerance on the variance (test_gpu_model_variance.py check 1), 64 eps
    # cond(mu I + W G) f^2 (1 + mu), here over f^2.
    B = path_weights(m, R)
    e = 2.0 * (R + 64) * EPS * (np.abs(Phi) @ np.abs(B)) + 4.0 * EPS * np.abs(got) / F
    tol = np.abs(Phi).sum(axis=1) ** 2 * 4.0 * R * EPS * lam[-1] + (2.0 * np.abs(D) * e + e * e).sum(axis=1)
    served = (case["quiet"] / F) ** 2
    if name in INDEFINITE:
        want = np.einsum("ij,jk,ik->i", Phi, case["Splus"], Phi)
        err = np.abs(q - want)
        print(f"{name}: max |sum D^2 - phi^T S+ phi| / tol = {np.max(err / tol):.4f}; max |sum D^2 - (std/f)^2| / tol = "
              f"{np.max(np.abs(q - served) / tol):.3e}")
        assert np.all(err <= tol), float(np.max(err / tol))
        assert np.any(np.abs(q - served) > tol)
    else:
        w = oracle_weights(case["X"], case["nw"], case["kernel"], case["l"])
        Z = features(case["co"], case["X"])
        cond = np.linalg.cond(MU * np.eye(R) + w[:, None] * (Z.T @ Z))
        tol = tol + 64.0 * EPS * cond * (1.0 + MU)
        err = np.abs(q - served)
        print(f"{name}: max |sum D^2 - (predict_std / f)^2| / tol = {np.max(err / tol):.3e} (max err {err.max():.2e})")
        assert np.all(err <= tol), float(np.max(err / tol))


def test_batch_independence_and_plumbing(case):
    """Check 6, bit for bit: rows in reversed order, the first row, the first 129 rows; numpy and device input; raw
    calls with ldim and ldo above n_new, which leave the padding at its fill value; and the same path evaluated alone
    or as column 0 or column T + 1 of a larger draw."""
    m, R, Xnew, torch = case["model"], case["R"], case["Xnew"], case["torch"]
    ns = T + 3
    xi = case["xi"][:, :ns]
    m.draw_paths(ns, xi=xi)
    full = m.paths(Xnew)
    assert np.array_equal(m.paths(Xnew), full)
    assert np.array_equal(m.paths(Xnew[::-1])[::-1], full)
    assert np.array_equal(m.paths(Xnew[:1]), full[:1])
    assert np.array_equal(m.paths(Xnew[:129]), full[:129])
    t = m.paths(torch.tensor(Xnew, device="cuda"))
    assert t.is_cuda and t.shape == (NNEW, ns) and t.t().is_contiguous() and np.array_equal(t.cpu().numpy(), full)
    for device in (None, torch):
        rc, o, nout = raw_paths(m, Xnew, NNEW + 3, NNEW + 5, device=device)
        assert rc == 0 and nout == 0 and np.array_equal(o[:NNEW], full) and np.all(o[NNEW:] == 7.0)
    assert m.paths(np.zeros((0, case["nw"]))).shape == (0, ns)
    xd = torch.tensor(np.asfortranarray(xi).T.copy(), device="cuda").t()  # a device xi
    assert np.array_equal(m.draw_paths(ns, xi=xd).paths(Xnew), full)
    for col in (0, T + 1):
        alone = m.draw_paths(1, xi=xi[:, col:col + 1]).paths(Xnew)
        assert np.array_equal(alone[:, 0], full[:, col]), col
    c = case["nw"] - 1
    m.draw_paths(ns, xi=xi)
    term = m.paths(Xnew, window=c)
    assert np.array_equal(m.draw_paths(1, xi=xi[:, T + 1:T + 2]).paths(Xnew, window=c)[:, 0], term[:, T + 1])


def test_host_output_in_chunks(torch_cuda):
    """Check 6, continued (nw = 1): a host output larger than the library's 64 MB staging buffer is produced in chunks
    of points; 33000 points x 259 paths (68 MB, two chunks, the second partial and no multiple of 128) give the bits of
    the device route, which is one launch, with the outside points NaN and counted across the chunks."""
    case = build_case("nw1_gauss", torch_cuda)
    m, torch = case["model"], torch_cuda
    ns, n_new = COUNTS[-1], 33000
    chunk = (8 << 20) // ns // 128 * 128
    assert chunk < n_new < 2 * chunk and (n_new - chunk) % 128
    X = np.resize(case["Xnew"][:, 0], n_new)[:, None].copy()
    X[[5, chunk + 7], 0] = case["hi"][0] + 0.01 * (case["hi"][0] - case["lo"][0]) + 1.0
    m.draw_paths(ns, xi=case["xi"][:, :ns])
    dev = m.paths(torch.tensor(X, device="cuda"), strict=False)
    assert m.n_outside == 2
    host = m.paths(X, strict=False)
    assert m.n_outside == 2 and host.shape == (n_new, ns)
    assert np.array_equal(host, dev.cpu().numpy(), equal_nan=True)
    assert np.array_equal(np.isnan(host).all(axis=1), np.isin(np.arange(n_new), [5, chunk + 7]))
    assert np.array_equal(host[:NNEW][6:], m.paths(case["Xnew"])[6:])


def test_outside_points(case):
    """Check 7: two rows just beyond a window's radius are NaN in every path of paths() and of paths(window=that one),
    finite in paths(window=another); n_outside is 2 and strict raises; every other row keeps its bits."""
    m, nw, co, Xnew = case["model"], case["nw"], case["co"], case["Xnew"]
    ns = T + 1
    m.draw_paths(ns, xi=case["xi"][:, :ns])
    full = m.paths(Xnew)
    c = nw // 2
    lo, hi = case["lo"][c], case["hi"][c]
    X = Xnew.copy()
    X[10, c] = X[500, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    bad = np.zeros(NNEW, dtype=bool)
    bad[[10, 500]] = True
    got = m.paths(X, strict=False)
    assert m.n_outside == 2
    assert np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], full[~bad])
    with pytest.raises(ValueError, match="2 of 1000"):
        m.paths(X)
    term = m.paths(Xnew, window=c)
    got = m.paths(X, window=c, strict=False)
    assert m.n_outside == 2 and np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], term[~bad])
    with pytest.raises(ValueError, match="2 of 1000"):
        m.paths(X, window=c)
    if nw > 1:
        other = (c + 1) % nw
        got = m.paths(X, window=other)  # strict: the same points are inside
        assert m.n_outside == 0 and np.all(np.isfinite(got)) and np.array_equal(got, m.paths(Xnew, window=other))
    rc, o, nout = raw_paths(m, X, NNEW, NNEW)
    assert rc == 0 and nout == 2 and np.array_equal(np.isnan(o).all(axis=1), bad)
    assert np.array_equal(np.isnan(o).any(axis=1), bad)


def test_state(case):
    """Check 8: no paths -> RuntimeError and -4 with nothing written; no variance -> the fit_variance message and -3;
    fit_variance again drops the factor and the paths; predict, predict_std, predict_effects and S keep their bits; a
    model rebuilt by from_coefficients(..., S=S) draws the same paths for the same xi, to the bit."""
    m, nw, R, Xnew, co, b = case["model"], case["nw"], case["R"], case["Xnew"], case["co"], case["before"]
    L = amd.lib()
    ns = 3
    xi = case["xi"][:, :ns]
    full = m.draw_paths(ns, xi=xi).paths(Xnew)
    # refused calls leave the paths in place and write nothing
    assert L.Nfft4GPAmdModelDrawPaths(m.h, np.asfortranarray(xi).ctypes.data, 0, R) == -1
    assert L.Nfft4GPAmdModelDrawPaths(m.h, np.asfortranarray(xi).ctypes.data, ns, R - 1) == -1
    assert m.n_paths == ns and np.array_equal(m.paths(Xnew), full)
    X10 = Xnew[:10]
    for why, kw in dict(d=dict(d=nw + 1), ldim=dict(ldim=9), ldo=dict(ldo=9), window_low=dict(window=-2),
                        window_high=dict(window=nw)).items():
        a = dict(ldim=10, ldo=10, window=-1, d=None)
        a.update(kw)
        rc, o, nout = raw_paths(m, X10, a["ldim"], a["ldo"], window=a["window"], d=a["d"], n_new=10)
        assert rc == -1 and nout == -1 and np.all(o == 7.0), why
    with pytest.raises(ValueError):
        m.paths(Xnew, window=nw)
    # a model without a variance, then with one and nothing drawn
    m2 = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                           co["hyper"])
    with pytest.raises(RuntimeError, match="draw_paths"):
        m2.paths(Xnew)
    rc, o, nout = raw_paths(m2, X10, 10, 10, ns=2)
    assert rc == -4 and nout == -1 and np.all(o == 7.0)
    with pytest.raises(RuntimeError, match="fit_variance"):
        m2.draw_paths(2, seed=0)
    with pytest.raises(RuntimeError, match="fit_variance"):
        m2.fit_sampler()
    xf = np.asfortranarray(xi)
    assert L.Nfft4GPAmdModelFitSampler(m2.h, None) == -3
    assert L.Nfft4GPAmdModelDrawPaths(m2.h, xf.ctypes.data, ns, R) == -3
    Fbuf = np.full((R, R), 7.0)
    assert L.Nfft4GPAmdModelSamplerFactor(m2.h, Fbuf.ctypes.data) == -3 and np.all(Fbuf == 7.0)
    m2.free()
    m3 = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                           co["hyper"], S=co["S"])
    assert L.Nfft4GPAmdModelDrawPaths(m3.h, xf.ctypes.data, ns, R) == -4
    assert L.Nfft4GPAmdModelSamplerFactor(m3.h, Fbuf.ctypes.data) == -4 and np.all(Fbuf == 7.0)
    Bbuf = np.full((R, ns), 7.0, order="F")
    assert L.Nfft4GPAmdModelPathWeights(m3.h, Bbuf.ctypes.data) == -4 and np.all(Bbuf == 7.0)
    rc, o, nout = raw_paths(m3, X10, 10, 10, ns=2)
    assert rc == -4 and nout == -1 and np.all(o == 7.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        assert np.array_equal(m3.draw_paths(ns, xi=xi).paths(Xnew), full)  # fits on first use
    assert m3.sampler_defect == m.sampler_defect and np.array_equal(sampler_factor(m3, R), case["Fm"])
    m3.free()
    # a new S drops the factor and the paths
    m.fit_variance(case["X"])
    assert m.n_paths == 0 and m.sampler_defect is None
    assert L.Nfft4GPAmdModelSamplerFactor(m.h, Fbuf.ctypes.data) == -4
    with pytest.raises(RuntimeError, match="draw_paths"):
        m.paths(Xnew)
    assert np.array_equal(m.predict(Xnew), b["mean"]) and np.array_equal(m.predict_std(Xnew), b["std"])
    assert np.array_equal(m.predict_effects(Xnew), b["eff"]) and np.array_equal(m.coefficients()["S"], b["S"])
    quiet_fit(m)  # the shared model as the other checks expect it
    assert np.array_equal(sampler_factor(m, R), case["Fm"])
    assert np.array_equal(m.draw_paths(ns, xi=xi).paths(Xnew), full)

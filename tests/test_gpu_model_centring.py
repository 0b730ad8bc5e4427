"""The fitted model's centring on a reference sample (Nfft4GPAmdModelFitCentring / Centring / SetCentring /
PredictEffectsCentred / Intercept, csrc/model_centring.hip and k_model_effects<., true>; FittedModel.fit_centring,
predict_effects(centred=True), intercept, importance).

Cases as in test_gpu_model_effects.py (the points, features and weights of test_gpu_model_variance.py are imported):
n = 1500, f = 1.3, mu = 0.01 with nw = 1, 5 (Gaussian and Matern-1/2; the std kernel's groups of 2 windows end in a
group of 1) and 33 (a partial group for the 8-window mean passes), and n = 400 with 64 windows (n < R); 1000 new
points, rows 0 and 1 the per-feature minimum and maximum.  The reductions also at n = 2 and n = 1025, one point past a
1024-point workgroup."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
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
_built = {}


def raw_centred(model, X, ldim, ldo, w0, wn, std=True, mean=True, device=None, d=None, centred=True):
    """Nfft4GPAmdModelPredictEffectsCentred (or the uncentred call) on column-major buffers of leading dimensions ldim
    and ldo, outputs filled with 7 beforehand; (status, effects ldo x wn, effect_std ldo x wn, n_outside)"""
    rows, dd = X.shape
    buf = np.zeros((dd, max(ldim, rows)))
    buf[:, :rows] = X.T
    shape = (max(wn, 1), max(ldo, 1))
    nout = C.c_longlong(-1)
    L = amd.lib()
    fn = L.Nfft4GPAmdModelPredictEffectsCentred if centred else L.Nfft4GPAmdModelPredictEffects
    if device is None:
        e, s = np.full(shape, 7.0), np.full(shape, 7.0)
        rc = fn(model.h, buf.ctypes.data, rows, ldim, dd if d is None else d, w0, wn, e.ctypes.data if mean else None,
                s.ctypes.data if std else None, ldo, C.byref(nout))
        return rc, e.T, s.T, nout.value
    bd = device.tensor(buf, device="cuda")
    e = device.full(shape, 7.0, dtype=device.float64, device="cuda")
    s = device.full(shape, 7.0, dtype=device.float64, device="cuda")
    rc = fn(model.h, bd.data_ptr(), rows, ldim, dd if d is None else d, w0, wn, e.data_ptr() if mean else None,
            s.data_ptr() if std else None, ldo, C.byref(nout))
    return rc, e.cpu().numpy().T, s.cpu().numpy().T, nout.value


def raw_intercept(model, std=True):
    b, sb = C.c_double(7.0), C.c_double(7.0)
    rc = amd.lib().Nfft4GPAmdModelIntercept(model.h, C.byref(b), C.byref(sb) if std else None)
    return rc, b.value, sb.value


def held(model):
    """the centring's three arrays, copies"""
    return model.feature_mean.copy(), model.effect_mean.copy(), model.importance.copy()


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b))


def build_case(name, torch):
    """one model per case, with everything the checks share computed once"""
    if name in _built:
        return _built[name]
    n, nw, kernel, l = CASES[name]
    X, alpha, Xnew, lo, hi = make_points(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, MU) == 0
    model = amd.FittedModel.from_operator(op, torch.tensor(alpha, device="cuda"))
    # check 11, first half: nothing centred is served before the fit, and nothing is written
    assert not model.has_centring and "effect_mean" not in model.coefficients()
    rc, e, s, nout = raw_centred(model, Xnew, NNEW, NNEW, 0, nw, std=False)
    assert rc == -5 and np.all(e == 7.0) and np.all(s == 7.0) and nout == -1
    assert raw_intercept(model) == (-5, 7.0, 7.0) and raw_intercept(model, std=False) == (-5, 7.0, 7.0)
    for call in (lambda: model.predict_effects(Xnew, centred=True), lambda: model.effect_curve(0, Xnew[:, 0], centred=True),
                 model.intercept, lambda: model.effect_mean, lambda: model.importance, lambda: model.feature_mean):
        with pytest.raises(RuntimeError, match="fit_centring"):
            call()
    # check 7, last part and check 11: a centring without a variance serves the means and refuses the stds
    assert model.fit_centring(X) is model and model.has_centring and not model.has_variance
    first = held(model)
    eff_plain_centred = model.predict_effects(Xnew, centred=True)
    assert model.intercept() == raw_intercept(model, std=False)[1]
    with pytest.raises(RuntimeError, match="fit_variance"):
        model.intercept(std=True)
    with pytest.raises(RuntimeError, match="fit_variance"):
        model.predict_effects(Xnew, std=True, centred=True)
    rc, e, s, nout = raw_centred(model, Xnew, NNEW, NNEW, 0, nw, std=True)
    assert rc == -3 and np.all(e == 7.0) and np.all(s == 7.0) and nout == -1
    assert raw_intercept(model) == (-3, 7.0, 7.0)
    # check 10: a model with the same table, a variance and no centring, its bits recorded, then centred
    co = model.coefficients()
    model.free()
    model = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                              co["hyper"])
    assert not model.has_centring
    model.fit_variance(X)
    before = dict(mean=model.predict(Xnew), std=model.predict_std(Xnew), S=model.coefficients()["S"].copy())
    eff, sd = model.predict_effects(Xnew, std=True)
    eff_train, sd_train = model.predict_effects(X, std=True)
    model.fit_centring(X)
    assert same(held(model), first)  # the centring does not depend on S
    co = model.coefficients()
    ceff, csd = model.predict_effects(Xnew, std=True, centred=True)
    n_outside_full = model.n_outside
    ceff_train, csd_train = model.predict_effects(X, std=True, centred=True)
    # the restatement per window with the dense A = f^2 (Z W Z^T + mu I) of the variance tests, A^{-1} Z solved once:
    # var~_c = f^2 phi~^T W_c phi~ - k~^T A^{-1} k~, phi~ = phi_c - m_c, k~ = f^2 Z_c W_c phi~, m numpy's own means
    Z, P = features(co, X), features(co, Xnew)
    m_ref = Z.mean(axis=0)
    w = oracle_weights(X, nw, kernel, l)
    A = F * F * ((Z * w) @ Z.T + MU * np.eye(n))
    cond = np.linalg.cond(MU * np.eye(33 * nw) + w[:, None] * (Z.T @ Z))
    ZtAiZ = Z.T @ np.linalg.solve(A, Z)

    def var_restated(Phi):
        out = np.empty((Phi.shape[0], nw))
        for c in range(nw):
            sl = slice(33 * c, 33 * c + 33)
            Kw = Phi[:, sl] * w[sl]
            out[:, c] = F * F * np.einsum("ij,ij->i", Kw, Phi[:, sl]) - F ** 4 * np.einsum(
                "ij,jk,ik->i", Kw, ZtAiZ[sl, sl], Kw)
        return out

    mw = m_ref * w
    var_b = F * F * (mw @ m_ref) - F ** 4 * (mw @ ZtAiZ @ mw)
    _built[name] = dict(name=name, n=n, nw=nw, kernel=kernel, l=l, X=X, alpha=alpha, Xnew=Xnew, lo=lo, hi=hi, op=op,
                        model=model, co=co, cond=cond, Z=Z, m_ref=m_ref, var_new=var_restated(P - m_ref),
                        var_train=var_restated(Z - m_ref), var_b=var_b, eff=eff, sd=sd, eff_train=eff_train,
                        sd_train=sd_train, ceff=ceff, csd=csd, ceff_train=ceff_train, csd_train=csd_train,
                        eff_plain_centred=eff_plain_centred, before=before, n_outside_full=n_outside_full,
                        first=first, torch=torch)
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


def check_feature_means(name, fm, Z):
    """check 1 on the n rows whose features are Z"""
    nw = Z.shape[1] // 33
    err = np.max(np.abs(fm - Z.mean(axis=0)))
    print(f"{name}: max |feature_mean - numpy| {err:.2e}, bound {64.0 * EPS:.2e}")
    assert fm.shape == (33 * nw,) and err <= 64.0 * EPS
    assert np.all(fm[::33] == 1.0)


def check_effect_moments(name, em, imp, e):
    """check 2 on the n x nw uncentred effects e of the reference sample; prints the largest observed / bound"""
    n, nw = e.shape
    worst_mean = worst_var = 0.0
    for c in range(nw):
        col = e[:, c]
        mean = math.fsum(col) / n
        delta = (n + 2) * EPS * (math.fsum(np.abs(col)) / n)
        ref = math.fsum((col - mean) ** 2) / n
        bound = (n + 8) * EPS * ref + delta ** 2
        worst_mean = max(worst_mean, abs(em[c] - mean) / delta)
        worst_var = max(worst_var, abs(imp[c] ** 2 - ref) / bound)
        assert abs(em[c] - mean) <= delta, (c, em[c], mean, delta)
        assert abs(imp[c] ** 2 - ref) <= bound, (c, imp[c] ** 2, ref, bound)
    print(f"{name}: effect_mean error / bound {worst_mean:.3f}, importance^2 error / bound {worst_var:.3f}")


def test_feature_means(case):
    """Check 1: feature_mean against numpy's features(co, X).mean(0) within 64 2^-52 per entry (the features are
    bounded by 1 and their rotation error is <= 16 steps); the constant slot of every window is exactly 1."""
    check_feature_means(case["name"], case["model"].feature_mean, case["Z"])
    assert case["co"]["n_ref"] == case["n"]


def test_effect_means_and_importances(case):
    """Check 2: with e = predict_effects(X), |e_c - fsum(e[:, c]) / n| <= d_c = (n + 2) 2^-52 mean|e[:, c]| and
    |imp_c^2 - ref_c| <= (n + 8) 2^-52 ref_c + d_c^2, ref_c = fsum((e[:, c] - fsum-mean)^2) / n (the first-order term
    in the mean's error vanishes: the deviations sum to zero)."""
    m = case["model"]
    assert m.effect_mean.shape == (case["nw"],) and m.importance.shape == (case["nw"],)
    check_effect_moments(case["name"], m.effect_mean, m.importance, case["eff_train"])


@pytest.mark.parametrize("n", [2, 1025])
def test_reductions_at_the_edges(n, torch_cuda):
    """Checks 1, 2 and 9 at n = 2 (one wave's two lanes) and n = 1025 (one point past a 1024-point workgroup: two
    workgroups' partial sums), on the rows of the 5-window Gaussian case; host and device pointers give the same
    bits."""
    case = build_case("nw5_gauss", torch_cuda)
    co, X = case["co"], case["X"][:n]
    m = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                          co["hyper"])
    a = held(m.fit_centring(X))
    assert m.coefficients()["n_ref"] == n
    check_feature_means(f"n {n}", a[0], features(co, X))
    check_effect_moments(f"n {n}", a[1], a[2], m.predict_effects(X))
    assert same(held(m.fit_centring(X)), a)
    assert same(held(m.fit_centring(torch_cuda.tensor(X, device="cuda"))), a)
    m.free()


def test_centred_effects_are_the_effects_minus_their_means(case):
    """Check 3: predict_effects(P, centred=True) == predict_effects(P) - effect_mean, bit for bit, at the new points
    and at the training points."""
    em = case["model"].effect_mean
    assert case["n_outside_full"] == 0
    assert case["ceff"].shape == (NNEW, case["nw"]) and case["ceff"].flags.f_contiguous
    assert np.array_equal(case["ceff"], case["eff"] - em)
    assert np.array_equal(case["ceff_train"], case["eff_train"] - em)
    assert np.array_equal(case["eff_plain_centred"], case["ceff"])  # mean only, before the variance was fitted


def test_decomposition(case):
    """Check 4: |b + sum_c e~_ic - predict_i| <= (2 nw + 4) 2^-52 (sum_c |e_ic| + sum_c |e_c|)."""
    m, nw = case["model"], case["nw"]
    b, em = m.intercept(), m.effect_mean
    for pts, ceff, eff in ((case["Xnew"], case["ceff"], case["eff"]), (case["X"], case["ceff_train"],
                                                                       case["eff_train"])):
        err = np.abs(b + ceff.sum(axis=1) - m.predict(pts))
        bound = (2 * nw + 4) * EPS * (np.abs(eff).sum(axis=1) + np.abs(em).sum())
        print(f"{case['name']}: max |b + sum of centred effects - predict| / bound = {np.max(err / bound):.3f}")
        assert np.all(err <= bound), float(np.max(err / bound))


def test_centred_std_against_the_dense_restatement(case):
    """Check 5: centred effect_std^2 against numpy's f^2 phi~^T W_c phi~ - k~^T A^{-1} k~ per window, phi~ = phi_c - m_c
    with numpy's own feature means and the dense A of the variance tests.  Bound: the project's 64 2^-52
    cond(mu I + W G) f^2 (1 + mu) on the variance, at the new and the training points.  Also prints the mean raw and
    centred std.  Observed on an MI355X (new / training points): nw1 4.8e-15 / 4.8e-15 (bound 1.4e-7), nw5 Gaussian
    1.6e-15 / 1.7e-15 (7.1e-9), nw5 Matern 1.1e-15 / 1.2e-15 (2.5e-9), nw33 2.7e-16 / 3.2e-16 (4.4e-9), n400 nw64
    4.8e-16 / 4.7e-16 (1.0e-9); mean raw / centred std 0.0112 / 0.0107, 0.2317 / 0.0127, 0.3178 / 0.0146,
    0.1014 / 0.0133 and 0.0980 / 0.0621."""
    bound = 64.0 * EPS * case["cond"] * F * F * (1.0 + MU)
    assert np.all(np.isfinite(case["csd"])) and np.all(np.isfinite(case["csd_train"]))
    for name, got, want in (("new", case["csd"] ** 2, case["var_new"]), ("train", case["csd_train"] ** 2,
                                                                         case["var_train"])):
        err = np.max(np.abs(got - want))
        print(f"{case['name']} ({name}): |centred effect_std^2 - var~_c| {err:.2e}, bound {bound:.2e}, cond "
              f"{case['cond']:.2e}, var~_c in [{want.min():.3e}, {want.max():.3e}]")
        assert err <= bound, (err, bound)
    print(f"{case['name']}: mean raw effect std {case['sd'].mean():.4f}, mean centred std {case['csd'].mean():.4f}, "
          f"ratio {case['sd'].mean() / case['csd'].mean():.2f}")


@pytest.mark.parametrize("name", ["nw1_gauss", "nw5_gauss"])
def test_the_constant_drops_out_exactly(name, torch_cuda):
    """Check 6: S whose only non-zero entries are S[33c, 33c] = 1 and a centring with arbitrary means but
    m[33c] = 1: the centred std is exactly 0.0 at every point and the uncentred std is |f|.  Fails if the means are
    subtracted anywhere but before the quadratic form, or if the constant's slot is not exact."""
    case = build_case(name, torch_cuda)
    co, nw = case["co"], case["nw"]
    S = np.zeros((33 * nw, 33 * nw))
    S[np.arange(0, 33 * nw, 33), np.arange(0, 33 * nw, 33)] = 1.0
    rng = np.random.default_rng(5)
    fm = rng.uniform(-1.0, 1.0, 33 * nw)
    fm[::33] = 1.0
    centring = dict(n_ref=11, feature_mean=fm, effect_mean=rng.standard_normal(nw), effect_sd=rng.random(nw))
    m = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                          co["hyper"], S=S, centring=centring)
    assert np.array_equal(m.feature_mean, fm) and np.array_equal(m.effect_mean, centring["effect_mean"])
    assert np.array_equal(m.importance, centring["effect_sd"]) and m.coefficients()["n_ref"] == 11
    for pts in (case["Xnew"], case["X"]):
        _, s0 = m.predict_effects(pts, std=True, centred=True)
        assert np.all(s0 == 0.0), float(np.max(np.abs(s0)))
        _, s1 = m.predict_effects(pts, std=True)
        assert np.all(s1 == abs(F)), float(np.max(np.abs(s1 - F)))
    assert m.intercept(std=True)[1] == math.sqrt(abs(F * F * nw))  # m^T S m = nw: the sum of the constants' squares
    bad = fm.copy()
    bad[33 * (nw - 1)] = 1.0 + EPS
    with pytest.raises(RuntimeError):
        amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                          co["hyper"], centring=dict(centring, feature_mean=bad))
    m.free()


def test_intercept(case):
    """Check 7: intercept() is the in-order sum of effect_mean, bit for bit; std_b^2 against the dense
    f^2 m^T W m - k^T A^{-1} k, k = f^2 Z W m, within check 5's bound (it comes out near f^2 mu / n).  Observed on an
    MI355X: 5.3e-16, 3.3e-17, 7.0e-17, 1.7e-16 and 1.0e-16 over the five cases; std_b^2 1.12665e-5 against f^2 mu / n
    1.12667e-5 at n = 1500."""
    m, nw = case["model"], case["nw"]
    b = 0.0
    for v in m.effect_mean:
        b += float(v)
    assert m.intercept() == b
    b2, sb = m.intercept(std=True)
    assert b2 == b and raw_intercept(m) == (0, b, sb)
    bound = 64.0 * EPS * case["cond"] * F * F * (1.0 + MU)
    err = abs(sb * sb - case["var_b"])
    print(f"{case['name']}: intercept {b:.6f}, std_b^2 {sb * sb:.6e}, dense {case['var_b']:.6e}, |difference| {err:.2e}, "
          f"bound {bound:.2e}, f^2 mu / n {F * F * MU / case['n']:.6e}")
    assert err <= bound, (err, bound)
    assert m.intercept(std=True) == (b, sb)  # a second call


def test_batching_and_placement(case):
    """Check 8, bit for bit: batches of 1, 7 and 333 rows; a second call; window=c and sub-ranges; ldim and ldo larger
    than n_new with the padding rows left at their fill value; host and device pointers; effect_curve."""
    m, nw, Xnew, ceff, csd, torch = (case[k] for k in ("model", "nw", "Xnew", "ceff", "csd", "torch"))
    e2, s2 = m.predict_effects(Xnew, std=True, centred=True)
    assert np.array_equal(e2, ceff) and np.array_equal(s2, csd)
    assert np.array_equal(m.predict_effects(Xnew, centred=True), ceff)
    for k in (1, 7, 333):
        parts = [m.predict_effects(Xnew[i:i + k], std=True, centred=True) for i in range(0, NNEW, k)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), ceff), k
        assert np.array_equal(np.concatenate([p[1] for p in parts]), csd), k
    for device in (None, torch):
        rc, e, s, nout = raw_centred(m, Xnew, NNEW + 3, NNEW + 5, 0, nw, device=device)
        assert rc == 0 and nout == 0
        assert np.array_equal(e[:NNEW], ceff) and np.array_equal(s[:NNEW], csd)
        assert np.all(e[NNEW:] == 7.0) and np.all(s[NNEW:] == 7.0)
        rc, e, s, nout = raw_centred(m, Xnew, NNEW, NNEW, 0, nw, mean=False, device=device)
        assert rc == 0 and np.all(e == 7.0) and np.array_equal(s, csd)
        rc, e, s, nout = raw_centred(m, Xnew, NNEW, NNEW, 0, nw, std=False, device=device)
        assert rc == 0 and np.all(s == 7.0) and np.array_equal(e, ceff)
    te, ts = m.predict_effects(torch.tensor(Xnew, device="cuda"), std=True, centred=True)
    assert te.is_cuda and ts.is_cuda and te.shape == (NNEW, nw)
    assert np.array_equal(te.cpu().numpy(), ceff) and np.array_equal(ts.cpu().numpy(), csd)
    feature = case["co"]["feature"]
    for c in sorted({0, nw // 2, nw - 1}):
        e1, s1 = m.predict_effects(Xnew, std=True, window=c, centred=True)
        assert e1.shape == (NNEW,) and np.array_equal(e1, ceff[:, c]) and np.array_equal(s1, csd[:, c])
        assert np.array_equal(m.predict_effects(Xnew, window=c, centred=True), ceff[:, c])
        e1, s1 = m.effect_curve(c, Xnew[:, feature[c]], std=True, centred=True)
        assert np.array_equal(e1, ceff[:, c]) and np.array_equal(s1, csd[:, c])
        t1 = m.effect_curve(c, torch.tensor(Xnew[:, feature[c]], device="cuda"), centred=True)
        assert t1.is_cuda and np.array_equal(t1.cpu().numpy(), ceff[:, c])
    for w0, wn in sorted({(min(3, nw - 1), max(1, min(nw - 3, 7))), (nw - 1, 1), (nw // 2, nw - nw // 2)}):
        for std in (True, False):
            rc, e, s, nout = raw_centred(m, Xnew, NNEW, NNEW, w0, wn, std=std)
            assert rc == 0 and nout == 0 and np.array_equal(e, ceff[:, w0:w0 + wn]), (w0, wn)
            assert np.array_equal(s, csd[:, w0:w0 + wn]) if std else np.all(s == 7.0), (w0, wn)


def test_the_fit_is_deterministic(case):
    """Check 9: fit_centring twice, with numpy X, with a device tensor, and through the raw entry point with a larger
    ldim on host and device buffers: identical feature_mean, effect_mean and importance."""
    m, X, n, nw, torch = case["model"], case["X"], case["n"], case["nw"], case["torch"]
    first = case["first"]
    assert same(held(m.fit_centring(X)), first)
    assert same(held(m.fit_centring(torch.tensor(X, device="cuda"))), first)
    buf = np.zeros((nw, n + 7))
    buf[:, :n] = X.T
    L = amd.lib()
    assert L.Nfft4GPAmdModelFitCentring(m.h, buf.ctypes.data, n, n + 7, nw) == 0
    assert same(held(m), first)
    bd = torch.tensor(buf, device="cuda")
    assert L.Nfft4GPAmdModelFitCentring(m.h, bd.data_ptr(), n, n + 7, nw) == 0
    assert same(held(m), first)


def test_nothing_else_moves(case):
    """Check 10: after fit_centring, predict, predict_std, predict_effects(std=True) and S return the bits they returned
    before; fit_variance after fit_centring keeps the centring (and gives the same S)."""
    m, Xnew, b = case["model"], case["Xnew"], case["before"]
    assert np.array_equal(m.predict(Xnew), b["mean"]) and np.array_equal(m.predict_std(Xnew), b["std"])
    e, s = m.predict_effects(Xnew, std=True)
    assert np.array_equal(e, case["eff"]) and np.array_equal(s, case["sd"])
    assert np.array_equal(m.coefficients()["S"], b["S"])
    m.fit_variance(case["X"])
    assert m.has_centring and same(held(m), case["first"])
    assert np.array_equal(m.coefficients()["S"], b["S"])
    e, s = m.predict_effects(Xnew, std=True, centred=True)
    assert np.array_equal(e, case["ceff"]) and np.array_equal(s, case["csd"])


def test_refusals(case):
    """Check 11, second half: a fit on an X with one row pushed outside the domain returns -2 and the earlier centring
    is still there, unchanged; a wrong d, ldim < n, n < 1 and a NULL X return -1; the centred call's -1 conditions
    write nothing."""
    m, nw, n, X = case["model"], case["nw"], case["n"], case["X"]
    Xbad = X.copy()
    Xbad[3, 0] = case["hi"][0] + (case["hi"][0] - case["lo"][0])
    with pytest.raises(ValueError, match="outside"):
        m.fit_centring(Xbad)
    L = amd.lib()
    buf = np.asfortranarray(Xbad)
    assert L.Nfft4GPAmdModelFitCentring(m.h, buf.ctypes.data, n, n, nw) == -2
    assert m.has_centring and same(held(m), case["first"])
    good = np.asfortranarray(X)
    assert L.Nfft4GPAmdModelFitCentring(m.h, good.ctypes.data, n, n, nw + 1) == -1
    assert L.Nfft4GPAmdModelFitCentring(m.h, good.ctypes.data, n, n - 1, nw) == -1
    assert L.Nfft4GPAmdModelFitCentring(m.h, good.ctypes.data, 0, n, nw) == -1
    assert L.Nfft4GPAmdModelFitCentring(m.h, None, n, n, nw) == -1
    with pytest.raises(ValueError):
        m.fit_centring(np.zeros((10, nw + 1)))
    assert same(held(m), case["first"])
    X10 = case["Xnew"][:10]
    refused = dict(d=dict(d=nw + 1), ldim=dict(ldim=9), ldo=dict(ldo=9), w0_negative=dict(w0=-1), wn_zero=dict(wn=0),
                   past_the_end=dict(w0=1, wn=nw), w0_past=dict(w0=nw, wn=1))
    for why, kw in refused.items():
        a = dict(ldim=10, ldo=10, w0=0, wn=nw, d=None)
        a.update(kw)
        rc, e, s, nout = raw_centred(m, X10, a["ldim"], a["ldo"], a["w0"], a["wn"], d=a["d"])
        assert rc == -1 and nout == -1 and np.all(e == 7.0) and np.all(s == 7.0), why
    e, s = m.predict_effects(np.zeros((0, nw)), std=True, centred=True)
    assert e.shape == (0, nw) and s.shape == (0, nw)
    fm, em, sd = held(m)
    assert L.Nfft4GPAmdModelSetCentring(m.h, 0, fm.ctypes.data, em.ctypes.data, sd.ctypes.data, nw) == -1
    assert L.Nfft4GPAmdModelSetCentring(m.h, n, fm.ctypes.data, em.ctypes.data, sd.ctypes.data, nw + 1) == -1
    assert L.Nfft4GPAmdModelSetCentring(m.h, n, None, em.ctypes.data, sd.ctypes.data, nw) == -1
    assert same(held(m), case["first"])


def test_outside_points(case):
    """Check 12: points pushed outside one window each are NaN in that window's centred effect and std only, every
    other entry keeps its bits, and they are counted in n_outside as in the uncentred call."""
    m, nw, co = case["model"], case["nw"], case["co"]
    X = case["Xnew"].copy()
    rows, cols = (10, 20, 30, 40), (0, nw - 1, nw // 2, nw // 2)
    for r, c in zip(rows[:3], cols[:3]):
        lo, hi = case["lo"][c], case["hi"][c]
        X[r, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    X[40, nw // 2] = np.nan
    bad = np.zeros((NNEW, nw), dtype=bool)
    bad[rows, cols] = True
    e, s = m.predict_effects(X, std=True, strict=False, centred=True)
    assert m.n_outside == 4
    assert np.array_equal(np.isnan(e), bad) and np.array_equal(np.isnan(s), bad)
    assert np.array_equal(e[~bad], case["ceff"][~bad]) and np.array_equal(s[~bad], case["csd"][~bad])
    m.predict_effects(X, std=True, strict=False)
    assert m.n_outside == 4  # the uncentred count
    with pytest.raises(ValueError, match="4 of 1000"):
        m.predict_effects(X, std=True, centred=True)
    for c in sorted(set(cols)):
        hit = bad[:, c]
        e1, s1 = m.predict_effects(X, std=True, strict=False, window=c, centred=True)
        assert m.n_outside == hit.sum()
        assert np.array_equal(np.isnan(e1), hit) and np.array_equal(e1[~hit], case["ceff"][~hit, c])
        assert np.array_equal(np.isnan(s1), hit) and np.array_equal(s1[~hit], case["csd"][~hit, c])


def test_persistence(case, tmp_path):
    """Check 13: a centred model round-trips through .npz and serves the same bits; a model without a centring saves
    exactly today's keys, plus S when it has one."""
    m, co, Xnew = case["model"], case["co"], case["Xnew"]
    path = os.path.join(tmp_path, "centred.npz")
    m.save(path)
    with np.load(path) as z:
        assert sorted(z.files) == sorted(["H", "centre", "scale", "feature", "d", "kernel", "hyper", "S", "n_ref",
                                          "feature_mean", "effect_mean", "effect_sd"])
    m2 = amd.FittedModel.load(path)
    assert m2.has_centring and m2.has_variance and same(held(m2), held(m))
    assert m2.coefficients()["n_ref"] == case["n"]
    e, s = m2.predict_effects(Xnew, std=True, centred=True)
    assert np.array_equal(e, case["ceff"]) and np.array_equal(s, case["csd"])
    assert m2.intercept(std=True) == m.intercept(std=True)
    m2.free()
    base = ["H", "centre", "scale", "feature", "d", "kernel", "hyper"]
    for S, keys in ((None, base), (co["S"], base + ["S"])):
        m3 = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"], co["kernel"],
                                               co["hyper"], S=S)
        assert not m3.has_centring and sorted(m3.coefficients()) == sorted(keys)
        plain = os.path.join(tmp_path, f"plain{len(keys)}.npz")
        m3.save(plain)
        with np.load(plain) as z:
            assert sorted(z.files) == sorted(keys)
        m4 = amd.FittedModel.load(plain)
        assert not m4.has_centring and m4.has_variance == (S is not None)
        assert np.array_equal(m4.predict(Xnew), case["before"]["mean"])
        m4.free()
        m3.free()


def test_builders(torch_cuda):
    """Check 14 (n = 400, 3 windows): FeatureGP.model(X, y, hyper, centring=True) and gp_model(..., variance=True,
    centring=True) give the same centring, bit for bit, as fit_centring(X) on the model they return without the flag.
    Two builds of a model do not hold the same table to the bit (the operator's spread adds its grids with atomics:
    "reproducible to rounding"), so the model without the flag is taken with the flagged build's own table, through
    from_coefficients; the features' means do not read the table and are also compared between two separate builds,
    whose effect means are printed side by side."""
    n, nw = 400, 3
    rng = np.random.default_rng(77)
    X = rng.random((n, nw))
    y = np.sin(4.0 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.standard_normal(n)
    win = np.arange(nw, dtype=np.int32)
    hyper = (F, 0.2, MU)
    op = amd.NFFTAdditiveKernel(np.asfortranarray(X), win, nw, 1)
    assert op.setup(amd.GAUSSIAN, F, 0.2, MU) == 0
    fgp = amd.FeatureGP(op, X, y)
    builders = {
        "FeatureGP.model": lambda **kw: fgp.model(X, y, hyper, transform=3, **kw),
        "gp_model": lambda **kw: amd.gp_model(X, win, nw, 1, y, hyper, tol=1e-10, maxits=n, transform=3, variance=True,
                                              **kw),
        "gp_model exact": lambda **kw: amd.gp_model(X, win, nw, 1, y, hyper, transform=3, op=op, exact=True, **kw),
    }
    for name, build in builders.items():
        with_flag, without = build(centring=True), build()
        assert with_flag.has_centring and with_flag.has_variance and not without.has_centring, name
        got = held(with_flag)
        co = with_flag.coefficients()
        assert co["n_ref"] == n
        twin = amd.FittedModel.from_coefficients(co["H"], co["centre"], co["scale"], co["feature"], co["d"],
                                                 co["kernel"], co["hyper"], S=co["S"])
        assert not twin.has_centring and same(got, held(twin.fit_centring(X))), name
        other = held(without.fit_centring(X))
        assert np.array_equal(got[0], other[0]), name
        print(f"{name}: two builds' tables differ by {np.max(np.abs(co['H'] - without.coefficients()['H'])):.2e}, "
              f"their effect means by {np.max(np.abs(got[1] - other[1])):.2e}")
        for m in (with_flag, without, twin):
            m.free()
    fgp.free()
    op.free()

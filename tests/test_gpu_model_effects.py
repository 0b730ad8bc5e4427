"""The fitted model's per-window effects (Nfft4GPAmdModelPredictEffects, csrc/model.hip k_model_effects;
FittedModel.predict_effects / effect_curve): effect[i, c] = f^2 Horner(H_c), the value predict adds for window c, and
effect_std[i, c] = sqrt|f^2 phi_c^T S_cc phi_c|, the posterior standard deviation of window c's term.

Cases as in test_gpu_model_variance.py (its points, features and weights are imported): n = 1500, f = 1.3, mu = 0.01
with nw = 1, 5 (Gaussian and Matern-1/2) and 33 (a partial last window group for any group size <= 32), and n = 400
with 64 windows; 1000 new points, rows 0 and 1 the per-feature minimum and maximum (1000 is no multiple of a
workgroup's 512 or 1024 points)."""
import ctypes as C

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
SERVED = {"nw5_gauss": (0, 1, 2, 3, 4), "nw5_matern": (0, 1, 2, 3, 4), "nw33_gauss": (0, 16, 32)}  # check 4's windows
_built = {}


def build_case(name, torch):
    """one model per case, with everything the checks share computed once"""
    if name in _built:
        return _built[name]
    n, nw, kernel, l = CASES[name]
    X, alpha, Xnew, lo, hi = make_points(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, MU) == 0
    model = amd.FittedModel.from_operator(op, torch.tensor(alpha, device="cuda"))
    # check 7, first half: the terms need no variance, their std does
    assert not model.has_variance
    eff_plain = model.predict_effects(Xnew)
    with pytest.raises(RuntimeError, match="fit_variance"):
        model.predict_effects(Xnew, std=True)
    rc, e, s, nout = raw_effects(model, Xnew, NNEW, NNEW, 0, nw, std=True)
    assert rc == -3 and np.all(e == 7.0) and np.all(s == 7.0) and nout == -1
    model.fit_variance(X)
    co = model.coefficients()
    before = dict(mean=model.predict(Xnew), std=model.predict_std(Xnew), S=co["S"].copy())
    eff, sd = model.predict_effects(Xnew, std=True)
    n_outside_full = model.n_outside
    eff_train, sd_train = model.predict_effects(X, std=True)
    # the restatement per window: var_c = f^2 phi_c^T W_c phi_c - k_c^T A^{-1} k_c, k_c = f^2 Z_c W_c phi_c, with the
    # dense A = f^2 (Z W Z^T + mu I) of the variance tests; A^{-1} Z is solved once and shared by all windows and points
    Z, P = features(co, X), features(co, Xnew)
    w = oracle_weights(X, nw, kernel, l)
    A = F * F * ((Z * w) @ Z.T + MU * np.eye(n))
    cond = np.linalg.cond(MU * np.eye(33 * nw) + w[:, None] * (Z.T @ Z))
    AiZ = np.linalg.solve(A, Z)

    def var_restated(Phi):
        out = np.empty((Phi.shape[0], nw))
        for c in range(nw):
            sl = slice(33 * c, 33 * c + 33)
            Kw = Phi[:, sl] * w[sl]  # rows phi_c^T W_c: k_c^T = f^2 (phi_c^T W_c) Z_c^T
            out[:, c] = F * F * np.einsum("ij,ij->i", Kw, Phi[:, sl]) - F ** 4 * np.einsum(
                "ij,jk,ik->i", Kw, Z[:, sl].T @ AiZ[:, sl], Kw)
        return out

    _built[name] = dict(name=name, n=n, nw=nw, kernel=kernel, l=l, X=X, alpha=alpha, Xnew=Xnew, lo=lo, hi=hi, op=op,
                        model=model, co=co, cond=cond, var_new=var_restated(P), var_train=var_restated(Z),
                        eff_plain=eff_plain, eff=eff, sd=sd, eff_train=eff_train, sd_train=sd_train, before=before,
                        n_outside_full=n_outside_full, torch=torch)
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


def raw_effects(model, X, ldim, ldo, w0, wn, std=True, mean=True, device=None, d=None, n_new=None):
    """Nfft4GPAmdModelPredictEffects on column-major buffers of leading dimensions ldim and ldo, outputs filled with
    7 beforehand; (status, effects ldo x wn, effect_std ldo x wn, n_outside), the arrays in Fortran order"""
    rows, dd = X.shape
    n_new = rows if n_new is None else n_new
    buf = np.zeros((dd, max(ldim, rows)))
    buf[:, :rows] = X.T
    shape = (max(wn, 1), max(ldo, 1))
    nout = C.c_longlong(-1)
    L = amd.lib()
    if device is None:
        e, s = np.full(shape, 7.0), np.full(shape, 7.0)
        rc = L.Nfft4GPAmdModelPredictEffects(model.h, buf.ctypes.data, n_new, ldim, dd if d is None else d, w0, wn,
                                             e.ctypes.data if mean else None, s.ctypes.data if std else None, ldo,
                                             C.byref(nout))
        return rc, e.T, s.T, nout.value
    bd = device.tensor(buf, device="cuda")
    e = device.full(shape, 7.0, dtype=device.float64, device="cuda")
    s = device.full(shape, 7.0, dtype=device.float64, device="cuda")
    rc = L.Nfft4GPAmdModelPredictEffects(model.h, bd.data_ptr(), n_new, ldim, dd if d is None else d, w0, wn,
                                         e.data_ptr() if mean else None, s.data_ptr() if std else None, ldo,
                                         C.byref(nout))
    return rc, e.cpu().numpy().T, s.cpu().numpy().T, nout.value


def one_window_model(co, c, with_S=False):
    S = co["S"][33 * c:33 * c + 33, 33 * c:33 * c + 33] if with_S else None
    return amd.FittedModel.from_coefficients(co["H"][c:c + 1], co["centre"][c:c + 1], co["scale"][c:c + 1],
                                             co["feature"][c:c + 1], co["d"], co["kernel"], co["hyper"], S=S)


def test_mean_is_the_one_window_models_predict(case):
    """Check 1: column c equals, bit for bit, predict of the one-window model built from H_c: 0.0 + v == v and the
    decode is shared.  At the new points and at the training points."""
    assert case["n_outside_full"] == 0
    assert case["eff"].shape == (NNEW, case["nw"]) and case["eff"].flags.f_contiguous
    assert np.all(np.isfinite(case["eff"])) and np.all(np.isfinite(case["sd"]))
    for c in range(case["nw"]):
        m1 = one_window_model(case["co"], c)
        assert np.array_equal(m1.predict(case["Xnew"]), case["eff"][:, c]), c
        assert np.array_equal(m1.predict(case["X"]), case["eff_train"][:, c]), c
        m1.free()


def test_effects_sum_to_predict(case):
    """Check 2: |sum_c effects[i, c] - predict[i]| <= (nw + 2) 2^-52 sum_c |effects[i, c]|: nw - 1 roundings in each
    of the two sums and one per product."""
    nw, m = case["nw"], case["model"]
    for pts, eff in ((case["Xnew"], case["eff"]), (case["X"], case["eff_train"])):
        mean = m.predict(pts)
        err = np.abs(eff.sum(axis=1) - mean)
        bound = (nw + 2) * EPS * np.abs(eff).sum(axis=1)
        print(f"{case['name']}: max |sum of effects - predict| / bound = {np.max(err / bound):.3f}")
        assert np.all(err <= bound), float(np.max(err / bound))


def test_std_against_the_dense_restatement(case):
    """Check 3: effect_std^2 against numpy's f^2 phi_c^T W_c phi_c - k_c^T A^{-1} k_c per window with the dense A of the
    variance tests.  Bound: the project's 64 2^-52 cond(mu I + W G) f^2 (1 + mu) on the variance.  Observed on an
    MI355X (new / training points): nw1 1.1e-14 / 1.2e-14 (bound 1.4e-7), nw5 Gaussian 7.6e-14 / 7.6e-14 (7.1e-9),
    nw5 Matern 1.3e-13 / 1.3e-13 (2.5e-9), nw33 4.7e-15 / 4.8e-15 (4.4e-9), n400 nw64 9.4e-16 / 9.4e-16 (1.0e-9)."""
    bound = 64.0 * EPS * case["cond"] * F * F * (1.0 + MU)
    for name, got, want in (("new", case["sd"] ** 2, case["var_new"]), ("train", case["sd_train"] ** 2,
                                                                         case["var_train"])):
        err = np.max(np.abs(got - want))
        print(f"{case['name']} ({name}): |effect_std^2 - var_c| {err:.2e}, bound {bound:.2e}, cond {case['cond']:.2e}, "
              f"var_c in [{want.min():.3e}, {want.max():.3e}]")
        assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", list(SERVED))
def test_std_against_the_served_route(name, torch_cuda):
    """Check 4: the one-window model of check 1 with S = S_cc: its predict_std(noise=False)^2 against effect_std^2.
    Bound 1100 2^-52 f^2 sum_jk |S_cc[j, k]|: both are sums of the same 1089 products of entries with |phi| <= 1, in
    two different orders.  Observed on an MI355X: at most 1.3e-16 (nw5 Gaussian), 1.5e-16 (nw5 Matern) and 1.6e-17
    (nw33) against bounds of 2.0e-13, 1.7e-13 and 3.0e-14."""
    case = build_case(name, torch_cuda)
    S = case["co"]["S"]
    for c in SERVED[name]:
        m1 = one_window_model(case["co"], c, with_S=True)
        bound = 1100.0 * EPS * F * F * np.abs(S[33 * c:33 * c + 33, 33 * c:33 * c + 33]).sum()
        for pts, sd in ((case["Xnew"], case["sd"]), (case["X"], case["sd_train"])):
            err = np.max(np.abs(m1.predict_std(pts, noise=False) ** 2 - sd[:, c] ** 2))
            print(f"{name} window {c}: |predict_std^2 - effect_std^2| {err:.2e}, bound {bound:.2e}")
            assert err <= bound, (c, err, bound)
        m1.free()


def test_batching_and_reproducibility(case):
    """Check 5, bit for bit: batches of 1, 7 and 333; a second call; ldim and ldo larger than n_new with the padding
    rows left at their fill value; host and device pointers; window=c, w0 / wn sub-ranges and effect_curve against
    the matching columns."""
    m, nw, Xnew, eff, sd, torch = case["model"], case["nw"], case["Xnew"], case["eff"], case["sd"], case["torch"]
    assert np.array_equal(case["eff_plain"], eff)  # mean only, before the variance was fitted
    e2, s2 = m.predict_effects(Xnew, std=True)
    assert np.array_equal(e2, eff) and np.array_equal(s2, sd)
    assert np.array_equal(m.predict_effects(Xnew), eff)
    for k in (1, 7, 333):
        parts = [m.predict_effects(Xnew[i:i + k], std=True) for i in range(0, NNEW, k)]
        assert np.array_equal(np.concatenate([p[0] for p in parts]), eff), k
        assert np.array_equal(np.concatenate([p[1] for p in parts]), sd), k
    for device in (None, torch):
        rc, e, s, nout = raw_effects(m, Xnew, NNEW + 3, NNEW + 5, 0, nw, device=device)
        assert rc == 0 and nout == 0
        assert np.array_equal(e[:NNEW], eff) and np.array_equal(s[:NNEW], sd)
        assert np.all(e[NNEW:] == 7.0) and np.all(s[NNEW:] == 7.0)
        rc, e, s, nout = raw_effects(m, Xnew, NNEW, NNEW, 0, nw, mean=False, device=device)
        assert rc == 0 and np.all(e == 7.0) and np.array_equal(s, sd)
        rc, e, s, nout = raw_effects(m, Xnew, NNEW, NNEW, 0, nw, std=False, device=device)
        assert rc == 0 and np.all(s == 7.0) and np.array_equal(e, eff)
    te, ts = m.predict_effects(torch.tensor(Xnew, device="cuda"), std=True)
    assert te.is_cuda and ts.is_cuda and te.shape == (NNEW, nw) and te.t().is_contiguous()
    assert np.array_equal(te.cpu().numpy(), eff) and np.array_equal(ts.cpu().numpy(), sd)
    feature = case["co"]["feature"]
    for c in sorted({0, nw // 2, nw - 1}):
        e1, s1 = m.predict_effects(Xnew, std=True, window=c)
        assert e1.shape == (NNEW,) and np.array_equal(e1, eff[:, c]) and np.array_equal(s1, sd[:, c])
        assert np.array_equal(m.predict_effects(Xnew, window=c), eff[:, c])
        e1, s1 = m.effect_curve(c, Xnew[:, feature[c]], std=True)
        assert np.array_equal(e1, eff[:, c]) and np.array_equal(s1, sd[:, c])
        assert np.array_equal(m.effect_curve(c, Xnew[:, feature[c]]), eff[:, c])
        t1 = m.effect_curve(c, torch.tensor(Xnew[:, feature[c]], device="cuda"))
        assert t1.is_cuda and np.array_equal(t1.cpu().numpy(), eff[:, c])
    # a range starting in the middle of a group of windows, and the last window alone
    for w0, wn in sorted({(min(3, nw - 1), max(1, min(nw - 3, 7))), (nw - 1, 1), (nw // 2, nw - nw // 2)}):
        for std in (True, False):
            rc, e, s, nout = raw_effects(m, Xnew, NNEW, NNEW, w0, wn, std=std)
            assert rc == 0 and nout == 0 and np.array_equal(e, eff[:, w0:w0 + wn]), (w0, wn)
            assert np.array_equal(s, sd[:, w0:w0 + wn]) if std else np.all(s == 7.0), (w0, wn)


def test_domain(case):
    """Check 6: four points pushed outside in one window each: exactly those (point, window) pairs are NaN in both
    arrays, every other entry keeps its bits, n_outside == 4 and strict raises; asked for another window alone, the
    same points are inside and the count is 0."""
    m, nw, co = case["model"], case["nw"], case["co"]
    X = case["Xnew"].copy()
    rows, cols = (10, 20, 30, 40), (0, nw - 1, nw // 2, nw // 2)
    for r, c in zip(rows[:3], cols[:3]):
        lo, hi = case["lo"][c], case["hi"][c]
        X[r, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    X[40, nw // 2] = np.nan
    bad = np.zeros((NNEW, nw), dtype=bool)
    bad[rows, cols] = True
    e, s = m.predict_effects(X, std=True, strict=False)
    assert m.n_outside == 4
    assert np.array_equal(np.isnan(e), bad) and np.array_equal(np.isnan(s), bad)
    assert np.array_equal(e[~bad], case["eff"][~bad]) and np.array_equal(s[~bad], case["sd"][~bad])
    e = m.predict_effects(X, strict=False)
    assert m.n_outside == 4 and np.array_equal(np.isnan(e), bad) and np.array_equal(e[~bad], case["eff"][~bad])
    with pytest.raises(ValueError, match="4 of 1000"):
        m.predict_effects(X, std=True)
    with pytest.raises(ValueError, match="4 of 1000"):
        m.predict_effects(X)
    assert np.isnan(m.predict(X, strict=False)).sum() == 4 and m.n_outside == 4  # predict's count, all windows asked
    rc, e, s, nout = raw_effects(m, X, NNEW, NNEW, 0, nw, mean=False, std=False)  # only the count
    assert rc == 0 and nout == 4 and np.all(e == 7.0) and np.all(s == 7.0)
    buf = np.asfortranarray(X)
    out = np.zeros((NNEW, nw), order="F")
    assert amd.lib().Nfft4GPAmdModelPredictEffects(m.h, buf.ctypes.data, NNEW, NNEW, nw, 0, nw, out.ctypes.data, None,
                                                   NNEW, None) == 0  # n_outside may be NULL
    assert np.array_equal(np.isnan(out), bad)
    other = [c for c in range(nw) if c not in cols][:1]  # a window none of the four points left (none when nw = 1)
    for c in sorted(set(cols)) + other:
        hit = bad[:, c]
        e1, s1 = m.predict_effects(X, std=True, strict=False, window=c)
        assert m.n_outside == hit.sum()
        assert np.array_equal(np.isnan(e1), hit) and np.array_equal(e1[~hit], case["eff"][~hit, c])
        assert np.array_equal(np.isnan(s1), hit) and np.array_equal(s1[~hit], case["sd"][~hit, c])
    for c in other:
        e1 = m.predict_effects(X, window=c)  # strict: the same points are inside
        assert m.n_outside == 0 and np.array_equal(e1, case["eff"][:, c])


def test_conventions_and_refusals(case):
    """Check 7: each -1 condition, with nothing written; n_new = 0; and predict, predict_std and S keep their bits."""
    m, nw, Xnew = case["model"], case["nw"], case["Xnew"]
    X10 = Xnew[:10]
    refused = dict(
        d=dict(d=nw + 1), ldim=dict(ldim=9), ldo=dict(ldo=9), w0_negative=dict(w0=-1), wn_zero=dict(wn=0),
        wn_negative=dict(wn=-1), past_the_end=dict(w0=1, wn=nw), w0_past=dict(w0=nw, wn=1))
    for why, kw in refused.items():
        a = dict(ldim=10, ldo=10, w0=0, wn=nw, d=None)
        a.update(kw)
        rc, e, s, nout = raw_effects(m, X10, a["ldim"], a["ldo"], a["w0"], a["wn"], d=a["d"], n_new=10)
        assert rc == -1 and nout == -1 and np.all(e == 7.0) and np.all(s == 7.0), why
    nout = C.c_longlong(-1)
    L = amd.lib()
    assert L.Nfft4GPAmdModelPredictEffects(m.h, None, 10, 10, nw, 0, nw, None, None, 10, C.byref(nout)) == -1
    assert nout.value == -1
    with pytest.raises(ValueError):
        m.predict_effects(X10[:, :nw - 1] if nw > 1 else np.zeros((10, 2)))
    with pytest.raises(ValueError):
        m.predict_effects(X10, window=nw)
    with pytest.raises(ValueError):
        m.effect_curve(-1, X10[:, 0])
    assert L.Nfft4GPAmdModelPredictEffects(m.h, None, 0, 0, nw, 0, nw, None, None, 0, C.byref(nout)) == 0
    assert nout.value == 0
    e, s = m.predict_effects(np.zeros((0, nw)), std=True)
    assert e.shape == (0, nw) and s.shape == (0, nw)
    assert m.predict_effects(np.zeros((0, nw)), window=0).shape == (0,)
    b = case["before"]
    assert np.array_equal(m.predict(Xnew), b["mean"]) and np.array_equal(m.predict_std(Xnew), b["std"])
    assert np.array_equal(m.coefficients()["S"], b["S"])


def test_effects_carry_the_operators_accuracy(torch_cuda):
    """Check 8 (nw = 5 Gaussian): per window c a one-window operator over X with the window list [c], the same kernel,
    f, l, mu and alpha; its model's predict / nw is the same quantity through code this change does not touch
    (centres and scales are per window).  e_c is that model's relative error against the dense f^2 K_c(X*, X) alpha /
    nw at the new points; the effect column's relative error against the same dense product is at most 2 e_c (check
    3's rule in test_gpu_model.py).  Observed on an MI355X: e_c 1.5e-7 .. 1.2e-6 over
    the five windows and the effect column's error equal to it to the digits printed (ratio 1.00)."""
    case = build_case("nw5_gauss", torch_cuda)
    X, Xnew, alpha, nw, l = case["X"], case["Xnew"], case["alpha"], case["nw"], case["l"]
    for c in range(nw):
        r = np.abs(Xnew[:, c][:, None] - X[:, c][None, :])
        dense = F * F * (np.exp(-r * r / (2.0 * l * l)) @ alpha) / nw
        op = amd.NFFTAdditiveKernel(X, np.array([c], dtype=np.int32), 1, 1)
        assert op.setup(case["kernel"], F, l, MU) == 0
        m1 = amd.FittedModel.from_operator(op, alpha)
        e_c = np.max(np.abs(m1.predict(Xnew) / nw - dense)) / np.max(np.abs(dense))
        e_eff = np.max(np.abs(case["eff"][:, c] - dense)) / np.max(np.abs(dense))
        print(f"window {c}: one-window operator e_c {e_c:.3e}, effect column {e_eff:.3e}, ratio {e_eff / e_c:.2f}")
        m1.free()
        op.free()
        assert e_eff <= 2.0 * e_c, (c, e_eff, e_c)

"""The exact GP loss, gradient, solve, variance matrix and mean in feature space (Nfft4GPAmdFeatureGp*,
csrc/feature_gp.hip; FeatureGP, gp_fit / gp_model with exact=True).

Cases as in test_gpu_model.py: n = 1500, X ~ U[0,1)^nw with one 1-D window per feature, f = 1.3, mu = 0.01,
y = sin(3 sum x) + 0.1 noise; nw = 33 pads to 36 windows (R_p != R); n = 40 with 3 windows has n < R; n = 2 with one
window is the smallest data set the operator accepts (at n = 1 its setup refuses: the window's radius is 0 and the
reference's scaling 0.25 / radius is undefined; test_one_point checks that this surfaces as a refusal).

The reference everywhere is dense numpy on the host: Z from numpy features of the model's quantised coordinate
(test_gpu_model.table_eval's rule), W from Nfft4GPAmdModelFeatureWeights (pinned against the oracle in
test_model_variance_host.py), W' from its twin (test_feature_gp_host.py), then slogdet / solve / inv of
A = f^2 (Z W Z^T + mu I).  Bound everywhere: 64 2^-52 cond(mu I + W G) relative to 1 + |value|, LU's backward-error
scale, the form test_gpu_model_variance.py uses."""
import ctypes as C
import math

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu

NNEW, F, MU = 1000, 1.3, 0.01
CASES = {  # n, nw, kernel, l
    "nw1_gauss": (1500, 1, amd.GAUSSIAN, 0.3),
    "nw5_gauss": (1500, 5, amd.GAUSSIAN, 0.1),
    "nw5_matern": (1500, 5, amd.MATERN12, 0.3),
    "nw33_gauss": (1500, 33, amd.GAUSSIAN, 0.1),
    "n40_nw3_gauss": (40, 3, amd.GAUSSIAN, 0.3),
    "n2_nw1_gauss": (2, 1, amd.GAUSSIAN, 0.3),
}


def make_data(n, nw, seed=None):
    rng = np.random.default_rng(1234 + nw + n if seed is None else seed)
    X = rng.random((n, nw))
    y = np.sin(3.0 * X.sum(axis=1)) + 0.1 * rng.standard_normal(n)
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((NNEW, nw))
    Xnew[0], Xnew[1] = lo, hi
    return X, y, Xnew, lo, hi


def window_map(op):
    """the handle's centres, scales and features, through a model of it"""
    m = amd.FittedModel.from_operator(op, np.zeros(op.n))
    co = m.coefficients()
    m.free()
    return co


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


def weights(co, kernel, l, grad=False):
    nw = len(co["centre"])
    fn = amd.lib().Nfft4GPAmdModelFeatureWeightsGrad if grad else amd.lib().Nfft4GPAmdModelFeatureWeights
    w = np.empty((nw, 33))
    for c in range(nw):
        assert fn(int(kernel), float(l), float(co["scale"][c]), nw, w[c].ctypes.data) == 0
    return w.ravel()


def transform(x, kind):
    """the library's transform of the three hyperparameters: values and derivatives"""
    t, dt = C.c_double(), C.c_double()
    out = []
    for v in x:
        assert amd.lib().Nfft4GPTransform(kind, float(v), 0, C.byref(t), C.byref(dt)) == 0
        out.append((t.value, dt.value))
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def dense(co, kernel, Z, y, x, kind):
    """the dense loss and its analytic gradient at x (before the transform `kind`), and what the other tests need"""
    n = Z.shape[0]
    (f, l, mu), dt = transform(x, kind)
    w, dw = weights(co, kernel, l), weights(co, kernel, l, grad=True)
    M = (Z * w) @ Z.T + mu * np.eye(n)
    A = f * f * M
    sign, lad = np.linalg.slogdet(A)
    Ainv = np.linalg.inv(A)
    a = np.linalg.solve(A, y)
    dA = [2.0 * f * M, f * f * (Z * dw) @ Z.T, f * f * np.eye(n)]
    loss = 0.5 * (y @ a / n + lad / n + math.log(2.0 * math.pi))
    grad = np.array([0.5 * (-(a @ (D @ a)) / n + np.sum(Ainv * D) / n) for D in dA]) * dt
    cond = np.linalg.cond(mu * np.eye(Z.shape[1]) + w[:, None] * (Z.T @ Z))
    return dict(loss=loss, grad=grad, sign=int(sign), A=A, a=a, w=w, u=f * f * (Z.T @ a), cond=cond, f=f, l=l, mu=mu,
                bound=64.0 * 2.0 ** -52 * cond)


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request, torch_cuda):
    n, nw, kernel, l = CASES[request.param]
    X, y, Xnew, lo, hi = make_data(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(kernel, F, l, MU) == 0
    co = window_map(op)
    fgp = amd.FeatureGP(op, X, y)
    assert (fgp.n, fgp.nw, fgp.R, fgp.kernel) == (n, nw, 33 * nw, kernel)
    Z = features(co, X)
    ref = dense(co, kernel, Z, y, (F, l, MU), 3)  # once per case; shared, never written
    out = dict(name=request.param, n=n, nw=nw, kernel=kernel, l=l, X=X, y=y, Xnew=Xnew, lo=lo, hi=hi, op=op, co=co,
               fgp=fgp, Z=Z, ref=ref, torch=torch_cuda)
    yield out
    fgp.free()
    op.free()


def check(name, got, want, bound):
    err = abs(got - want) / (1.0 + abs(want))
    print(f"{name}: got {got:.15e}, dense {want:.15e}, error {err:.2e}, bound {bound:.2e}")
    assert err <= bound, (name, err, bound)


def softplus_inverse(t):
    return math.log(math.expm1(t))


def test_loss_and_gradient(case):
    """Check 1: the loss and the three gradient components against the dense loss and its analytic gradient, with
    the identity transform, with the softplus, and with a mask."""
    fgp, co = case["fgp"], case["co"]
    x3 = (F, case["l"], MU)
    loss, grad = fgp.loss(x3, transform=3)
    ref = case["ref"]
    print(f"{case['name']}: cond(mu I + W G) {ref['cond']:.2e}, det sign {fgp.det_sign} (dense {ref['sign']})")
    check("loss (identity)", loss, ref["loss"], ref["bound"])
    for i, nm in enumerate("f l mu".split()):
        check(f"dloss/d{nm} (identity)", grad[i], ref["grad"][i], ref["bound"])
    assert fgp.det_sign == ref["sign"]
    lm, gm = fgp.loss(x3, transform=3, mask=[1, 0, 1])
    assert lm == loss and gm[1] == 0.0 and gm[0] == grad[0] and gm[2] == grad[2]
    l2, g2 = fgp.loss(x3, transform=3)  # the mask does not stick
    assert l2 == loss and np.array_equal(g2, grad)
    x0 = [softplus_inverse(v) for v in x3]
    ref0 = dense(co, case["kernel"], case["Z"], case["y"], x0, 0)
    loss0, grad0 = fgp.loss(x0)
    check("loss (softplus)", loss0, ref0["loss"], ref0["bound"])
    for i, nm in enumerate("f l mu".split()):
        check(f"dloss/d{nm} (softplus)", grad0[i], ref0["grad"][i], ref0["bound"])


def test_moments(case):
    """Check 2: G, b and y^T y against numpy to 1e-12 of n; two creates give the same bits."""
    fgp, Z, y, n = case["fgp"], case["Z"], case["y"], case["n"]
    G, b, yy = fgp.moments()
    eg, eb, ey = np.max(np.abs(G - Z.T @ Z)), np.max(np.abs(b - Z.T @ y)), abs(yy - y @ y)
    print(f"{case['name']}: |G - Z^T Z| {eg:.2e}, |b - Z^T y| {eb:.2e}, |yy - y^T y| {ey:.2e}, allowed {1e-12 * n:.2e}")
    assert max(eg, eb, ey) <= 1e-12 * n
    again = amd.FeatureGP(case["op"], case["torch"].tensor(case["X"], device="cuda"),
                          case["torch"].tensor(y, device="cuda"))  # device pointers this time
    G2, b2, yy2 = again.moments()
    again.free()
    assert np.array_equal(G, G2) and np.array_equal(b, b2) and yy == yy2


def test_moments_across_a_chunk_boundary(torch_cuda):
    """Check 2, second part: 33 windows (R_p = 1296) take chunks of 25 888 points, so n = 26 001 crosses one chunk
    boundary; the moments against numpy there, and two creates bitwise equal."""
    n, nw = 26001, 33
    X, y, _, _, _ = make_data(n, nw)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(amd.GAUSSIAN, F, 0.1, MU) == 0
    co = window_map(op)
    fgp = amd.FeatureGP(op, X, y)
    G, b, yy = fgp.moments()
    Z = features(co, X)
    eg, eb, ey = np.max(np.abs(G - Z.T @ Z)), np.max(np.abs(b - Z.T @ y)), abs(yy - y @ y)
    print(f"n {n}: |G - Z^T Z| {eg:.2e}, |b - Z^T y| {eb:.2e}, |yy - y^T y| {ey:.2e}, allowed {1e-12 * n:.2e}")
    assert max(eg, eb, ey) <= 1e-12 * n
    again = amd.FeatureGP(op, X, y)
    G2, b2, yy2 = again.moments()
    assert np.array_equal(G, G2) and np.array_equal(b, b2) and yy == yy2
    for o in (again, fgp, op):
        o.free()


def raw_solve(case, ldim, device=None):
    n, nw, X, y = case["n"], case["nw"], case["X"], case["y"]
    buf = np.zeros((nw, ldim))
    buf[:, :n] = X.T
    L = amd.lib()
    if device is None:
        alpha = np.full(n, 7.0)
        rc = L.Nfft4GPAmdFeatureGpSolve(case["fgp"].h, buf.ctypes.data, n, ldim, nw, y.ctypes.data, F, case["l"], MU,
                                        alpha.ctypes.data)
        return rc, alpha
    bd, yd = device.tensor(buf, device="cuda"), device.tensor(y, device="cuda")
    ad = device.full((n,), 7.0, dtype=device.float64, device="cuda")
    rc = L.Nfft4GPAmdFeatureGpSolve(case["fgp"].h, bd.data_ptr(), n, ldim, nw, yd.data_ptr(), F, case["l"], MU,
                                    ad.data_ptr())
    return rc, ad.cpu().numpy()


def test_solve(case):
    """Check 3: |A alpha - y|_inf <= bound |y|_inf with the dense A; host and device pointers and a larger leading
    dimension give the same bits."""
    fgp, ref, y = case["fgp"], case["ref"], case["y"]
    alpha = fgp.solve(case["X"], y, F, case["l"], MU)
    res = np.max(np.abs(ref["A"] @ alpha - y))
    allowed = ref["bound"] * np.max(np.abs(y))
    print(f"{case['name']}: |A alpha - y|_inf {res:.2e}, allowed {allowed:.2e} (cond {ref['cond']:.2e})")
    assert res <= allowed
    rc, a1 = raw_solve(case, case["n"] + 5)
    assert rc == 0 and np.array_equal(a1, alpha)
    rc, a2 = raw_solve(case, case["n"] + 5, device=case["torch"])
    assert rc == 0 and np.array_equal(a2, alpha)
    t = fgp.solve(case["torch"].tensor(case["X"], device="cuda"), case["torch"].tensor(y, device="cuda"), F,
                  case["l"], MU)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), alpha)
    # any right-hand side (one more pass forms Z^T r): the same bound, with r = y too
    r = np.random.default_rng(11).standard_normal(case["n"])
    ar = fgp.solve(case["X"], y, F, case["l"], MU, rhs=r)
    res = np.max(np.abs(ref["A"] @ ar - r))
    print(f"{case['name']}: |A alpha_r - r|_inf {res:.2e}, allowed {ref['bound'] * np.max(np.abs(r)):.2e}")
    assert res <= ref["bound"] * np.max(np.abs(r))
    ay = fgp.solve(case["X"], y, F, case["l"], MU, rhs=y)
    assert np.max(np.abs(ref["A"] @ ay - y)) <= allowed


def test_predict(case):
    """Check 4: the mean against the dense phi*^T (w o u); batches of 1, 63, 257 and all points give the same bits; the
    domain rows of test_gpu_model.test_domain (beyond the radius, NaN, inf) are NaN and counted."""
    fgp, ref, co, nw, Xnew = case["fgp"], case["ref"], case["co"], case["nw"], case["Xnew"]
    full = fgp.predict(Xnew, F, case["l"], MU)
    want = features(co, Xnew) @ (ref["w"] * ref["u"])
    err = np.max(np.abs(full - want) / (1.0 + np.abs(want)))
    print(f"{case['name']}: |mean - dense| / (1 + |dense|) {err:.2e}, bound {ref['bound']:.2e}")
    assert fgp.n_outside == 0 and err <= ref["bound"]
    for k in (1, 63, 257):
        got = np.concatenate([fgp.predict(Xnew[i:i + k], F, case["l"], MU) for i in range(0, NNEW, k)])
        assert np.array_equal(got, full), k
    t = fgp.predict(case["torch"].tensor(Xnew, device="cuda"), F, case["l"], MU)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), full)
    X = Xnew.copy()
    rows, cols = (10, 20, 30), (0, nw - 1, nw // 2)
    for r, c in zip(rows, cols):
        lo, hi = case["lo"][c], case["hi"][c]
        X[r, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    X[40, nw // 2] = np.nan
    X[50, 0] = np.inf
    got = fgp.predict(X, F, case["l"], MU, strict=False)
    bad = np.zeros(NNEW, dtype=bool)
    bad[[10, 20, 30, 40, 50]] = True
    assert fgp.n_outside == 5 and np.all(np.isnan(got[bad])) and np.array_equal(got[~bad], full[~bad])
    with pytest.raises(ValueError, match="5 of 1000"):
        fgp.predict(X, F, case["l"], MU)


def test_model(case):
    """Check 5: FeatureGP.model's mean against the dense posterior mean K(X*, X) A^{-1} y is no further than twice
    what gp_model's FGMRES route (tol 1e-10) is on the same inputs; its predict_std equals fit_variance's on the same
    model to the bound."""
    fgp, ref, co, nw, Xnew, X, y = (case[k] for k in ("fgp", "ref", "co", "nw", "Xnew", "X", "y"))
    hyper = (F, case["l"], MU)
    want = features(co, Xnew) @ (ref["w"] * ref["u"])  # f^2 Phi* W Z^T A^{-1} y
    m = fgp.model(X, y, hyper, transform=3)
    assert m.has_variance and (m.f, m.l, m.mu) == hyper
    e_exact = np.max(np.abs(m.predict(Xnew) - want))
    n = case["n"]
    mk = amd.gp_model(X, np.arange(nw, dtype=np.int32), nw, 1, y, hyper, tol=1e-10, maxits=min(n, 600), transform=3,
                      op=case["op"])
    e_krylov = np.max(np.abs(mk.predict(Xnew) - want))
    mk.free()
    print(f"{case['name']}: |mean - dense| exact route {e_exact:.2e}, FGMRES route {e_krylov:.2e}")
    assert e_exact <= 2.0 * e_krylov
    std = m.predict_std(Xnew)
    m.fit_variance(X)
    std_fit = m.predict_std(Xnew)
    err = np.max(np.abs(std - std_fit) / (1.0 + np.abs(std_fit)))
    print(f"{case['name']}: |std - std(fit_variance)| / (1 + std) {err:.2e}, bound {ref['bound']:.2e}")
    assert err <= ref["bound"]
    m.free()
    m2 = amd.gp_model(X, np.arange(nw, dtype=np.int32), nw, 1, y, hyper, transform=3, op=case["op"], exact=True)
    assert m2.has_variance and np.array_equal(m2.predict_std(Xnew), std)
    m2.free()


def adam_by_hand(fgp, x0, steps, lr, transform, beta1=0.9, beta2=0.999, eps=1e-8):
    """Nfft4GPOptimizationAdamStep's arithmetic, operation for operation, on FeatureGP.loss"""
    x = [float(v) for v in x0]
    m, v = [0.0] * 3, [0.0] * 3
    xs, losses, gnorms = [list(x)], [], []
    for it in range(steps):
        loss, g = fgp.loss(x, transform=transform)
        c1, c2 = 1.0 - math.pow(beta1, it + 1.0), 1.0 - math.pow(beta2, it + 1.0)
        gg = 0.0
        xn = [0.0] * 3
        for i in range(3):
            gi = float(g[i])
            m[i] = beta1 * m[i] + (1.0 - beta1) * gi
            v[i] = beta2 * v[i] + (1.0 - beta2) * gi * gi
            xn[i] = x[i] - lr * (m[i] / c1) / (math.sqrt(v[i] / c2) + eps)
            gg += gi * gi
        losses.append(loss)
        gnorms.append(math.sqrt(gg))
        x = xn
        xs.append(list(x))
    return np.array(xs), np.array(losses), np.array(gnorms)


def test_training(torch_cuda):
    """Check 6: gp_fit(..., exact=True) for 5 steps equals a hand-written Adam loop over FeatureGP.loss bit for bit,
    and two runs are bitwise equal."""
    n, nw, kernel, l = CASES["nw5_gauss"]
    X, y, _, _, _ = make_data(n, nw)
    win = np.arange(nw, dtype=np.int32)
    x0 = np.array([0.5, -1.0, -3.0])
    runs = [amd.gp_fit(X, win, nw, 1, y, x0, 5, lr=0.05, tol=1e-12, exact=True) for _ in range(2)]
    for a, b in zip(runs[0][:3], runs[1][:3]):
        assert np.array_equal(a, b)
    hyper, loss, gnorm, flag = runs[0]
    assert flag == 1 and hyper.shape == (6, 3) and loss.shape == (5,)
    op = amd.NFFTAdditiveKernel(np.asfortranarray(X), win, nw, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 1.0, 0.1) == 0  # the moments do not depend on the setup's hyperparameters
    fgp = amd.FeatureGP(op, X, y)
    hx, hl, hg = adam_by_hand(fgp, x0, 5, 0.05, 0)
    print(f"losses {loss}, by hand {hl}")
    assert np.array_equal(hyper, hx) and np.array_equal(loss, hl) and np.array_equal(gnorm, hg)
    assert loss[-1] < loss[0]
    # with a mask and the identity transform, through the same entry points
    h2 = amd.gp_fit(X, win, nw, 1, y, [F, l, MU], 2, lr=0.01, exact=True, transform=3, mask=[1, 0, 1], op=op)[0]
    assert np.all(h2[:, 1] == l) and np.all(h2[1:, 0] != F)
    fgp.free()
    op.free()


def test_negative_determinant(torch_cuda):
    """Check 7: Gaussian l = 0.3, 3 windows, n = 400, mu = 1e-4 (seed 0): numpy's dense slogdet has sign -1 (A is
    indefinite: W has negative entries).  det_sign reports it and the loss is the dense log|det| loss; the bound is
    the usual one, wider here only through its cond of about 1e10."""
    n, nw, l, mu = 400, 3, 0.3, 1e-4
    X, y, _, _, _ = make_data(n, nw, seed=0)
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(amd.GAUSSIAN, F, l, mu) == 0
    co = window_map(op)
    ref = dense(co, amd.GAUSSIAN, features(co, X), y, (F, l, mu), 3)
    assert ref["sign"] == -1, "the case must have a negative dense determinant"
    fgp = amd.FeatureGP(op, X, y)
    assert fgp.det_sign == 0  # nothing evaluated yet
    loss, grad = fgp.loss((F, l, mu), transform=3)
    print(f"cond {ref['cond']:.2e}, det sign {fgp.det_sign}")
    assert fgp.det_sign == -1
    check("loss (negative determinant)", loss, ref["loss"], ref["bound"])
    for i, nm in enumerate("f l mu".split()):
        check(f"dloss/d{nm} (negative determinant)", grad[i], ref["grad"][i], ref["bound"])
    fgp.free()
    op.free()


def test_one_point(torch_cuda):
    """n = 1 with one window: the operator's setup refuses a window of radius 0, so there is no set-up handle and the
    create call refuses in turn (a message, no object)."""
    X, y = np.array([[0.4]]), np.array([0.7])
    op = amd.NFFTAdditiveKernel(X, np.zeros(1, dtype=np.int32), 1, 1)
    assert op.setup(amd.GAUSSIAN, F, 0.3, MU) != 0
    assert not amd.lib().Nfft4GPAmdFeatureGpCreate(op.h, X.ctypes.data, 1, 1, 1, y.ctypes.data)
    with pytest.raises(RuntimeError):
        amd.FeatureGP(op, X, y)
    op.free()


def test_refusals(torch_cuda):
    """Check 8: a 2-feature window, a row shard, a handle with no setup, a wrong n, an X that is not the handle's data,
    mu <= 0 and more than 128 windows."""
    L = amd.lib()
    rng = np.random.default_rng(5)
    n = 300
    X = np.asfortranarray(rng.random((n, 4)))
    y = rng.standard_normal(n)

    def create(op, X, n, y):
        return L.Nfft4GPAmdFeatureGpCreate(op.h, X.ctypes.data, n, X.shape[0], X.shape[1], y.ctypes.data)

    op2 = amd.NFFTAdditiveKernel(X, np.arange(4, dtype=np.int32), 2, 2)  # two features per window
    assert op2.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not create(op2, X, n, y)
    with pytest.raises(RuntimeError):
        amd.FeatureGP(op2, X, y)
    op2.free()
    win = np.arange(4, dtype=np.int32)
    shard = amd.NFFTAdditiveKernel(X, win, 4, 1, shard=(0, n // 2))  # a row shard
    assert shard.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not create(shard, X, n // 2, y) and not create(shard, X, n, y)
    shard.free()
    op = amd.NFFTAdditiveKernel(X, win, 4, 1)
    assert not create(op, X, n, y)  # no setup yet
    assert op.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not create(op, X, n - 1, y)  # a wrong n
    assert not L.Nfft4GPAmdFeatureGpCreate(op.h, X.ctypes.data, n, n, 3, y.ctypes.data)  # a wrong d
    assert not L.Nfft4GPAmdFeatureGpCreate(op.h, None, n, n, 4, y.ctypes.data)
    Xo = np.asfortranarray(X + 0.75)  # not the handle's data: most rows leave the domain
    assert not create(op, Xo, n, y)
    fgp = amd.FeatureGP(op, X, y)
    with pytest.raises(RuntimeError):
        fgp.loss((F, 0.3, 0.0), transform=3)  # mu = 0
    with pytest.raises(RuntimeError):
        fgp.loss((F, 0.3, -0.01), transform=3)
    with pytest.raises(RuntimeError):
        fgp.solve(X, y, F, 0.3, 0.0)
    with pytest.raises(RuntimeError):
        fgp.solve(Xo, y, F, 0.3, MU)  # status -2: rows outside the domain
    with pytest.raises(RuntimeError):
        fgp.variance(F, 0.3, -1.0)
    with pytest.raises(ValueError):
        fgp.loss((F, 0.3, MU), transform=7)
    assert L.Nfft4GPAmdFeatureGpPredict(fgp.h, F, 0.3, MU, X.ctypes.data, n, n, 3, y.ctypes.data, None) == -1
    loss, _ = fgp.loss((F, 0.3, MU), transform=3)  # still usable
    assert np.isfinite(loss)
    fgp.free()
    op.free()
    nw = 129  # more than 128 windows
    Xw = np.asfortranarray(rng.random((50, nw)))
    opw = amd.NFFTAdditiveKernel(Xw, np.arange(nw, dtype=np.int32), nw, 1)
    assert opw.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not create(opw, Xw, 50, rng.standard_normal(50))
    opw.free()

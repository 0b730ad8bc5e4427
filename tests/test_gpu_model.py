"""The fitted model (Nfft4GPAmdModel*, csrc/model.hip; model.FittedModel): the operator's table of interpolation
polynomials for alpha, evaluated at new points.

Base case: n = 1500, X ~ U[0,1)^d with one 1-D window per feature, f = 1.3, mu = 0.01, alpha standard normal; 1000
new points uniform in the training set's per-feature [min, max] (rows 0 and 1 are the per-feature minimum and
maximum), all inside the radius the training points were scaled to."""
import ctypes as C
import os

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

pytestmark = pytest.mark.gpu

N, NNEW, F, MU = 1500, 1000, 1.3, 0.01
CASES = {  # nw, kernel, l, precision bits
    "nw1_gauss": (1, amd.GAUSSIAN, 0.3, 64),
    "nw5_gauss": (5, amd.GAUSSIAN, 0.1, 64),
    "nw5_matern": (5, amd.MATERN12, 0.3, 64),
    "nw33_gauss": (33, amd.GAUSSIAN, 0.1, 64),  # a partial last window group whatever the group size <= 32
    "nw5_gauss_32bit": (5, amd.GAUSSIAN, 0.1, 32),
}


def dense_product(Xa, Xb, alpha, kernel, l):
    """f^2 (1/nw) sum_c K_c(Xa, Xb) alpha: Gaussian exp(-r^2 / 2 l^2) or Matern-1/2 exp(-r / l) per feature"""
    out = np.zeros(Xa.shape[0])
    for c in range(Xa.shape[1]):
        r = np.abs(Xa[:, c][:, None] - Xb[:, c][None, :])
        K = np.exp(-r * r / (2.0 * l * l)) if kernel == amd.GAUSSIAN else np.exp(-r / l)
        out += K @ alpha
    return F * F * out / Xa.shape[1]


def table_eval(co, X, f):
    """the model's rule in numpy: per window xs = (x - centre) scale, q = round-half-away(xs 2^32) mod 2^32, cell =
    the top 6 bits, s = the remaining 26 bits << 6 with bit 31 flipped as an int32; Horner; windows added in order"""
    acc = np.zeros(X.shape[0])
    for c in range(len(co["centre"])):
        xs = (X[:, co["feature"][c]] - co["centre"][c]) * co["scale"][c]
        t = xs * 4294967296.0
        q = (np.sign(t) * np.floor(np.abs(t) + 0.5)).astype(np.int64) % (1 << 32)
        cell = q >> 26
        s = ((((q & 0x3FFFFFF) << 6) ^ 0x80000000).astype(np.uint32).view(np.int32)).astype(np.float64)
        h = co["H"][c][cell]  # [point][degree]
        v = h[:, 7].copy()
        for k in range(6, -1, -1):
            v = v * s + h[:, k]
        acc = acc + v
    return f * f * acc


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def case(request, torch_cuda):
    torch = torch_cuda
    nw, kernel, l, bits = CASES[request.param]
    rng = np.random.default_rng(1234 + nw)
    X = rng.random((N, nw))
    alpha = rng.standard_normal(N)
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((NNEW, nw))
    Xnew[0], Xnew[1] = lo, hi
    win = np.arange(nw, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, nw, 1)
    if bits == 32:
        op.set_precision(32)
    assert op.setup(kernel, F, l, MU) == 0
    ad = torch.tensor(alpha, device="cuda")
    y_before = op.matsymv(ad).cpu().numpy()
    model = amd.FittedModel.from_operator(op, ad)
    y_after = op.matsymv(ad).cpu().numpy()
    out = dict(name=request.param, nw=nw, kernel=kernel, l=l, bits=bits, X=X, alpha=alpha, Xnew=Xnew, lo=lo, hi=hi,
               op=op, model=model, y_before=y_before, y_after=y_after, y_train=y_before - F * F * MU * alpha,
               dense_train=dense_product(X, X, alpha, kernel, l), dense_new=dense_product(Xnew, X, alpha, kernel, l),
               full=model.predict(Xnew), n_outside_full=model.n_outside, torch=torch)
    yield out
    model.free()
    op.free()


def raw_predict(model, X, ldim, d=None, device=None):
    """Nfft4GPAmdModelPredict on a column-major buffer of leading dimension ldim; (status, mean, n_outside)"""
    n_new, dd = X.shape
    buf = np.zeros((dd, ldim))
    buf[:, :n_new] = X.T
    nout = C.c_longlong(-1)
    L = amd.lib()
    if device is None:
        mean = np.full(n_new, 7.0)
        rc = L.Nfft4GPAmdModelPredict(model.h, buf.ctypes.data, n_new, ldim, dd if d is None else d, mean.ctypes.data,
                                      C.byref(nout))
        return rc, mean, nout.value
    bd = device.tensor(buf, device="cuda")
    md = device.full((n_new,), 7.0, dtype=device.float64, device="cuda")
    rc = L.Nfft4GPAmdModelPredict(model.h, bd.data_ptr(), n_new, ldim, dd if d is None else d, md.data_ptr(),
                                  C.byref(nout))
    return rc, md.cpu().numpy(), nout.value


def test_training_points_reproduce_the_matvec(case):
    """Check 1: predict(X) = op.matsymv(alpha) - f^2 mu alpha.  The layout moves an offset by at most 8 2^-32 of a cell
    (its index bits) and a 16-mode function on 64 cells has slope <= 2 pi 16 / 64 per cell: <= 3e-9 per unit of
    max|f|; the test allows 1e-8 of max|y| (1e-6 in the 32-bit mode, that mode's own bound in test_gpu_precision)."""
    m = case["model"]
    got = m.predict(case["X"])
    assert m.n_outside == 0
    err = np.max(np.abs(got - case["y_train"])) / np.max(np.abs(case["y_train"]))
    print(f"{case['name']}: model at the training points vs matvec: {err:.2e} of max|y|")
    assert err <= (1e-6 if case["bits"] == 32 else 1e-8), err


def test_kernel_against_numpy_evaluation_of_the_table(case):
    """Check 2: the kernel against the exported table evaluated in numpy by the same cell / offset rule: rounding."""
    m = case["model"]
    co = m.coefficients()
    assert co["H"].shape == (case["nw"], 64, 8) and list(co["feature"]) == list(range(case["nw"]))
    assert (m.nw, m.d, m.kernel, m.f, m.l, m.mu) == (case["nw"], case["nw"], case["kernel"], F, case["l"], MU)
    for X, got in ((case["Xnew"], case["full"]), (case["X"], m.predict(case["X"]))):
        want = table_eval(co, X, F)
        err = np.max(np.abs(got - want)) / np.max(np.abs(want))
        print(f"{case['name']}: kernel vs numpy table evaluation: {err:.2e} of max|mean|")
        assert err <= 1e-12, err


def test_new_points_carry_the_operators_accuracy(case):
    """Check 3: against the dense product K(X*, X) alpha the model at new points is no further than twice what the
    existing matvec is at the training points (0.9 - 1.15 times in the CPU emulation; 2 covers the maximum being
    taken over another sample)."""
    assert case["n_outside_full"] == 0 and np.all(np.isfinite(case["full"]))
    e_new = np.max(np.abs(case["full"] - case["dense_new"])) / np.max(np.abs(case["dense_new"]))
    e_train = np.max(np.abs(case["y_train"] - case["dense_train"])) / np.max(np.abs(case["dense_train"]))
    print(f"{case['name']}: e_new {e_new:.3e}, e_train {e_train:.3e}, ratio {e_new / e_train:.2f}")
    assert e_new <= 2.0 * e_train, (e_new, e_train)


def test_batching_and_reproducibility(case):
    """Check 4: any batch gives the bits of the one call over all points; so do a second call, a leading dimension
    of n_new + 3 and device pointers."""
    m, Xnew, full = case["model"], case["Xnew"], case["full"]
    for k in (1, 63, 257, 1000):
        a = m.predict(Xnew[:k])
        assert np.array_equal(a, full[:k]), k
        assert np.array_equal(m.predict(Xnew[:k]), a), k
        rc, b, nout = raw_predict(m, Xnew[:k], k + 3)
        assert rc == 0 and nout == 0 and np.array_equal(b, full[:k]), k
        rc, c, nout = raw_predict(m, Xnew[:k], k + 3, device=case["torch"])
        assert rc == 0 and nout == 0 and np.array_equal(c, full[:k]), k
    t = m.predict(case["torch"].tensor(Xnew, device="cuda"))
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), full)
    # a later batch of the same points: rows [257, 1000)
    assert np.array_equal(m.predict(Xnew[257:]), full[257:])


def test_domain(case):
    """Check 5: three rows with one coordinate 1 % of the range beyond the training points -- on the side that is
    further from the window's centre, the side that defines the radius (the nearer side's 1 % can still lie within
    it) -- and one row with a NaN: those four are NaN and counted, every other row keeps its bits."""
    m, nw = case["model"], case["nw"]
    co = m.coefficients()
    X = case["Xnew"].copy()
    rows, cols = (10, 20, 30), (0, nw - 1, nw // 2)
    for r, c in zip(rows, cols):
        lo, hi = case["lo"][c], case["hi"][c]
        X[r, c] = hi + 0.01 * (hi - lo) if hi - co["centre"][c] >= co["centre"][c] - lo else lo - 0.01 * (hi - lo)
    X[40, nw // 2] = np.nan
    got = m.predict(X, strict=False)
    assert m.n_outside == 4
    bad = np.zeros(NNEW, dtype=bool)
    bad[[10, 20, 30, 40]] = True
    assert np.all(np.isnan(got[bad]))
    assert np.array_equal(got[~bad], case["full"][~bad])
    with pytest.raises(ValueError, match="4 of 1000"):
        m.predict(X)
    # an infinite coordinate is outside too; n_outside may be NULL
    X[50, 0] = np.inf
    assert np.isnan(m.predict(X, strict=False)[50]) and m.n_outside == 5
    buf = np.asfortranarray(X)
    mean = np.zeros(NNEW)
    assert amd.lib().Nfft4GPAmdModelPredict(m.h, buf.ctypes.data, NNEW, NNEW, nw, mean.ctypes.data, None) == 0
    assert np.array_equal(np.isnan(mean), np.isnan(got) | (np.arange(NNEW) == 50))


def test_matvec_is_unaffected(case):
    """Check 6 (third part): the operator's matvec before and after from_operator, to its run-to-run level."""
    d = np.max(np.abs(case["y_after"] - case["y_before"])) / np.max(np.abs(case["y_before"]))
    assert d <= 1e-13, d


def test_independence_and_save_load(torch_cuda, tmp_path):
    """Check 6: the model outlives its operator; save / load gives the same bits."""
    torch = torch_cuda
    rng = np.random.default_rng(77)
    nw = 5
    X = rng.random((N, nw))
    alpha = rng.standard_normal(N)
    Xnew = X.min(axis=0) + (X.max(axis=0) - X.min(axis=0)) * rng.random((NNEW, nw))
    op = amd.NFFTAdditiveKernel(X, np.arange(nw, dtype=np.int32), nw, 1)
    assert op.setup(amd.MATERN12, F, 0.3, MU) == 0
    m = amd.FittedModel.from_operator(op, alpha)  # a host alpha
    m2 = amd.FittedModel.from_operator(op, torch.tensor(alpha, device="cuda"))
    a = m.predict(Xnew)
    assert np.max(np.abs(m2.predict(Xnew) - a)) <= 1e-13 * np.max(np.abs(a))  # two spreads: the matvec's rounding
    m2.free()
    op.free()
    del op
    assert np.array_equal(m.predict(Xnew), a)
    path = os.path.join(tmp_path, "model.npz")
    m.save(path)
    m3 = amd.FittedModel.load(path)
    m.free()
    assert (m3.nw, m3.d, m3.kernel, m3.f, m3.l, m3.mu) == (nw, nw, amd.MATERN12, F, 0.3, MU)
    assert np.array_equal(m3.predict(Xnew), a)
    m3.free()


def test_refusals(torch_cuda):
    """Check 7: a 2-feature window, no setup call and a wrong n give NULL; predict with a wrong d gives -1."""
    L = amd.lib()
    rng = np.random.default_rng(5)
    X = rng.random((N, 4))
    alpha = rng.standard_normal(N)
    op2 = amd.NFFTAdditiveKernel(X, np.arange(4, dtype=np.int32), 2, 2)
    assert op2.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not L.Nfft4GPAmdModelCreate(op2.h, alpha.ctypes.data, N)
    with pytest.raises(RuntimeError):
        amd.FittedModel.from_operator(op2, alpha)
    op2.free()
    op = amd.NFFTAdditiveKernel(X, np.arange(4, dtype=np.int32), 4, 1)
    assert not L.Nfft4GPAmdModelCreate(op.h, alpha.ctypes.data, N)  # no setup yet
    assert op.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not L.Nfft4GPAmdModelCreate(op.h, alpha.ctypes.data, N - 1)
    assert not L.Nfft4GPAmdModelCreate(None, alpha.ctypes.data, N)
    shard = amd.NFFTAdditiveKernel(X, np.arange(4, dtype=np.int32), 4, 1, shard=(0, 752))
    assert shard.setup(amd.GAUSSIAN, F, 0.3, MU) == 0
    assert not L.Nfft4GPAmdModelCreate(shard.h, alpha.ctypes.data, 752)
    shard.free()
    m = amd.FittedModel.from_operator(op, alpha)
    rc, mean, _ = raw_predict(m, X[:10, :3], 10)
    assert rc == -1 and np.all(mean == 7.0)
    rc, _, _ = raw_predict(m, X[:10], 10, d=5)
    assert rc == -1
    with pytest.raises(ValueError):
        m.predict(X[:10, :3])
    nout = C.c_longlong(-1)
    assert L.Nfft4GPAmdModelPredict(m.h, None, 0, 0, 4, None, C.byref(nout)) == 0 and nout.value == 0
    m.free()
    op.free()

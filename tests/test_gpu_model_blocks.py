"""The fitted model and FeatureGP over more than one workgroup of every serving kernel, with rows outside the domain
in the first, an inner and the last workgroup (csrc/window_points.hpp: the domain test, the workgroup's outside count,
the table's staging; csrc/internal.h BlockCounts: the host's sum over the workgroups' counts).

n = 1500 training points, n_new = 2100 new points, 9 one-feature Gaussian windows, the other model tests' f = 1.3,
mu = 0.01 and l = 0.1.  2100 points are 3 workgroups of the kernels that take 1024 points (k_model_predict,
k_model_effects<false>, k_fgp_apply), 5 at 512 (k_model_effects<true>), 9 at 256 (k_model_outside) and 17 at 128
(k_model_std, k_model_paths).  9 windows are one full and one partial group of 8 for the mean, an odd count for the
std-effects' groups of 2, and 9 padded to 12 for the MFMA walks.

Bad rows: rows {0, 127, 128, 511, 512, 1023, 1024, 2099} of the clean Xnew -- the first and last point of workgroups
at every size -- are moved outside window (row % 9) by test_gpu_model.test_domain's recipe (1 % of the range beyond
the training points, on the side further from the window's centre); row 1500 is NaN in window 8.  Every comparison is
of bits: a row that is not bad keeps the clean call's value."""
import ctypes as C

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu

N, NNEW, NW, F, MU, L = 1500, 2100, 9, 1.3, 0.01, 0.1
BAD_ROWS = (0, 127, 128, 511, 512, 1023, 1024, 2099)
NAN_ROW, NAN_WINDOW = 1500, 8
RANGES = ((8, 1), (2, 5))


@pytest.fixture(scope="module")
def case(torch_cuda):
    rng = np.random.default_rng(1234 + NW)
    X = rng.random((N, NW))
    alpha = rng.standard_normal(N)
    y = rng.standard_normal(N)
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((NNEW, NW))
    op = amd.NFFTAdditiveKernel(X, np.arange(NW, dtype=np.int32), NW, 1)
    assert op.setup(amd.GAUSSIAN, F, L, MU) == 0
    model = amd.FittedModel.from_operator(op, alpha)
    model.fit_variance(X)
    fgp = amd.FeatureGP(op, X, y)
    centre = model.coefficients()["centre"]
    Xbad = Xnew.copy()
    bad = np.zeros((NNEW, NW), dtype=bool)  # the (row, window) pairs outside
    for r in BAD_ROWS:
        c = r % NW
        Xbad[r, c] = hi[c] + 0.01 * (hi[c] - lo[c]) if hi[c] - centre[c] >= centre[c] - lo[c] else \
            lo[c] - 0.01 * (hi[c] - lo[c])
        bad[r, c] = True
    Xbad[NAN_ROW, NAN_WINDOW] = np.nan
    bad[NAN_ROW, NAN_WINDOW] = True
    assert bad.any(axis=1).sum() == 9
    yield dict(model=model, fgp=fgp, Xnew=Xnew, Xbad=Xbad, bad=bad, badrow=bad.any(axis=1))
    fgp.free()
    model.free()
    op.free()


def check_rows(got, clean, badrow, name):
    """got is NaN exactly at the bad rows (in every column) and has the clean call's bits everywhere else"""
    got, clean = np.asarray(got), np.asarray(clean)
    assert np.all(np.isfinite(clean)), name
    nan = np.isnan(got)
    want = badrow if got.ndim == 1 else np.repeat(badrow[:, None], got.shape[1], axis=1)
    assert np.array_equal(nan, want), name
    assert np.array_equal(got[~nan], clean[~nan]), name


def check_pairs(got, clean, badpair, name):
    """got (n_new x windows) is NaN exactly at the bad (row, window) pairs and has the clean call's bits elsewhere"""
    got, clean = np.asarray(got), np.asarray(clean)
    assert np.all(np.isfinite(clean)), name
    assert np.array_equal(np.isnan(got), badpair), name
    assert np.array_equal(got[~badpair], clean[~badpair]), name


def test_all_windows(case):
    """predict, predict_std, predict_effects (with and without std), paths over all windows (1 and 129 drawn paths) and
    FeatureGP's predict: 9 rows outside, NaN exactly there, the clean call's bits everywhere else."""
    m, fgp, Xnew, Xbad, bad, badrow = (case[k] for k in ("model", "fgp", "Xnew", "Xbad", "bad", "badrow"))
    clean = m.predict(Xnew)
    assert m.n_outside == 0
    got = m.predict(Xbad, strict=False)
    assert m.n_outside == 9
    check_rows(got, clean, badrow, "predict")
    for noise in (True, False):
        clean = m.predict_std(Xnew, noise=noise)
        assert m.n_outside == 0
        got = m.predict_std(Xbad, strict=False, noise=noise)
        assert m.n_outside == 9
        check_rows(got, clean, badrow, f"predict_std noise={noise}")
    clean = m.predict_effects(Xnew)
    assert m.n_outside == 0
    got = m.predict_effects(Xbad, strict=False)
    assert m.n_outside == 9
    check_pairs(got, clean, bad, "effects")
    clean_e, clean_s = m.predict_effects(Xnew, std=True)
    assert m.n_outside == 0 and np.array_equal(clean_e, clean)
    got_e, got_s = m.predict_effects(Xbad, std=True, strict=False)
    assert m.n_outside == 9
    check_pairs(got_e, clean_e, bad, "effects with std")
    check_pairs(got_s, clean_s, bad, "effect_std")
    for ns in (1, 129):
        m.draw_paths(ns, seed=ns)
        clean = m.paths(Xnew)
        assert m.n_outside == 0 and clean.shape == (NNEW, ns)
        got = m.paths(Xbad, strict=False)
        assert m.n_outside == 9
        check_rows(got, clean, badrow, f"paths ns={ns}")
    clean = fgp.predict(Xnew, F, L, MU)
    assert fgp.n_outside == 0
    got = fgp.predict(Xbad, F, L, MU, strict=False)
    assert fgp.n_outside == 9
    check_rows(got, clean, badrow, "FeatureGP predict")


def raw_effects(model, X, w0, wn, std):
    """Nfft4GPAmdModelPredictEffects over the windows [w0, w0 + wn) on host arrays; (effects, effect_std, n_outside)"""
    Xf = np.asfortranarray(X)
    n = X.shape[0]
    eff = np.empty((n, wn), order="F")
    sd = np.empty((n, wn), order="F") if std else None
    nout = C.c_longlong(-1)
    rc = amd.lib().Nfft4GPAmdModelPredictEffects(model.h, Xf.ctypes.data, n, n, X.shape[1], w0, wn, eff.ctypes.data,
                                                 sd.ctypes.data if std else None, n, C.byref(nout))
    assert rc == 0
    return eff, sd, nout.value


def test_window_ranges(case):
    """predict_effects over the windows [8, 9) and [2, 7), and paths of window 8 (Nfft4GPAmdModelEvalPaths takes one
    window or all of them, so the range of 5 is predict_effects' alone): the count is of the rows with a bad pair in
    the range, and so is the NaN pattern; the values are the all-window call's columns."""
    m, Xnew, Xbad, bad = (case[k] for k in ("model", "Xnew", "Xbad", "bad"))
    full_e, full_s = m.predict_effects(Xnew, std=True)
    for w0, wn in RANGES:
        sub = bad[:, w0:w0 + wn]
        want = int(sub.any(axis=1).sum())
        assert want == {(8, 1): 2, (2, 5): 3}[(w0, wn)]
        for std in (False, True):
            ce, cs, nout = raw_effects(m, Xnew, w0, wn, std)
            assert nout == 0 and np.array_equal(ce, full_e[:, w0:w0 + wn])
            assert not std or np.array_equal(cs, full_s[:, w0:w0 + wn])
            ge, gs, nout = raw_effects(m, Xbad, w0, wn, std)
            assert nout == want, (w0, wn, std, nout)
            check_pairs(ge, ce, sub, f"effects [{w0}, {w0 + wn}) std={std}")
            if std:
                check_pairs(gs, cs, sub, f"effect_std [{w0}, {w0 + wn})")
    w0 = RANGES[0][0]
    for ns in (1, 129):
        m.draw_paths(ns, seed=ns)
        clean = m.paths(Xnew, window=w0)
        assert m.n_outside == 0
        got = m.paths(Xbad, window=w0, strict=False)
        assert m.n_outside == int(bad[:, w0].sum()) == 2
        check_rows(got, clean, bad[:, w0], f"paths window={w0} ns={ns}")


def test_fit_variance_refuses_the_bad_rows(case):
    """Nfft4GPAmdModelFitVariance on the bad array returns -2 and leaves S as it was: predict_std keeps its bits."""
    m, Xnew, Xbad = case["model"], case["Xnew"], case["Xbad"]
    before = m.predict_std(Xnew)
    Xf = np.asfortranarray(Xbad)
    assert amd.lib().Nfft4GPAmdModelFitVariance(m.h, Xf.ctypes.data, NNEW, NNEW, NW) == -2
    assert m.has_variance and np.array_equal(m.predict_std(Xnew), before)

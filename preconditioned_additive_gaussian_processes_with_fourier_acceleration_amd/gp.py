"""GP loss and prediction on the NFFT additive operator, over the C ABI.

``gp_loss``     Nfft4GPGpLoss (SRC/optimizer/gp_loss.c:96-307) with Nfft4GPNFFTAdditiveKernelGaussianKernel /
                Nfft4GPAdditiveNFFTMatSymv / Nfft4GPAdditiveNFFTGradMatSymv as kernel, matvec and grad matvec,
                no preconditioner (TEST1-style call of the north-star operator inside the loss); or, over
                one process per GPU, a dist.DistributedAdditiveKernel with Nfft4GPAmdDistGaussianKernel /
                Nfft4GPAmdDistMatSymv / Nfft4GPAmdDistGradMatSymv (BASELINE configs[4]).
``gp_predict``  Nfft4GPAdditiveNFFTGpPredict (SRC/external/nfft_interface.c:873-1068): posterior mean and,
                optionally, standard deviation at new points (a second handle over [X; Xp], as TEST4 does).
``gp_fit``      the reference's training sequence (TESTS/TEST4/foo.cpp:268-347): Nfft4GPGpProblemSetup, then
                Nfft4GPOptimizationAdam* stepping on Nfft4GPGpProblemLoss.
``gp_model``    solve (K + mu I) alpha = y once and keep the result as a model.FittedModel, which predicts new
                points without the training data (mean, standard deviation, and each window's effect with its
                own standard deviation: FittedModel.predict_effects / effect_curve).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .feature_gp import FeatureGP
from .model import FittedModel
from .nfft import GAUSSIAN, NFFTAdditiveKernel

_vp = C.c_void_p
_GPLOSS_ARGS = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _vp, C.c_int, _vp, C.c_int, _vp,
                _lib.dp, _lib.dp]
_PREDICT_ARGS = [_vp, _vp, _vp, C.c_int, C.c_int, C.c_int, _vp, C.c_int, C.c_int, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                 _vp, _vp, _vp, _vp, _vp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, _vp, C.POINTER(_lib.dp),
                 C.POINTER(_lib.dp)]


def gp_loss(X, windows, nwindows, dwindows, y, hyper, maxits=50, nvecs=10, rademacher=None, tol=1e-6,
            transform=0, mask=None, print_level=-1, op=None):
    """(loss, grad) of Nfft4GPGpLoss for the additive NFFT Gaussian kernel; ``hyper`` = (f, l, mu) before
    the transform (0 softplus, 1 sigmoid, 2 exp, 3 identity).  ``op``: an existing NFFTAdditiveKernel over
    the same X to reuse, as the reference's optimizer loop reuses its kernel handle across loss calls
    (its points, centring and scale stay those of its first setup, nfft_interface.c:150); or a
    dist.DistributedAdditiveKernel (every rank calls gp_loss collectively): with partition "rows", ``y``
    and ``rademacher`` hold this rank's rows [op.row_begin, op.row_end) only; with "components" they are
    whole.  Every rank returns the same loss and gradient."""
    from .dist import DistributedAdditiveKernel
    # the points only build a new handle: a given op holds its own (the kernel setup does not read `data`,
    # nfft_api.cpp), so no column-major copy of X is made then (256 MB at config C, ~0.1 s of host time)
    X = np.asarray(X, dtype=np.float64)
    if op is None:
        X = np.asfortranarray(X)
    n, d = X.shape
    setup_fn, mv, dmv = ("Nfft4GPNFFTAdditiveKernelGaussianKernel", "Nfft4GPAdditiveNFFTMatSymv",
                         "Nfft4GPAdditiveNFFTGradMatSymv")
    if op is None:
        op = NFFTAdditiveKernel(X, windows, nwindows, dwindows)
    elif isinstance(op, DistributedAdditiveKernel):
        if op.n_global != n:
            raise ValueError("op was created over a different number of points")
        n = op.n  # this rank's rows (the whole n for components)
        setup_fn, mv, dmv = "Nfft4GPAmdDistGaussianKernel", "Nfft4GPAmdDistMatSymv", "Nfft4GPAmdDistGradMatSymv"
    elif op.n != n:
        raise ValueError("op was created over a different number of points")
    if len(y) != n:
        raise ValueError(f"{len(y)} labels for {n} rows")
    L = _lib.lib()
    fn = L.Nfft4GPGpLoss
    fn.argtypes = _GPLOSS_ARGS
    fn.restype = C.c_int
    x = np.ascontiguousarray(np.asarray(hyper, dtype=np.float64))
    lab = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    if rademacher is None:
        R, r_ptr = None, None
    elif hasattr(rademacher, "data_ptr"):  # a torch tensor (n * nvecs, column-major probes); device OK
        R, r_ptr = rademacher, rademacher.data_ptr()
    else:
        R = np.asfortranarray(np.asarray(rademacher, dtype=np.float64))
        r_ptr = R.ctypes.data
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.int32))
    loss = np.zeros(1)
    grad = np.zeros(3)
    rc = fn(x.ctypes.data, X.ctypes.data, lab.ctypes.data, n, n, d,
            _lib.fnptr(setup_fn), op.h, None, _lib.fnptr(mv), _lib.fnptr(dmv),
            None, None, None, None, None, None, None, None, None, None, 0, float(tol), int(maxits), int(maxits),
            int(nvecs), r_ptr, int(transform),
            m.ctypes.data if m is not None else None, int(print_level), None, loss.ctypes.data_as(_lib.dp),
            grad.ctypes.data_as(_lib.dp))
    if rc:
        raise RuntimeError("Nfft4GPGpLoss failed")
    return float(loss[0]), grad


def gp_predict(X, Xp, windows, nwindows, dwindows, y, hyper, maxits=100, tol=1e-8, with_std=False,
               transform=0, print_level=-1):
    """(mean, std or None) of Nfft4GPAdditiveNFFTGpPredict at the rows of Xp."""
    X = np.asfortranarray(np.asarray(X, dtype=np.float64))
    Xp = np.asfortranarray(np.asarray(Xp, dtype=np.float64))
    n, d = X.shape
    npred = Xp.shape[0]
    Xa = np.asfortranarray(np.vstack([X, Xp]))
    op = NFFTAdditiveKernel(X, windows, nwindows, dwindows)
    opa = NFFTAdditiveKernel(Xa, windows, nwindows, dwindows)
    L = _lib.lib()
    fn = L.Nfft4GPAdditiveNFFTGpPredict
    fn.argtypes = _PREDICT_ARGS
    fn.restype = C.c_int
    x = np.ascontiguousarray(np.asarray(hyper, dtype=np.float64))
    lab = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    mean = np.zeros(npred)
    std = np.zeros(npred)
    mp = C.cast(mean.ctypes.data, _lib.dp)
    sp = C.cast(std.ctypes.data, _lib.dp)
    rc = fn(x.ctypes.data, X.ctypes.data, lab.ctypes.data, n, n, d, Xp.ctypes.data, npred, npred, Xa.ctypes.data,
            _lib.fnptr("Nfft4GPNFFTAdditiveKernelGaussianKernel"), op.h, opa.h, None, op.matvec_fnptr, None, None,
            None, None, None, None, 0, float(tol), int(maxits), int(transform), int(print_level), None,
            C.byref(mp), C.byref(sp) if with_std else None)
    if rc:
        raise RuntimeError("Nfft4GPAdditiveNFFTGpPredict failed")
    return mean, (std if with_std else None)


def gp_fit(X, windows, nwindows, dwindows, y, hyper0, steps, lr=0.01, beta1=0.9, beta2=0.999, eps=1e-8, tol=1e-3,
           op=None, exact=False, objective="mll", **loss_kwargs):
    """Adam on the GP loss, run by the library: Nfft4GPGpProblemSetup carries gp_loss's arguments,
    Nfft4GPOptimizationAdamStep calls Nfft4GPGpProblemLoss and updates the hyperparameters (``hyper0`` = (f, l, mu)
    before the transform), for at most ``steps`` steps or until the gradient norm falls below ``tol``.
    ``loss_kwargs`` are gp_loss's: maxits, nvecs, rademacher, transform, mask, print_level (and loss_tol, its tol).
    Returns (hyper_history [nits + 1, 3], loss_history [nits], grad_norm_history [nits], flag): entry k of the
    loss and gradient-norm histories belongs to hyper_history[k]; flag is the last step's status (1 steps
    reached, 2 gradient norm below tol, -1 the loss failed).  The library prints one line per step, as the
    reference does.
    ``exact=True`` (1-D windows): the same Adam entry points step on Nfft4GPAmdFeatureGpLoss instead -- the loss and
    gradient of the operator's finite-rank form, exact and deterministic, with no solve and no probes (of
    ``loss_kwargs`` only transform and mask apply); the kernel is the one ``op`` was last set up with, Gaussian for
    a new op.
    ``objective``: "mll" (the default), the marginal likelihood above, or "loo" (with ``exact=True`` only): the
    leave-one-out predictive density of the same operator, Nfft4GPAmdFeatureGpLooLoss over X and y bound to the
    FeatureGP, through the same Adam entry points."""
    if objective not in ("mll", "loo"):
        raise ValueError('objective is "mll" or "loo"')
    if objective == "loo" and not exact:
        raise ValueError('objective="loo" needs exact=True: the leave-one-out loss exists in feature space only')
    unknown = set(loss_kwargs) - {"maxits", "nvecs", "rademacher", "transform", "mask", "print_level", "loss_tol"}
    if unknown:
        raise TypeError(f"unknown loss arguments: {sorted(unknown)}")
    maxits = int(loss_kwargs.get("maxits", 50))
    nvecs = int(loss_kwargs.get("nvecs", 10))
    rademacher = loss_kwargs.get("rademacher")
    transform = int(loss_kwargs.get("transform", 0))
    mask = loss_kwargs.get("mask")
    print_level = int(loss_kwargs.get("print_level", -1))
    loss_tol = float(loss_kwargs.get("loss_tol", 1e-6))
    steps = int(steps)
    if steps < 1:
        raise ValueError("steps must be at least 1")
    X = np.asarray(X, dtype=np.float64)
    if op is None:
        X = np.asfortranarray(X)  # a given op holds its own points (gp_loss)
        op = NFFTAdditiveKernel(X, windows, nwindows, dwindows)
    elif not isinstance(op, NFFTAdditiveKernel):
        raise TypeError("gp_fit runs on an NFFTAdditiveKernel")
    n, d = X.shape
    if op.n != n:
        raise ValueError("op was created over a different number of points")
    if len(y) != n:
        raise ValueError(f"{len(y)} labels for {n} rows")
    lab = np.ascontiguousarray(np.asarray(y, dtype=np.float64))
    x0 = np.ascontiguousarray(np.asarray(hyper0, dtype=np.float64))
    if x0.size != 3:
        raise ValueError("hyper0 = (f, l, mu)")
    if rademacher is None:
        R, r_ptr = None, None
    elif hasattr(rademacher, "data_ptr"):
        R, r_ptr = rademacher, rademacher.data_ptr()
    else:
        R = np.asfortranarray(np.asarray(rademacher, dtype=np.float64))
        r_ptr = R.ctypes.data
    m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.int32))
    L = _lib.lib()
    if exact:
        return _gp_fit_exact(L, op, X, lab, x0, steps, lr, beta1, beta2, eps, tol, transform, m, objective)
    adam = L.Nfft4GPOptimizationAdamCreate()
    prob = L.Nfft4GPGPProblemCreate()
    try:
        rc = L.Nfft4GPGpProblemSetup(
            prob, 1, _lib.fnptr("Nfft4GPOptimizationAdamStep"), adam,  # NFFT4GP_OPTIMIZER_ADAM
            X.ctypes.data, n, n, d, lab.ctypes.data,
            _lib.fnptr("Nfft4GPNFFTAdditiveKernelGaussianKernel"), op.h, None,
            _lib.fnptr("Nfft4GPAdditiveNFFTMatSymv"), _lib.fnptr("Nfft4GPAdditiveNFFTGradMatSymv"),
            None, None, None, None, None, None, None, None, None, None,  # no preconditioner
            0, loss_tol, maxits, maxits, nvecs, r_ptr, transform, m.ctypes.data if m is not None else None,
            print_level,
            None, 0, 0, 0, None, None, 0, 1e-6, 0, 100, 0, 0)  # the prediction fields are not used here
        if rc or L.Nfft4GPOptimizationAdamSetProblem(adam, _lib.fnptr("Nfft4GPGpProblemLoss"), prob, 3) or \
                L.Nfft4GPOptimizationAdamSetOptions(adam, steps, float(tol), float(beta1), float(beta2), float(eps),
                                                    float(lr)) or \
                L.Nfft4GPOptimizationAdamInit(adam, x0.ctypes.data):
            raise RuntimeError("the optimiser setup failed")
        flag = 0
        while flag == 0:
            flag = L.Nfft4GPOptimizationAdamStep(adam)
        hyper, loss, gnorm = _adam_histories(adam, steps)
    finally:
        L.Nfft4GPOptimizationAdamFree(adam)
        L.Nfft4GPGPProblemFree(prob)
    del R
    return hyper, loss, gnorm, int(flag)


def _adam_histories(adam, steps):
    st = _lib.OptimizerAdamStruct.from_address(adam)
    nits = st._nits
    hyper = np.ctypeslib.as_array(st._x_history, shape=(nits + 1, 3)).copy()
    loss = np.ctypeslib.as_array(st._loss_history, shape=(steps + 1,))[:nits].copy()
    gnorm = np.ctypeslib.as_array(st._grad_norm_history, shape=(steps + 1,))[:nits].copy()
    return hyper, loss, gnorm


def _set_up_once(op, x0, transform):
    """a FeatureGP needs a handle whose points are fixed: one setup call at the starting hyperparameters when ``op``
    has had none (the centres and scales do not depend on them)"""
    if op._kernel is None:
        f, l, mu = FeatureGP.transformed(x0, transform)
        if op.setup(GAUSSIAN, f=f, l=l, mu=mu) != 0:
            raise RuntimeError("the kernel setup failed")


def _gp_fit_exact(L, op, X, lab, x0, steps, lr, beta1, beta2, eps, tol, transform, mask, objective="mll"):
    _set_up_once(op, x0, transform)
    fgp = FeatureGP(op, X, lab)
    adam = L.Nfft4GPOptimizationAdamCreate()
    try:
        fn = "Nfft4GPAmdFeatureGpLoss"
        if objective == "loo":
            fgp.bind(X, lab)
            fn = "Nfft4GPAmdFeatureGpLooLoss"
        if L.Nfft4GPAmdFeatureGpSetOptions(fgp.h, int(transform), mask.ctypes.data if mask is not None else None) or \
                L.Nfft4GPOptimizationAdamSetProblem(adam, _lib.fnptr(fn), fgp.h, 3) or \
                L.Nfft4GPOptimizationAdamSetOptions(adam, steps, float(tol), float(beta1), float(beta2), float(eps),
                                                    float(lr)) or \
                L.Nfft4GPOptimizationAdamInit(adam, x0.ctypes.data):
            raise RuntimeError("the optimiser setup failed")
        flag = 0
        while flag == 0:
            flag = L.Nfft4GPOptimizationAdamStep(adam)
        hyper, loss, gnorm = _adam_histories(adam, steps)
    finally:
        L.Nfft4GPOptimizationAdamFree(adam)
        fgp.free()
    return hyper, loss, gnorm, int(flag)


def gp_model(X, windows, nwindows, dwindows, y, hyper, tol=1e-8, maxits=100, transform=0, op=None, variance=False,
             exact=False, centring=False):
    """The fitted model at the hyperparameters ``hyper`` = (f, l, mu) before the transform: sets the kernel up
    (Gaussian, or the kernel ``op`` was last set up with), solves f^2 (K + mu I) alpha = y with FGMRES on the
    device and returns FittedModel.from_operator(op, alpha).  ``op``: an NFFTAdditiveKernel over X to reuse.
    ``variance=True`` also fits the model's variance matrix on X, so that ``predict_std`` works, and
    ``predict_effects(..., std=True)`` / ``effect_curve(..., std=True)``: each window's term with its standard
    deviation (the terms alone need no variance).
    ``centring=True`` also centres the model on X (FittedModel.fit_centring): ``predict_effects(..., centred=True)``,
    ``intercept`` and ``importance``.
    ``exact=True`` (1-D windows): FeatureGP.model instead -- alpha from the feature-space solve and the variance
    matrix from the same factorisation, no FGMRES (tol, maxits and variance do not apply: S is always loaded)."""
    import torch

    from .solvers import fgmres
    X = np.asarray(X, dtype=np.float64)
    kernel = GAUSSIAN
    if op is None:
        op = NFFTAdditiveKernel(np.asfortranarray(X), windows, nwindows, dwindows)
    elif not isinstance(op, NFFTAdditiveKernel):
        raise TypeError("gp_model runs on an NFFTAdditiveKernel")
    elif op._kernel is not None:
        kernel = op._kernel
    if op.n != X.shape[0] or len(y) != op.n:
        raise ValueError("X, y and op must have the same number of points")
    if exact:
        _set_up_once(op, hyper, transform)
        fgp = FeatureGP(op, X, y)
        try:
            return fgp.model(X, y, hyper, transform=transform, centring=centring)
        finally:
            fgp.free()
    L = _lib.lib()
    t, dt = C.c_double(), C.c_double()
    flm = []
    for v in np.asarray(hyper, dtype=np.float64).ravel()[:3]:
        if L.Nfft4GPTransform(int(transform), float(v), 0, C.byref(t), C.byref(dt)) != 0:
            raise RuntimeError("Nfft4GPTransform failed")
        flm.append(t.value)
    if op.setup(kernel, f=flm[0], l=flm[1], mu=flm[2]) != 0:
        raise RuntimeError("the kernel setup failed")
    b = torch.as_tensor(np.ascontiguousarray(np.asarray(y, dtype=np.float64)), device="cuda")
    alpha = fgmres(op, b, kdim=int(maxits), maxits=int(maxits), tol=float(tol))[0]
    model = FittedModel.from_operator(op, alpha)
    if variance:
        model.fit_variance(X)
    if centring:
        model.fit_centring(X)
    return model

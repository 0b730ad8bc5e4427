"""A fitted additive GP as a table of interpolation polynomials (Nfft4GPAmdModel*, csrc/model.hip).

``FittedModel.from_operator(op, alpha)`` keeps what the operator's matvec builds for alpha = (K + mu I)^-1 y --
nw x 64 x 8 coefficients plus one feature, centre and scale per window -- and ``predict`` evaluates it at new
points: no layout of the new points, no solve and no training data.  1-D windows only; points outside the radius
the training points were scaled to are refused (NaN).  ``fit_variance(X)`` adds the 33 nw x 33 nw matrix S of the
operator's finite-rank form, after which ``predict_std`` gives the predictive standard deviation the same way.
The model is additive, f(x) = sum_c g_c(x_c): ``predict_effects`` gives each window's term and, with ``std=True``,
its posterior standard deviation (S's diagonal blocks), and ``effect_curve`` one window's term along its own feature.
``fit_centring(X)`` keeps the means of the features and of every window's term over the training points: after it
``predict_effects(..., centred=True)`` gives the terms about those means with the std of the centred term (the
shared constant's uncertainty drops out), ``intercept`` the one constant and ``importance`` the windows' ranking.
``draw_paths`` / ``paths`` / ``sample`` give joint draws of the latent function from the same S: a draw is a function,
the same one at every point set it is evaluated at.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_NCELL, _NC = 64, 8  # cells per window, coefficients per cell (csrc/internal.h kNos, kNC)
PATHS_TILE = 128     # sample paths a workgroup of k_model_paths holds at once (csrc/model.hip kMqCols)


class FittedModel:
    def __init__(self, handle: int):
        if not handle:
            raise RuntimeError("no model handle")
        self.h = handle
        nw, d, k = C.c_int(), C.c_int(), C.c_int()
        hyp = (C.c_double * 3)()
        if _lib.lib().Nfft4GPAmdModelInfo(self.h, C.byref(nw), C.byref(d), C.byref(k), hyp) != 0:
            raise RuntimeError("Nfft4GPAmdModelInfo failed")
        self.nw, self.d, self.kernel = nw.value, d.value, k.value
        self.f, self.l, self.mu = hyp[0], hyp[1], hyp[2]

    @classmethod
    def from_operator(cls, op, alpha) -> "FittedModel":
        """The model of a whole-row NFFTAdditiveKernel after its setup(); alpha: numpy or a torch device tensor of
        op.n entries.  The operator may be freed afterwards."""
        from .nfft import _check_len, _ptr
        _check_len("alpha", alpha, op.n)
        h = _lib.lib().Nfft4GPAmdModelCreate(op.h, _ptr(alpha)[0], op.n)
        if not h:
            raise RuntimeError("Nfft4GPAmdModelCreate refused the operator (see stderr)")
        return cls(h)

    @staticmethod
    def _points(Xnew):
        """(X column-major, output array, X pointer, output pointer, ldim, n_new, d) for numpy or a device tensor"""
        if isinstance(Xnew, np.ndarray) or not hasattr(Xnew, "data_ptr"):
            X = np.asfortranarray(np.asarray(Xnew, dtype=np.float64))
            if X.ndim != 2:
                raise ValueError("Xnew must be n_new x d")
            n_new, d = X.shape
            out = np.empty(n_new)
            return X, out, X.ctypes.data, out.ctypes.data, max(n_new, 1), n_new, d
        import torch
        if Xnew.dim() != 2 or Xnew.dtype != torch.float64:
            raise ValueError("Xnew must be an n_new x d float64 tensor")
        n_new, d = Xnew.shape
        X = Xnew.t().contiguous().t()  # column-major storage
        out = torch.empty(n_new, dtype=torch.float64, device=Xnew.device)
        return X, out, X.data_ptr(), out.data_ptr(), max(n_new, 1), n_new, d

    def _outside(self, nout, n_new, strict, what):
        self.n_outside = int(nout.value)
        if strict and self.n_outside:
            raise ValueError(f"{self.n_outside} of {n_new} points lie outside the model's domain (the radius of the "
                             f"training points, per window); {what}(..., strict=False) returns NaN for them")

    def predict(self, Xnew, strict: bool = True):
        """The posterior mean at the rows of Xnew (n_new x d; numpy -> numpy, a torch device tensor -> a device
        tensor).  A point outside the model's domain is NaN; ``strict`` raises ValueError with their count."""
        X, mean, xp, mp, ld, n_new, d = self._points(Xnew)
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the model was fitted on {self.d}")
        nout = C.c_longlong(0)
        rc = _lib.lib().Nfft4GPAmdModelPredict(self.h, xp, int(n_new), int(ld), int(d), mp, C.byref(nout))
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelPredict failed with status {rc}")
        self._outside(nout, n_new, strict, "predict")
        return mean

    @property
    def has_variance(self) -> bool:
        R = C.c_int(0)
        return _lib.lib().Nfft4GPAmdModelVarianceInfo(self.h, C.byref(R)) == 0 and R.value > 0

    def fit_variance(self, X):
        """Build the variance matrix S (33 nw squared) from the training points X (n x d, numpy or a device
        tensor): afterwards ``predict_std`` needs neither X nor a solve.  A row outside the model's domain raises
        ValueError and leaves the model as it was."""
        Xc, _, xp, _, ld, n, d = self._points(X)
        if d != self.d:
            raise ValueError(f"X has {d} columns; the model was fitted on {self.d}")
        rc = _lib.lib().Nfft4GPAmdModelFitVariance(self.h, xp, int(n), int(ld), int(d))
        if rc == -2:
            raise ValueError("rows of X lie outside the model's domain (see stderr); the model is unchanged")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelFitVariance failed with status {rc} (see stderr)")
        self.sampler_defect = None  # the factor of the previous S and its paths went with it
        return self

    # ---- centring on a reference sample (Nfft4GPAmdModelFitCentring / Centring / Intercept) ----
    def fit_centring(self, X):
        """Centre the model on the reference sample X (n x d, numpy or a device tensor; the training points): keeps
        the features' means, every window's effect mean and its standard deviation over the sample.  Afterwards
        ``predict_effects(..., centred=True)``, ``intercept`` and ``importance`` work; ``fit_variance`` keeps the
        centring.  A row outside the model's domain raises ValueError and leaves the model, an earlier centring
        included, as it was."""
        Xc, _, xp, _, ld, n, d = self._points(X)
        if d != self.d:
            raise ValueError(f"X has {d} columns; the model was fitted on {self.d}")
        rc = _lib.lib().Nfft4GPAmdModelFitCentring(self.h, xp, int(n), int(ld), int(d))
        if rc == -2:
            raise ValueError("rows of X lie outside the model's domain (see stderr); the model is unchanged")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelFitCentring failed with status {rc} (see stderr)")
        return self

    def _centring(self):
        """(n_ref, feature_mean, effect_mean, effect_sd), or None when the model holds no centring"""
        n_ref = C.c_int(0)
        fm, em, sd = np.empty(33 * self.nw), np.empty(self.nw), np.empty(self.nw)
        rc = _lib.lib().Nfft4GPAmdModelCentring(self.h, C.byref(n_ref), fm.ctypes.data, em.ctypes.data, sd.ctypes.data)
        if rc == -5:
            return None
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelCentring failed with status {rc}")
        return n_ref.value, fm, em, sd

    def _centring_or_raise(self):
        held = self._centring()
        if held is None:
            raise RuntimeError("the model holds no centring: call fit_centring(X) first")
        return held

    @property
    def has_centring(self) -> bool:
        return _lib.lib().Nfft4GPAmdModelCentring(self.h, None, None, None, None) == 0

    @property
    def feature_mean(self):
        """the 33 nw features' means over the reference sample, in S's feature order (every window's first is 1)"""
        return self._centring_or_raise()[1]

    @property
    def effect_mean(self):
        """every window's mean of its term over the reference sample (nw): what ``centred=True`` subtracts"""
        return self._centring_or_raise()[2]

    @property
    def importance(self):
        """every window's standard deviation of its term over the reference sample (nw), in the units of y: the
        natural ranking of the windows"""
        return self._centring_or_raise()[3]

    def intercept(self, std: bool = False):
        """The model's constant b = sum of ``effect_mean`` (added in window order), so that predict(x) = b + the sum
        of the centred effects; ``std=True`` returns (b, std_b), std_b = sqrt|f^2 m^T S m| the posterior standard
        deviation of the latent function's mean over the reference sample (needs ``fit_variance`` or a loaded S)."""
        b, sb = C.c_double(0.0), C.c_double(0.0)
        rc = _lib.lib().Nfft4GPAmdModelIntercept(self.h, C.byref(b), C.byref(sb) if std else None)
        if rc == -5:
            raise RuntimeError("the model holds no centring: call fit_centring(X) first")
        if rc == -3:
            raise RuntimeError("the model holds no variance: call fit_variance(X) first")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelIntercept failed with status {rc}")
        return (b.value, sb.value) if std else b.value

    def predict_std(self, Xnew, strict: bool = True, noise: bool = True):
        """The predictive standard deviation sqrt|f^2 (mu + phi^T S phi)| at the rows of Xnew, with the conventions
        of ``predict``; ``noise=False`` drops the mu term.  Needs ``fit_variance`` (or a loaded S) first."""
        X, std, xp, sp, ld, n_new, d = self._points(Xnew)
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the model was fitted on {self.d}")
        nout = C.c_longlong(0)
        rc = _lib.lib().Nfft4GPAmdModelPredictStd(self.h, xp, int(n_new), int(ld), int(d), sp, int(bool(noise)),
                                                  C.byref(nout))
        if rc == -3:
            raise RuntimeError("the model holds no variance: call fit_variance(X) first")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelPredictStd failed with status {rc}")
        self._outside(nout, n_new, strict, "predict_std")
        return std

    def predict_effects(self, Xnew, std: bool = False, strict: bool = True, window=None, centred: bool = False):
        """Each window's term of the posterior mean at the rows of Xnew: an (n_new, nw) array whose column c is
        f^2 times window c's table at the point's coordinate feature[c] -- the value ``predict`` adds for that window,
        so the columns sum to ``predict`` up to the rounding of one sum.  numpy gives a Fortran-ordered numpy array, a
        torch device tensor a device tensor (the transpose view of an (nw, n_new) buffer).  ``std=True`` returns the
        pair (effects, effect_std), effect_std[i, c] = sqrt|f^2 phi_c^T S_cc phi_c| the posterior standard deviation
        of window c's term without noise (needs ``fit_variance`` or a loaded S).  ``window=c`` returns 1-D results
        for that window alone and reads only column feature[c].  A (point, window) pair outside the window's domain is
        NaN and leaves the point's other windows as they are; ``n_outside`` counts the points with such a pair among
        the windows asked for and ``strict`` raises on them, as in ``predict``.

        The constant is shared among the windows (each carries 1/nw of it) and the data identify only its sum, so a
        window's raw std includes the constant's uncertainty.  ``centred=True`` (after ``fit_centring``) gives what a
        plot of an additive model shows: column c minus ``effect_mean[c]``, bit for bit, and the std of that centred
        term, sqrt|f^2 (phi_c - m_c)^T S_cc (phi_c - m_c)|, from which the constant's uncertainty has dropped out;
        ``intercept`` holds the one constant."""
        if isinstance(Xnew, np.ndarray) or not hasattr(Xnew, "data_ptr"):
            X = np.asfortranarray(np.asarray(Xnew, dtype=np.float64))
            torch = None
        else:
            import torch
            if Xnew.dtype != torch.float64:
                raise ValueError("Xnew must be an n_new x d float64 tensor")
            X = Xnew.t().contiguous().t() if Xnew.dim() == 2 else Xnew
        if X.ndim != 2:
            raise ValueError("Xnew must be n_new x d")
        n_new, d = X.shape
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the model was fitted on {self.d}")
        w0, wn = (0, self.nw) if window is None else (int(window), 1)
        if not 0 <= w0 < self.nw:
            raise ValueError(f"window must be in [0, {self.nw})")

        def buffer():
            if torch is None:
                a = np.empty((n_new, wn), order="F")
                return a, a.ctypes.data
            b = torch.empty((wn, n_new), dtype=torch.float64, device=Xnew.device)
            return b.t(), b.data_ptr()
        eff, ep = buffer()
        sd, sp = buffer() if std else (None, None)
        nout = C.c_longlong(0)
        xp = X.ctypes.data if torch is None else X.data_ptr()
        L = _lib.lib()
        fn = L.Nfft4GPAmdModelPredictEffectsCentred if centred else L.Nfft4GPAmdModelPredictEffects
        rc = fn(self.h, xp, int(n_new), max(int(n_new), 1), int(d), w0, wn, ep, sp, max(int(n_new), 1), C.byref(nout))
        if rc == -5:
            raise RuntimeError("the model holds no centring: call fit_centring(X) first")
        if rc == -3:
            raise RuntimeError("the model holds no variance: call fit_variance(X) first")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelPredictEffects{'Centred' if centred else ''} failed with status {rc}")
        self._outside(nout, n_new, strict, "predict_effects")
        if window is not None:
            eff, sd = eff[:, 0], (sd[:, 0] if std else None)
        return (eff, sd) if std else eff

    def effect_curve(self, c, values, std: bool = False, centred: bool = False):
        """Window c's term at the given values of its own feature (1-D, numpy or a torch device tensor), for plotting:
        ``predict_effects(X, window=c)`` on an n x d input whose column feature[c] holds the values.  The raw std
        carries the shared constant's uncertainty; ``centred=True`` gives the centred term and its std (see
        ``predict_effects``)."""
        return self.predict_effects(self._curve_points(c, values), std=std, strict=True, window=int(c),
                                    centred=centred)

    def _curve_points(self, c, values):
        """an n x d input (numpy, or a device tensor like ``values``) whose column feature[c] holds the values"""
        c = int(c)
        if not 0 <= c < self.nw:
            raise ValueError(f"window must be in [0, {self.nw})")
        feature = np.empty(self.nw, dtype=np.int32)
        if _lib.lib().Nfft4GPAmdModelCoefficients(self.h, None, None, None, feature.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdModelCoefficients failed")
        if isinstance(values, np.ndarray) or not hasattr(values, "data_ptr"):
            v = np.asarray(values, dtype=np.float64).ravel()
            X = np.zeros((v.size, self.d), order="F")
            X[:, feature[c]] = v
        else:
            import torch
            v = values.reshape(-1)
            X = torch.zeros((self.d, v.numel()), dtype=torch.float64, device=values.device).t()
            X[:, int(feature[c])] = v
        return X

    # ---- joint posterior sample paths (Nfft4GPAmdModelFitSampler / DrawPaths / EvalPaths) ----
    sampler_defect = None  # set by fit_sampler: sum |lambda < 0| / sum |lambda| of S, the share the sampler drops

    def fit_sampler(self):
        """Factor the variance matrix for sampling: S = V Lambda V^T, F = V sqrt(max(Lambda, 0)), so that F F^T is S
        without its negative part (S is not always positive semidefinite: the kernel's Fourier coefficients have
        negative entries at long length scales).  Sets ``sampler_defect`` = sum |lambda < 0| / sum |lambda| and
        ``sampler_eigen_range`` = (lambda_min, lambda_max); issues a RuntimeWarning when lambda_min < -R 2^-52
        lambda_max, i.e. beyond the eigensolver's rounding: the paths' spread then departs from ``predict_std``,
        which keeps the negative part under its absolute value.  Needs ``fit_variance`` (or a loaded S)."""
        info = (C.c_double * 3)()
        rc = _lib.lib().Nfft4GPAmdModelFitSampler(self.h, info)
        if rc == -3:
            raise RuntimeError("the model holds no variance: call fit_variance(X) first")
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelFitSampler failed with status {rc} (see stderr)")
        self.sampler_defect = float(info[0])
        self.sampler_eigen_range = (float(info[1]), float(info[2]))
        R = 33 * self.nw
        if info[1] < -R * 2.0 ** -52 * info[2]:
            import warnings
            warnings.warn(f"the variance matrix S is indefinite: its negative eigenvalues are {self.sampler_defect:.3e} "
                          f"of the sum of |eigenvalues| (lambda_min {info[1]:.3e}, lambda_max {info[2]:.3e}) and the "
                          "sampler drops them, so the spread of the paths departs from predict_std, which keeps the "
                          "negative part under its absolute value", RuntimeWarning, stacklevel=2)
        return self

    @property
    def n_paths(self) -> int:
        """the number of paths held by the model (0 when nothing is drawn)"""
        ns = C.c_int(0)
        if _lib.lib().Nfft4GPAmdModelPathsInfo(self.h, C.byref(ns)) != 0:
            raise RuntimeError("Nfft4GPAmdModelPathsInfo failed")
        return ns.value

    def draw_paths(self, n_paths: int, seed=None, xi=None):
        """Draw ``n_paths`` functions from the joint posterior of the latent function: theta = F xi with xi of
        standard normals, ``numpy.random.default_rng(seed).standard_normal((33 nw, n_paths))`` unless ``xi`` (that
        shape; numpy or a float64 device tensor) is given.  The draw stays in the model until the next one, so
        ``paths`` evaluates the same functions at any number of point sets.  Fits the sampler on first use."""
        n_paths = int(n_paths)
        R = 33 * self.nw
        if n_paths < 1:
            raise ValueError("n_paths must be at least 1")
        if xi is None:
            xi = np.random.default_rng(seed).standard_normal((R, n_paths))
        if isinstance(xi, np.ndarray) or not hasattr(xi, "data_ptr"):
            xi = np.asfortranarray(np.asarray(xi, dtype=np.float64))
            if xi.shape != (R, n_paths):
                raise ValueError(f"xi must be {R} x {n_paths}")
            xp = xi.ctypes.data
        else:
            import torch
            if tuple(xi.shape) != (R, n_paths) or xi.dtype != torch.float64:
                raise ValueError(f"xi must be a {R} x {n_paths} float64 tensor")
            xi = xi.t().contiguous().t()  # column-major storage
            xp = xi.data_ptr()
        L = _lib.lib()
        rc = L.Nfft4GPAmdModelDrawPaths(self.h, xp, n_paths, R)
        if rc in (-3, -4):
            self.fit_sampler()
            rc = L.Nfft4GPAmdModelDrawPaths(self.h, xp, n_paths, R)
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelDrawPaths failed with status {rc}")
        return self

    def paths(self, Xnew, window=None, strict: bool = True):
        """The drawn paths at the rows of Xnew: an (n_new, n_paths) array, column s = predict(Xnew) + f Phi(Xnew) B[:, s]
        -- a draw of the latent function; observation noise is independent N(0, f^2 mu) per point, for the caller to
        add.  numpy gives a Fortran-ordered numpy array, a torch device tensor a device tensor (the transpose view of
        an (n_paths, n_new) buffer).  ``window=c`` gives window c's term of each path around
        ``predict_effects(window=c)`` (only column feature[c] matters); one window's path carries its share of the
        constant and is not centred (``predict_effects(..., centred=True)`` is).  A point outside the domain of a window that is summed is
        NaN in every path; ``n_outside`` and ``strict`` behave as in ``predict_effects``."""
        if isinstance(Xnew, np.ndarray) or not hasattr(Xnew, "data_ptr"):
            X = np.asfortranarray(np.asarray(Xnew, dtype=np.float64))
            torch = None
        else:
            import torch
            if Xnew.dtype != torch.float64:
                raise ValueError("Xnew must be an n_new x d float64 tensor")
            X = Xnew.t().contiguous().t() if Xnew.dim() == 2 else Xnew
        if X.ndim != 2:
            raise ValueError("Xnew must be n_new x d")
        n_new, d = X.shape
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the model was fitted on {self.d}")
        w = -1 if window is None else int(window)
        if window is not None and not 0 <= w < self.nw:
            raise ValueError(f"window must be in [0, {self.nw})")
        ns = self.n_paths
        if ns == 0:
            raise RuntimeError("the model holds no paths: call draw_paths(n_paths) first")
        if torch is None:
            out = np.empty((n_new, ns), order="F")
            op, xp = out.ctypes.data, X.ctypes.data
        else:
            buf = torch.empty((ns, n_new), dtype=torch.float64, device=Xnew.device)
            out, op, xp = buf.t(), buf.data_ptr(), X.data_ptr()
        nout = C.c_longlong(0)
        rc = _lib.lib().Nfft4GPAmdModelEvalPaths(self.h, xp, int(n_new), max(int(n_new), 1), int(d), w, op,
                                                 max(int(n_new), 1), C.byref(nout))
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelEvalPaths failed with status {rc}")
        self._outside(nout, n_new, strict, "paths")
        return out

    def sample(self, Xnew, n_samples: int, seed=None, window=None):
        """``draw_paths(n_samples, seed)`` then ``paths(Xnew, window)``: joint draws of the latent function at Xnew."""
        return self.draw_paths(n_samples, seed=seed).paths(Xnew, window=window)

    def path_curve(self, c, values):
        """Window c's term of every drawn path at the given values of its own feature (1-D, numpy or a torch device
        tensor): ``effect_curve``'s twin, (n, n_paths).  A window's path carries its share of the constant and stays
        uncentred: subtract a path's mean over your own points, or see ``predict_effects(..., centred=True)`` for the
        centred term and its std."""
        return self.paths(self._curve_points(c, values), window=int(c))

    def coefficients(self) -> dict:
        """H (nw x 64 x 8), centre, scale, feature (nw each) and the scalars, as numpy arrays; S when a variance is
        held; feature_mean, effect_mean, effect_sd and n_ref when a centring is."""
        H = np.empty((self.nw, _NCELL, _NC))
        centre, scale = np.empty(self.nw), np.empty(self.nw)
        feature = np.empty(self.nw, dtype=np.int32)
        if _lib.lib().Nfft4GPAmdModelCoefficients(self.h, H.ctypes.data, centre.ctypes.data, scale.ctypes.data,
                                                  feature.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdModelCoefficients failed")
        co = {"H": H, "centre": centre, "scale": scale, "feature": feature, "d": self.d, "kernel": self.kernel,
              "hyper": np.array([self.f, self.l, self.mu])}
        if self.has_variance:
            R = 33 * self.nw
            S = np.empty((R, R))
            if _lib.lib().Nfft4GPAmdModelVariance(self.h, S.ctypes.data) != 0:
                raise RuntimeError("Nfft4GPAmdModelVariance failed")
            co["S"] = S  # features per window: cos 2 pi k xs, k = 0..16, then sin 2 pi k xs, k = 1..16
        held = self._centring()
        if held is not None:
            co["n_ref"], co["feature_mean"], co["effect_mean"], co["effect_sd"] = held
        return co

    @classmethod
    def from_coefficients(cls, H, centre, scale, feature, d, kernel, hyper, S=None, centring=None) -> "FittedModel":
        """``centring``: a dict with ``coefficients()``' keys n_ref, feature_mean, effect_mean and effect_sd."""
        H = np.ascontiguousarray(H, dtype=np.float64)
        centre = np.ascontiguousarray(centre, dtype=np.float64)
        scale = np.ascontiguousarray(scale, dtype=np.float64)
        feature = np.ascontiguousarray(feature, dtype=np.int32)
        hyper = np.ascontiguousarray(hyper, dtype=np.float64)
        nw = centre.size
        if H.size != nw * _NCELL * _NC or scale.size != nw or feature.size != nw or hyper.size != 3:
            raise ValueError("H must hold nw*64*8 values and centre, scale, feature nw each; hyper = (f, l, mu)")
        h = _lib.lib().Nfft4GPAmdModelFromCoefficients(int(nw), int(d), int(kernel), hyper.ctypes.data, H.ctypes.data,
                                                       centre.ctypes.data, scale.ctypes.data, feature.ctypes.data)
        if not h:
            raise RuntimeError("Nfft4GPAmdModelFromCoefficients failed (see stderr)")
        m = cls(h)
        if S is not None:
            S = np.ascontiguousarray(S, dtype=np.float64)
            if S.shape != (33 * nw, 33 * nw):
                raise ValueError("S must be 33 nw x 33 nw")
            if _lib.lib().Nfft4GPAmdModelSetVariance(m.h, S.ctypes.data, int(S.shape[0])) != 0:
                raise RuntimeError("Nfft4GPAmdModelSetVariance failed (see stderr)")
        if centring is not None:
            fm, em, sd = (np.ascontiguousarray(centring[k], dtype=np.float64)
                          for k in ("feature_mean", "effect_mean", "effect_sd"))
            if fm.shape != (33 * nw,) or em.shape != (nw,) or sd.shape != (nw,):
                raise ValueError("centring: feature_mean must hold 33 nw values, effect_mean and effect_sd nw each")
            if _lib.lib().Nfft4GPAmdModelSetCentring(m.h, int(centring["n_ref"]), fm.ctypes.data, em.ctypes.data,
                                                     sd.ctypes.data, int(nw)) != 0:
                raise RuntimeError("Nfft4GPAmdModelSetCentring failed: n_ref >= 1 and every window's first "
                                   "feature_mean exactly 1")
        return m

    def save(self, path):
        """Write the model to an .npz file (numpy.savez appends the suffix when path lacks it)."""
        np.savez(path, **self.coefficients())

    @classmethod
    def load(cls, path) -> "FittedModel":
        with np.load(path) as z:
            centring = None
            if "n_ref" in z.files:
                centring = {k: z[k] for k in ("n_ref", "feature_mean", "effect_mean", "effect_sd")}
            return cls.from_coefficients(z["H"], z["centre"], z["scale"], z["feature"], int(z["d"]),
                                         int(z["kernel"]), z["hyper"], S=z["S"] if "S" in z.files else None,
                                         centring=centring)

    def free(self):
        if getattr(self, "h", None):
            _lib.lib().Nfft4GPAmdModelFree(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

"""A fitted additive GP as a table of interpolation polynomials (Nfft4GPAmdModel*, csrc/model.hip).

``FittedModel.from_operator(op, alpha)`` keeps what the operator's matvec builds for alpha = (K + mu I)^-1 y --
nw x 64 x 8 coefficients plus one feature, centre and scale per window -- and ``predict`` evaluates it at new
points: no layout of the new points, no solve and no training data.  1-D windows only; points outside the radius
the training points were scaled to are refused (NaN).  ``fit_variance(X)`` adds the 33 nw x 33 nw matrix S of the
operator's finite-rank form, after which ``predict_std`` gives the predictive standard deviation the same way.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_NCELL, _NC = 64, 8  # cells per window, coefficients per cell (csrc/internal.h kNos, kNC)


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
        return self

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

    def coefficients(self) -> dict:
        """H (nw x 64 x 8), centre, scale, feature (nw each) and the scalars, as numpy arrays."""
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
        return co

    @classmethod
    def from_coefficients(cls, H, centre, scale, feature, d, kernel, hyper, S=None) -> "FittedModel":
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
        return m

    def save(self, path):
        """Write the model to an .npz file (numpy.savez appends the suffix when path lacks it)."""
        np.savez(path, **self.coefficients())

    @classmethod
    def load(cls, path) -> "FittedModel":
        with np.load(path) as z:
            return cls.from_coefficients(z["H"], z["centre"], z["scale"], z["feature"], int(z["d"]),
                                         int(z["kernel"]), z["hyper"], S=z["S"] if "S" in z.files else None)

    def free(self):
        if getattr(self, "h", None):
            _lib.lib().Nfft4GPAmdModelFree(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

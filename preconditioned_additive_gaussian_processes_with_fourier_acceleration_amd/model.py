"""A fitted additive GP as a table of interpolation polynomials (Nfft4GPAmdModel*, csrc/model.hip).

``FittedModel.from_operator(op, alpha)`` keeps what the operator's matvec builds for alpha = (K + mu I)^-1 y --
nw x 64 x 8 coefficients plus one feature, centre and scale per window -- and ``predict`` evaluates it at new
points: no layout of the new points, no solve and no training data.  1-D windows only; points outside the radius
the training points were scaled to are refused (NaN).
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

    def predict(self, Xnew, strict: bool = True):
        """The posterior mean at the rows of Xnew (n_new x d; numpy -> numpy, a torch device tensor -> a device
        tensor).  A point outside the model's domain is NaN; ``strict`` raises ValueError with their count."""
        if isinstance(Xnew, np.ndarray) or not hasattr(Xnew, "data_ptr"):
            X = np.asfortranarray(np.asarray(Xnew, dtype=np.float64))
            if X.ndim != 2:
                raise ValueError("Xnew must be n_new x d")
            n_new, d = X.shape
            mean = np.empty(n_new)
            xp, mp, ld = X.ctypes.data, mean.ctypes.data, max(n_new, 1)
        else:
            import torch
            if Xnew.dim() != 2 or Xnew.dtype != torch.float64:
                raise ValueError("Xnew must be an n_new x d float64 tensor")
            n_new, d = Xnew.shape
            X = Xnew.t().contiguous().t()  # column-major storage
            mean = torch.empty(n_new, dtype=torch.float64, device=Xnew.device)
            xp, mp, ld = X.data_ptr(), mean.data_ptr(), max(n_new, 1)
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the model was fitted on {self.d}")
        nout = C.c_longlong(0)
        rc = _lib.lib().Nfft4GPAmdModelPredict(self.h, xp, int(n_new), int(ld), int(d), mp, C.byref(nout))
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdModelPredict failed with status {rc}")
        self.n_outside = int(nout.value)
        if strict and self.n_outside:
            raise ValueError(f"{self.n_outside} of {n_new} points lie outside the model's domain (the radius of the "
                             "training points, per window); predict(..., strict=False) returns NaN for them")
        return mean

    def coefficients(self) -> dict:
        """H (nw x 64 x 8), centre, scale, feature (nw each) and the scalars, as numpy arrays."""
        H = np.empty((self.nw, _NCELL, _NC))
        centre, scale = np.empty(self.nw), np.empty(self.nw)
        feature = np.empty(self.nw, dtype=np.int32)
        if _lib.lib().Nfft4GPAmdModelCoefficients(self.h, H.ctypes.data, centre.ctypes.data, scale.ctypes.data,
                                                  feature.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdModelCoefficients failed")
        return {"H": H, "centre": centre, "scale": scale, "feature": feature, "d": self.d, "kernel": self.kernel,
                "hyper": np.array([self.f, self.l, self.mu])}

    @classmethod
    def from_coefficients(cls, H, centre, scale, feature, d, kernel, hyper) -> "FittedModel":
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
        return cls(h)

    def save(self, path):
        """Write the model to an .npz file (numpy.savez appends the suffix when path lacks it)."""
        np.savez(path, **self.coefficients())

    @classmethod
    def load(cls, path) -> "FittedModel":
        with np.load(path) as z:
            return cls.from_coefficients(z["H"], z["centre"], z["scale"], z["feature"], int(z["d"]),
                                         int(z["kernel"]), z["hyper"])

    def free(self):
        if getattr(self, "h", None):
            _lib.lib().Nfft4GPAmdModelFree(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

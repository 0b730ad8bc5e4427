"""The exact GP loss, gradient, solve and variance matrix in feature space (Nfft4GPAmdFeatureGp*, csrc/feature_gp.hip).

With 1-D windows the operator is A = f^2 (Z W Z^T + mu I) with 33 trigonometric features per window, and only the
diagonal W depends on the hyperparameters.  ``FeatureGP(op, X, y)`` forms G = Z^T Z, b = Z^T y and y^T y once; every
``loss``, ``solve``, ``variance`` and ``predict`` after that is 33 nw x 33 nw work: no Krylov iteration, no probe
vectors, no pass over the training points (``solve`` and ``predict`` read the points they are given, once).
``bind(X, y)`` then ``loo`` and ``loo_predict``: the exact leave-one-out loss, its gradient and every training point's
held-out prediction, one pass over the bound points with three R x R quadratic forms each.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from .model import FittedModel


class FeatureGP:
    def __init__(self, op, X, y):
        """``op``: a whole-row NFFTAdditiveKernel with one feature per window, after its setup(); ``X`` (n x d) the
        points it was created over and ``y`` (n) the labels, numpy or torch device tensors."""
        from .nfft import _check_len, _ptr
        Xc, _, xp, _, ld, n, d = FittedModel._points(X)
        y = self._vector(y)
        _check_len("y", y, n)
        self.h = _lib.lib().Nfft4GPAmdFeatureGpCreate(op.h, xp, int(n), int(ld), int(d), _ptr(y)[0])
        if not self.h:
            raise RuntimeError("Nfft4GPAmdFeatureGpCreate refused the operator or the data (see stderr)")
        nn, nw, R, k = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        _lib.lib().Nfft4GPAmdFeatureGpInfo(self.h, C.byref(nn), C.byref(nw), C.byref(R), C.byref(k))
        self.n, self.nw, self.R, self.kernel, self.d = nn.value, nw.value, R.value, k.value, d
        self.op = op
        self.n_outside = 0
        self._bound = None

    @staticmethod
    def _vector(y):
        if hasattr(y, "data_ptr"):
            return y.contiguous()
        return np.ascontiguousarray(np.asarray(y, dtype=np.float64))

    @staticmethod
    def transformed(hyper, transform=0):
        """(f, l, mu) after the transform (0 softplus, 1 sigmoid, 2 exp, 3 identity)"""
        t, dt = C.c_double(), C.c_double()
        out = []
        for v in np.asarray(hyper, dtype=np.float64).ravel()[:3]:
            if _lib.lib().Nfft4GPTransform(int(transform), float(v), 0, C.byref(t), C.byref(dt)) != 0:
                raise RuntimeError("Nfft4GPTransform failed")
            out.append(t.value)
        return out

    def loss(self, hyper, transform=0, mask=None):
        """(loss, grad) at ``hyper`` = (f, l, mu) before the transform: gp_loss's quantities, exact for this
        operator.  ``mask``: 3 ints, 0 zeroes that gradient component."""
        L = _lib.lib()
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.int32))
        if L.Nfft4GPAmdFeatureGpSetOptions(self.h, int(transform), m.ctypes.data if m is not None else None) != 0:
            raise ValueError("unknown transform")
        x = np.ascontiguousarray(np.asarray(hyper, dtype=np.float64))
        if x.size != 3:
            raise ValueError("hyper = (f, l, mu)")
        loss, grad = np.zeros(1), np.zeros(3)
        if L.Nfft4GPAmdFeatureGpLoss(self.h, x.ctypes.data, loss.ctypes.data, grad.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdFeatureGpLoss failed: mu or l not positive after the transform, a zero pivot, "
                               "or a result that is not finite")
        return float(loss[0]), grad

    @property
    def det_sign(self) -> int:
        """the sign of det(mu I + W G) at the last evaluation (the operator is not always definite); 0: none yet"""
        s = C.c_int(0)
        _lib.lib().Nfft4GPAmdFeatureGpStatus(self.h, C.byref(s), None)
        return s.value

    def bind(self, X, y):
        """Bind the data of the constructor for ``loo`` and ``loo_predict`` (the object does not hold X).  numpy
        arrays are copied to the device once; torch device tensors are borrowed and kept alive here.
        ``bind(None, None)`` unbinds."""
        from .nfft import _check_len, _ptr
        L = _lib.lib()
        if X is None:
            L.Nfft4GPAmdFeatureGpLooBind(self.h, None, 0, 0, 0, None)
            self._bound = None
            return
        Xc, _, xp, _, ld, n, d = FittedModel._points(X)
        y = self._vector(y)
        _check_len("y", y, n)
        if L.Nfft4GPAmdFeatureGpLooBind(self.h, xp, int(n), int(ld), int(d), _ptr(y)[0]) != 0:
            self._bound = None
            raise ValueError(f"X must be the {self.n} x {self.d} data the object was created over (see stderr)")
        self._bound = (Xc, y)  # device tensors are borrowed by the library: alive as long as they are bound

    def loo(self, hyper, transform=0, mask=None):
        """(loss, grad) of the leave-one-out objective at ``hyper`` = (f, l, mu) before the transform: the negative
        mean log predictive density of every training point given the others, exact for this operator, with
        ``loss``'s conventions.  Needs ``bind``; ``n_nonpositive`` counts the points whose [A^{-1}]_ii was <= 0."""
        L = _lib.lib()
        m = None if mask is None else np.ascontiguousarray(np.asarray(mask, dtype=np.int32))
        if L.Nfft4GPAmdFeatureGpSetOptions(self.h, int(transform), m.ctypes.data if m is not None else None) != 0:
            raise ValueError("unknown transform")
        x = np.ascontiguousarray(np.asarray(hyper, dtype=np.float64))
        if x.size != 3:
            raise ValueError("hyper = (f, l, mu)")
        loss, grad = np.zeros(1), np.zeros(3)
        if L.Nfft4GPAmdFeatureGpLooLoss(self.h, x.ctypes.data, loss.ctypes.data, grad.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdFeatureGpLooLoss failed: nothing bound, a bound row outside the domain, mu or "
                               "l not positive after the transform, a zero pivot, or a result that is not finite")
        return float(loss[0]), grad

    def loo_predict(self, f, l, mu):
        """(mean, var): what each training point would have been predicted as from the other n - 1, and that
        prediction's variance (of y: with the noise), at the transformed hyperparameters.  numpy when numpy was
        bound, device tensors when torch device tensors were.  A point with [A^{-1}]_ii <= 0 has a negative
        variance; ``n_nonpositive`` counts them."""
        bound = getattr(self, "_bound", None)
        if bound is None:
            raise RuntimeError("no data is bound: FeatureGP.bind(X, y) first")
        if not hasattr(bound[0], "data_ptr"):
            mean, var = np.empty(self.n), np.empty(self.n)
            mp, vp = mean.ctypes.data, var.ctypes.data
        else:
            import torch
            mean, var = (torch.empty(self.n, dtype=torch.float64, device=bound[0].device) for _ in range(2))
            mp, vp = mean.data_ptr(), var.data_ptr()
        if _lib.lib().Nfft4GPAmdFeatureGpLooPredict(self.h, float(f), float(l), float(mu), mp, vp, None) != 0:
            raise RuntimeError("Nfft4GPAmdFeatureGpLooPredict failed (see stderr)")
        return mean, var

    @property
    def n_nonpositive(self) -> int:
        """the number of points with [A^{-1}]_ii <= 0 at the last ``loo`` or ``loo_predict`` (the operator is not
        always definite); they are counted, never folded away"""
        k = C.c_longlong(0)
        _lib.lib().Nfft4GPAmdFeatureGpLooStatus(self.h, C.byref(k))
        return int(k.value)

    def solve(self, X, y, f, l, mu, rhs=None):
        """alpha = A^{-1} y at the transformed hyperparameters; X, y the data of the constructor (numpy -> numpy, a
        torch device X -> a device tensor).  ``rhs``: solve for this right-hand side instead of y (one more pass over
        X forms Z^T rhs)."""
        from .nfft import _check_len, _ptr
        Xc, alpha, xp, ap, ld, n, d = FittedModel._points(X)
        y = self._vector(y if rhs is None else rhs)
        _check_len("y", y, n)
        fn = _lib.lib().Nfft4GPAmdFeatureGpSolve if rhs is None else _lib.lib().Nfft4GPAmdFeatureGpSolveRhs
        rc = fn(self.h, xp, int(n), int(ld), int(d), _ptr(y)[0], float(f), float(l), float(mu), ap)
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdFeatureGpSolve failed with status {rc} (see stderr)")
        return alpha

    def variance(self, f, l, mu):
        """S = mu (mu I + W G)^{-1} W symmetrised, R x R: what FittedModel.fit_variance builds"""
        S = np.empty((self.R, self.R))
        if _lib.lib().Nfft4GPAmdFeatureGpVariance(self.h, float(f), float(l), float(mu), S.ctypes.data) != 0:
            raise RuntimeError("Nfft4GPAmdFeatureGpVariance failed (see stderr)")
        return S

    def predict(self, Xnew, f, l, mu, strict: bool = True):
        """The posterior mean at the rows of Xnew, with FittedModel.predict's conventions"""
        X, mean, xp, mp, ld, n_new, d = FittedModel._points(Xnew)
        if d != self.d:
            raise ValueError(f"Xnew has {d} columns; the object was created on {self.d}")
        nout = C.c_longlong(0)
        rc = _lib.lib().Nfft4GPAmdFeatureGpPredict(self.h, float(f), float(l), float(mu), xp, int(n_new), int(ld),
                                                   int(d), mp, C.byref(nout))
        if rc != 0:
            raise RuntimeError(f"Nfft4GPAmdFeatureGpPredict failed with status {rc}")
        self.n_outside = int(nout.value)
        if strict and self.n_outside:
            raise ValueError(f"{self.n_outside} of {n_new} points lie outside the domain (the radius of the training "
                             f"points, per window); predict(..., strict=False) returns NaN for them")
        return mean

    def moments(self):
        """(G [R, R], b [R], y^T y) on the host"""
        G, b, yy = np.empty((self.R, self.R)), np.empty(self.R), C.c_double()
        if _lib.lib().Nfft4GPAmdFeatureGpMoments(self.h, G.ctypes.data, b.ctypes.data, C.byref(yy)) != 0:
            raise RuntimeError("Nfft4GPAmdFeatureGpMoments failed")
        return G, b, yy.value

    def model(self, X, y, hyper, transform=0, centring=False) -> FittedModel:
        """The fitted model at ``hyper``: sets the operator up there, solves in feature space, and returns
        FittedModel.from_operator(op, alpha) with S loaded -- no Krylov solve and no second Gram.  The model's table
        is the operator's (its matvec differs from the finite-rank form by the NFFT's 1e-8), and a table applied to
        the other form's alpha errs by that difference times |alpha|_1; so alpha takes one step of iterative
        refinement against the operator's own matvec: alpha += A^{-1} (y - op alpha), one matvec and one pass for
        Z^T r.  ``centring=True`` also centres the model on X (FittedModel.fit_centring)."""
        import torch
        f, l, mu = self.transformed(hyper, transform)
        if self.op.setup(self.kernel, f=f, l=l, mu=mu) != 0:
            raise RuntimeError("the kernel setup failed")
        Xd = X if hasattr(X, "data_ptr") else torch.as_tensor(np.asarray(X, dtype=np.float64), device="cuda")
        yd = y if hasattr(y, "data_ptr") else torch.as_tensor(np.asarray(y, dtype=np.float64), device="cuda")
        alpha = self.solve(Xd, yd, f, l, mu)
        alpha = alpha + self.solve(Xd, yd, f, l, mu, rhs=yd - self.op.matsymv(alpha))
        m = FittedModel.from_operator(self.op, alpha)
        S = self.variance(f, l, mu)
        if _lib.lib().Nfft4GPAmdModelSetVariance(m.h, S.ctypes.data, int(self.R)) != 0:
            m.free()
            raise RuntimeError("Nfft4GPAmdModelSetVariance failed (see stderr)")
        if centring:
            m.fit_centring(Xd)
        return m

    def free(self):
        if getattr(self, "h", None):
            _lib.lib().Nfft4GPAmdFeatureGpFree(self.h)
            self.h = None
            self._bound = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

"""Extended-precision references of one Gram-Schmidt sweep, and the error bound the Krylov kernels are held to
(tests/test_gpu_krylov_kernels.py on the device, tests/test_krylov_sweep_ref_host.py on float64 emulations).

Everything is numpy in np.longdouble (64-bit mantissa on x86), written from the definition of the operation, not
from the kernels.  The references are step-consistent: each step is formed from the DEVICE's own earlier
scalars, so the device's rounding does not compound from step to step and one textbook bound holds per quantity.

The bound (u = 2^-53).  A value the device holds after t fused multiply-adds w <- fl(w - h v) differs from the
exact recurrence with the same h by at most gamma_t a_k, where a_k = |w_k| + sum_t |h_t| |v_t,k| bounds every
intermediate.  An inner product of n such values with exact v, summed in ANY order with or without FMAs, adds
at most gamma_n sum_k a_k |v_k| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1: the
constant depends only on the count of operations, not their order).  So with t = j updates behind it

    |h_j dev - h_j ref| <= (n + 2 j + 2) u sum_k a_k |v_j,k|        (a_k for |v_j,k| when h_j is the norm)
    |w_k dev - w_k ref| <= (2 t + 2) u a_k                          after t updates

where 2 j + 2 is generous for the j roundings carried in (the norm carries them twice) plus the second-order
terms of gamma.  The constants come from this count alone; nothing here was fitted to what the kernels give.
"""
import numpy as np

LD = np.longdouble
U = LD(2.0) ** -53
WG = 4096      # elements one workgroup of the one-pass kernels covers (1024 threads x 4)
SLOT = 1024    # elements of one of its four e-slots


def make_inputs(seed, n, m, rows=2):
    """w (n) and `rows` bases of m columns (m, n), random and far from orthonormal: |w_k| in [0.5, 1.5],
    |v_k| in [0.5, 1.5] c_j / sqrt(n) with column scales c_j in [0.5, 2], random signs.  Every inner product
    is O(1), no entry is near zero, so one misaddressed element moves a sum by at least 1 / (8 n^1.5) of
    sum |w| |v| -- against a bound of n u of it."""
    rng = np.random.default_rng(seed)

    def mag(shape):
        return (0.5 + rng.random(shape)) * rng.choice([-1.0, 1.0], size=shape)

    w = mag(n)
    out = [w]
    for _ in range(rows):
        c = 0.5 + 1.5 * rng.random((max(m, 1), 1))
        out.append(mag((max(m, 1), n)) * c / np.sqrt(n))
    return out


def _ratio(err, bound):
    """max err / bound; a non-finite error, or any error over a zero bound, is inf"""
    err = np.atleast_1d(np.asarray(err, dtype=LD))
    bound = np.atleast_1d(np.asarray(bound, dtype=LD))
    if not np.all(np.isfinite(err)):
        return float("inf")
    r = np.zeros(err.shape, dtype=LD)
    pos = bound > 0
    r[pos] = err[pos] / bound[pos]
    r[(~pos) & (err > 0)] = np.inf
    return float(r.max()) if r.size else 0.0


def mgs_ratios(w, V, i, h_dev, w_dev):
    """The MGS sweep of w (n) against V[0..i) ((i, n) rows), then ||w||^2: h_dev[0..i], w_dev from the device.
    Returns (worst |h_dev - h_ref| / bound, worst |w_dev - w_ref| / bound)."""
    n = w.shape[0]
    wl = w.astype(LD)
    a = np.abs(wl)
    hd = np.asarray(h_dev, dtype=LD)
    rh = 0.0
    for j in range(i + 1):
        if j > 0:
            vp = V[j - 1].astype(LD)
            wl = wl - hd[j - 1] * vp
            a = a + np.abs(hd[j - 1]) * np.abs(vp)
        if j < i:
            vj = V[j].astype(LD)
            ref = np.sum(wl * vj)
            bound = (n + 2 * j + 2) * U * np.sum(a * np.abs(vj))
        else:
            ref = np.sum(wl * wl)
            bound = (n + 2 * j + 2) * U * np.sum(a * a)
        rh = max(rh, _ratio(np.abs(hd[j] - ref), bound))
    rw = _ratio(np.abs(np.asarray(w_dev, dtype=LD) - wl), (2 * i + 2) * U * a)
    return rh, rw


class ClassicalRef:
    """One classical pass from the incoming w: h[0..m) = V^T w, h[m + 1] = ||w||^2 before, w -= Z h with the
    device's h, h[m] = ||w||^2 after.  `carried`: roundings w already carries (CGS2's second pass: a0 and the
    count from the first), a0 their magnitude bound."""

    def __init__(self, w, V, Z, m, a0=None, carried=0):
        self.n = w.shape[0]
        self.m = m
        self.wl = np.asarray(w, dtype=LD)
        self.a0 = np.abs(self.wl) if a0 is None else a0
        self.t0 = carried
        Vl = V[:m].astype(LD)
        self.Zl = Vl if Z is V else Z[:m].astype(LD)
        self.absZ = np.abs(self.Zl)
        self.proj = Vl @ self.wl
        self.proj_bound = (self.n + 2 * carried + 2) * U * (np.abs(Vl) @ self.a0)
        self.before = np.sum(self.wl * self.wl)
        self.before_bound = (self.n + 2 * carried + 2) * U * np.sum(self.a0 * self.a0)

    def update(self, h_dev):
        """(w_ref, a, t): the update with the device's projections, its magnitude bound and rounding count"""
        hd = np.asarray(h_dev[:self.m], dtype=LD)
        wl = self.wl - hd @ self.Zl
        a = self.a0 + np.abs(hd) @ self.absZ
        return wl, a, self.t0 + self.m

    def ratios(self, h_dev, w_dev, with_norm=True):
        """worst ratio over the projections (and the norm before), over w, and of the norm after"""
        hd = np.asarray(h_dev, dtype=LD)
        m = self.m
        rp = _ratio(np.abs(hd[:m] - self.proj), self.proj_bound)
        if with_norm:
            rp = max(rp, _ratio(np.abs(hd[m + 1] - self.before), self.before_bound))
        wl, a, t = self.update(h_dev)
        rw = _ratio(np.abs(np.asarray(w_dev, dtype=LD) - wl), (2 * t + 2) * U * a)
        rn = _ratio(np.abs(hd[m] - np.sum(wl * wl)), (self.n + 2 * t + 2) * U * np.sum(a * a))
        return rp, rw, rn


def cgs2_ratios(w, V, m, h_dev, w_dev):
    """Ctx::block_cgs2's layout: h[0..m) pass 1, h[m] after it, h[m + 1] before it, h[m + 2 .. 2m + 2) pass 2,
    h[2m + 2] after pass 2, h[2m + 3] the decision.  Returns (decision of the reference, distance of the
    reference's norm ratio from the 0.7071 gate, worst ratio of pass 1's scalars, of pass 2's scalars (0 when
    skipped), of w)."""
    hd = np.asarray(h_dev, dtype=LD)
    p1 = ClassicalRef(w, V, V, m)
    w1, a1, t1 = p1.update(hd)
    rp, _, rn = p1.ratios(hd, np.asarray(w1, dtype=np.float64))  # w after pass 1 is seen only when pass 2 is skipped
    after = np.sum(w1 * w1)
    q = float(np.sqrt(after) / np.sqrt(p1.before))
    again = q < 0.7071
    r1 = max(rp, rn)
    if not again:
        rw = _ratio(np.abs(np.asarray(w_dev, dtype=LD) - w1), (2 * t1 + 2) * U * a1)
        return 0, q, r1, 0.0, rw
    p2 = ClassicalRef(w1, V, V, m, a0=a1, carried=t1)
    rp2, rw, rn2 = p2.ratios(hd[m + 2:], w_dev, with_norm=False)
    return 1, q, r1, max(rp2, rn2), rw


# ---- float64 emulations of the one-pass MGS sweep, for the host-only test of the check itself -----------------

MUTANTS = ("drop_last", "skip_slot", "stale_h", "norm_early", "double_partial")


def emulate_mgs(w, V, i, mutant=None):
    """What a one-pass MGS kernel computes, in float64: workgroup g sums its 4096 elements, the partials are added
    in workgroup order.  mutant: None (correct) or one of MUTANTS --
      drop_last       the last element takes no part (a bound `k < n - 1`)
      skip_slot       the last workgroup's first 1024-element slot takes no part
      stale_h         step j updates with h_{j-2} (j >= 2)
      norm_early      the norm is taken before the last update
      double_partial  the last workgroup's partial is counted twice
    Returns (h[0..i], w)."""
    n = w.shape[0]
    wv = w.astype(np.float64).copy()
    live = np.ones(n, dtype=bool)
    if mutant == "drop_last":
        live[n - 1] = False
    G = (n + WG - 1) // WG
    if mutant == "skip_slot":
        live[(G - 1) * WG:min(n, (G - 1) * WG + SLOT)] = False
    h = np.zeros(i + 1)

    def total(x):
        part = [float(np.sum(x[g * WG:(g + 1) * WG])) for g in range(G)]
        if mutant == "double_partial":
            part.append(part[-1])
        t = 0.0
        for p in part:
            t += p
        return t

    for j in range(i + 1):
        if j > 0 and not (mutant == "norm_early" and j == i):
            hp = h[j - 2] if (mutant == "stale_h" and j >= 2) else h[j - 1]
            wv[live] = wv[live] - hp * V[j - 1][live]
        x = wv * (V[j] if j < i else wv)
        h[j] = total(np.where(live, x, 0.0))
        if mutant == "norm_early" and j == i and i > 0:
            wv[live] = wv[live] - h[i - 1] * V[i - 1][live]
    return h, wv

"""Timing of the feature-space GP (FeatureGP, csrc/feature_gp.hip), hipEvents on the library stream, medians after
warm-up, at config C's shapes (n = 1e6, 32 one-feature windows, Gaussian, (f, l, mu) = (1, 0.1, 0.01), the bench's
loss leg's labels):

  1. create: the moments G = Z^T Z, b = Z^T y, y^T y from device arrays;
  2. one loss-plus-gradient evaluation (l moved by 1e-6 per call, so that every call factors anew);
  3. solve and predict of n_new = 1e6 points at hyperparameters whose factor the object already holds (what follows
     a loss evaluation at them), device pointers;
  4. FeatureGP.model, wall clock (setup of the operator, solve, one refinement step, table, S);
  5. the leave-one-out leg: Nfft4GPAmdFeatureGpLooLoss (l moved per call as in 2, so every call factors anew) and
     Nfft4GPAmdFeatureGpLooPredict with device outputs (the factor held), over the bound training points;
  6. in the same run, gp_loss at the bench's settings (50 Lanczos steps x 10 probes, tol 1e-6) on the same data and
     operator: the yardstick, wall clock as the bench measures it, and its value beside the exact one.

    python tools/feature_gp_probe.py [--n 1000000 --nw 32 --nnew 1000000 --reps 10 --out FILE.json]
"""
import argparse
import contextlib
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nw", type=int, default=32)
    ap.add_argument("--nnew", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    L = amd.lib()
    rng = np.random.default_rng(906)
    n, nw, nnew = a.n, a.nw, a.nnew
    f, l, mu = 1.0, 0.1, 0.01
    X = np.asfortranarray(rng.random((n, nw)))
    y = rng.random(n) - 0.5
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((nnew, nw))
    win = np.arange(nw, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, nw, 1)
    assert op.setup(amd.GAUSSIAN, f, l, mu) == 0

    def timed(fn, reps, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return statistics.median(ms), min(ms)

    res = {"n": n, "nw": nw, "n_new": nnew, "R": 33 * nw, "reps": a.reps, "hyper": [f, l, mu]}
    Xt = torch.tensor(np.ascontiguousarray(X.T), device="cuda")  # [d][n]: column-major n x d
    yd = torch.tensor(y, device="cuda")

    def create():
        h = L.Nfft4GPAmdFeatureGpCreate(op.h, Xt.data_ptr(), n, n, nw, yd.data_ptr())
        assert h
        L.Nfft4GPAmdFeatureGpFree(h)
    res["create_ms"], res["create_min_ms"] = timed(create, max(3, a.reps // 2), warm=1)

    fgp = amd.FeatureGP(op, Xt.t(), yd)
    calls = [0]

    def loss():
        calls[0] += 1
        return fgp.loss((f, l + 1e-6 * calls[0], mu), transform=3)
    res["loss_grad_ms"], res["loss_grad_min_ms"] = timed(loss, a.reps)
    exact_loss, exact_grad = fgp.loss((f, l, mu), transform=3)
    res["loss"], res["grad"], res["det_sign"] = exact_loss, [float(g) for g in exact_grad], fgp.det_sign

    alpha = torch.empty(n, dtype=torch.float64, device="cuda")

    def solve():
        assert L.Nfft4GPAmdFeatureGpSolve(fgp.h, Xt.data_ptr(), n, n, nw, yd.data_ptr(), f, l, mu, alpha.data_ptr()) == 0
    res["solve_ms"], res["solve_min_ms"] = timed(solve, a.reps)
    r = yd - op.matsymv(alpha)
    res["solve_residual_against_the_operator"] = float(r.abs().max() / yd.abs().max())

    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, Xt.data_ptr(), n, n, nw, yd.data_ptr()) == 0

    def loo_loss():
        calls[0] += 1
        return fgp.loo((f, l + 1e-6 * calls[0], mu), transform=3)
    res["loo_loss_ms"], res["loo_loss_min_ms"] = timed(loo_loss, a.reps)
    loo, loo_grad = fgp.loo((f, l, mu), transform=3)
    res["loo_loss"], res["loo_grad"], res["loo_nonpositive"] = loo, [float(g) for g in loo_grad], fgp.n_nonpositive
    lmean, lvar = (torch.empty(n, dtype=torch.float64, device="cuda") for _ in range(2))

    def loo_predict():
        assert L.Nfft4GPAmdFeatureGpLooPredict(fgp.h, f, l, mu, lmean.data_ptr(), lvar.data_ptr(), None) == 0
    res["loo_predict_ms"], res["loo_predict_min_ms"] = timed(loo_predict, a.reps)
    res["loo_rmse"] = float(torch.sqrt(torch.mean((lmean - yd) ** 2)))
    assert L.Nfft4GPAmdFeatureGpLooBind(fgp.h, None, 0, 0, 0, None) == 0
    del lmean, lvar

    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")
    mean = torch.empty(nnew, dtype=torch.float64, device="cuda")

    def predict():
        assert L.Nfft4GPAmdFeatureGpPredict(fgp.h, f, l, mu, Xd.data_ptr(), nnew, nnew, nw, mean.data_ptr(), None) == 0
    res["predict_ms"], res["predict_min_ms"] = timed(predict, a.reps)
    res["predict_us_per_point"] = res["predict_ms"] * 1e3 / nnew
    del Xd, mean

    wall = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        m = fgp.model(Xt.t(), yd, (f, l, mu), transform=3)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        m.free()
    res["model_wall_ms"] = statistics.median(wall[1:])

    R = torch.tensor(np.where(rng.random((10, n)) < 0.5, -1.0, 1.0), device="cuda")  # probe-major
    wall, kl, kg = [], None, None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with contextlib.redirect_stdout(sys.stderr):
            kl, kg = amd.gp_loss(X, win, nw, 1, y, (f, l, mu), maxits=50, nvecs=10, rademacher=R, tol=1e-6, transform=3,
                                 op=op)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["gp_loss_wall_ms"] = statistics.median(wall[1:])
    res["gp_loss"], res["gp_loss_grad"] = kl, [float(g) for g in kg]
    fgp.free()
    op.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()

"""Timing of the fitted model's predictive standard deviation, hipEvents on the library stream, medians after warm-up.

At config C's shapes (n = 1e6, 32 one-feature windows, n_new = 1e6; the model is built from centres and scales
alone, the fit does not touch an operator):

  1. Nfft4GPAmdModelFitVariance, split by the library's own clock into features / Grams / system + LU;
  2. Nfft4GPAmdModelPredictStd, device pointers, no outside count, against the fp64 matrix peak (78.6 TF) counted
     at n_new R^2 flops, R = 33 nw (half of 2 n_new R^2: the kernel uses S's symmetry).

With --parent, at n = 2e5, 16 windows, 32 points: the only route without a model, gp_predict(with_std=True) (a joint
handle over [X; Xnew] and one FGMRES solve per point), wall clock per point, and predict_std at the same shape.

    python tools/model_std_probe.py [--n 1000000 --nw 32 --nnew 1000000 --reps 10 --parent --out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd  # noqa: E402

PEAK_F64_MATRIX = 78.6e12


def synthetic_model(X, f, l, mu):
    """a model with the setup's centres and scales (mean, radius 1/4) and an empty table: enough for the variance"""
    nw = X.shape[1]
    centre = X.mean(axis=0)
    scale = 0.25 / np.abs(X - centre).max(axis=0)
    return amd.FittedModel.from_coefficients(np.zeros((nw, 64, 8)), centre, scale, np.arange(nw, dtype=np.int32), nw,
                                             amd.GAUSSIAN, [f, l, mu])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nw", type=int, default=32)
    ap.add_argument("--nnew", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parent", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    L = amd.lib()
    rng = np.random.default_rng(906)
    n, nw, nnew = a.n, a.nw, a.nnew
    X = rng.random((n, nw))
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xnew = lo + (hi - lo) * rng.random((nnew, nw))

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

    res = {"n": n, "nw": nw, "n_new": nnew, "R": 33 * nw, "reps": a.reps}
    model = synthetic_model(X, 1.0, 0.3, 0.01)
    Xt = torch.tensor(np.ascontiguousarray(X.T), device="cuda")  # [d][n]: column-major n x d
    parts = []

    def fit():
        assert L.Nfft4GPAmdModelFitVariance(model.h, Xt.data_ptr(), n, n, nw) == 0
        ms3 = (C.c_double * 3)()
        assert L.Nfft4GPAmdModelFitTimes(model.h, ms3) == 0
        parts.append(tuple(ms3))
    res["fit_ms"], res["fit_min_ms"] = timed(fit, max(3, a.reps // 2), warm=1)
    parts = parts[1:]
    for i, name in enumerate(("fit_features_ms", "fit_gram_ms", "fit_lu_ms")):
        res[name] = statistics.median(p[i] for p in parts)
    del Xt

    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")
    std = torch.empty(nnew, dtype=torch.float64, device="cuda")

    def serve():
        assert L.Nfft4GPAmdModelPredictStd(model.h, Xd.data_ptr(), nnew, nnew, nw, std.data_ptr(), 1, None) == 0
    med, best = timed(serve, a.reps)
    flops = nnew * (33.0 * nw) ** 2
    res["predict_std_ms"], res["predict_std_min_ms"] = med, best
    res["predict_std_us_per_point"] = med * 1e3 / nnew
    res["predict_std_fraction_of_f64_matrix_peak"] = flops / (med * 1e-3) / PEAK_F64_MATRIX
    res["std_range"] = [float(std.min()), float(std.max())]
    model.free()
    del Xd, std

    if a.parent:
        pn, pnw, pts = 200_000, 16, 32
        Xs = rng.random((pn, pnw))
        y = np.sin(6 * Xs).sum(1) + 0.05 * rng.standard_normal(pn)
        plo, phi = Xs.min(axis=0), Xs.max(axis=0)
        Xp = plo + (phi - plo) * rng.random((pts, pnw))
        win = np.arange(pnw, dtype=np.int32)
        hyper = np.array([1.0, 0.3, 0.01])
        wall = []
        for i in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            _, s_ref = amd.gp_predict(Xs, Xp, win, pnw, 1, y, hyper, maxits=200, tol=1e-8, transform=3, with_std=True)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            _, _ = amd.gp_predict(Xs, Xp, win, pnw, 1, y, hyper, maxits=200, tol=1e-8, transform=3)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            if i:
                wall.append(((t1 - t0) - (t2 - t1)) * 1e3 / pts)  # the std's share: with minus without
        res["parent_shape"] = {"n": pn, "nw": pnw, "points": pts}
        res["parent_gp_predict_std_ms_per_point"] = statistics.median(wall)
        m2 = synthetic_model(Xs, 1.0, 0.3, 0.01)
        m2.fit_variance(Xs)
        Xpd = torch.tensor(np.ascontiguousarray(Xp.T), device="cuda")
        sd = torch.empty(pts, dtype=torch.float64, device="cuda")

        def serve32():
            assert L.Nfft4GPAmdModelPredictStd(m2.h, Xpd.data_ptr(), pts, pts, pnw, sd.data_ptr(), 1, None) == 0
        med32, _ = timed(serve32, 20)
        res["model_predict_std_ms_per_point_same_shape"] = med32 / pts
        res["model_vs_parent_max_rel_std"] = float(np.max(np.abs(sd.cpu().numpy() - s_ref) / s_ref))
        m2.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

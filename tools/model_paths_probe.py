"""Timing of the fitted model's sample paths, hipEvents on the library stream, medians after warm-up.

At n_new = 1e6 and 32 one-feature windows (the model is built from centres and scales alone and its S fitted on n
training points), for ns = 1, 16, 64 and 256 paths:

  1. Nfft4GPAmdModelFitSampler (once per window count in --fit-nw: wall clock of the call and the library's own clock
     of the eigendecomposition);
  2. Nfft4GPAmdModelDrawPaths, xi on the device;
  3. Nfft4GPAmdModelEvalPaths, device pointers, no outside count: k_model_predict into a scratch vector, then
     k_model_paths; against the fp64 matrix peak (78.6 TF) counted at 2 n_new R_p ns flops, R_p = 36 nw.

The call allocates its scratch (the mean) inside the timed region, as a caller sees it.  The composed route that this
probe once timed next to it (k_model_features into a chunk of Z, Z B on gemm_f64 and an add of the mean) lost at every
count and was removed; its numbers are in profiles/model_paths_probe.json.

    python tools/model_paths_probe.py [--n 200000 --nw 32 --nnew 1000000 --reps 10 --fit-nw 32 64 --out FILE.json]
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
    """a model with the setup's centres and scales (mean, radius 1/4) and an empty table: the mean is 0"""
    nw = X.shape[1]
    centre = X.mean(axis=0)
    scale = 0.25 / np.abs(X - centre).max(axis=0)
    return amd.FittedModel.from_coefficients(np.zeros((nw, 64, 8)), centre, scale, np.arange(nw, dtype=np.int32), nw,
                                             amd.GAUSSIAN, [f, l, mu])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200_000)
    ap.add_argument("--nw", type=int, default=32)
    ap.add_argument("--nnew", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ns", type=int, nargs="+", default=[1, 16, 64, 256])
    ap.add_argument("--fit-nw", type=int, nargs="+", default=[32, 64])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available()
    L = amd.lib()
    rng = np.random.default_rng(906)
    n, nw, nnew = a.n, a.nw, a.nnew

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

    res = {"n": n, "nw": nw, "n_new": nnew, "R": 33 * nw, "reps": a.reps, "sampler_fit": [], "paths": []}
    model = None
    for fnw in sorted(set(a.fit_nw) | {nw}):
        X = rng.random((n, fnw))
        m = synthetic_model(X, 1.0, 0.1, 0.01)
        m.fit_variance(X)
        wall, inner = [], []
        for _ in range(4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            info = (C.c_double * 3)()
            assert L.Nfft4GPAmdModelFitSampler(m.h, info) == 0
            wall.append((time.perf_counter() - t0) * 1e3)
            ms = C.c_double(0.0)
            assert L.Nfft4GPAmdModelSamplerFitTime(m.h, C.byref(ms)) == 0
            inner.append(ms.value)
        res["sampler_fit"].append({"nw": fnw, "R": 33 * fnw, "fit_sampler_ms": statistics.median(wall[1:]),
                                   "eigendecomposition_ms": statistics.median(inner[1:]), "first_call_ms": wall[0],
                                   "defect": info[0], "lambda_min": info[1], "lambda_max": info[2]})
        if fnw == nw:
            model, lo, hi = m, X.min(axis=0), X.max(axis=0)
        else:
            m.free()
        del X
    Xnew = lo + (hi - lo) * rng.random((nnew, nw))
    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")  # [d][n_new]: column-major n_new x d
    del Xnew
    R, Rp = 33 * nw, 36 * ((nw + 3) // 4 * 4)
    for ns in a.ns:
        xi = torch.tensor(rng.standard_normal((ns, R)), device="cuda")  # [ns][R]: column-major R x ns
        out = torch.empty((ns, nnew), dtype=torch.float64, device="cuda")
        row = {"ns": ns}

        def draw():
            assert L.Nfft4GPAmdModelDrawPaths(model.h, xi.data_ptr(), ns, R) == 0
        row["draw_paths_ms"], _ = timed(draw, a.reps)

        def fused():
            assert L.Nfft4GPAmdModelEvalPaths(model.h, Xd.data_ptr(), nnew, nnew, nw, -1, out.data_ptr(), nnew, None) == 0

        f1, _ = timed(fused, a.reps)
        f2, fbest = timed(fused, a.reps)
        row["eval_paths_ms"], row["eval_paths_min_ms"] = min(f1, f2), fbest
        row["eval_paths_medians_ms"] = [f1, f2]
        row["eval_paths_fraction_of_f64_matrix_peak"] = 2.0 * nnew * Rp * ns / (row["eval_paths_ms"] * 1e-3) / PEAK_F64_MATRIX
        row["output_GB"] = 8e-9 * nnew * ns
        row["max_abs_value"] = float(out.abs().max())
        res["paths"].append(row)
        del xi, out
    model.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

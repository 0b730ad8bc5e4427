"""Timing of the fitted model's per-window effects, hipEvents on the library stream, medians after warm-up.

At config C's serving shape (n_new = 1e6, 32 one-feature windows, device pointers, no outside count; the model has a
random table on the setup's centres and scales and a variance fitted on --n training points), in one run:

  1. Nfft4GPAmdModelPredict (k_model_predict), with the bytes it must move: the coordinates once and the mean;
  2. Nfft4GPAmdModelPredictEffects, effects only: the coordinates once and one n_new x nw array;
  3. the same with effect_std: two arrays, and 2 * 594 flops per (point, window) against the fp64 vector peak;
  4. the only route to the same numbers without the entry point: nw one-window models built with from_coefficients
     from H_c and S_cc, each calling Nfft4GPAmdModelPredict and Nfft4GPAmdModelPredictStd (no noise); the values of
     the two routes are compared (the means bit for bit).

    python tools/model_effects_probe.py [--n 20000 --nw 32 --nnew 1000000 --reps 20 --out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd  # noqa: E402

PEAK_F64_VECTOR = 78.6e12
QUAD_FLOPS = 2 * (561 + 33)  # per (point, window): 561 FMAs over the upper triangle, 33 closing FMAs


def probe_model(rng, X, f, l, mu):
    """the setup's centres and scales (mean, radius 1/4), a random table, S fitted on X"""
    nw = X.shape[1]
    centre = X.mean(axis=0)
    scale = 0.25 / np.abs(X - centre).max(axis=0)
    H = rng.standard_normal((nw, 64, 8)) * 2.0 ** (-32.0 * np.arange(8))  # polynomials in s = 2^32 x the offset
    m = amd.FittedModel.from_coefficients(H, centre, scale, np.arange(nw, dtype=np.int32), nw, amd.GAUSSIAN,
                                          [f, l, mu])
    return m.fit_variance(X)


def timed(torch, fn, reps, warm=3):
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--nw", type=int, default=32)
    ap.add_argument("--nnew", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
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
    model = probe_model(rng, X, 1.3, 0.3, 0.01)
    co = model.coefficients()
    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")  # [d][n_new]: column-major n_new x d
    mean = torch.empty(nnew, dtype=torch.float64, device="cuda")
    eff = torch.empty((nw, nnew), dtype=torch.float64, device="cuda")
    esd = torch.empty((nw, nnew), dtype=torch.float64, device="cuda")
    res = {"n": n, "nw": nw, "n_new": nnew, "reps": a.reps}
    col = 8.0 * nnew * nw  # one n_new x nw array of doubles

    def predict():
        assert L.Nfft4GPAmdModelPredict(model.h, Xd.data_ptr(), nnew, nnew, nw, mean.data_ptr(), None) == 0

    def effects():
        assert L.Nfft4GPAmdModelPredictEffects(model.h, Xd.data_ptr(), nnew, nnew, nw, 0, nw, eff.data_ptr(), None,
                                               nnew, None) == 0

    def effects_std():
        assert L.Nfft4GPAmdModelPredictEffects(model.h, Xd.data_ptr(), nnew, nnew, nw, 0, nw, eff.data_ptr(),
                                               esd.data_ptr(), nnew, None) == 0

    for name, fn, nbytes in (("predict", predict, col + 8.0 * nnew), ("effects", effects, 2 * col),
                             ("effects_std", effects_std, 3 * col)):
        med, best = timed(torch, fn, a.reps)
        res[name + "_ms"], res[name + "_min_ms"] = med, best
        res[name + "_bytes"] = nbytes
        res[name + "_TB_per_s"] = nbytes / (med * 1e-3) / 1e12
    res["effects_std_fraction_of_f64_vector_peak"] = (QUAD_FLOPS * float(nnew) * nw / (res["effects_std_ms"] * 1e-3)
                                                      / PEAK_F64_VECTOR)

    # the composed route: one model per window, two calls each
    ones = [amd.FittedModel.from_coefficients(co["H"][c:c + 1], co["centre"][c:c + 1], co["scale"][c:c + 1],
                                              co["feature"][c:c + 1], nw, amd.GAUSSIAN, co["hyper"],
                                              S=co["S"][33 * c:33 * c + 33, 33 * c:33 * c + 33]) for c in range(nw)]
    ceff, csd = torch.empty_like(eff), torch.empty_like(esd)

    def composed_mean():
        for c, m1 in enumerate(ones):
            assert L.Nfft4GPAmdModelPredict(m1.h, Xd.data_ptr(), nnew, nnew, nw, ceff[c].data_ptr(), None) == 0

    def composed():
        composed_mean()
        for c, m1 in enumerate(ones):
            assert L.Nfft4GPAmdModelPredictStd(m1.h, Xd.data_ptr(), nnew, nnew, nw, csd[c].data_ptr(), 0, None) == 0

    res["composed_mean_ms"], res["composed_mean_min_ms"] = timed(torch, composed_mean, max(3, a.reps // 4), warm=1)
    res["composed_ms"], res["composed_min_ms"] = timed(torch, composed, max(3, a.reps // 4), warm=1)
    res["composed_over_effects_std"] = res["composed_ms"] / res["effects_std_ms"]
    res["composed_mean_over_effects"] = res["composed_mean_ms"] / res["effects_ms"]
    res["means_bitwise_equal"] = bool(torch.equal(ceff, eff))
    res["max_abs_std_difference"] = float((csd - esd).abs().max())
    res["effect_std_range"] = [float(esd.min()), float(esd.max())]
    for m1 in ones:
        m1.free()
    model.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

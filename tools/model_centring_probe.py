"""Timing of the fitted model's centring, hipEvents on the library stream, medians after warm-up.

At config C's serving shape (n_new = 1e6, 32 one-feature windows, device pointers, no outside count; the model has a
random table on the setup's centres and scales and a variance fitted on --n training points), in one process:

  1. Nfft4GPAmdModelFitCentring on the n_new points as the reference sample: the outside count, Z^T 1 and the two
     passes of k_model_effect_moments;
  2. the four serving passes in alternation, round after round: uncentred effects, centred effects, uncentred with
     std, centred with std, and the uncentred pass with std a second time.  The two uncentred std timings of a round
     run the same code: their medians' distance is the run's noise, and a centred / uncentred difference below it is
     not a difference;
  3. Nfft4GPAmdModelIntercept with its std (m^T S m once per call).

The centred values are compared with the uncentred ones minus effect_mean (bit for bit).

    python tools/model_centring_probe.py [--n 20000 --nw 32 --nnew 1000000 --rounds 20 --out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd  # noqa: E402
from model_effects_probe import PEAK_F64_VECTOR, QUAD_FLOPS, probe_model  # noqa: E402


def once(torch, fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=20_000)
    ap.add_argument("--nw", type=int, default=32)
    ap.add_argument("--nnew", type=int, default=1_000_000)
    ap.add_argument("--rounds", type=int, default=20)
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
    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")  # [d][n_new]: column-major n_new x d
    eff = torch.empty((nw, nnew), dtype=torch.float64, device="cuda")
    esd = torch.empty((nw, nnew), dtype=torch.float64, device="cuda")
    ceff, csd = torch.empty_like(eff), torch.empty_like(esd)
    res = {"n": n, "nw": nw, "n_new": nnew, "rounds": a.rounds}

    def fit():
        assert L.Nfft4GPAmdModelFitCentring(model.h, Xd.data_ptr(), nnew, nnew, nw) == 0

    def serve(centred, std):
        fn = L.Nfft4GPAmdModelPredictEffectsCentred if centred else L.Nfft4GPAmdModelPredictEffects
        e, s = (ceff, csd) if centred else (eff, esd)

        def call():
            assert fn(model.h, Xd.data_ptr(), nnew, nnew, nw, 0, nw, e.data_ptr(), s.data_ptr() if std else None, nnew,
                      None) == 0
        return call

    b, sb = C.c_double(), C.c_double()

    def intercept():
        assert L.Nfft4GPAmdModelIntercept(model.h, C.byref(b), C.byref(sb)) == 0

    for _ in range(2):
        fit()
    torch.cuda.synchronize()
    ms = [once(torch, fit) for _ in range(max(3, a.rounds // 2))]
    res["fit_centring_ms"], res["fit_centring_min_ms"] = statistics.median(ms), min(ms)
    passes = {"effects": serve(False, False), "effects_centred": serve(True, False),
              "effects_std": serve(False, True), "effects_std_centred": serve(True, True),
              "effects_std_again": serve(False, True)}
    for fn in passes.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name in passes}
    for _ in range(a.rounds):
        for name, fn in passes.items():
            times[name].append(once(torch, fn))
    for name, t in times.items():
        res[name + "_ms"], res[name + "_min_ms"] = statistics.median(t), min(t)
    base = res["effects_std_ms"]
    res["noise_ms"] = abs(res["effects_std_again_ms"] - base)
    res["centred_std_minus_uncentred_ms"] = res["effects_std_centred_ms"] - base
    res["centred_std_over_uncentred"] = res["effects_std_centred_ms"] / base
    res["centred_mean_minus_uncentred_ms"] = res["effects_centred_ms"] - res["effects_ms"]
    res["effects_std_centred_fraction_of_f64_vector_peak"] = (
        (QUAD_FLOPS + 2 * 33) * float(nnew) * nw / (res["effects_std_centred_ms"] * 1e-3) / PEAK_F64_VECTOR)
    ms = [once(torch, intercept) for _ in range(3 + a.rounds)][3:]
    res["intercept_ms"], res["intercept_min_ms"] = statistics.median(ms), min(ms)
    res["intercept"], res["intercept_std"] = b.value, sb.value
    em = torch.tensor(model.effect_mean, device="cuda")
    res["centred_is_uncentred_minus_mean_bitwise"] = bool(torch.equal(ceff, eff - em[:, None]))
    res["mean_raw_std"], res["mean_centred_std"] = float(esd.mean()), float(csd.mean())
    model.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

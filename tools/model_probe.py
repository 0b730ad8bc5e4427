"""Timing of the fitted model at config C's shapes (n = 1e6, 32 one-feature windows, n_new = 1e6), hipEvents on the
library stream, medians of --reps runs after warm-up:

  1. Nfft4GPAmdModelCreate (spread + grid + the table's copy);
  2. Nfft4GPAmdModelPredict, device pointers, no outside count;
  3. the only route to one batch without a model: the joint handle over [X; Xnew] (creation + kernel setup, i.e.
     the layout of n + n_new points) plus one matvec (the solve excluded).

predict is reported against its HBM stream, 8 n_new (nw + 1) bytes, and against the interpolation kernel of the
operator's matvec at this size (timed here with Nfft4GPAmdKernelBench, layout bytes / time).

    python tools/model_probe.py [--n 1000000 --nw 32 --nnew 1000000 --reps 20 --out profiles/model_probe.json]
"""
import argparse
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--joint-reps", type=int, default=None, help="runs of route 3 (default: --reps)")
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
    win = np.arange(nw, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, nw, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 0.3, 0.01) == 0
    alpha = torch.tensor(rng.standard_normal(n), device="cuda")

    def timed(fn, reps, warm=3):
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

    res = {"n": n, "nw": nw, "n_new": nnew, "reps": a.reps}
    # 1. ModelCreate
    def create():
        h = L.Nfft4GPAmdModelCreate(op.h, alpha.data_ptr(), n)
        assert h
        L.Nfft4GPAmdModelFree(h)
    res["model_create_ms"], _ = timed(create, a.reps)

    # 2. predict
    model = amd.FittedModel.from_operator(op, alpha)
    Xd = torch.tensor(np.ascontiguousarray(Xnew.T), device="cuda")  # [d][n_new]: column-major n_new x d
    mean = torch.empty(nnew, dtype=torch.float64, device="cuda")

    def predict():
        assert L.Nfft4GPAmdModelPredict(model.h, Xd.data_ptr(), nnew, nnew, nw, mean.data_ptr(), None) == 0
    med, best = timed(predict, max(a.reps, 50), warm=5)
    stream_bytes = 8.0 * nnew * (nw + 1)
    res["predict_ms"], res["predict_min_ms"] = med, best
    res["predict_stream_bytes"] = stream_bytes
    res["predict_TBps"] = stream_bytes / (med * 1e-3) / 1e12
    assert model.predict(Xnew[:1000]).shape == (1000,)

    # the operator's own interpolation at this size: layout bytes per second
    y = op.matsymv(alpha)
    ms_interp = op.kernel_bench("interp", alpha, y, reps=50)
    lay = op.layout_info()["layout_bytes"]
    res["k_interp_ms"] = ms_interp
    res["k_interp_TBps"] = (lay + 16.0 * n) / (ms_interp * 1e-3) / 1e12
    res["predict_vs_k_interp_rate"] = res["predict_TBps"] / res["k_interp_TBps"]

    # 3. the joint handle over [X; Xnew] + one matvec (wall clock: the layout's setup has host stages)
    Xa = np.asfortranarray(np.vstack([X, Xnew]))
    xa = torch.zeros(n + nnew, dtype=torch.float64, device="cuda")
    xa[:n] = alpha
    jr = a.joint_reps or a.reps
    wall = []
    for i in range(jr + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        opa = amd.NFFTAdditiveKernel(Xa, win, nw, 1)
        assert opa.setup(amd.GAUSSIAN, 1.0, 0.3, 0.01) == 0
        t1 = time.perf_counter()
        opa.matsymv(xa)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        opa.free()
        if i:  # the first run warms up
            wall.append(((t2 - t0) * 1e3, (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    res["joint_total_ms"] = statistics.median(w[0] for w in wall)
    res["joint_handle_ms"] = statistics.median(w[1] for w in wall)
    res["joint_matvec_ms"] = statistics.median(w[2] for w in wall)
    res["joint_reps"] = jr
    model.free()
    op.free()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

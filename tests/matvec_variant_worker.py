"""Child program of test_gpu_matvec_variants.py (not a test: pytest does not collect it).

    python matvec_variant_worker.py CASES OUT.npz

CASES is a JSON list of names from CASES below, or the path of a file that holds one.  Five of the matvec's
switches (NFFT4GP_AMD_INTERP_HL, _HL_SLOTS, _INTERP_THREADS, _INTERP2_THREADS, _GRID_ATOMIC) are read once per
process, so the parent starts one worker per setting with the variables in the worker's environment.  For every
case x deterministic mode x record width the worker builds a handle and writes to OUT.npz, under
"<case>/<det>/<bits>/<name>":

    info      layout_info() as JSON
    y         matsymv(x) with beta = 0 onto a NaN-filled y
    y_ab      matsymv(x, 0.7, -1.5, y0)
    g         gradmatsymv(x)
    m0, m1    the columns of Nfft4GPAmdAdditiveMatSymvMulti on (x, x2), beta = 0 onto NaN
    pcg_x, pcg_hist   amd.pcg(b, maxits = 5, tol = 0) from a zero start (the fused matvec-dot)

The inputs come from inputs(name), seeded by the case's name: the parent calls it again for the oracle."""
import json
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F, L, MU = 1.3, 0.3, 0.01
ALPHA, BETA = 0.7, -1.5
GAUSSIAN, MATERN12 = 0, 1

# name: (n, windows, kernel, environment read when the handle is created, points)
CASES = {
    # one group, fewer than k_interp_hl's slots; one block
    "one_group": (700, 3, MATERN12, {}, "uniform"),
    # groups of 3 + 2 windows; a last block of 3 points: fewer tiles than waves, waves without a tile in any group
    "ragged_tail": (2 * 1024 + 3, 5, GAUSSIAN, {}, "grid_ends"),
    # 3 + 3 + 1: the first restage (group 2 into slot 0), a one-window last group
    "three_groups": (2051, 7, GAUSSIAN, {"NFFT4GP_AMD_CG": "3"}, "uniform"),
    # 11 groups (3, 3, ..., 2): each of two slots is restaged five times
    "many_groups": (1500, 32, GAUSSIAN, {}, "uniform"),
    # the largest LDS footprint; on 512 threads all 8 epilogue registers per thread
    "big_block": (4064 + 37, 16, GAUSSIAN, {"NFFT4GP_AMD_BLOCK": "4064", "NFFT4GP_AMD_CG": "8"}, "uniform"),
}

# run by the parent in its own process, not by a worker: 514 blocks of 256 points (a last block of 5), past the
# 512 at which the launchers turn to 512-thread interpolation workgroups and to partial grids
IN_PROCESS = {
    "many_blocks": (513 * 256 + 5, 5, GAUSSIAN, {"NFFT4GP_AMD_BLOCK": "256"}, "uniform"),
}


def case(name):
    return CASES[name] if name in CASES else IN_PROCESS[name]


def inputs(name):
    """X (n x windows), x, x2, y0, b of a case."""
    n, d, _, _, pts = case(name)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if pts == "grid_ends":
        # test_gpu_spread_fold.py grid_ends: both ends of every feature's range (taps that wrap around the grid),
        # the range itself, and exact duplicates
        X = 0.02 * rng.random((n, d))
        X[n // 2:] += 0.98
        X[0], X[-1] = 0.0, 1.0
        X[-201:-1] = X[1:201]
    else:
        X = rng.random((n, d))
    x, x2, y0, b = (rng.random(n) - 0.5 for _ in range(4))
    return X, x, x2, y0, b


def make_op(amd, name, det, bits, env=None, shard=None):
    """The case's handle (shard: of the rows [shard[0], shard[1]) only), set up; `env` (and the case's own) is in
    os.environ only around the constructor."""
    n, d, kernel, case_env, _ = case(name)
    X = inputs(name)[0]
    env = dict(case_env, **(env or {}))
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        op = amd.NFFTAdditiveKernel(X, np.arange(d, dtype=np.int32), d, 1, shard=shard)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if bits == 32:
        op.set_precision(32)
    assert op.setup(kernel, F, L, MU) == 0
    op.set_deterministic(bool(det))
    return op


def record(amd, torch, op, name, pcg=True):
    """Every output the parent compares, as numpy arrays."""
    from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

    _, x, x2, y0, b = inputs(name)
    n = x.size
    dev = "cuda"
    xd = torch.tensor(x, device=dev)
    out = {"info": np.array(json.dumps(op.layout_info()))}
    y = torch.full((n,), float("nan"), dtype=torch.float64, device=dev)
    out["y"] = op.matsymv(xd, 1.0, 0.0, y)
    out["y_ab"] = op.matsymv(xd, ALPHA, BETA, torch.tensor(y0, device=dev))
    out["g"] = op.gradmatsymv(xd)
    V = torch.tensor(np.stack([x, x2]), device=dev)
    Y = torch.full((2, n), float("nan"), dtype=torch.float64, device=dev)
    rc = _lib.lib().Nfft4GPAmdAdditiveMatSymvMulti(op.h, n, 2, 1.0, V.data_ptr(), n, 0.0, Y.data_ptr(), n)
    assert rc == 0, rc
    out["m0"], out["m1"] = Y[0], Y[1]
    if pcg:
        sol = torch.zeros(n, dtype=torch.float64, device=dev)
        _, _, hist, _ = amd.pcg(op, torch.tensor(b, device=dev), sol, maxits=5, tol=0.0)
        out["pcg_x"], out["pcg_hist"] = sol, hist
    torch.cuda.synchronize()
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else np.asarray(v)) for k, v in out.items()}


def main(argv):
    import torch

    import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

    spec, out_path = argv[1], argv[2]
    if os.path.isfile(spec):
        with open(spec) as fh:
            spec = fh.read()
    names = json.loads(spec)
    assert torch.cuda.is_available(), "the worker needs a HIP device"
    out = {}
    for name in names:
        for det in (0, 1):
            for bits in (64, 32):
                op = make_op(amd, name, det, bits)
                for k, v in record(amd, torch, op, name).items():
                    out[f"{name}/{det}/{bits}/{k}"] = v
                op.free()
    np.savez(out_path, **out)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))

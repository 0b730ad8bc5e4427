"""The spread's fold of the moment table into grid values on the matrix unit (nfft_kernels.hip fold_window_mfma,
NFFT4GP_AMD_SPREAD_FOLD=1, the default) against the chain of 80 FMAs per grid value (=0).

Both forms compute g[gi] = sum_t sum_d C[t][d] M[(gi + m - t) mod 64][d] from the same moment table; they differ
only in the order of the fp64 sums, so in deterministic mode (everything else bitwise reproducible) the matvec and
the gradient matvec of two handles over the same data agree to the bound this project uses for re-associations of
the same sums, 1e-12 normwise (test_gpu_determinism.py); a CPU emulation of the two orders gives ~4e-16.  The
switch is read when a handle is created, so every case builds its handles under monkeypatch.setenv.

Against the oracle the matrix-unit fold is held to the bounds of test_gpu_nfft.py (1e-8 at these length scales)
and, in the 32-bit mode, of test_gpu_precision.py (1e-6)."""
import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu

TOL_REASSOC = 1e-12   # test_gpu_determinism.py: re-associations of the same sums
TOL_TIGHT = 1e-8      # test_gpu_nfft.py, fp64 records
TOL_CONTRACT = 1e-6   # test_gpu_precision.py, 32-bit records
F, L, MU = 1.0, 1.0, 0.01


def uniform(n, d):
    rng = np.random.default_rng(906)
    return rng.random((n, d)), rng.random(n) - 0.5


def grid_ends(n, d):
    """Half of the points in the lowest 2 % and half in the highest 2 % of every feature's range (taps that wrap
    around the 64-cell grid), and 200 exact duplicates."""
    rng = np.random.default_rng(906)
    X = 0.02 * rng.random((n, d))
    X[n // 2:] += 0.98
    X[0], X[-1] = 0.0, 1.0  # the range itself
    X[-201:-1] = X[1:201]
    return X, rng.random(n) - 0.5


# name: (points, n, windows, extra environment, precision, kernel)
SHAPES = {
    "ragged_3plus2": (uniform, 3000, 5, {}, 64, amd.GAUSSIAN),       # ragged last block; groups of 3 + 2 windows
    "one_window": (uniform, 700, 1, {}, 64, amd.GAUSSIAN),
    # all eight waves fold, and their rows 8-9 (1024 doubles) fill nearly the whole alpha slice
    "cg8": (uniform, 5000, 8, {"NFFT4GP_AMD_CG": "8"}, 64, amd.GAUSSIAN),
    "grid_ends": (grid_ends, 3000, 6, {}, 64, amd.GAUSSIAN),
    "bits32": (uniform, 3000, 5, {}, 32, amd.GAUSSIAN),              # c_taps_u, fp32 moments
    "matern": (uniform, 3000, 5, {}, 64, amd.MATERN12),
}


# blocks of 256 points, 4 windows per group: an alpha slice of 288 doubles
SMALL_BLOCK = (uniform, 2000, 4, {"NFFT4GP_AMD_BLOCK": "256", "NFFT4GP_AMD_CG": "4"}, 64, amd.GAUSSIAN)


def make_op(monkeypatch, shape, fold, det):
    pts, n, d, env, bits, kernel = SHAPES[shape] if isinstance(shape, str) else shape
    X, x = pts(n, d)
    monkeypatch.setenv("NFFT4GP_AMD_SPREAD_FOLD", str(fold))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    op = amd.NFFTAdditiveKernel(X, np.arange(d, dtype=np.int32), d, 1)
    if bits == 32:
        op.set_precision(32)
    assert op.setup(kernel, F, L, MU) == 0
    op.set_deterministic(det)
    return op, X, x


def nrel(a, b):
    return float((a - b).norm() / b.norm())


def fold_pair(torch, monkeypatch, shape, det):
    """(y, g) of the chain and of the matrix-unit fold over the same data."""
    out = []
    for fold in (0, 1):
        op, _, x = make_op(monkeypatch, shape, fold, det)
        xd = torch.tensor(x, device="cuda")
        y = op.matsymv(xd)
        g = op.gradmatsymv(xd)
        torch.cuda.synchronize()
        out.append((y, g))
        op.free()
    return out


@pytest.mark.parametrize("shape", list(SHAPES))
def test_fold_equivalence_partial_grids(torch_cuda, monkeypatch, shape):
    """Deterministic mode (the spread writes partial grids, k_grid sums them in fixed order)."""
    (y0, g0), (y1, g1) = fold_pair(torch_cuda, monkeypatch, shape, det=True)
    e, eg = nrel(y1, y0), nrel(g1, g0)
    print(f"{shape}: MFMA fold against the chain, deterministic: matvec {e:.2e}, gradient {eg:.2e}")
    assert e <= TOL_REASSOC and eg <= TOL_REASSOC, (e, eg)
    # another order of the same sums: if not one bit differs, the switch selected the same fold twice
    assert not (torch_cuda.equal(y0, y1) and torch_cuda.equal(g0, g1))


def test_fold_equivalence_atomic_grid_sum(torch_cuda, monkeypatch):
    """Plain mode: a handle of this size adds its grid values into the nw x 64 sums with global atomics."""
    (y0, g0), (y1, g1) = fold_pair(torch_cuda, monkeypatch, "ragged_3plus2", det=False)
    e, eg = nrel(y1, y0), nrel(g1, g0)
    print(f"MFMA fold against the chain, atomic grid sum: matvec {e:.2e}, gradient {eg:.2e}")
    assert e <= TOL_REASSOC and eg <= TOL_REASSOC, (e, eg)


@pytest.mark.parametrize("shape,tol", [("ragged_3plus2", TOL_TIGHT), ("grid_ends", TOL_TIGHT),
                                       ("bits32", TOL_CONTRACT)])
def test_mfma_fold_against_oracle(torch_cuda, monkeypatch, shape, tol):
    from oracle import OracleAdditiveNFFT
    op, X, x = make_op(monkeypatch, shape, 1, det=False)
    n, d = X.shape
    win = np.arange(d, dtype=np.int32)
    y = np.asarray(op.matsymv(x))
    g = np.asarray(op.gradmatsymv(x))
    op.free()
    orc = OracleAdditiveNFFT(X, win, d, 1)
    orc.setup(SHAPES[shape][5], F, L, MU)
    y_ref, g_ref = orc.matsymv(x), orc.gradmatsymv(x)
    e = float(np.linalg.norm(y - y_ref) / np.linalg.norm(y_ref))
    eg = [float(np.linalg.norm(g[s] - g_ref[s]) / np.linalg.norm(g_ref[s]))
          for s in (slice(k * n, (k + 1) * n) for k in range(3))]
    print(f"{shape}: MFMA fold against the oracle: matvec {e:.2e}, gradient {', '.join(f'{v:.2e}' for v in eg)}")
    assert e <= tol and max(eg) <= tol, (e, eg)


def test_mfma_fold_reproducible(torch_cuda, monkeypatch):
    torch = torch_cuda
    op, _, x = make_op(monkeypatch, "ragged_3plus2", 1, det=True)
    xd = torch.tensor(x, device="cuda")
    y1, y2 = op.matsymv(xd), op.matsymv(xd)
    g1, g2 = op.gradmatsymv(xd), op.gradmatsymv(xd)
    torch.cuda.synchronize()
    op.free()
    assert torch.equal(y1, y2)
    assert torch.equal(g1, g2)


def test_small_block_falls_back_to_the_chain(torch_cuda, monkeypatch):
    """Blocks of 256 points with 4 windows per group: the alpha slice holds 288 doubles, fewer than the 512 that rows
    8-9 of four windows' products need, so NFFT4GP_AMD_SPREAD_FOLD=1 runs the chain: bitwise equal results."""
    torch = torch_cuda
    op, _, _ = make_op(monkeypatch, SMALL_BLOCK, 1, det=True)
    info = op.layout_info()
    op.free()
    assert info["block"] == 256 and info["comps_per_group"] == 4, info
    (y0, g0), (y1, g1) = fold_pair(torch, monkeypatch, SMALL_BLOCK, det=True)
    assert torch.equal(y0, y1)
    assert torch.equal(g0, g1)

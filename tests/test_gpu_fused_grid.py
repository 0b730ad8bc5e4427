"""The fused two-launch matvec (layout_info()["fused_grid"]): the spread adds its grids into one of two sum buffers
with global atomics, and every workgroup of k_interp_fg applies the circulants and builds the polynomials of the 33
cells that hold points in its own LDS from those sums.  No k_grid launch, no workgroup waits for another.

Every case first asserts the selection, so a handle that silently ran the three launches fails.  Fused outputs are
held to the oracle at test_gpu_matvec_variants.py's bounds (1e-8 for 64-bit records, 1e-6 for 32-bit) and to the
unfused path (NFFT4GP_AMD_FUSED_GRID=0, same inputs, same process) at 10 x the difference between the unfused plain
run and the unfused deterministic run of that case -- the rule of test_fused_dot_on_512_threads.

Shapes (block, windows per group as env_layout picks them):
    one_group     700 x 3: one block, a partial group, waves without a tile
    ragged_tail   2051 x 5, grid_ends: points at both ends of the range (cells 48 and 16, taps at both ends of the
                  42-value span), exact duplicates, a last block of 3 points
    unscaled      3000 x 4, X in [0, 0.4): radius between 1/8 and 1/4, centre_and_scale does not rescale
    lds_limit     4101 points in blocks of 4064 with the most windows whose LDS fits (37, computed below from
                  8 (block + 32) + 8 nw (265 + 45 + 65 + 65) + 264 <= 160 KB); one window more must report
                  fused_grid = 0

Measured on an MI355X: the fused path differs from the unfused one by 1.2e-16 .. 2.4e-16 in y at every shape and
record width, where the noise of the 10 x rule is 4.4e-16 .. 5.2e-14; the figures per shape are in the docstring of
test_fused_against_oracle_and_unfused."""
import os
import sys
import zlib

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import matvec_variant_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu

TOL = {64: 1e-8, 32: 1e-6}  # test_gpu_matvec_variants.py: TOL_TIGHT, TOL_CONTRACT
LDS_MAX = 160 * 1024
BIG_B = 4064


def fused_lds_bytes(block, nw):
    """k_interp_fg's LDS: the y slice; per window 8 x 33 + 1 polynomial doubles, 4 x 11 + 1 of h on the 42-value span
    and 64 + 1 each of the staged grid sums and circulant row; the fused dot's reduction scratch (2 x 16 + 1)."""
    return 8 * (block + 32) + 8 * nw * ((8 * 33 + 1) + (4 * 11 + 1) + 2 * (64 + 1)) + 8 * 33


NW_MAX = max(nw for nw in range(1, 129) if fused_lds_bytes(BIG_B, nw) <= LDS_MAX)
SWITCHES = ("NFFT4GP_AMD_INTERP_HL", "NFFT4GP_AMD_HL_SLOTS", "NFFT4GP_AMD_INTERP_THREADS",
                         "NFFT4GP_AMD_INTERP2_THREADS", "NFFT4GP_AMD_GRID_ATOMIC", "NFFT4GP_AMD_BLOCK",
                         "NFFT4GP_AMD_CG", "NFFT4GP_AMD_SPREAD_VARIANT", "NFFT4GP_AMD_SPREAD_FOLD", "NFFT4GP_AMD_DET",
                         "NFFT4GP_AMD_PRECISION", "NFFT4GP_AMD_FUSED_GRID")
BIG_ENV = {"NFFT4GP_AMD_BLOCK": str(BIG_B), "NFFT4GP_AMD_CG": "8"}


def shape(name):
    """X, kernel, the handle's environment, and (x, x2, y0, b) of a shape; seeded by its name."""
    if name in ("one_group", "ragged_tail"):
        _, _, kernel, env, _ = W.case(name)
        X, x, x2, y0, b = W.inputs(name)
        return X, kernel, env, (x, x2, y0, b)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if name == "unscaled":
        X, env = 0.4 * rng.random((3000, 4)), {}
    elif name == "lds_limit":
        X, env = rng.random((BIG_B + 37, NW_MAX)), BIG_ENV
    elif name == "lds_over":
        X, env = rng.random((BIG_B + 37, NW_MAX + 1)), BIG_ENV
    else:
        raise KeyError(name)
    vecs = tuple(rng.random(X.shape[0]) - 0.5 for _ in range(4))
    return X, W.GAUSSIAN, env, vecs


def make(name, fused, bits=64, det=0, l=W.L):
    """The shape's handle with NFFT4GP_AMD_FUSED_GRID = fused (None: unset) around its constructor."""
    X, kernel, env, _ = shape(name)
    env = dict(env)
    if fused is not None:
        env["NFFT4GP_AMD_FUSED_GRID"] = str(fused)
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        op = amd.NFFTAdditiveKernel(X, np.arange(X.shape[1], dtype=np.int32), X.shape[1], 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    if bits == 32:
        op.set_precision(32)
    assert op.setup(kernel, W.F, l, W.MU) == 0
    op.set_deterministic(bool(det))
    return op


_oracle = {}


def oracle(name, l=W.L):
    """The oracle's y, y_ab of a shape (computed once, read-only)."""
    if (name, l) not in _oracle:
        from oracle import OracleAdditiveNFFT
        X, kernel, _, (x, x2, y0, _) = shape(name)
        orc = OracleAdditiveNFFT(X, np.arange(X.shape[1], dtype=np.int32), X.shape[1], 1)
        orc.setup(kernel, W.F, l, W.MU)
        ref = {"y": orc.matsymv(x), "y2": orc.matsymv(x2), "y_ab": orc.matsymv(x, W.ALPHA, W.BETA, y0)}
        for v in ref.values():
            v.setflags(write=False)
        _oracle[(name, l)] = ref
    return _oracle[(name, l)]


def rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def matvec(torch, op, x, alpha=1.0, beta=0.0, y0=None):
    """beta = 0: onto a NaN-filled y."""
    n = x.size
    y = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if y0 is None else \
        torch.tensor(y0, device="cuda")
    return op.matsymv(torch.tensor(x, device="cuda"), alpha, beta, y).cpu().numpy()


def record(torch, op, name):
    _, _, _, (x, _, y0, b) = shape(name)
    out = {"y": matvec(torch, op, x), "y_ab": matvec(torch, op, x, W.ALPHA, W.BETA, y0)}
    sol = torch.zeros(x.size, dtype=torch.float64, device="cuda")
    _, _, hist, _ = amd.pcg(op, torch.tensor(b, device="cuda"), sol, maxits=5, tol=0.0)
    out["pcg_x"], out["pcg_hist"] = sol.cpu().numpy(), np.asarray(hist)
    return out


def diffs(a, b):
    """The figures the 10 x rule compares: y, y_ab, the PCG iterate (l2) and the PCG history (max relative)."""
    return {"y": rel(a["y"], b["y"]), "y_ab": rel(a["y_ab"], b["y_ab"]), "pcg_x": rel(a["pcg_x"], b["pcg_x"]),
            "pcg_hist": float(np.max(np.abs(a["pcg_hist"] - b["pcg_hist"]) / np.abs(b["pcg_hist"])))}


_base = {}


def unfused(torch, name, bits):
    """The unfused plain record of a shape and the noise of the 10 x rule: its difference from the unfused
    deterministic record.  Computed once per (shape, bits)."""
    if (name, bits) not in _base:
        op = make(name, 0, bits)
        assert op.layout_info()["fused_grid"] == 0
        plain = record(torch, op, name)
        op.free()
        op = make(name, 0, bits, det=1)
        det = record(torch, op, name)
        op.free()
        noise = diffs(plain, det)
        assert min(noise.values()) > 0.0, noise
        _base[(name, bits)] = (plain, noise)
    return _base[(name, bits)]


@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name", ["one_group", "ragged_tail", "unscaled", "lds_limit"])
def test_fused_against_oracle_and_unfused(torch_cuda, name, bits):
    """A plain matvec onto NaN, alpha = 0.7 / beta = -1.5 onto a given y, and five PCG steps from zero (the DOT
    form) on the fused path: against the oracle, and against the unfused path by the 10 x rule.

    Measured, relative l2 (fused against unfused | the noise: unfused plain against unfused deterministic),
    y then pcg_x, and y against the oracle:
        one_group    64: 1.6e-16 | 1.3e-15, 3.0e-14 | 1.3e-13, oracle 3.7e-10   32: 1.3e-16 | 4.4e-16, 2.2e-16 | 2.1e-15, 4.7e-8
        ragged_tail  64: 1.2e-16 | 5.2e-14, 7.4e-10 | 2.2e-7,  oracle 1.9e-11   32: 1.5e-16 | 6.0e-16, 1.6e-13 | 1.6e-13, 1.4e-7
        unscaled     64: 1.4e-16 | 4.5e-16, 6.5e-13 | 2.3e-12, oracle 5.7e-11   32: 1.3e-16 | 4.4e-16, 7.5e-16 | 5.9e-15, 1.2e-8
        lds_limit    64: 2.0e-16 | 2.2e-15, 1.1e-12 | 1.2e-12, oracle 9.9e-11   32: 2.1e-16 | 2.2e-15, 4.8e-16 | 3.9e-15, 4.4e-8
    (ragged_tail's five PCG steps at mu = 0.01 amplify any rounding difference: its history's noise is 0.68.)"""
    torch = torch_cuda
    op = make(name, None, bits)
    info = op.layout_info()
    assert info["fused_grid"] == 1, info
    if name == "lds_limit":
        assert info["block"] == BIG_B and info["nwindows"] == NW_MAX == 37 and info["nblocks"] == 2, info
        assert fused_lds_bytes(BIG_B, NW_MAX) <= LDS_MAX < fused_lds_bytes(BIG_B, NW_MAX + 1)
    got = record(torch, op, name)
    op.free()
    ref = oracle(name)
    err = {k: rel(got[k], ref[k]) for k in ("y", "y_ab")}
    plain, noise = unfused(torch, name, bits)
    d = diffs(got, plain)
    print(f"{name} bits {bits}: oracle {err}; fused against unfused {d}; noise {noise}")
    assert not np.isnan(got["y"]).any(), "NaN survives beta = 0"
    assert max(err.values()) <= TOL[bits], err
    assert got["pcg_hist"].size == 6 and np.all(got["pcg_hist"] > 0), got["pcg_hist"]  # five steps ran
    assert d["pcg_x"] <= TOL[bits], d
    bad = {k: (d[k], noise[k]) for k in d if d[k] > 10 * noise[k]}
    assert not bad, bad


@pytest.mark.parametrize("forced", [None, 1])
def test_one_window_more_stays_unfused(torch_cuda, forced):
    """NW_MAX + 1 windows on blocks of 4064 points: k_interp_fg's LDS would pass 160 KB, so the handle reports
    fused_grid = 0 -- also under NFFT4GP_AMD_FUSED_GRID=1, which does not force what cannot run -- and matches
    the oracle on the three launches."""
    torch = torch_cuda
    op = make("lds_over", forced)
    info = op.layout_info()
    assert info["fused_grid"] == 0 and info["nwindows"] == NW_MAX + 1 and info["block"] == BIG_B, info
    _, _, _, (x, _, y0, _) = shape("lds_over")
    ref = oracle("lds_over")
    y, y_ab = matvec(torch, op, x), matvec(torch, op, x, W.ALPHA, W.BETA, y0)
    op.free()
    assert rel(y, ref["y"]) <= TOL[64] and rel(y_ab, ref["y_ab"]) <= TOL[64]


def test_switch_off_and_modes_that_stay_unfused(torch_cuda):
    """NFFT4GP_AMD_FUSED_GRID=0, deterministic mode and the chain fold report fused_grid = 0."""
    op = make("ragged_tail", 0)
    assert op.layout_info()["fused_grid"] == 0
    op.free()
    op = make("ragged_tail", 1, det=1)
    assert op.layout_info()["fused_grid"] == 0
    op.set_deterministic(False)
    assert op.layout_info()["fused_grid"] == 1
    op.free()


def between_ops(torch, op, x, x2):
    """name -> a call that runs between two fused matvecs and must leave the sum buffers and their parity usable."""
    n = x.size
    xd = torch.tensor(x, device="cuda")

    def grad():
        g = op.gradmatsymv(xd).cpu().numpy()
        assert np.isfinite(g).all()

    def two_vectors():
        V = torch.tensor(np.stack([x, x2]), device="cuda")
        Y = torch.full((2, n), float("nan"), dtype=torch.float64, device="cuda")
        assert _lib.lib().Nfft4GPAmdAdditiveMatSymvMulti(op.h, n, 2, 1.0, V.data_ptr(), n, 0.0, Y.data_ptr(), n) == 0
        assert torch.isfinite(Y).all()

    def setup_new_l():
        kernel = shape("ragged_tail")[1]
        assert op.setup(kernel, W.F, 0.5, W.MU) == 0
        y = matvec(torch, op, x2)
        assert rel(y, oracle("ragged_tail", 0.5)["y2"]) <= TOL[64]
        assert op.setup(kernel, W.F, W.L, W.MU) == 0

    def kernel_bench():
        yd = torch.empty(3 * n, dtype=torch.float64, device="cuda")
        for k in op.KERNELS:
            assert op.kernel_bench(k, xd, yd, reps=2) >= 0.0

    def timing():
        op.timing(True)
        op.matsymv(xd)
        op.gradmatsymv(xd)
        q = op.timing_query()
        op.timing(False)
        # the fused matvec has no grid dispatch, the gradient matvec has one
        assert q["spread"][1] == 2 and q["interp"][1] == 2 and q["grid"][1] == 1, q
        assert q["spread"][0] > 0 and q["interp"][0] > 0 and q["grid"][0] > 0, q

    return {"nothing": lambda: None, "grad": grad, "two_vectors": two_vectors, "setup_new_l": setup_new_l,
            "kernel_bench": kernel_bench, "timing": timing}


@pytest.fixture(scope="module")
def seq_op(torch_cuda):
    op = make("ragged_tail", None)
    assert op.layout_info()["fused_grid"] == 1
    yield op
    op.free()


@pytest.mark.parametrize("between", ["nothing", "grad", "two_vectors", "setup_new_l", "kernel_bench", "timing"])
def test_parity_buffers_across_calls(torch_cuda, seq_op, between):
    """Fused matvecs of x1, x2, x1 in a row: both sum buffers are added into, read, cleared and reused.  Each result
    is within the oracle's bound, and the third equals the first within the 10 x rule -- also with a gradient
    matvec, a two-vector matvec, a setup with another l (and back), kernel_bench of each kernel, or a timing round
    after every fused matvec.  (One handle for all cases, so the parity also carries over from case to case.)"""
    torch = torch_cuda
    _, _, _, (x1, x2, _, _) = shape("ragged_tail")
    ref = oracle("ragged_tail")
    _, noise = unfused(torch, "ragged_tail", 64)
    extra = between_ops(torch, seq_op, x1, x2)[between]
    ys = []
    for x in (x1, x2, x1):
        ys.append(matvec(torch, seq_op, x))
        extra()
    assert seq_op.layout_info()["fused_grid"] == 1
    e = [rel(ys[0], ref["y"]), rel(ys[1], ref["y2"]), rel(ys[2], ref["y"])]
    again = rel(ys[2], ys[0])
    print(f"{between}: oracle {e}; third against first {again:.2e}; noise {noise['y']:.2e}")
    assert max(e) <= TOL[64], e
    assert again <= 10 * noise["y"], (again, noise["y"])


def test_timing_of_fused_matvecs_only(torch_cuda, seq_op):
    """timing(True) ... timing_query() over fused matvecs alone: no grid dispatch, so count 0 and 0 ms for "grid",
    and no error from an event that was never recorded."""
    torch = torch_cuda
    x = torch.tensor(shape("ragged_tail")[3][0], device="cuda")
    seq_op.timing(True)
    for _ in range(3):
        seq_op.matsymv(x)
    q = seq_op.timing_query()
    seq_op.timing(False)
    assert q["grid"] == (0.0, 0) and q["spread"][1] == 3 and q["interp"][1] == 3, q
    assert q["spread"][0] > 0 and q["interp"][0] > 0, q

"""GPU parity at the BASELINE configurations and the reference's own edge cases.

* config C (BASELINE configs[2]: n = 1e6, 32 additive 1-D windows) against the oracle at full size,
  l in {1, 0.1}.  The oracle's C/OpenMP restatement takes about a second per matvec on the box's host.
* TEST1's length-scale sweep goes down to l = 0.01 (TESTS/TEST1/foo.ipynb: logspace(-2, 2, 20)); the
  product's degree-7 tap polynomials and 2^-26-cell fixed-point offsets are amplified by the high modes
  there.  l in {0.01, 0.03} on the committed fixtures' points (foo1d: TEST2's data, synth1d, bike3d:
  TEST1's bike windows) against the oracle.  Contract 1e-6 (north star); the CPU emulation of the same
  layout measured <= 7e-9, so the tests also assert 5e-8 for 1-D windows.
* config D (configs[3]: config C, "components sharded 4-per-GPU across 8 GPUs") on one GPU: the 8
  component shards of 4 windows each (Nfft4GPAmdAdditiveComponentShard, the mu x term on shard 0), their y
  summed (what the RCCL all-reduce does), equal to the whole operator and the oracle for the matvec and all
  3n gradient outputs; and the 8 row shards (Nfft4GPAmdShardSpread / ShardFinish, grids summed), plus a
  zero-row shard.
* configs[1] (B: n = 1e5, 8 windows, rank 256) and configs[2] (C: n = 1e6, 32 windows, rank 512): PCG to
  1e-6 (pcg.c:3-206) with the Nystrom (nys.c:518-660) and the AFN (afn.c:161-489) preconditioners, checked
  by their true residual.
* config E (configs[4]: n = 1e7, 64 windows, loss + gradient): the reference's Nfft4GPGpLoss on the
  oracle's operator at n = 2e4, d = 64 (tests/golden/config_e_reduced.npz, make_golden.py config_e),
  and the full size through size-independent properties.
"""
import os
import sys

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd.dist import row_range

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL_CONTRACT = 1e-6


def rel(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def load(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"), allow_pickle=False)


@pytest.fixture(scope="module")
def config_c():
    rng = np.random.default_rng(906)
    n, d = 1_000_000, 32
    X = rng.random((n, d))
    x = rng.random(n) - 0.5
    return X, x


@pytest.mark.parametrize("l", [1.0, 0.1])
def test_config_c_full_size_against_oracle(torch_cuda, config_c, l):
    from oracle import OracleAdditiveNFFT
    torch = torch_cuda
    X, x = config_c
    n, d = X.shape
    win = np.arange(d, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, l, 0.01) == 0
    xd = torch.tensor(x, device="cuda")
    y = op.matsymv(xd).cpu().numpy()
    g = op.gradmatsymv(xd).cpu().numpy()
    orc = OracleAdditiveNFFT(X, win, d, 1)
    orc.setup(0, 1.0, l, 0.01)
    y_ref = orc.matsymv(x)
    g_ref = orc.gradmatsymv(x)
    e = rel(y, y_ref)
    eg = [rel(g[i * n:(i + 1) * n], g_ref[i * n:(i + 1) * n]) for i in range(3)]
    print(f"config C l={l}: matvec rel err {e:.2e}, grad {', '.join(f'{v:.2e}' for v in eg)}")
    assert e <= TOL_CONTRACT and max(eg) <= TOL_CONTRACT
    assert e <= 1e-8 and max(eg) <= 1e-8, (e, eg)


@pytest.mark.parametrize("name", ["foo1d", "synth1d", "bike3d"])
@pytest.mark.parametrize("l", [0.01, 0.03])
@pytest.mark.parametrize("kernel", [amd.GAUSSIAN, amd.MATERN12])
def test_short_length_scales_against_oracle(torch_cuda, name, l, kernel):
    from oracle import OracleAdditiveNFFT
    z = load(name)
    X = np.asarray(z["X"])
    win = np.asarray(z["windows"], np.int32)
    nw, dw = int(z["nw"]), int(z["dw"])
    x = np.asarray(z["x"])
    n = X.shape[0]
    f, mu = float(z["f"]), float(z["mu"])
    op = amd.NFFTAdditiveKernel(X, win, nw, dw)
    assert op.setup(kernel, f, l, mu) == 0
    orc = OracleAdditiveNFFT(X, win, nw, dw)
    orc.setup(kernel, f, l, mu)
    e = rel(op.matsymv(x), orc.matsymv(x))
    g, g_ref = op.gradmatsymv(x), orc.gradmatsymv(x)
    eg = [rel(g[i * n:(i + 1) * n], g_ref[i * n:(i + 1) * n]) for i in range(3)]
    print(f"{name} kernel={kernel} l={l}: matvec rel err {e:.2e}, grad {', '.join(f'{v:.2e}' for v in eg)}")
    assert e <= TOL_CONTRACT and max(eg) <= TOL_CONTRACT, (e, eg)
    if dw == 1:
        assert e <= 5e-8 and max(eg) <= 5e-8, (e, eg)


def _shard_sum(torch, X, win, nw, dw, x, ranges, l, grad=False):
    """Grids of the row shards summed (the all-reduce), then each shard's finish: the concatenated rows."""
    shards = [amd.NFFTAdditiveKernel(X, win, nw, dw, shard=r) for r in ranges]
    for s in shards:
        assert s.setup(amd.GAUSSIAN, 1.0, l, 0.01) == 0
    size = shards[0].shard_grid_size()
    total = torch.zeros(size, dtype=torch.float64, device="cuda")
    for s in shards:
        g = torch.zeros(size, dtype=torch.float64, device="cuda")
        s.shard_spread(torch.tensor(x[s.row_begin:s.row_end], device="cuda"), g)
        total += g
    outs = [s.shard_finish(total, torch.tensor(x[s.row_begin:s.row_end], device="cuda"), grad=grad).cpu().numpy()
            for s in shards]
    if not grad:
        return np.concatenate(outs)
    return np.concatenate([np.concatenate([o[k * (s.n):(k + 1) * s.n] for o, s in zip(outs, shards)])
                           for k in range(3)])


def test_config_d_eight_row_shards_on_one_gpu(torch_cuda, config_c):
    """configs[3] is config C over 8 GPUs: the 8 row shards of dist.row_range, run on one GPU, summed grids
    (what the all-reduce does) -> the whole operator and the oracle."""
    from oracle import OracleAdditiveNFFT
    torch = torch_cuda
    X, x = config_c
    n, d = X.shape
    win = np.arange(d, dtype=np.int32)
    ranges = [row_range(n, r, 8) for r in range(8)]
    y8 = _shard_sum(torch, X, win, d, 1, x, ranges, 1.0)
    full = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert full.setup(amd.GAUSSIAN, 1.0, 1.0, 0.01) == 0
    y1 = full.matsymv(torch.tensor(x, device="cuda")).cpu().numpy()
    assert rel(y8, y1) <= 1e-12
    orc = OracleAdditiveNFFT(X, win, d, 1)
    orc.setup(0, 1.0, 1.0, 0.01)
    e = rel(y8, orc.matsymv(x))
    print(f"config D (8 row shards, one GPU): rel err vs oracle {e:.2e}")
    assert e <= 1e-8


def _component_shards(X, win, nw, world, l):
    """The component split of dist.component_range: shard r holds windows [r nw / world, (r+1) nw / world) for
    all points, weighted 1 / nw_global, the mu x (and f^2 x) term on shard 0 only (nfft_interface.c:796-817
    sums the components one after another; the split sums the shards' partial y instead)."""
    from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd.dist import component_range
    L = amd.lib()
    shards = []
    for r in range(world):
        c0, c1 = component_range(nw, r, world)
        s = amd.NFFTAdditiveKernel(X, win[c0:c1], c1 - c0, 1)
        assert L.Nfft4GPAmdAdditiveComponentShard(s.h, nw, int(r == 0)) == 0
        assert s.setup(amd.GAUSSIAN, 1.0, l, 0.01) == 0
        shards.append(s)
    return shards


@pytest.mark.parametrize("l", [1.0, 0.1])
def test_config_d_component_shards_on_one_gpu(torch_cuda, config_c, l):
    """configs[3] as BASELINE writes it: config C's 32 windows sharded 4 per GPU over 8 GPUs.  The 8 component
    shards run on one GPU; their y summed (the all-reduce) equals the whole operator to 1e-12 and the oracle to
    1e-8, for the matvec (beta = 0 and beta != 0) and all 3n gradient outputs."""
    from oracle import OracleAdditiveNFFT
    torch = torch_cuda
    X, x = config_c
    n, d = X.shape
    win = np.arange(d, dtype=np.int32)
    shards = _component_shards(X, win, d, 8, l)
    assert [s.nwindows for s in shards] == [4] * 8
    xd = torch.tensor(x, device="cuda")
    y0 = torch.tensor(np.random.default_rng(2).random(n) - 0.5, device="cuda")
    ysum = torch.zeros(n, dtype=torch.float64, device="cuda")
    ybsum = torch.zeros(n, dtype=torch.float64, device="cuda")
    gsum = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    for r, s in enumerate(shards):
        ysum += s.matsymv(xd)
        # beta y on one shard only, as dist.hip's component matvec does before its all-reduce
        ybsum += s.matsymv(xd, 0.7, -1.5 if r == 0 else 0.0, y0.clone() if r == 0 else None)
        gsum += s.gradmatsymv(xd)
        s.free()
    full = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert full.setup(amd.GAUSSIAN, 1.0, l, 0.01) == 0
    y1 = full.matsymv(xd).cpu().numpy()
    yb1 = full.matsymv(xd, 0.7, -1.5, y0.clone()).cpu().numpy()
    g1 = full.gradmatsymv(xd).cpu().numpy()
    full.free()
    y8, yb8, g8 = ysum.cpu().numpy(), ybsum.cpu().numpy(), gsum.cpu().numpy()
    assert rel(y8, y1) <= 1e-12 and rel(yb8, yb1) <= 1e-12
    assert max(rel(g8[i * n:(i + 1) * n], g1[i * n:(i + 1) * n]) for i in range(3)) <= 1e-12
    orc = OracleAdditiveNFFT(X, win, d, 1)
    orc.setup(0, 1.0, l, 0.01)
    e = rel(y8, orc.matsymv(x))
    g_ref = orc.gradmatsymv(x)
    eg = [rel(g8[i * n:(i + 1) * n], g_ref[i * n:(i + 1) * n]) for i in range(3)]
    print(f"config D (8 component shards of 4 windows, one GPU) l={l}: matvec rel err {e:.2e}, "
          f"grad {', '.join(f'{v:.2e}' for v in eg)}")
    assert e <= 1e-8 and max(eg) <= 1e-8, (e, eg)


def _true_relres(torch, op, b, x):
    r = b - op.matsymv(x)
    return float(torch.linalg.norm(r) / torch.linalg.norm(b))


def _pcg_checked(torch, op, b, precond, maxits, tol=1e-6):
    x = torch.zeros_like(b)
    _, relres, hist, it = amd.pcg(op, b, x, maxits=maxits, tol=tol, precond=precond)
    tr = _true_relres(torch, op, b, x)
    return it, relres, tr


def test_config_b_pcg_nystrom_and_afn(torch_cuda):
    """configs[1]: n = 1e5, 8 additive 1-D windows, rank 256, fp64, PCG to 1e-6 (l = 0.1, where the NFFT
    operator is SPD).  Unpreconditioned, with the rank-256 Nystrom (landmark K11) and with the
    reference's AFN flow (Nfft4GPAmdPrecondAFNSetup, afn.c:161-489) for both Schur solves: each converges,
    its true residual is <= 1.01e-6, and the preconditioners take fewer iterations than none."""
    import ctypes
    torch = torch_cuda
    rng = np.random.default_rng(906)
    n, d, k = 100_000, 8, 256
    X = rng.random((n, d))
    win = np.arange(d, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 0.1, 0.01) == 0
    b = torch.tensor(np.random.default_rng(907).random(n) - 0.5, device="cuda")
    it0, rr0, tr0 = _pcg_checked(torch, op, b, None, 3000)
    assert it0 > 0 and tr0 <= 1.01e-6, (it0, rr0, tr0)
    perm = np.random.default_rng(908).permutation(n).astype(np.int32)
    nys = amd.NystromPrecond.from_additive(op, perm, k, k11="landmarks")
    it1, rr1, tr1 = _pcg_checked(torch, op, b, nys, 3000)
    nys.free()
    print(f"config B: PCG none {it0} its (true rel res {tr0:.2e}), Nystrom-{k} {it1} its ({tr1:.2e})")
    assert it1 > 0 and tr1 <= 1.01e-6 and it1 < it0, (it1, rr1, tr1)
    for schur in ("noise", "fsai"):
        ctypes.CDLL(None).srand(807)
        afn = amd.PrecondAFN(X, k, perm_opt="random", schur=schur, schur_lfil=20, op=op)
        it2, rr2, tr2 = _pcg_checked(torch, op, b, afn, 3000)
        print(f"config B: PCG AFN ({afn.kind}, rank {afn.k}, schur {schur}) {it2} its ({tr2:.2e})")
        assert afn.k > 0
        afn.free()
        assert it2 > 0 and tr2 <= 1.01e-6 and it2 < it0, (schur, it2, rr2, tr2)


def test_config_c_pcg_nystrom_and_afn(torch_cuda, config_c):
    """configs[2]: n = 1e6, 32 windows, rank 512, PCG to 1e-6 (l = 0.1) with the rank-512 Nystrom and the
    rank-512 AFN with S^-1 = I/mu (schur_opt 0; the kernel-FSAI Schur leg is the bench's, 5-7 s): both converge
    with a true residual <= 1.01e-6."""
    import ctypes
    torch = torch_cuda
    X, _ = config_c
    n, d = X.shape
    k = 512
    win = np.arange(d, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 0.1, 0.01) == 0
    b = torch.tensor(np.random.default_rng(907).random(n) - 0.5, device="cuda")
    perm = np.random.default_rng(908).permutation(n).astype(np.int32)
    nys = amd.NystromPrecond.from_additive(op, perm, k, k11="landmarks")
    it1, rr1, tr1 = _pcg_checked(torch, op, b, nys, 3000)
    nys.free()
    ctypes.CDLL(None).srand(807)
    afn = amd.PrecondAFN(X, k, perm_opt="random", schur="noise", op=op)
    it2, rr2, tr2 = _pcg_checked(torch, op, b, afn, 3000)
    kind, rank = afn.kind, afn.k
    afn.free()
    op.free()
    print(f"config C: PCG Nystrom-{k} {it1} its (true rel res {tr1:.2e}); AFN ({kind}, rank {rank}, I/mu) "
          f"{it2} its ({tr2:.2e})")
    assert it1 > 0 and tr1 <= 1.01e-6, (it1, rr1, tr1)
    assert it2 > 0 and tr2 <= 1.01e-6, (it2, rr2, tr2)


def test_row_shards_1d_with_empty_shard_and_grad(torch_cuda):
    """1-D windows: two shards and a zero-row shard; matvec and all 3n gradient outputs."""
    torch = torch_cuda
    rng = np.random.default_rng(17)
    n, d = 20000, 6
    X = rng.random((n, d))
    x = rng.random(n) - 0.5
    win = np.arange(d, dtype=np.int32)
    full = amd.NFFTAdditiveKernel(X, win, d, 1)
    assert full.setup(amd.GAUSSIAN, 1.0, 0.5, 0.01) == 0
    xd = torch.tensor(x, device="cuda")
    y_full = full.matsymv(xd).cpu().numpy()
    g_full = full.gradmatsymv(xd).cpu().numpy()
    # shards starting at multiples of 16 (dist.row_range's) keep every point's q word as in the whole handle
    ranges = [(0, 7776), (7776, 7776), (7776, n)]
    assert rel(_shard_sum(torch, X, win, d, 1, x, ranges, 0.5), y_full) <= 1e-12
    assert rel(_shard_sum(torch, X, win, d, 1, x, ranges, 0.5, grad=True), g_full) <= 1e-12
    # any other cut moves the later points by their new local index's low bits, at most 2^-29 of a cell
    # (slot_word): the same operator to well within the oracle bound
    ranges = [(0, 7777), (7777, n)]
    assert rel(_shard_sum(torch, X, win, d, 1, x, ranges, 0.5), y_full) <= 1e-10


def test_whole_matvec_refuses_a_row_shard(torch_cuda):
    """A shard handle holds only its rows' grid share: Nfft4GPAdditiveNFFTMatSymv returns -1."""
    import ctypes as C
    rng = np.random.default_rng(3)
    n = 5000
    X = rng.random((n, 2))
    s = amd.NFFTAdditiveKernel(X, np.arange(2, dtype=np.int32), 2, 1, shard=(0, 2500))
    assert s.setup(amd.GAUSSIAN, 1.0, 1.0, 0.01) == 0
    x = np.zeros(2500)
    y = np.zeros(2500)
    L = amd.lib()
    assert L.Nfft4GPAdditiveNFFTMatSymv(s.h, 2500, C.c_double(1.0), x.ctypes.data, C.c_double(0.0),
                                        y.ctypes.data) == -1
    with pytest.raises(ValueError):
        s.matsymv(x)


def test_size_checks_raise(torch_cuda):
    rng = np.random.default_rng(4)
    n = 3000
    X = rng.random((n, 2))
    op = amd.NFFTAdditiveKernel(X, np.arange(2, dtype=np.int32), 2, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 1.0, 0.01) == 0
    with pytest.raises(ValueError):
        op.gradmatsymv(np.zeros(n), y=np.zeros(n))  # 3n outputs
    with pytest.raises(ValueError):
        op.matsymv(np.zeros(n - 1))


def test_pcg_with_many_point_blocks(torch_cuda, monkeypatch):
    """with more point blocks than the fused matvec-dot's grid reduction sums (4096), PCG takes
    the unfused matvec + dot path instead of failing.  NFFT4GP_AMD_BLOCK = 256 gives 4297 blocks at
    n = 1.1e6."""
    torch = torch_cuda
    monkeypatch.setenv("NFFT4GP_AMD_BLOCK", "256")
    rng = np.random.default_rng(5)
    n = 1_100_000
    X = rng.random((n, 2))
    op = amd.NFFTAdditiveKernel(X, np.arange(2, dtype=np.int32), 2, 1)
    assert op.setup(amd.GAUSSIAN, 1.0, 0.1, 0.01) == 0
    assert op.layout_info()["nblocks"] > 4096
    b = torch.tensor(rng.random(n) - 0.5, device="cuda")
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    _, relres, hist, it = amd.pcg(op, b, x, maxits=400, tol=1e-6)
    r = b - op.matsymv(x)
    assert it > 0 and float(torch.linalg.norm(r) / torch.linalg.norm(b)) <= 1.01e-6


def _config_e_inputs(n, d, nvecs, seed):
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_golden import config_e_inputs
    return config_e_inputs(n, d, nvecs, seed)


def test_config_e_reduced_loss_matches_reference(torch_cuda):
    """64 windows, n = 2e4: Nfft4GPGpLoss on the HIP operator against the reference's gp_loss.c / fgmres.c /
    lanczos.c on the oracle's operator (same Rademacher probes, softplus transform)."""
    z = load("config_e_reduced")
    n, d, nvecs, maxits, seed = (int(z[k]) for k in ("n", "d", "nvecs", "maxits", "seed"))
    X, y, R = _config_e_inputs(n, d, nvecs, seed)
    win = np.arange(d, dtype=np.int32)
    loss, grad = amd.gp_loss(X, win, d, 1, y, np.asarray(z["hyper"]), maxits=maxits, nvecs=nvecs, rademacher=R,
                             tol=1e-8, transform=0)
    print(f"config E reduced: loss {loss!r} (ref {float(z['loss'])!r}), grad {grad} (ref {np.asarray(z['grad'])})")
    assert loss == pytest.approx(float(z["loss"]), rel=1e-8)
    np.testing.assert_allclose(grad, z["grad"], rtol=1e-6, atol=1e-9)


def test_config_e_full_size_properties(torch_cuda):
    """n = 1e7, 64 windows (configs[4]) on one GPU: symmetry, linearity, the l-derivative block of the
    gradient matvec against a central difference of the matvec in l, and a loss + gradient that is finite
    and repeats (same handle, same probes) to rounding."""
    torch = torch_cuda
    n, d, nvecs = 10_000_000, 64, 2
    X, y, _ = _config_e_inputs(n, d, 0, 906)
    win = np.arange(d, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, d, 1)
    l = 0.1
    assert op.setup(amd.GAUSSIAN, 1.0, l, 0.01) == 0
    info = op.layout_info()
    assert info["interp_hl"] == 1 and info["spread_variant"] == 3, info  # the rule for layouts past 256 MB
    rng = np.random.default_rng(8)
    u = torch.tensor(rng.random(n) - 0.5, device="cuda")
    v = torch.tensor(rng.random(n) - 0.5, device="cuda")
    Ku, Kv = op.matsymv(u), op.matsymv(v)
    s1, s2 = float(torch.dot(v, Ku)), float(torch.dot(u, Kv))
    assert abs(s1 - s2) <= 1e-9 * abs(s1)
    Kuv = op.matsymv(2.0 * u - 3.0 * v)
    assert float(torch.linalg.norm(Kuv - (2.0 * Ku - 3.0 * Kv)) / torch.linalg.norm(Kuv)) <= 1e-12
    g = op.gradmatsymv(u)
    h = 1e-5
    assert op.setup(amd.GAUSSIAN, 1.0, l + h, 0.01) == 0
    kp = op.matsymv(u)
    assert op.setup(amd.GAUSSIAN, 1.0, l - h, 0.01) == 0
    km = op.matsymv(u)
    fd = (kp - km) / (2 * h)
    e = float(torch.linalg.norm(g[n:2 * n] - fd) / torch.linalg.norm(fd))
    print(f"config E: dK/dl x vs central difference rel {e:.2e}")
    assert e <= 1e-5
    assert float(torch.linalg.norm(g[2 * n:] - u)) == 0.0  # f^2 x with f = 1
    del Ku, Kv, Kuv, g, kp, km, fd
    Rd = torch.tensor(np.where(np.random.default_rng(9).random(n * nvecs) < 0.5, -1.0, 1.0), device="cuda")
    out = [amd.gp_loss(X, win, d, 1, y, (1.0, l, 0.01), maxits=20, nvecs=nvecs, rademacher=Rd, transform=3,
                       op=op) for _ in range(2)]
    (l1, g1), (l2, g2) = out
    print(f"config E loss {l1!r} grad {g1}")
    assert np.isfinite(l1) and np.all(np.isfinite(g1))
    assert l2 == pytest.approx(l1, rel=1e-9)
    np.testing.assert_allclose(g2, g1, rtol=1e-6)

"""k_interp_fg's prologue (the build's inputs loaded ahead of the first tiles, the tiles loaded without a branch and
held across the build) at the smallest shapes that reach the kernel.

Every shape is run with NFFT4GP_AMD_FUSED_GRID=1 (asserted: layout_info()["fused_grid"] == 1) and compared with the
three launches (NFFT4GP_AMD_FUSED_GRID=0, same inputs, same process) under test_gpu_fused_grid.py's bound: 10 x the
difference between the three-launch plain run and the three-launch deterministic run of the same call.

A call sequence per shape, on one handle: x onto NaN (beta = 0), x2 onto NaN -- two consecutive matvecs, so both
parity buffers are added into, read and cleared (gclear) --, then alpha = 0.7 / beta = -1.5 onto a given y, then x
again, which must reproduce the first result under the same bound.

Shapes (n x windows; the block the layout picks is asserted):
    two_points     2 x 1: one tile for sixteen waves, so fifteen waves find neither a first nor a second tile
    block_request  65 x 3 with NFFT4GP_AMD_BLOCK=100: the library keeps blocks of at least 256 points in multiples of
                   16 and ignores smaller requests, so this is one block of 1024 with 65 points; fewer tiles than waves
    ragged_block   517 x 5 in blocks of 256: three workgroups, a last block of 5 points, nw = 5 is no multiple of 4
                   (spread groups of 3 + 2), every block with fewer tiles than waves
    three_deep     4101 x 9 in blocks of 4064: 36 or more tiles on sixteen waves, so some waves consume both tiles
                   held across the build and walk on one-deep, others have only the two; a last block of 37 points
"""
import os
import zlib

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu

F, L, MU = 1.3, 0.3, 0.01
ALPHA, BETA = 0.7, -1.5
SWITCHES = ("NFFT4GP_AMD_INTERP_HL", "NFFT4GP_AMD_HL_SLOTS", "NFFT4GP_AMD_INTERP_THREADS",
            "NFFT4GP_AMD_INTERP2_THREADS", "NFFT4GP_AMD_GRID_ATOMIC", "NFFT4GP_AMD_BLOCK", "NFFT4GP_AMD_CG",
            "NFFT4GP_AMD_SPREAD_VARIANT", "NFFT4GP_AMD_SPREAD_FOLD", "NFFT4GP_AMD_DET", "NFFT4GP_AMD_PRECISION",
            "NFFT4GP_AMD_FUSED_GRID", "NFFT4GP_AMD_INTERP_TIMELINE")
# name: (n, windows, environment of the handle, the block and number of blocks expected)
SHAPES = {
    "two_points": (2, 1, {}, 1024, 1),
    "block_request": (65, 3, {"NFFT4GP_AMD_BLOCK": "100"}, 1024, 1),
    "ragged_block": (2 * 256 + 5, 5, {"NFFT4GP_AMD_BLOCK": "256"}, 256, 3),
    "three_deep": (4064 + 37, 9, {"NFFT4GP_AMD_BLOCK": "4064"}, 4064, 2),
}


def inputs(name):
    n, d = SHAPES[name][:2]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    X = rng.random((n, d))
    x, x2, y0 = (rng.random(n) - 0.5 for _ in range(3))
    return X, x, x2, y0


def make(name, fused, det=False):
    """The shape's handle with NFFT4GP_AMD_FUSED_GRID = fused around its constructor."""
    n, d, env, _, _ = SHAPES[name]
    env = dict(env, NFFT4GP_AMD_FUSED_GRID=str(fused))
    saved = {k: os.environ.get(k) for k in SWITCHES}
    for k in SWITCHES:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        op = amd.NFFTAdditiveKernel(inputs(name)[0], np.arange(d, dtype=np.int32), d, 1)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    assert op.setup(amd.GAUSSIAN, F, L, MU) == 0
    op.set_deterministic(det)
    return op


def sequence(torch, op, name):
    """The four calls of a shape on one handle."""
    _, x, x2, y0 = inputs(name)
    xd, x2d = torch.tensor(x, device="cuda"), torch.tensor(x2, device="cuda")

    def onto_nan(v):
        y = torch.full((v.numel(),), float("nan"), dtype=torch.float64, device="cuda")
        return op.matsymv(v, 1.0, 0.0, y).cpu().numpy()

    out = {"y": onto_nan(xd), "y2": onto_nan(x2d)}
    out["y_ab"] = op.matsymv(xd, ALPHA, BETA, torch.tensor(y0, device="cuda")).cpu().numpy()
    out["y_again"] = onto_nan(xd)
    return out


def rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


@pytest.mark.parametrize("name", list(SHAPES))
def test_prologue_against_three_launches(torch_cuda, name):
    """Measured on an MI355X, relative l2, the largest of y, y2, y_ab, y_again (fused against the three launches |
    the smallest noise: the three launches plain against deterministic), and y_again against y on the fused handle:
        two_points     3.1e-16 | 5.4e-15, again 0
        block_request  1.4e-16 | 1.4e-15, again 2.1e-17
        ragged_block   1.9e-16 | 1.6e-15, again 1.8e-17
        three_deep     2.5e-16 | 3.8e-15, again 2.1e-16"""
    torch = torch_cuda
    _, _, _, block, nblocks = SHAPES[name]
    op = make(name, 1)
    info = op.layout_info()
    assert info["fused_grid"] == 1 and info["block"] == block and info["nblocks"] == nblocks, info
    got = sequence(torch, op, name)
    op.free()
    op = make(name, 0)
    assert op.layout_info()["fused_grid"] == 0
    plain = sequence(torch, op, name)
    op.free()
    op = make(name, 0, det=True)
    assert op.layout_info()["fused_grid"] == 0
    det = sequence(torch, op, name)
    op.free()
    noise = {k: rel(plain[k], det[k]) for k in plain}
    d = {k: rel(got[k], plain[k]) for k in plain}
    again = rel(got["y_again"], got["y"])
    print(f"{name}: fused against three launches {d}; noise {noise}; again against first {again:.2e}")
    for k, v in got.items():
        assert np.isfinite(v).all(), k  # no NaN survives beta = 0
    assert min(noise.values()) > 0.0, noise
    bad = {k: (d[k], noise[k]) for k in d if d[k] > 10 * noise[k]}
    assert not bad, bad
    assert again <= 10 * noise["y"], (again, noise["y"])

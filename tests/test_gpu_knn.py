"""The FSAI pattern's KNN (Nfft4GPDistanceEuclidKnn, kernels.c:121-278: row i >= lfil holds the lfil-1
nearest earlier points by (squared distance, index), then i) on the GPU: the one-launch screens (k_knn_tile,
the default, and k_knn_screen) must give exactly the rows of the fp64 two-pass scan (k_knn_bounded) and of the
radix select over every point (k_knn), on random, clustered, tied and badly centred data, for every row and
for a list of rows; rows a screen cannot settle fall back to the exact scans (counted)."""
import ctypes as C
import time

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu


def knn_call(X, lfil, variant, ja, rows=None):
    """The debug hook's return code and fallback count; ja is written only on success."""
    X = np.asfortranarray(X, dtype=np.float64)
    n, d = X.shape
    f = amd.lib().Nfft4GPAmdDebugKnn
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p,
                  C.c_int]
    f.restype = C.c_int
    nfail = C.c_int(-1)
    if rows is None:
        rc = f(X.ctypes.data, n, n, d, lfil, variant, ja.ctypes.data, C.byref(nfail), None, 0)
    else:
        rows = np.ascontiguousarray(rows, dtype=np.int32)
        rc = f(X.ctypes.data, n, n, d, lfil, variant, ja.ctypes.data, C.byref(nfail), rows.ctypes.data, len(rows))
    return rc, nfail.value


def knn(X, lfil, variant, rows=None):
    m = X.shape[0] - lfil if rows is None else len(rows)
    ja = np.full(m * lfil, -1, np.int32)
    rc, nfail = knn_call(X, lfil, variant, ja, rows)
    assert rc == 0
    return ja.reshape(m, lfil), nfail


def brute(X, lfil, rows):
    out = {}
    for i in rows:
        t = X[:i] - X[i]
        d2 = np.zeros(i)
        for c in range(X.shape[1]):  # the fma chain's order; ties by index
            d2 = d2 + t[:, c] * t[:, c]
        out[i] = np.lexsort((np.arange(i), d2))[: lfil - 1]
    return out


def check_same(X, lfil, expect_few_fallbacks=True):
    """Variants 0, 2, 3 and 4 give the same rows; returns variant 3's rows and the rows that the 32-row screen
    (variant 3) and the default (variant 4) could not settle."""
    b, _ = knn(X, lfil, 0)
    c, _ = knn(X, lfil, 2)
    e, nf3 = knn(X, lfil, 3)  # the one-launch 32-row screen
    f, nf4 = knn(X, lfil, 4)  # the one-launch 256-row bf16-split screen
    n = X.shape[0]
    assert np.array_equal(b, c) and np.array_equal(e, c) and np.array_equal(f, c)
    if expect_few_fallbacks:
        assert nf3 <= max(2, (n - lfil) // 100), nf3
        assert nf4 <= max(2, (n - lfil) // 100), nf4
    assert np.array_equal(e[:, -1], np.arange(lfil, n))
    return e, nf3, nf4


# the cases below n = 5000 are the smallest shapes that reach each block's index arithmetic:
#   (700, 3, 20)    tile, one chunk: row groups of 256 / 256 / 168, a partial wave of 8 rows, odd and even tile counts
#   (333, 17, 25)   tile, two chunks, the largest K it takes (24), n no multiple of 64
#   (300, 32, 2)    K = 1 in every variant
#   (70, 16, 5)     fewer rows than one wave, about two point tiles
#   (4500, 8, 33)   no tile: the 32-row screen at STEPS 4, the sample capped at 4096, the first stream boundary
#   (500, 32, 26)   lfil one past the tile's limit, STEPS 16
#   (400, 64, 20)   STEPS 32, the bounded scan's largest d
#   (300, 200, 10)  d > 64: every variant is the radix select
@pytest.mark.parametrize("n,d,lfil", [(20000, 32, 20), (6000, 3, 20), (5000, 64, 32), (3000, 8, 2), (300, 5, 64),
                                      (700, 3, 20), (333, 17, 25), (300, 32, 2), (70, 16, 5), (4500, 8, 33),
                                      (500, 32, 26), (400, 64, 20), (300, 200, 10)])
def test_knn_screen_matches_exact_random(torch_cuda, n, d, lfil):
    X = np.random.default_rng(n + d).random((n, d))
    # beyond 64 features no screen applies: the radix select takes every row, and the count says so
    a, nf3, nf4 = check_same(X, lfil, expect_few_fallbacks=d <= 64)
    if d > 64:
        assert nf3 == n - lfil and nf4 == n - lfil
    rows = [lfil, lfil + 1, n // 2, n - 1] if n >= 5000 else range(lfil, n)
    ref = brute(X, lfil, rows)
    for i in rows:
        assert np.array_equal(a[i - lfil, :-1], ref[i]), i


def test_knn_stream_first_quarter_boundary(torch_cuda):
    """Rows past 20480 earlier points meet the first quarter-spaced boundary of the 32-row screen's stream (round
    80): the screens give the fp64 scan's rows at n = 21000, and the brute-force rows at the end."""
    n, d, lfil = 21000, 3, 20
    X = np.random.default_rng(n + d).random((n, d))
    b, _ = knn(X, lfil, 0)
    e, nf3 = knn(X, lfil, 3)
    f, nf4 = knn(X, lfil, 4)
    assert np.array_equal(e, b) and np.array_equal(f, b)
    assert nf3 <= max(2, (n - lfil) // 100), nf3
    assert nf4 <= max(2, (n - lfil) // 100), nf4
    rows = range(n - 32, n)
    ref = brute(X, lfil, rows)
    for i in rows:
        assert np.array_equal(b[i - lfil, :-1], ref[i]), i


@pytest.mark.parametrize("n,d,lfil", [(700, 3, 20), (500, 32, 26)])
def test_knn_row_list(torch_cuda, n, d, lfil):
    """The row-list form (a row shard's own rows): a list with gaps, no multiple of 16, 32 or 256 long, first row
    above lfil and last below n - 1, gives those rows of the full pattern and of brute force, in list order."""
    X = np.random.default_rng(n + d).random((n, d))
    rng = np.random.default_rng(2)  # a seed whose lists have the properties asserted next, at both shapes
    rows = sorted(rng.choice(np.arange(lfil, n), size=n // 3, replace=False))
    assert rows[0] > lfil and rows[-1] < n - 1 and len(rows) % 16 != 0
    ref = brute(X, lfil, rows)
    for v in (0, 2, 3, 4):
        full, _ = knn(X, lfil, v)
        part, _ = knn(X, lfil, v, rows)
        assert np.array_equal(part, full[np.array(rows) - lfil]), v
        assert np.array_equal(part[:, -1], rows), v
        for r, i in enumerate(rows):
            assert np.array_equal(part[r, :-1], ref[i]), (v, i)


@pytest.mark.parametrize("variant", [1, 5])
def test_knn_unknown_variant_rejected(torch_cuda, variant):
    """A variant that names no path (the retired two-launch screen's 1 included) is an error, not an empty
    pattern: the hook returns -1 and leaves ja_out as it was."""
    X = np.random.default_rng(7).random((200, 4))
    ja = np.full((200 - 10) * 10, -7, np.int32)
    rc, _ = knn_call(X, 10, variant, ja)
    assert rc == -1
    assert np.all(ja == -7)


def test_knn_screen_clustered_and_ties(torch_cuda):
    rng = np.random.default_rng(3)
    centres = rng.random((20, 16)) * 10
    X = centres[rng.integers(0, 20, 15000)] + 0.01 * rng.standard_normal((15000, 16))
    # clusters 1e-2 wide at |x| ~ 20: the fp32 margin exceeds the neighbour distances, so most rows go on to
    # the fp64 scan (and what that leaves to the radix select) -- still the exact rows
    _, nf, nf4 = check_same(X, 20, expect_few_fallbacks=False)
    assert nf > 64
    assert nf4 > 64
    # coordinates on a coarse grid: many exactly equal distances, ties broken by index
    G = np.round(rng.random((8000, 6)) * 4) / 4
    check_same(G, 20, expect_few_fallbacks=False)


def test_knn_screen_far_from_origin_falls_back_exactly(torch_cuda):
    """Coordinates far from the origin against their spread: the fp32 margin swamps the bins, every row
    goes to the exact radix select, and the rows are still exact."""
    X = 1e4 + np.random.default_rng(5).random((4000, 8))
    a, nf, nf4 = check_same(X, 20, expect_few_fallbacks=False)
    assert nf > 0
    assert nf4 > 0


def test_knn_screen_speed_config_c_slice(torch_cuda):
    """Timing at n = 2e5, d = 32 (config C's features): the screened scans against the fp64 scans."""
    X = np.random.default_rng(906).random((200000, 32))
    t, r, nf = {}, {}, {}
    for v in (4, 3, 0):
        knn(X[:30000], 20, v)
        t0 = time.time()
        r[v], nf[v] = knn(X, 20, v)
        t[v] = time.time() - t0
    assert np.array_equal(r[3], r[0]) and np.array_equal(r[4], r[0])
    print(f"KNN n=2e5 d=32: tiled screen {t[4]:.3f} s (fallback rows {nf[4]}), one-launch screen {t[3]:.3f} s "
          f"(fallback rows {nf[3]}), fp64 {t[0]:.3f} s")
    assert nf[3] <= 2000 and nf[4] <= 2000


@pytest.mark.parametrize("kind", ["random", "clustered"])
def test_knn_stream_quarter_boundaries(torch_cuda, kind):
    """n = 9e4 takes the 32-row screen's stream well into its boundaries at every quarter of the points seen
    (past 16384 points), where each row tightens its limit and drops candidates: the rows of the 32-row and the
    tiled screen equal the fp64 scan's on random and clustered data."""
    rng = np.random.default_rng(11)
    n, d = 90000, 8
    if kind == "random":
        X = rng.random((n, d))
    else:
        centres = rng.random((50, d))
        X = centres[rng.integers(0, 50, n)] + 0.02 * rng.standard_normal((n, d))
    b, _ = knn(X, 20, 0)
    e, nf3 = knn(X, 20, 3)
    f, nf4 = knn(X, 20, 4)
    assert np.array_equal(e, b) and np.array_equal(f, b)
    if kind == "random":
        assert nf3 <= (n - 20) // 100, nf3
        assert nf4 <= (n - 20) // 100, nf4

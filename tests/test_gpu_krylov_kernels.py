"""The Krylov orthogonalisation kernels of csrc/krylov.hip, one sweep at a time, against an extended-precision
reference of that sweep (tests/krylov_sweep_ref.py: numpy in long double, written from the definition; the bound
is the textbook gamma_n one derived there, not fitted to the kernels).

Every sweep runs through the solvers' own launch code (Nfft4GPAmdDebugOrthoSweep -> Ctx::gs / mgs_chain /
block_gs / block_cgs2 / lanczos_local), so the presets, the grid choice, the alignment rule of the 16-byte loads
and the error word are part of what is tested, and each test asserts WHICH kernel ran before it looks at a value.
The shapes are the smallest at which each kernel can go wrong: workgroup counts 1, 2, 7, 8, 9 and 17 (the edges of
reduce.hpp's two-level ticket), a lone last element, a partial first e-slot, one just into the second, an odd n;
every k_mgs_wide<1024, S> on 1, 2 and 9 workgroups with a full, a ragged and a partly empty last pass.  Every
device array is a slice of a larger tensor with 4096 NaNs on either side: a read past n makes a sum NaN, a write
past n breaks the guard, and both are asserted after every call.

Each test prints its worst error / bound; DESIGN.md section 5 records them.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import krylov_sweep_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 4096
WG = R.WG
MGS_STEPS, MGS_ONE, BLOCK, CGS2, LOCAL = 0, 1, 2, 3, 4
SWITCHES = ("NFFT4GP_AMD_MGS_WIDE", "NFFT4GP_AMD_MGS_CHAIN", "NFFT4GP_AMD_LANCZOS_LOCAL", "NFFT4GP_AMD_BD_FOLD",
            "NFFT4GP_AMD_BD_VEC")


def one_pass_ns(G):
    """n for G workgroups of 4096: all full; then a lone last element, a partial first e-slot, one element into
    the second e-slot, and all but one (odd n)"""
    return [G * WG] + [(G - 1) * WG + r for r in (1, 1023, 1025, 4095)]


ONE_PASS = {"tiny": [1, 63]}
ONE_PASS.update({f"G{G}": one_pass_ns(G) for G in (1, 2, 7, 8, 9, 17)})
N_UPDATE_69 = 70_002  # 69 workgroups of k_block_update (1024 each), 18 of k_block_dots; even, an odd count of pairs


class Guarded:
    """`host` on the device as a slice of a larger tensor, 4096 NaNs before and after; off: the slice starts
    `off` doubles past a 16-byte boundary"""

    def __init__(self, torch, host, off=0):
        host = np.ascontiguousarray(host, dtype=np.float64).ravel()
        self.torch = torch
        self.len = host.size
        self.lo = GUARD + off
        self.buf = torch.full((GUARD + 2 + self.len + GUARD,), float("nan"), dtype=torch.float64, device="cuda")
        self.view = self.buf[self.lo:self.lo + self.len]
        self.view.copy_(torch.from_numpy(host))
        self.orig = self.buf.clone()
        assert self.view.data_ptr() % 16 == 8 * (off % 2)

    @property
    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def bits(self, t):
        return t.view(self.torch.int64)

    def guards_intact(self):
        hi = self.lo + self.len
        return (self.torch.equal(self.bits(self.buf[:self.lo]), self.bits(self.orig[:self.lo]))
                and self.torch.equal(self.bits(self.buf[hi:]), self.bits(self.orig[hi:])))

    def unchanged(self):
        return self.torch.equal(self.bits(self.buf), self.bits(self.orig))

    def reset(self):
        self.buf.copy_(self.orig)

    def host(self):
        return self.view.cpu().numpy()


@pytest.fixture(scope="module")
def sweep(torch_cuda):
    L = amd.lib()
    f = L.Nfft4GPAmdDebugOrthoSweep
    f.restype = C.c_int
    f.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_longlong, C.c_int, C.c_int,
                  C.POINTER(C.c_double), C.POINTER(C.c_int)]

    def run(kind, w, V, Z, n, m, with_norm=0):
        """one sweep on fresh w; returns (h, w after, info dict); asserts the guards and the bases"""
        count = {MGS_STEPS: m + 1, MGS_ONE: m + 1, BLOCK: m + 2, CGS2: 2 * m + 4, LOCAL: m + 2}[kind]
        h = np.full(count, np.nan)
        info = (C.c_int * 6)(*([-99] * 6))
        w.reset()
        torch_cuda.cuda.synchronize()
        rc = f(kind, w.ptr, V.ptr, Z.ptr, n, m, with_norm, h.ctypes.data_as(C.POINTER(C.c_double)), info)
        torch_cuda.cuda.synchronize()
        assert rc == 0, (kind, n, m, rc)
        names = ("form", "grid", "vec", "fold", "lz_launched", "err")
        info = dict(zip(names, list(info)))
        assert info["err"] == 0, info
        assert w.guards_intact(), ("w's guards", kind, n, m)
        assert V.unchanged() and Z.unchanged(), ("V / Z written", kind, n, m)
        return h, w.host(), info

    return run


@pytest.fixture(autouse=True)
def clean_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int64), np.asarray(b).view(np.int64))


# ---- MGS: k_gs_step chain, k_mgs_chain ---------------------------------------------------------------------------

@pytest.mark.parametrize("key", list(ONE_PASS))
def test_mgs_one_pass_forms(torch_cuda, sweep, key):
    """The per-projection chain (k_gs_step<1024, 4>, as FGMRES's fallback launches it) within the bound of the
    step-consistent reference, and k_mgs_chain bitwise equal to it, for i in {0, 1, 2, 13} basis columns (0: the
    norm only) at every n of this workgroup count."""
    worst = [0.0, 0.0]
    for n in ONE_PASS[key]:
        G = (n + WG - 1) // WG
        for i in (0, 1, 2, 13):
            w, V = R.make_inputs(1000 + n + i, n, i, rows=1)
            wd, Vd = Guarded(torch_cuda, w), Guarded(torch_cuda, V[:max(i, 1)])
            h0, w0, inf0 = sweep(MGS_STEPS, wd, Vd, Vd, n, i)
            assert (inf0["form"], inf0["grid"]) == (-1, G), (n, i, inf0)
            h1, w1, inf1 = sweep(MGS_ONE, wd, Vd, Vd, n, i)
            assert (inf1["form"], inf1["grid"]) == (0, G), (n, i, inf1)
            rh, rw = R.mgs_ratios(w, V, i, h0, w0)
            worst = [max(worst[0], rh), max(worst[1], rw)]
            assert rh <= 1.0 and rw <= 1.0, (n, i, rh, rw)
            assert same_bits(h1, h0) and same_bits(w1, w0), ("k_mgs_chain != k_gs_step chain", n, i)
    print(f"MGS one-pass {key}: worst error / bound {worst[0]:.3g} (scalars), {worst[1]:.3g} (w)")


def wide_ns(S, g):
    """n that k_mgs_wide<1024, S> covers with g workgroups: every pass full; the last workgroup of the last pass
    ragged (odd n, a partial e-slot); the last pass empty for the trailing workgroups, one of them holding a lone
    element"""
    full = S * g * WG
    ragged = full - WG + 1023
    if g == 1:
        lone = (S - 1) * WG + 1
    else:
        lone = max((S - 1) * g * WG + WG + 1, (g - 1) * S * WG + 1)
    out = [full, ragged, lone]
    for n in out:
        assert (n + S * WG - 1) // (S * WG) == g and n > (S - 1) * g * WG
    return out


@pytest.mark.parametrize("S", [2, 4, 6, 8, 10, 12])
def test_mgs_wide_every_instantiation(torch_cuda, sweep, monkeypatch, S):
    """k_mgs_wide<1024, S>, forced by NFFT4GP_AMD_MGS_WIDE=S, on g in {1, 2, 9} workgroups: the form and the grid
    are asserted, the result is within the bound of the reference and bitwise equal to the per-projection chain
    on that grid."""
    monkeypatch.setenv("NFFT4GP_AMD_MGS_WIDE", str(S))
    worst = [0.0, 0.0]
    for g in (1, 2, 9):
        for n in wide_ns(S, g):
            for i in (1, 6):
                w, V = R.make_inputs(2000 + n + i, n, i, rows=1)
                wd, Vd = Guarded(torch_cuda, w), Guarded(torch_cuda, V)
                h1, w1, inf1 = sweep(MGS_ONE, wd, Vd, Vd, n, i)
                assert (inf1["form"], inf1["grid"]) == (S, g), (n, i, inf1)
                h0, w0, inf0 = sweep(MGS_STEPS, wd, Vd, Vd, n, i)
                assert (inf0["form"], inf0["grid"]) == (-1, g), (n, i, inf0)
                rh, rw = R.mgs_ratios(w, V, i, h1, w1)
                worst = [max(worst[0], rh), max(worst[1], rw)]
                assert rh <= 1.0 and rw <= 1.0, (S, n, i, rh, rw)
                assert same_bits(h1, h0) and same_bits(w1, w0), ("k_mgs_wide != k_gs_step chain", S, n, i)
    print(f"k_mgs_wide<1024, {S}>: worst error / bound {worst[0]:.3g} (scalars), {worst[1]:.3g} (w)")


def test_mgs_wide_switch_values(torch_cuda, sweep, monkeypatch):
    """NFFT4GP_AMD_MGS_WIDE: unset and 0 keep k_mgs_chain where its grid fits, and a value that is no S is ignored.
    NFFT4GP_AMD_MGS_CHAIN=0: no one-launch form runs (the entry point returns 1, as Ctx::mgs_chain does)."""
    n, i = 2 * WG + 5, 2
    w, V = R.make_inputs(7, n, i, rows=1)
    wd, Vd = Guarded(torch_cuda, w), Guarded(torch_cuda, V)
    for val in (None, "0", "3", "14", "1"):
        if val is not None:
            monkeypatch.setenv("NFFT4GP_AMD_MGS_WIDE", val)
        _, _, info = sweep(MGS_ONE, wd, Vd, Vd, n, i)
        assert (info["form"], info["grid"]) == (0, 3), (val, info)
    monkeypatch.setenv("NFFT4GP_AMD_MGS_CHAIN", "0")
    h = np.zeros(i + 1)
    info = (C.c_int * 6)()
    wd.reset()
    rc = amd.lib().Nfft4GPAmdDebugOrthoSweep(MGS_ONE, wd.ptr, Vd.ptr, Vd.ptr, n, i, 0,
                                             h.ctypes.data_as(C.POINTER(C.c_double)), info)
    assert rc == 1 and wd.unchanged()


# ---- block passes: k_block_dots<FOLD, VEC>, k_block_reduce, k_block_update<VEC> ------------------------------------

BLOCK_NS = sorted({n for ns in ONE_PASS.values() for n in ns} | {2, WG + 2, N_UPDATE_69})  # 2, 4098: small even n


@pytest.mark.parametrize("m", [1, 7, 8, 9, 16, 17])
def test_block_pass(torch_cuda, sweep, monkeypatch, m):
    """Ctx::block_gs in the four NFFT4GP_AMD_BD_FOLD x NFFT4GP_AMD_BD_VEC settings: the projections and the norm
    before from the incoming w, the update with Z != V, the norm after.  bd_vec must report 1 only on an even n
    with every array 16-byte aligned and the switch not 0.  Fold on and off: bitwise equal.  VEC 2 and 1: each
    within the bound (their summation orders differ).  With the arrays one double off alignment (with_norm 0)
    and with Z = V the same."""
    worst = [0.0, 0.0, 0.0]

    def held(ref, h, wv, with_norm, tag):
        r = ref.ratios(h, wv, with_norm=bool(with_norm))
        for q in range(3):
            worst[q] = max(worst[q], r[q])
        assert max(r) <= 1.0, (tag, r)

    for n in BLOCK_NS:
        w, V, Z = R.make_inputs(3000 + n + m, n, m, rows=2)
        # aligned, Z != V, with the norm column (m = 8: alone in a second column group)
        wd, Vd, Zd = (Guarded(torch_cuda, a) for a in (w, V, Z))
        ref = R.ClassicalRef(w, V, Z, m)
        res = {}
        for fold in ("1", "0"):
            for vec in ("1", "0"):
                monkeypatch.setenv("NFFT4GP_AMD_BD_FOLD", fold)
                monkeypatch.setenv("NFFT4GP_AMD_BD_VEC", vec)
                h, wv, info = sweep(BLOCK, wd, Vd, Zd, n, m, 1)
                assert info["fold"] == int(fold), (n, m, info)
                assert info["vec"] == (1 if vec == "1" and n % 2 == 0 else 0), (n, m, info)
                held(ref, h, wv, 1, (n, m, fold, vec))
                res[fold, vec] = (h, wv)
        for vec in ("1", "0"):
            assert same_bits(res["1", vec][0], res["0", vec][0]), ("fold changes h", n, m, vec)
            assert same_bits(res["1", vec][1], res["0", vec][1]), ("fold changes w", n, m, vec)
        monkeypatch.delenv("NFFT4GP_AMD_BD_VEC")
        # one double off 16-byte alignment: one row per load whatever n is; no norm column
        wo, Vo, Zo = (Guarded(torch_cuda, a, off=1) for a in (w, V, Z))
        out = []
        for fold in ("1", "0"):
            monkeypatch.setenv("NFFT4GP_AMD_BD_FOLD", fold)
            h, wv, info = sweep(BLOCK, wo, Vo, Zo, n, m, 0)
            assert (info["fold"], info["vec"]) == (int(fold), 0), (n, m, info)
            held(ref, h, wv, 0, (n, m, fold, "offset"))
            out.append((h[:m + 1], wv))
        assert same_bits(out[0][0], out[1][0]) and same_bits(out[0][1], out[1][1]), ("fold, offset", n, m)
        # one row per load on the same data, aligned or not: the same bits
        assert same_bits(out[0][0], res["1", "0"][0][:m + 1]) and same_bits(out[0][1], res["1", "0"][1])
        monkeypatch.delenv("NFFT4GP_AMD_BD_FOLD")
        # Z = V (no preconditioner), the defaults
        refa = R.ClassicalRef(w, V, V, m)
        h, wv, info = sweep(BLOCK, wd, Vd, Vd, n, m, 1)
        assert (info["fold"], info["vec"]) == (1, 1 - n % 2), (n, m, info)
        held(refa, h, wv, 1, (n, m, "alias"))
    print(f"block pass m {m}: worst error / bound {worst[0]:.3g} (projections, norm before), {worst[1]:.3g} (w), "
          f"{worst[2]:.3g} (norm after)")


def cgs2_inputs(seed, n, m):
    """V: m orthonormal columns scaled by 1 +- 0.01 (so V^T V != I and pass 2 has O(0.01) work to do); w_in almost
    in span(V), w_out almost orthogonal to it"""
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, m)))
    V = np.ascontiguousarray((Q * (1.0 + 0.01 * (2.0 * rng.random(m) - 1.0))).T)
    c = 0.5 + rng.random(m)
    r = rng.standard_normal(n)
    r -= Q @ (Q.T @ r)
    r /= np.linalg.norm(r)
    return V, V.T @ c + 1e-3 * r, r + 1e-3 * (V.T @ c)


@pytest.mark.parametrize("m", [1, 8, 17])
def test_cgs2_gate_and_passes(torch_cuda, sweep, m):
    """Ctx::block_cgs2 with the DGKS gate taken on the device.  w almost in span(V): the norm drops below 0.1 of
    its value, pass 2 runs, h[2m + 3] = 1, and pass 2's projections, norm and w are within the bound.  w almost
    orthogonal to V: the ratio is above 0.99, pass 2 is skipped, h[2m + 3] = 0 and w is bit for bit what pass 1
    alone (Ctx::block_gs) leaves."""
    worst = [0.0, 0.0, 0.0]
    for n in (63, WG + 1, 7 * WG + 1023, 9 * WG, 16 * WG + 1025, N_UPDATE_69):
        if n < 2 * m:
            continue
        V, w_in, w_out = cgs2_inputs(4000 + n + m, n, m)
        Vd = Guarded(torch_cuda, V)
        for w, want in ((w_in, 1), (w_out, 0)):
            wd = Guarded(torch_cuda, w)
            h, wv, info = sweep(CGS2, wd, Vd, Vd, n, m)
            assert (info["fold"], info["vec"]) == (1, 1 - n % 2), info
            again, q, r1, r2, rw = R.cgs2_ratios(w, V, m, h, wv)
            # far from the 0.7071 gate, so the reference and the device decide alike
            assert again == want and (q < 0.1 if want else q > 0.99), (n, m, want, q)
            assert h[2 * m + 3] == float(want), (n, m, h[2 * m + 3])
            worst = [max(worst[0], r1), max(worst[1], r2), max(worst[2], rw)]
            assert max(r1, r2, rw) <= 1.0, (n, m, want, r1, r2, rw)
            if not want:
                h1, w1, _ = sweep(BLOCK, wd, Vd, Vd, n, m, 1)
                assert same_bits(w1, wv) and same_bits(h1, h[:m + 2]), ("skipped pass 2 touched w", n, m)
    print(f"CGS2 m {m}: worst error / bound {worst[0]:.3g} (pass 1), {worst[1]:.3g} (pass 2), {worst[2]:.3g} (w)")


# ---- the Lanczos local pass: k_lanczos_local and block_gs in its place -----------------------------------------------

@pytest.mark.parametrize("alias", [0, 1], ids=["Z", "Z_is_V"])
@pytest.mark.parametrize("ml", [1, 2])
def test_lanczos_local_pass(torch_cuda, sweep, monkeypatch, ml, alias):
    """k_lanczos_local (asserted to have launched) and, with NFFT4GP_AMD_LANCZOS_LOCAL=0, Ctx::block_gs on the same
    data: each within the bound of the same reference (equal "at rounding level")."""
    worst = [0.0, 0.0, 0.0]
    for idx, n in enumerate(n for ns in ONE_PASS.values() for n in ns):
        w, V, Z = R.make_inputs(5000 + n + ml, n, ml, rows=2)
        off = idx % 2
        wd, Vd = Guarded(torch_cuda, w, off), Guarded(torch_cuda, V, off)
        Zd = Vd if alias else Guarded(torch_cuda, Z, off)
        ref = R.ClassicalRef(w, V, V if alias else Z, ml)
        h, wv, info = sweep(LOCAL, wd, Vd, Zd, n, ml)
        assert info["lz_launched"] == 1, (n, ml, info)
        r = ref.ratios(h, wv)
        monkeypatch.setenv("NFFT4GP_AMD_LANCZOS_LOCAL", "0")
        hb, wb, infb = sweep(LOCAL, wd, Vd, Zd, n, ml)
        monkeypatch.delenv("NFFT4GP_AMD_LANCZOS_LOCAL")
        assert infb["lz_launched"] == 0 and infb["fold"] == 1, (n, ml, infb)
        assert infb["vec"] == (1 if n % 2 == 0 and off == 0 else 0), (n, ml, off, infb)
        rb = ref.ratios(hb, wb)
        for q in range(3):
            worst[q] = max(worst[q], r[q], rb[q])
        assert max(r) <= 1.0, ("k_lanczos_local", n, ml, alias, r)
        assert max(rb) <= 1.0, ("block_gs", n, ml, alias, rb)
    print(f"local pass ml {ml} alias {alias}: worst error / bound {worst[0]:.3g} (projections, norm before), "
          f"{worst[1]:.3g} (w), {worst[2]:.3g} (norm after)")


# ---- state one kernel leaves for the next -------------------------------------------------------------------------

def test_repeated_and_interleaved_sweeps_are_bitwise(torch_cuda, sweep, monkeypatch):
    """The kernels share g_k.ticket and g_k.part (k_gs_step, k_block_update, k_mgs_chain, k_mgs_wide) and the
    local pass reuses its first ticket array for its fourth sum: a ticket left non-zero by one corrupts the next
    one's last arriver.  Every kind three times in a row, then three interleaved rounds, on 9 workgroups (the wide
    form on 3): each repeat is bitwise the first call of its kind, and the first is within the bound."""
    n, i, m = 9 * WG - 1, 6, 9
    w, V, Z = R.make_inputs(6000, n, m, rows=2)
    wd, Vd, Zd = (Guarded(torch_cuda, a) for a in (w, V, Z))
    Vq, w_in, _ = cgs2_inputs(6001, n, m)
    wq, Vqd = Guarded(torch_cuda, w_in), Guarded(torch_cuda, Vq)

    def wide():
        monkeypatch.setenv("NFFT4GP_AMD_MGS_WIDE", "4")
        try:
            return sweep(MGS_ONE, wd, Vd, Vd, n, i)
        finally:
            monkeypatch.delenv("NFFT4GP_AMD_MGS_WIDE")

    order = [
        ("gs", lambda: sweep(MGS_STEPS, wd, Vd, Vd, n, i)),
        ("block", lambda: sweep(BLOCK, wd, Vd, Zd, n, m, 1)),
        ("chain", lambda: sweep(MGS_ONE, wd, Vd, Vd, n, i)),
        ("local", lambda: sweep(LOCAL, wd, Vd, Zd, n, 2)),
        ("cgs2", lambda: sweep(CGS2, wq, Vqd, Vqd, n, m)),
        ("wide", wide),
        ("local1", lambda: sweep(LOCAL, wd, Vd, Vd, n, 1)),
    ]
    first = {}
    # each kind three times in a row, then three rounds of all of them, the middle round backwards
    seq = [kc for kc in order for _ in range(3)] + order + order[::-1] + order
    for pos, (name, call) in enumerate(seq):
        h, wv, info = call()
        if name not in first:
            first[name] = (h, wv, info)
        else:
            assert info == first[name][2], (name, pos)
            assert same_bits(h, first[name][0]) and same_bits(wv, first[name][1]), (name, pos)
    assert first["chain"][2]["form"] == 0 and first["wide"][2]["form"] == 4 and first["wide"][2]["grid"] == 3
    assert first["local"][2]["lz_launched"] == 1 and first["local1"][2]["lz_launched"] == 1
    assert first["cgs2"][0][2 * m + 3] == 1.0
    # and what was repeated is right
    for name in ("gs", "chain", "wide"):
        assert max(R.mgs_ratios(w, V, i, *first[name][:2])) <= 1.0, name
    assert max(R.ClassicalRef(w, V, Z, m).ratios(*first["block"][:2])) <= 1.0
    assert max(R.ClassicalRef(w, V, Z, 2).ratios(*first["local"][:2])) <= 1.0
    assert max(R.ClassicalRef(w, V, V, 1).ratios(*first["local1"][:2])) <= 1.0
    assert max(R.cgs2_ratios(w_in, Vq, m, *first["cgs2"][:2])[2:]) <= 1.0


# ---- through the solvers ---------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def small_op(torch_cuda):
    rng = np.random.default_rng(910)
    n, d = 100_003, 4
    X = rng.random((n, d))
    op = amd.NFFTAdditiveKernel(X, np.arange(d, dtype=np.int32), d, 1)
    assert op.setup(amd.GAUSSIAN, f=1.0, l=0.1, mu=0.01) == 0
    op.set_deterministic(True)
    b = torch_cuda.tensor(rng.random(n) - 0.5, device="cuda")
    yield op, b
    op.free()


@pytest.mark.parametrize("S", [2, 4, 6, 8, 10, 12])
def test_fgmres_with_each_wide_form_is_bitwise(torch_cuda, sweep, small_op, monkeypatch, S):
    """test_gpu_determinism.py's test_fgmres_mgs_sweep_wide_is_bitwise at n = 100 003 for every S: FGMRES with
    k_mgs_wide<1024, S> forced against the per-projection chain (NFFT4GP_AMD_MGS_CHAIN=0) on the same grid."""
    torch = torch_cuda
    op, b = small_op
    n = op.n
    monkeypatch.setenv("NFFT4GP_AMD_MGS_WIDE", str(S))
    w, V = R.make_inputs(8, n, 1, rows=1)
    _, _, info = sweep(MGS_ONE, Guarded(torch, w), Guarded(torch, V), Guarded(torch, V), n, 1)
    assert (info["form"], info["grid"]) == (S, (n + S * WG - 1) // (S * WG)), info
    amd.lib().Nfft4GPAmdSetFgmresOrtho(0)
    runs = []
    for chain in ("1", "0"):
        monkeypatch.setenv("NFFT4GP_AMD_MGS_CHAIN", chain)
        x = torch.zeros(n, dtype=torch.float64, device="cuda")
        _, relres, hist, it = amd.fgmres(op, b, x, kdim=20, maxits=20, tol=1e-14)
        torch.cuda.synchronize()
        runs.append((x, relres, np.asarray(hist), it))
    (x1, r1, h1, i1), (x2, r2, h2, i2) = runs
    print(f"S {S}: FGMRES(20) rel res {r1:.6e} / {r2:.6e}")
    assert i1 == i2 and i1 > 0
    assert r1 == r2
    np.testing.assert_array_equal(h1, h2)
    assert torch.equal(x1, x2)


LOGDET_SETTINGS = [{"NFFT4GP_AMD_LANCZOS_LOCAL": "0"}, {"NFFT4GP_AMD_BD_FOLD": "0"}, {"NFFT4GP_AMD_BD_VEC": "0"},
                   {"NFFT4GP_AMD_LANCZOS_LOCAL": "0", "NFFT4GP_AMD_BD_FOLD": "0"},
                   {"NFFT4GP_AMD_LANCZOS_LOCAL": "0", "NFFT4GP_AMD_BD_VEC": "0"},
                   {"NFFT4GP_AMD_LANCZOS_LOCAL": "0", "NFFT4GP_AMD_BD_FOLD": "0", "NFFT4GP_AMD_BD_VEC": "0"}]


@pytest.fixture(scope="module")
def logdet_case(torch_cuda):
    import test_gpu_krylov as TK
    z, k = TK.load("pcg_synth"), TK.load("krylov_synth")
    op = TK.HostDenseOp(np.asarray(z["X"]), float(k["f"]), float(k["l"]), float(k["mu"]))
    args = (op, int(k["maxits"]), int(k["nvecs"]), np.asarray(k["rademacher"], dtype=np.float64))
    saved = {key: os.environ.pop(key) for key in SWITCHES if key in os.environ}
    try:
        return args, amd.logdet(*args)
    finally:
        os.environ.update(saved)


@pytest.mark.parametrize("env", LOGDET_SETTINGS, ids=lambda e: "+".join(k[12:] + v for k, v in e.items()))
def test_logdet_under_each_switch(torch_cuda, logdet_case, monkeypatch, env):
    """The Lanczos quadrature on tests/golden/krylov_synth with the local pass as block_gs, the block dots'
    reduction as its own launch and one row per load: each within 1e-12 of the default (the bar of
    test_one_launch_sweeps_recover_after_a_wait_gives_up)."""
    args, (v0, g0) = logdet_case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    v, g = amd.logdet(*args)
    print(f"logdet {v!r} against {v0!r}: {abs(v - v0) / abs(v0):.2e}")
    assert v == pytest.approx(v0, rel=1e-12)
    np.testing.assert_allclose(g, g0, rtol=1e-10)

"""The training loop under the reference's names (csrc/optimizer.cpp): Nfft4GPOptimizationAdam* against the
reference's compiled adam.c on one loss callback, the stop flags, the struct layouts of optimizer_adam and
nfft4gp_gp_problem against the reference's headers, and Nfft4GPGpProblemSetup / Create field by field.  Host
code only: no GPU."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LIB = os.path.join(ROOT, "oracle", "_ref", "libnfft4gp_ref.so")
REFERENCE = "/root/reference"
SRC = os.path.join(ROOT, "tests", "dropin")

# loss(x) = 1/2 x^T A x - b^T x + 2, A symmetric positive definite: a fixed quadratic with a linear term
QA = np.array([[3.0, 0.5, -0.2], [0.5, 2.0, 0.3], [-0.2, 0.3, 1.5]])
QB = np.array([0.7, -1.1, 0.4])
X0 = np.array([0.9, -0.4, 1.7])


def make_loss(fail_from=None):
    calls = {"n": 0}

    def loss(_data, x, lossp, dloss):
        calls["n"] += 1
        if fail_from is not None and calls["n"] >= fail_from:
            return -1
        xv = np.array([x[0], x[1], x[2]])
        g = QA @ xv - QB
        if lossp:
            lossp[0] = 0.5 * float(xv @ QA @ xv) - float(QB @ xv) + 2.0
        if dloss:
            for i in range(3):
                dloss[i] = g[i]
        return 0

    return _lib.LOSS(loss), calls


def declare(L):
    """argtypes of the Adam entry points on any library that exports them"""
    vp, d = C.c_void_p, C.c_double
    L.Nfft4GPOptimizationAdamCreate.restype = vp
    L.Nfft4GPOptimizationAdamCreate.argtypes = []
    L.Nfft4GPOptimizationAdamFree.restype = None
    L.Nfft4GPOptimizationAdamFree.argtypes = [vp]
    L.Nfft4GPOptimizationAdamSetProblem.argtypes = [vp, vp, vp, C.c_int]
    L.Nfft4GPOptimizationAdamSetOptions.argtypes = [vp, C.c_int, d, d, d, d, d]
    L.Nfft4GPOptimizationAdamInit.argtypes = [vp, vp]
    L.Nfft4GPOptimizationAdamStep.argtypes = [vp]
    return L


def run_adam(L, cb, steps, maxits=25, tol=1e-12, lr=0.01, n=3):
    """Create / SetProblem / SetOptions / Init, then `steps` steps; (handle, struct, step statuses)"""
    h = L.Nfft4GPOptimizationAdamCreate()
    assert h
    assert L.Nfft4GPOptimizationAdamSetProblem(h, C.cast(cb, C.c_void_p), None, n) == 0
    assert L.Nfft4GPOptimizationAdamSetOptions(h, maxits, tol, 0.9, 0.999, 1e-8, lr) == 0
    x0 = np.ascontiguousarray(X0[:n])
    assert L.Nfft4GPOptimizationAdamInit(h, x0.ctypes.data) == 0
    rcs = [L.Nfft4GPOptimizationAdamStep(h) for _ in range(steps)]
    return h, _lib.OptimizerAdamStruct.from_address(h), rcs


def histories(st, maxits, n=3):
    arr = np.ctypeslib.as_array
    return {"x": arr(st._x_history, shape=((maxits + 1) * n,)).copy(),
            "loss": arr(st._loss_history, shape=(maxits + 1,)).copy(),
            "grad": arr(st._grad_history, shape=((maxits + 1) * n,)).copy(),
            "gnorm": arr(st._grad_norm_history, shape=(maxits + 1,)).copy()}


@pytest.mark.skipif(not os.path.exists(REF_LIB), reason="oracle/_ref not built")
def test_adam_matches_the_reference():
    """25 steps at lr 0.01 on the quadratic, the same ctypes callback for both libraries: every history and
    _nits equal to 1e-14 relative (not bitwise: a compiler may contract beta m + (1 - beta) g into an fma)."""
    ours = amd.lib()
    ref = declare(C.CDLL(REF_LIB))
    cb, _ = make_loss()
    ha, sa, ra = run_adam(ours, cb, 25)
    hb, sb, rb = run_adam(ref, cb, 25)
    assert ra == rb == [0] * 24 + [1]
    assert sa._nits == sb._nits == 25
    A, B = histories(sa, 25), histories(sb, 25)
    for k in A:
        scale = np.max(np.abs(B[k]))
        err = np.max(np.abs(A[k] - B[k])) / scale
        print(f"adam {k}: max difference {err:.2e} of {scale:.3e}")
        assert err <= 1e-14, (k, err)
    assert np.all(A["loss"][:25] > 0) and A["loss"][24] < A["loss"][0]
    assert np.array_equal(A["x"][:3], X0)
    ours.Nfft4GPOptimizationAdamFree(ha)
    ref.Nfft4GPOptimizationAdamFree(hb)


def test_adam_update_rule():
    """Without the reference: three steps against the textbook update in numpy."""
    L = amd.lib()
    cb, _ = make_loss()
    h, st, rcs = run_adam(L, cb, 3)
    H = histories(st, 25)
    x, m, v = X0.copy(), np.zeros(3), np.zeros(3)
    for t in range(3):
        g = QA @ x - QB
        assert np.allclose(H["x"][3 * t:3 * t + 3], x, rtol=1e-14, atol=0)
        assert np.allclose(H["grad"][3 * t:3 * t + 3], g, rtol=1e-14, atol=0)
        assert abs(H["gnorm"][t] - np.linalg.norm(g)) <= 1e-14 * np.linalg.norm(g)
        m = 0.9 * m + 0.1 * g
        v = 0.999 * v + 0.001 * g * g
        x = x - 0.01 * (m / (1 - 0.9 ** (t + 1))) / (np.sqrt(v / (1 - 0.999 ** (t + 1))) + 1e-8)
    assert np.allclose(H["x"][9:12], x, rtol=1e-14, atol=0)
    assert rcs == [0, 0, 0] and st._nits == 3
    L.Nfft4GPOptimizationAdamFree(h)


def test_adam_flags():
    L = amd.lib()
    cb, _ = make_loss()
    # tol = 1e30: the first step's gradient norm is below it
    h, st, rcs = run_adam(L, cb, 1, tol=1e30)
    assert rcs == [2] and st._nits == 1
    L.Nfft4GPOptimizationAdamFree(h)
    # maxits = 3: the third step reports it
    h, st, rcs = run_adam(L, cb, 3, maxits=3)
    assert rcs == [0, 0, 1] and st._nits == 3
    # options and the starting point are fixed after the first step
    assert L.Nfft4GPOptimizationAdamSetOptions(h, 10, 1e-6, 0.9, 0.999, 1e-8, 0.01) == -1
    assert L.Nfft4GPOptimizationAdamInit(h, X0.ctypes.data) == -1
    assert st._maxits == 3
    L.Nfft4GPOptimizationAdamFree(h)
    # a failing loss: -1 and _nits stays
    cbf, calls = make_loss(fail_from=3)
    h, st, rcs = run_adam(L, cbf, 3)
    assert rcs == [0, 0, -1] and st._nits == 2 and calls["n"] == 3
    L.Nfft4GPOptimizationAdamFree(h)


def test_adam_defaults_and_short_problem(capfd):
    """adam.c:9-30's defaults; with _n = 2 the step line prints two parameters (the reference prints three
    whatever _n is and reads past the history)."""
    L = amd.lib()
    h = L.Nfft4GPOptimizationAdamCreate()
    st = _lib.OptimizerAdamStruct.from_address(h)
    assert (st._maxits, st._tol, st._beta1, st._beta2, st._epsilon, st._alpha) == (1000, 1e-6, 0.9, 0.999, 1e-8, 0.001)
    assert st._n == 0 and st._nits == 0 and not st._floss and not st._fdata
    assert not st._m and not st._x_history and not st._loss_history
    L.Nfft4GPOptimizationAdamFree(h)

    def loss2(_data, x, lossp, dloss):
        lossp[0] = x[0] * x[0] + 2.0 * x[1] * x[1]
        dloss[0] = 2.0 * x[0]
        dloss[1] = 4.0 * x[1]
        return 0

    cb = _lib.LOSS(loss2)
    h, st, rcs = run_adam(L, cb, 1, maxits=1, n=2)
    assert rcs == [1]
    L.Nfft4GPOptimizationAdamFree(h)
    C.CDLL(None).fflush(None)
    out = capfd.readouterr().out
    assert "Iteration  | Loss            | Grad norm     \n" in out
    line = [ln for ln in out.splitlines() if "current params:" in ln][-1]
    assert line.startswith("         1 | ")
    head, after = line.split(" | current params (after transform): ")
    assert len(head.split("current params: ")[1].split(", ")) == 2 and len(after.split(", ")) == 2


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "SRC")), reason="reference sources absent")
def test_training_struct_layouts_match_the_reference(tmp_path):
    ref, ours = tmp_path / "off_ref", tmp_path / "off_ours"

    def cc(args):
        r = subprocess.run(args, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        return r.stdout

    cc(["gcc", "-std=gnu11", "-fopenmp", "-DUSE_REF", f"-I{REFERENCE}/SRC/optimizer",
        os.path.join(SRC, "train_offsets.c"), "-o", str(ref)])
    cc(["gcc", "-std=c11", "-Wall", "-Werror", f"-I{ROOT}/include", os.path.join(SRC, "train_offsets.c"), "-o",
        str(ours)])
    a, b = cc([str(ref)]), cc([str(ours)])
    assert a == b and a.count("\n") == 67
    # and the ctypes mirrors the other tests read through
    want = dict(ln.split(" ", 1) for ln in b.splitlines())
    for cls, name in ((_lib.OptimizerAdamStruct, "optimizer_adam"), (_lib.GpProblemStruct, "nfft4gp_gp_problem")):
        assert int(want[name]) == C.sizeof(cls)
        for fld, _ in cls._fields_:
            off, size = (int(v) for v in want[f"{name}.{fld}"].split())
            assert (getattr(cls, fld).offset, getattr(cls, fld).size) == (off, size), (name, fld)


def test_ctypes_mirrors_have_the_lp64_layout():
    """the same layout facts without the reference's headers (LP64: SRC/optimizer/adam.h:16-42, gp_problem.h:20-74)"""
    A, G = _lib.OptimizerAdamStruct, _lib.GpProblemStruct
    assert (A._maxits.offset, A._tol.offset, A._floss.offset, A._n.offset, A._beta1.offset) == (0, 8, 16, 32, 40)
    assert (A._nits.offset, A._loss_history.offset, A._x_history.offset, C.sizeof(A)) == (104, 112, 120, 144)
    assert (G._type.offset, G._fstep.offset, G._data_train.offset, G._data_train_n.offset) == (0, 8, 32, 40)
    assert len(G._fields_) == 45


def test_gp_problem_setup_stores_every_argument():
    L = amd.lib()
    p = L.Nfft4GPGPProblemCreate()
    assert p
    st = _lib.GpProblemStruct.from_address(p)
    # gp_problem.c:15-58
    defaults = {"_type": 0, "_tol_loss": 1e-4, "_maxits_loss": 50, "_nvecs_loss": 5, "_transform": 0,
                "_tol_predict": 1e-6, "_maxits_predict": 100}
    unset = {"_kernel_data_free", "_precond_kernel_data_free", "_retuire_std"}  # not assigned by the reference
    for name, _ in _lib.GP_PROBLEM_FIELDS:
        if name in unset:
            continue
        v = getattr(st, name)
        assert (v or 0) == defaults.get(name, 0), (name, v)
    # 44 distinct dummies: pointers are never followed by the setup
    names = [nm for nm, _ in _lib.GP_PROBLEM_FIELDS if nm != "_dwork"]
    assert len(names) == 44
    vals = []
    for i, (nm, t) in enumerate((nm, t) for nm, t in _lib.GP_PROBLEM_FIELDS if nm != "_dwork"):
        if nm == "_type":
            vals.append(2)
        elif nm == "_transform":
            vals.append(3)
        elif t is C.c_int:
            vals.append(1000 + i)
        elif t is C.c_double:
            vals.append(0.25 + i)
        else:
            vals.append(0x10000 + 64 * i)
    assert len(set(vals)) == 44
    assert L.Nfft4GPGpProblemSetup(p, *vals) == 0
    for nm, want in zip(names, vals):
        assert getattr(st, nm) == want, nm
    assert not st._dwork
    assert L.Nfft4GPGpProblemSetup(None, *vals) == -1
    L.Nfft4GPGPProblemFree(p)
    L.Nfft4GPGPProblemFree(None)

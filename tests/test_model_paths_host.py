"""The fitted model's sample paths, host side (no GPU): the six new entry points are declared in the header, matched
by the version script and typed in _lib.py, and each refuses a NULL model with -1 without writing anything."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {  # the argument counts of the issue's signatures
    "Nfft4GPAmdModelFitSampler": 2,
    "Nfft4GPAmdModelSamplerFactor": 2,
    "Nfft4GPAmdModelDrawPaths": 4,
    "Nfft4GPAmdModelPathsInfo": 2,
    "Nfft4GPAmdModelPathWeights": 2,
    "Nfft4GPAmdModelEvalPaths": 9,
}


@pytest.mark.parametrize("name", list(NARGS))
def test_symbol_is_declared_exported_and_typed(name):
    with open(os.path.join(ROOT, "include", "nfft4gp_amd.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, amd.__name__, "csrc", "exports.map")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    exported = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, header)
    assert decl, f"{name} is not declared in the header"
    assert len(decl.group(1).split(",")) == NARGS[name]
    assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not in exports.map's global list"
    fn = getattr(amd.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == NARGS[name]
    assert name in _lib._SIGS
    if name == "Nfft4GPAmdModelEvalPaths":
        assert fn.argtypes[-1] is C.POINTER(C.c_longlong)


def test_null_model_is_refused_and_writes_nothing():
    L = amd.lib()
    info = np.full(3, 7.0)
    assert L.Nfft4GPAmdModelFitSampler(None, info.ctypes.data) == -1 and np.all(info == 7.0)
    assert L.Nfft4GPAmdModelFitSampler(None, None) == -1
    Fm = np.full((33, 33), 7.0)
    assert L.Nfft4GPAmdModelSamplerFactor(None, Fm.ctypes.data) == -1 and np.all(Fm == 7.0)
    xi = np.asfortranarray(np.full((33, 2), 0.5))
    assert L.Nfft4GPAmdModelDrawPaths(None, xi.ctypes.data, 2, 33) == -1 and np.all(xi == 0.5)
    ns = C.c_int(-5)
    assert L.Nfft4GPAmdModelPathsInfo(None, C.byref(ns)) == -1 and ns.value == -5
    B = np.full((33, 2), 7.0, order="F")
    assert L.Nfft4GPAmdModelPathWeights(None, B.ctypes.data) == -1 and np.all(B == 7.0)
    X = np.asfortranarray(np.full((4, 2), 0.5))
    out = np.full((4, 2), 7.0, order="F")
    nout = C.c_longlong(-5)
    for window in (-1, 0):
        assert L.Nfft4GPAmdModelEvalPaths(None, X.ctypes.data, 4, 4, 2, window, out.ctypes.data, 4,
                                          C.byref(nout)) == -1
        assert nout.value == -5 and np.all(out == 7.0)
    assert L.Nfft4GPAmdModelEvalPaths(None, None, 0, 0, 2, -1, None, 0, C.byref(nout)) == -1 and nout.value == -5

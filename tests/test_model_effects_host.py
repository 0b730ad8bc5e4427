"""The fitted model's per-window effects, host side (no GPU): Nfft4GPAmdModelPredictEffects is declared in the header,
matched by the version script and typed in _lib.py, and refuses a NULL model without writing anything."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "Nfft4GPAmdModelPredictEffects"


def test_symbol_is_declared_exported_and_typed():
    with open(os.path.join(ROOT, "include", "nfft4gp_amd.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, amd.__name__, "csrc", "exports.map")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    exported = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    decl = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % NAME, header)
    assert decl, f"{NAME} is not declared in the header"
    assert len(decl.group(1).split(",")) == 11
    assert any(fnmatch.fnmatchcase(NAME, pat) for pat in exported), f"{NAME} is not in exports.map's global list"
    fn = getattr(amd.lib(), NAME)
    assert fn.restype is C.c_int and len(fn.argtypes) == 11
    assert fn.argtypes[-1] is C.POINTER(C.c_longlong)
    assert NAME in _lib._SIGS


def test_null_model_is_refused_and_writes_nothing():
    L = amd.lib()
    X = np.asfortranarray(np.full((4, 2), 0.5))
    eff, std = np.full((4, 2), 7.0, order="F"), np.full((4, 2), 7.0, order="F")
    nout = C.c_longlong(-5)
    assert L.Nfft4GPAmdModelPredictEffects(None, X.ctypes.data, 4, 4, 2, 0, 2, eff.ctypes.data, std.ctypes.data, 4,
                                           C.byref(nout)) == -1
    assert nout.value == -5 and np.all(eff == 7.0) and np.all(std == 7.0)
    assert L.Nfft4GPAmdModelPredictEffects(None, None, 0, 0, 2, 0, 1, None, None, 0, C.byref(nout)) == -1
    assert nout.value == -5

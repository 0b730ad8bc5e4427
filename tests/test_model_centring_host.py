"""The fitted model's centring, host side (no GPU): the five entry points of DESIGN 3.21 are declared in the header with
their argument counts, matched by the version script and typed in _lib.py, and each refuses a NULL model without
writing anything."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd
from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NARGS = {
    "Nfft4GPAmdModelFitCentring": 5,
    "Nfft4GPAmdModelCentring": 5,
    "Nfft4GPAmdModelSetCentring": 6,
    "Nfft4GPAmdModelPredictEffectsCentred": 11,
    "Nfft4GPAmdModelIntercept": 3,
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
    assert name in _lib._SIGS
    fn = getattr(amd.lib(), name)
    assert fn.restype is C.c_int and len(fn.argtypes) == NARGS[name]


def test_the_centred_call_has_the_uncentred_calls_arguments():
    assert _lib._SIGS["Nfft4GPAmdModelPredictEffectsCentred"] == _lib._SIGS["Nfft4GPAmdModelPredictEffects"]
    assert amd.lib().Nfft4GPAmdModelPredictEffectsCentred.argtypes[-1] is C.POINTER(C.c_longlong)


def test_null_model_is_refused_and_writes_nothing():
    L = amd.lib()
    X = np.asfortranarray(np.full((4, 2), 0.5))
    assert L.Nfft4GPAmdModelFitCentring(None, X.ctypes.data, 4, 4, 2) == -1
    n_ref = C.c_int(7)
    fm, em, sd = np.full(66, 7.0), np.full(2, 7.0), np.full(2, 7.0)
    assert L.Nfft4GPAmdModelCentring(None, C.byref(n_ref), fm.ctypes.data, em.ctypes.data, sd.ctypes.data) == -1
    assert n_ref.value == 7 and np.all(fm == 7.0) and np.all(em == 7.0) and np.all(sd == 7.0)
    assert L.Nfft4GPAmdModelCentring(None, None, None, None, None) == -1
    fm[::33] = 1.0
    assert L.Nfft4GPAmdModelSetCentring(None, 4, fm.ctypes.data, em.ctypes.data, sd.ctypes.data, 2) == -1
    eff, std = np.full((4, 2), 7.0, order="F"), np.full((4, 2), 7.0, order="F")
    nout = C.c_longlong(-5)
    assert L.Nfft4GPAmdModelPredictEffectsCentred(None, X.ctypes.data, 4, 4, 2, 0, 2, eff.ctypes.data, std.ctypes.data,
                                                  4, C.byref(nout)) == -1
    assert nout.value == -5 and np.all(eff == 7.0) and np.all(std == 7.0)
    assert L.Nfft4GPAmdModelPredictEffectsCentred(None, None, 0, 0, 2, 0, 1, None, None, 0, C.byref(nout)) == -1
    assert nout.value == -5
    b, sb = C.c_double(7.0), C.c_double(7.0)
    assert L.Nfft4GPAmdModelIntercept(None, C.byref(b), C.byref(sb)) == -1
    assert b.value == 7.0 and sb.value == 7.0
    assert L.Nfft4GPAmdModelIntercept(None, None, None) == -1

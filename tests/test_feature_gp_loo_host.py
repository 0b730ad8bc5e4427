"""The leave-one-out entry points of the feature-space GP, host side (no GPU): Nfft4GPAmdFeatureGpLooBind / LooLoss /
LooPredict / LooStatus refuse a NULL object and NULL outputs where outputs are required, and the four symbols are in
the header and exported by the version script."""
import ctypes as C
import fnmatch
import os
import re

import numpy as np

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("Nfft4GPAmdFeatureGpLooBind", "Nfft4GPAmdFeatureGpLooLoss", "Nfft4GPAmdFeatureGpLooPredict",
           "Nfft4GPAmdFeatureGpLooStatus")


def test_bad_arguments():
    L = amd.lib()
    w = np.zeros(4)
    k = C.c_longlong(7)
    assert L.Nfft4GPAmdFeatureGpLooBind(None, w.ctypes.data, 2, 2, 1, w.ctypes.data) == -1
    assert L.Nfft4GPAmdFeatureGpLooBind(None, None, 0, 0, 0, None) == -1
    assert L.Nfft4GPAmdFeatureGpLooLoss(None, w.ctypes.data, w.ctypes.data, w.ctypes.data) == -1
    assert L.Nfft4GPAmdFeatureGpLooPredict(None, 1.0, 0.3, 0.01, w.ctypes.data, w.ctypes.data, C.byref(k)) == -1
    assert L.Nfft4GPAmdFeatureGpLooPredict(None, 1.0, 0.3, 0.01, None, None, None) == -1
    assert L.Nfft4GPAmdFeatureGpLooStatus(None, C.byref(k)) == -1
    assert k.value == 7  # a refused call writes nothing
    # NULL outputs where outputs are required: checked before the object is touched, so any non-NULL address will do
    obj = C.create_string_buffer(8)
    assert L.Nfft4GPAmdFeatureGpLooLoss(obj, None, w.ctypes.data, w.ctypes.data) == -1
    assert L.Nfft4GPAmdFeatureGpLooLoss(obj, w.ctypes.data, None, w.ctypes.data) == -1
    assert L.Nfft4GPAmdFeatureGpLooLoss(obj, w.ctypes.data, w.ctypes.data, None) == -1
    assert L.Nfft4GPAmdFeatureGpLooStatus(obj, None) == -1


def test_symbols_are_declared_and_exported():
    with open(os.path.join(ROOT, "include", "nfft4gp_amd.h")) as fh:
        header = fh.read()
    with open(os.path.join(ROOT, amd.__name__, "csrc", "exports.map")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    exported = [p.strip() for p in re.search(r"global:(.*?)local:", text, re.S).group(1).split(";") if p.strip()]
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in the header"
        assert any(fnmatch.fnmatchcase(name, pat) for pat in exported), f"{name} is not in exports.map's global list"
        assert hasattr(L := amd.lib(), name) and getattr(L, name).restype is C.c_int

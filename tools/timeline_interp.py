"""Per-workgroup timeline of k_interp_fg (NFFT4GP_AMD_INTERP_TIMELINE=1: four s_memrealtime stamps at 100 MHz).

    python tools/timeline_interp.py [n] [d]        (default: the headline, 1000000 x 32)

Stamps: 0 entry, 1 after the staging barrier (sums, circulant rows and the cleared y slice in LDS), 2 after the
build's last barrier (H in LDS), 3 after the run loop's barrier.  The epilogue is the rest of the kernel."""
import ctypes as C
import os
import sys

import numpy as np
import torch

os.environ["NFFT4GP_AMD_INTERP_TIMELINE"] = "1"
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1000000
d = int(sys.argv[2]) if len(sys.argv) > 2 else 32
rng = np.random.default_rng(906)
X = rng.random((n, d))
x = rng.random(n) - 0.5
op = amd.NFFTAdditiveKernel(X, np.arange(d, dtype=np.int32), d, 1)
assert op.setup(amd.GAUSSIAN, 1.0, 1.0, 0.01) == 0
info = op.layout_info()
assert info["fused_grid"] == 1, info
xd = torch.tensor(x, device="cuda")
yd = torch.zeros(n, dtype=torch.float64, device="cuda")
f = amd.lib().Nfft4GPAmdDebugStamps
f.argtypes = [C.c_void_p, C.c_int]
nwg = info["nblocks"]
rows = []
for _ in range(5):  # warm
    op.matsymv(xd, 1.0, 0.0, yd)
for _ in range(20):  # one timeline per matvec: the stamps are the last launch's
    op.matsymv(xd, 1.0, 0.0, yd)
    out = np.zeros(nwg * 4, dtype=np.uint64)
    f(out.ctypes.data, nwg)
    rows.append(out.reshape(nwg, 4).astype(np.float64) * 10.0 / 1000.0)  # -> microseconds
s = np.stack(rows)  # [matvec][workgroup][stamp]
s -= s[:, :, 0].min(axis=1)[:, None, None]
print(f"n {n} d {d}: WGs {nwg}, 20 matvecs; us from the first workgroup's entry, all workgroups of all matvecs")
legs = [("entry", s[:, :, 0]), ("staging", s[:, :, 1] - s[:, :, 0]), ("build", s[:, :, 2] - s[:, :, 1]),
        ("prologue", s[:, :, 2] - s[:, :, 0]), ("run loop", s[:, :, 3] - s[:, :, 2]), ("to loop end", s[:, :, 3])]
for nm, v in legs:
    print(f"{nm:11s} mean {v.mean():6.2f}  p10 {np.percentile(v, 10):6.2f}  p50 {np.median(v):6.2f}  "
          f"p90 {np.percentile(v, 90):6.2f}  max {v.max():6.2f} us")
print(f"last loop end per matvec: median {np.median(s[:, :, 3].max(axis=1)):.2f} us")

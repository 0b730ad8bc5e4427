"""The 1-D matvec kernels that only large layouts select, forced at small sizes and compared with the oracle.

launch_interp, launch_matvec2, spread_fn and grid_atomic (nfft_kernels.hip) pick among about forty kernel
instantiations; a handle of a few thousand points takes k_spread variant 0, the atomic grid sum and the
1024-thread k_interp.  The rest is forced here with the switches the code has, and every test first asserts through
layout_info() (spread_variant, grid_atomic, interp_threads, interp_hl, hl_slots, interp2_threads) that the kernel it
means to test is the one the launchers pick -- a wrong selection fails, it does not skip.

Five switches are read once per process, so tests/matvec_variant_worker.py runs each setting (ENVS) in a child
process over five shapes (CASES there) that reach k_interp_hl's edges: fewer groups than slots, the first restage,
many recycles, a partial last group, waves without a tile, a last block with fewer tiles than waves, the largest
LDS footprint.  Per shape, deterministic mode and record width the child's matvec (beta = 0 onto NaN), matvec with
alpha and beta, gradient matvec and two-vector matvec are held to the oracle: 1e-8 normwise with 64-bit records
(TOL_TIGHT of test_gpu_nfft.py), 1e-6 with 32-bit records (TOL_CONTRACT of test_gpu_precision.py).  In
deterministic mode every setting equals `base` bit for bit (k_interp_hl and k_interp2 compute k_interp's sums, and
the deterministic rounding takes the order out of them).

hl_slots6 asks for six staging slots; a workgroup's 160 KB of LDS holds three beside big_block's y slice and its
groups of eight windows (six would need 229 KB, which no launch can have; pick_hl_slots takes the limit into
account), so the expected slot count is the largest one <= 6 that fits (hl_slots_that_fit, a restatement of
hl_lds_bytes).

The fused matvec-dot on 512 threads (t512 against base, deterministic): the two differ in the order of
block_sum0_s's sums only, so x and the residual history of five PCG steps may differ by ten times what base's own
plain-mode run differs from its deterministic one (one sample of a rounding-level quantity, hence the 10).
Measured on an MI355X, 512 against 1024 threads | base plain against deterministic, as (x, history):
    one_group    64: 4.6e-14, 1.9e-14 | 1.4e-13, 4.6e-15     32: 3.4e-16, 4.0e-16 | 2.2e-15, 8.6e-16
    ragged_tail  64: 1.2e-08, 2.8e-02 | 2.2e-07, 6.8e-01     32: 5.9e-14, 1.3e-12 | 2.6e-13, 5.8e-12
    three_groups 64: 4.4e-14, 1.2e-14 | 3.3e-13, 1.3e-14     32: 2.9e-16, 6.3e-16 | 6.1e-16, 6.5e-16
    many_groups  64: 8.2e-12, 3.5e-15 | 3.1e-12, 2.8e-15     32: 1.9e-15, 4.6e-15 | 1.7e-14, 3.4e-14
    big_block    64: 4.2e-13, 1.8e-14 | 1.9e-13, 1.1e-14     32: 3.0e-16, 3.3e-16 | 6.1e-15, 2.5e-15
(ragged_tail's duplicated points make its system nearly singular: five steps amplify a rounding to 1e-2.)

A child runs under a time limit of CHILD_TIMEOUT = 30 seconds (subprocess.run kills it when the limit passes): one
child took 2.3 s, mostly start-up, and five times that leaves nothing for a cold file cache.  After a child that ended by a signal, its time limit or any other failure,
no further child is started: the remaining child tests fail at once.  One child runs at a time.

In this process (per-handle switches): 514 blocks of 256 points -- the 512-thread k_interp plain / GRAD / DOT as
the launcher itself picks them and k_grid's partial-grid sum over three passes, the last one ragged -- and
k_spread's variants 3 (PIPE) and 2 (the chain's moment table); and the split finish of two row shards
(k_interp_part: NFFT4GP_AMD_SHARD_SPLIT, read per call, and layout_info()'s shard_split)."""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import matvec_variant_worker as W  # noqa: E402

pytestmark = pytest.mark.gpu

TOL_TIGHT = 1e-8      # test_gpu_nfft.py, 64-bit records
TOL_CONTRACT = 1e-6   # test_gpu_precision.py, 32-bit records
TOL_PCG = 1e-7        # test_gpu_md.py test_pcg_on_3d_windows: the true residual under the oracle's operator
MU_PCG = 1.0          # test_many_blocks_pcg: the operator is positive definite at l = 0.3 only for mu > 0.43
CHILD_TIMEOUT = 30    # seconds

# id: (the child's environment, what its handles must report)
ENVS = {
    "base": ({"NFFT4GP_AMD_INTERP_HL": "0"}, {"interp_hl": 0, "interp_threads": 1024}),
    "hl1024": ({"NFFT4GP_AMD_INTERP_HL": "1"}, {"interp_hl": 1, "interp_threads": 1024, "hl_slots": 2}),
    "hl512": ({"NFFT4GP_AMD_INTERP_HL": "1", "NFFT4GP_AMD_INTERP_THREADS": "512"},
              {"interp_hl": 1, "interp_threads": 512}),
    "hl_slots6": ({"NFFT4GP_AMD_INTERP_HL": "1", "NFFT4GP_AMD_HL_SLOTS": "6"},
                  {"interp_hl": 1, "interp_threads": 1024, "hl_slots": 6}),
    "t512": ({"NFFT4GP_AMD_INTERP_HL": "0", "NFFT4GP_AMD_INTERP_THREADS": "512",
              "NFFT4GP_AMD_INTERP2_THREADS": "512"},
             {"interp_hl": 0, "interp_threads": 512, "interp2_threads": 512}),
}
SWITCHES = ("NFFT4GP_AMD_INTERP_HL", "NFFT4GP_AMD_HL_SLOTS", "NFFT4GP_AMD_INTERP_THREADS",
            "NFFT4GP_AMD_INTERP2_THREADS", "NFFT4GP_AMD_GRID_ATOMIC", "NFFT4GP_AMD_BLOCK", "NFFT4GP_AMD_CG",
            "NFFT4GP_AMD_SPREAD_VARIANT", "NFFT4GP_AMD_SPREAD_FOLD", "NFFT4GP_AMD_DET", "NFFT4GP_AMD_PRECISION")

# what env_layout makes of each shape: asserted, since the edges a shape reaches follow from it
GEOMETRY = {
    "one_group": {"block": 1024, "nblocks": 1, "comps_per_group": 3, "ngroups": 1},
    "ragged_tail": {"block": 1024, "nblocks": 3, "comps_per_group": 3, "ngroups": 2},
    "three_groups": {"block": 1024, "nblocks": 3, "comps_per_group": 3, "ngroups": 3},
    "many_groups": {"block": 1024, "nblocks": 2, "comps_per_group": 3, "ngroups": 11},
    "big_block": {"block": 4064, "nblocks": 2, "comps_per_group": 8, "ngroups": 2},
}
VARIANTS = [(det, bits) for det in (0, 1) for bits in (64, 32)]
FIELDS = ("y", "y_ab", "g", "m0", "m1")


def hl_slots_that_fit(info, want):
    """The largest slot count <= want (>= 2) whose LDS fits a workgroup's 160 KB: the y slice of block + 32
    doubles, per slot comps_per_group windows of 64 x 8 + 1 doubles, and 1 + slots + 2 ngroups counters."""
    def lds(ns):
        return 8 * (info["block"] + 32) + 8 * ns * info["comps_per_group"] * 513 + 4 * (1 + ns + 2 * info["ngroups"])
    ns = want
    while ns > 2 and lds(ns) > 160 * 1024:
        ns -= 1
    return ns


def rel(a, ref):
    return float(np.linalg.norm(a - ref) / np.linalg.norm(ref))


def oracle_errors(rec, ref):
    """Normwise errors of a record's matvecs, gradient blocks and two-vector columns against the oracle's."""
    n = ref["y"].size
    e = {k: rel(rec[k], ref[k]) for k in ("y", "y_ab", "m0", "m1")}
    for i, nm in enumerate(("g_f", "g_l", "g_mu")):
        e[nm] = rel(rec["g"][i * n:(i + 1) * n], ref["g"][i * n:(i + 1) * n])
    return e


def check_oracle(rec, ref, bits, label):
    e = oracle_errors(rec, ref)
    print(f"{label}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    for k in ("y", "m0", "m1"):
        assert not np.isnan(rec[k]).any(), f"{label}: NaN survives beta = 0 in {k}"
    tol = TOL_TIGHT if bits == 64 else TOL_CONTRACT
    assert max(e.values()) <= tol, (label, e)


@pytest.fixture(scope="module")
def oracle_ref():
    """name -> the oracle's outputs for inputs(name), computed once and read-only."""
    from oracle import OracleAdditiveNFFT
    cache = {}

    def get(name):
        if name not in cache:
            n, d, kernel, _, _ = W.case(name)
            X, x, x2, y0, _ = W.inputs(name)
            orc = OracleAdditiveNFFT(X, np.arange(d, dtype=np.int32), d, 1)
            orc.setup(kernel, W.F, W.L, W.MU)
            ref = {"y": orc.matsymv(x), "y_ab": orc.matsymv(x, W.ALPHA, W.BETA, y0), "g": orc.gradmatsymv(x),
                   "m1": orc.matsymv(x2)}
            ref["m0"] = ref["y"]
            for v in ref.values():
                v.setflags(write=False)
            ref["orc"] = orc
            cache[name] = ref
        return cache[name]
    return get


# ---- child runs -------------------------------------------------------------------------------------------------
_runs = {}      # env id -> {"<case>/<det>/<bits>/<name>": array}, or the failure's text
_dead = []      # why no further child is started


def child(env_id):
    """The worker's records under ENVS[env_id], run once per module."""
    if env_id in _runs:
        if isinstance(_runs[env_id], str):
            pytest.fail(_runs[env_id])
        return _runs[env_id]
    if _dead:
        pytest.fail(f"no child is started after a failed one: {_dead[0]}")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(ENVS[env_id][0])
    out = os.path.join(tempfile.mkdtemp(prefix="matvec_variants_"), env_id + ".npz")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        os.path.join(HERE, "matvec_variant_worker.py"), json.dumps(list(W.CASES)), out]
    t0 = time.time()
    try:
        p = subprocess.run(cmd, env=env, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           text=True)
        why = None if p.returncode == 0 else f"child {env_id} ended with status {p.returncode}:\n{p.stdout[-3000:]}"
    except subprocess.TimeoutExpired as ex:  # subprocess.run has killed it
        tail = ex.stdout.decode(errors="replace") if isinstance(ex.stdout, bytes) else (ex.stdout or "")
        why = f"child {env_id} was killed at its time limit of {CHILD_TIMEOUT} s:\n{tail[-3000:]}"
    print(f"child {env_id}: {time.time() - t0:.1f} s")
    if why is not None:
        _runs[env_id] = why
        _dead.append(why.splitlines()[0])
        pytest.fail(why)
    with np.load(out) as z:
        _runs[env_id] = {k: z[k] for k in z.files}
    os.remove(out)
    return _runs[env_id]


def record_of(run, name, det, bits):
    pre = f"{name}/{det}/{bits}/"
    rec = {k[len(pre):]: v for k, v in run.items() if k.startswith(pre)}
    rec["info"] = json.loads(str(rec["info"]))
    return rec


@pytest.mark.parametrize("env_id", list(ENVS))
def test_child_selection_and_oracle(torch_cuda, oracle_ref, env_id):
    """Every handle of the child reports the kernels of ENVS and the geometry of GEOMETRY, and every output is
    within the oracle's bound."""
    run = child(env_id)
    for name in W.CASES:
        for det, bits in VARIANTS:
            rec = record_of(run, name, det, bits)
            info = rec["info"]
            label = f"{env_id} {name} det {det} bits {bits}"
            want = dict(ENVS[env_id][1], **GEOMETRY[name])
            want["spread_variant"] = 0
            want["grid_atomic"] = 0 if det else 1
            if "hl_slots" in want:
                want["hl_slots"] = hl_slots_that_fit(info, want["hl_slots"])
            got = {k: info[k] for k in want}
            assert got == want, (label, info)
            check_oracle(rec, oracle_ref(name), bits, label)
    if env_id == "hl_slots6":  # the setting means something: some shapes get six slots, more than they have groups
        six = [nm for nm in W.CASES if record_of(run, nm, 0, 64)["info"]["hl_slots"] == 6]
        assert {"one_group", "ragged_tail", "three_groups"} <= set(six), six


@pytest.mark.parametrize("env_id", [e for e in ENVS if e != "base"])
def test_child_deterministic_bits_equal_base(torch_cuda, env_id):
    """Deterministic mode: k_interp_hl (1024 and 512 threads, 2 and 6 slots), the 512-thread k_interp (plain and
    GRAD) and k_interp2<512> give the bits of the 1024-thread k_interp / k_interp2."""
    base, run = child("base"), child(env_id)
    bad = []
    for name in W.CASES:
        for bits in (64, 32):
            a, b = record_of(run, name, 1, bits), record_of(base, name, 1, bits)
            for k in FIELDS:
                if not np.array_equal(a[k], b[k]):
                    bad.append((name, bits, k, rel(a[k], b[k])))
    assert not bad, bad


def test_fused_dot_on_512_threads(torch_cuda):
    """k_interp<DOT, 512> (t512) against k_interp<DOT, 1024> (base), both deterministic: five PCG steps from zero."""
    base, run = child("base"), child("t512")

    def diff(a, b):
        return rel(a["pcg_x"], b["pcg_x"]), float(np.max(np.abs(a["pcg_hist"] - b["pcg_hist"]) / np.abs(b["pcg_hist"])))
    bad = []
    for name in W.CASES:
        for bits in (64, 32):
            ref = record_of(base, name, 1, bits)
            assert ref["pcg_hist"].size == 6 and np.all(ref["pcg_hist"] > 0), ref["pcg_hist"]  # five steps ran
            noise = diff(record_of(base, name, 0, bits), ref)
            got = diff(record_of(run, name, 1, bits), ref)
            print(f"{name} bits {bits}: 512 against 1024 threads: x {got[0]:.2e}, history {got[1]:.2e}; "
                  f"base's plain against deterministic run: x {noise[0]:.2e}, history {noise[1]:.2e}")
            if got[0] > 10 * noise[0] or got[1] > 10 * noise[1]:
                bad.append((name, bits, got, noise))
    assert not bad, bad


# ---- in this process: many blocks -------------------------------------------------------------------------------
def free_switches(monkeypatch):
    """The handles of this process follow their layouts alone; nothing runs here after a child that failed."""
    if _dead:
        pytest.fail(f"not run after a failed child: {_dead[0]}")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("det,bits", VARIANTS)
def test_many_blocks_against_oracle(torch_cuda, monkeypatch, oracle_ref, det, bits):
    """514 blocks: the launcher itself picks 512-thread k_interp (plain and GRAD); the spread writes partial grids
    and k_grid sums 514 of them per window in three passes of 256, the last one of 2."""
    free_switches(monkeypatch)
    op = W.make_op(amd, "many_blocks", det, bits)
    info = op.layout_info()
    assert info["nblocks"] == 514 and info["block"] == 256 and info["n"] == 513 * 256 + 5, info
    assert info["interp_threads"] == 512 and info["grid_atomic"] == 0 and info["interp_hl"] == 0, info
    assert info["spread_variant"] == 0, info
    rec = W.record(amd, torch_cuda, op, "many_blocks", pcg=False)
    op.free()
    check_oracle(rec, oracle_ref("many_blocks"), bits, f"many_blocks det {det} bits {bits}")


def test_many_blocks_pcg(torch_cuda, monkeypatch):
    """PCG to 1e-8 on 514 blocks (the fused matvec-dot on 512 threads): converged, and the true residual under the
    oracle's operator is at the tolerance.

    The solve runs at mu = MU_PCG = 1, not at the matvec tests' 0.01: at l = 0.3 the NFFT operator is indefinite
    without enough noise.  The reference's regularised kernel has Fourier coefficients below zero; a Lanczos run on
    the oracle's operator of these 131 333 points (f = 1.3, l = 0.3) gives a smallest eigenvalue of -0.72 at mu = 0,
    so f^2 mu must exceed 0.72 (mu > 0.43).  At mu = 0.01 and 0.1 the reference's own pcg.c on the oracle's operator
    stops at its (p, Ap) <= 0 exit around step 30 with a residual of 4.6 / 10 times |b|, and this library's PCG
    does the same on 65 blocks of 2032 points and 1024 threads as on these 514; at mu = 1 pcg.c converges in 85
    steps.  The handle is the matvec tests' (same layout, same H tables up to the noise term)."""
    torch = torch_cuda
    from oracle import OracleAdditiveNFFT
    free_switches(monkeypatch)
    n, d, kernel, _, _ = W.case("many_blocks")
    op = W.make_op(amd, "many_blocks", 0, 64)
    assert op.setup(kernel, W.F, W.L, MU_PCG) == 0
    info = op.layout_info()
    assert info["nblocks"] == 514 and info["interp_threads"] == 512, info
    X, _, _, _, b = W.inputs("many_blocks")
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    x, rr, hist, it = amd.pcg(op, torch.tensor(b, device="cuda"), x, maxits=1000, tol=1e-8)
    op.free()
    orc = OracleAdditiveNFFT(X, np.arange(d, dtype=np.int32), d, 1)
    orc.setup(kernel, W.F, W.L, MU_PCG)
    r = b - orc.matsymv(x.cpu().numpy())
    true = float(np.linalg.norm(r) / np.linalg.norm(b))
    print(f"many_blocks PCG: {it} iterations, residual {rr:.2e}, true residual under the oracle {true:.2e}")
    assert it > 0 and rr <= 1e-8, (it, rr)
    assert true <= TOL_PCG, true


# ---- in this process: spread variants ---------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [3, 2])
@pytest.mark.parametrize("name", ["ragged_tail", "big_block"])
def test_spread_variants(torch_cuda, monkeypatch, oracle_ref, name, variant):
    """NFFT4GP_AMD_SPREAD_VARIANT=3 (PIPE: the next tile's load moved before the moments) and =2 (the moment table
    of the chain fold).  Plain mode against the oracle; deterministic mode bit for bit against variant 0 -- for
    variant 2 against variant 0 under NFFT4GP_AMD_SPREAD_FOLD=0, as both then run the chain fold."""
    free_switches(monkeypatch)
    env = {"NFFT4GP_AMD_SPREAD_VARIANT": str(variant)}
    env0 = {"NFFT4GP_AMD_SPREAD_VARIANT": "0"}
    if variant == 2:
        env0["NFFT4GP_AMD_SPREAD_FOLD"] = "0"
    bad = []
    for det, bits in VARIANTS:
        op = W.make_op(amd, name, det, bits, env)
        info = op.layout_info()
        assert info["spread_variant"] == variant and info["interp_hl"] == 0, info
        assert {k: info[k] for k in GEOMETRY[name]} == GEOMETRY[name], info
        rec = W.record(amd, torch_cuda, op, name, pcg=False)
        op.free()
        if not det:
            check_oracle(rec, oracle_ref(name), bits, f"{name} spread variant {variant} bits {bits}")
            continue
        op0 = W.make_op(amd, name, det, bits, env0)
        assert op0.layout_info()["spread_variant"] == 0
        rec0 = W.record(amd, torch_cuda, op0, name, pcg=False)
        op0.free()
        bad += [(bits, k, rel(rec[k], rec0[k])) for k in FIELDS if not np.array_equal(rec[k], rec0[k])]
    assert not bad, bad


# ---- in this process: the row shards' split finish --------------------------------------------------------------
@pytest.mark.parametrize("bits", [64, 32])
@pytest.mark.parametrize("name,S,parts", [("three_groups", 2, [1, 2]), ("three_groups", 3, [1, 1, 1]),
                                          ("many_groups", 4, [2, 3, 3, 3])])
def test_shard_split_finish(torch_cuda, monkeypatch, oracle_ref, name, S, parts, bits):
    """k_interp_part: two row shards (dist.row_range) whose finish runs S workgroups per block, each over a
    contiguous range of window groups (NFFT4GP_AMD_SHARD_SPLIT, read per call); `parts` is the number of groups
    per workgroup.  The shards' blocks are 512 points, so that every shard has more than one.  The grids are summed
    as the all-reduce does (_shard_sum of test_gpu_configs.py); the concatenated rows of the finish with beta = 0
    onto NaN and with (ALPHA, BETA) are held to the oracle, and with 64-bit records to the whole handle at 1e-12
    (test_config_d_eight_row_shards_on_one_gpu's bound: the shards start at multiples of 16, so the operator is the
    whole handle's up to the order of its sums)."""
    from preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd.dist import row_range
    torch = torch_cuda
    free_switches(monkeypatch)
    n = W.case(name)[0]
    _, x, _, y0, _ = W.inputs(name)
    shards = [W.make_op(amd, name, 0, bits, {"NFFT4GP_AMD_BLOCK": "512"}, shard=row_range(n, r, 2)) for r in range(2)]
    total = torch.zeros(shards[0].shard_grid_size(), dtype=torch.float64, device="cuda")
    for s in shards:
        g = torch.zeros_like(total)
        s.shard_spread(torch.tensor(x[s.row_begin:s.row_end], device="cuda"), g)
        total += g
    monkeypatch.setenv("NFFT4GP_AMD_SHARD_SPLIT", str(S))
    ys, yabs = [], []
    for s in shards:
        info = s.layout_info()  # shard_split reads the variable as the finish does
        ng = GEOMETRY[name]["ngroups"]
        assert info["shard_split"] == S and info["ngroups"] == ng and info["block"] == 512, info
        assert info["nblocks"] >= 2 and info["n"] == s.n, info
        assert [(p + 1) * ng // S - p * ng // S for p in range(S)] == parts
        xs = torch.tensor(x[s.row_begin:s.row_end], device="cuda")
        y = torch.full((s.n,), float("nan"), dtype=torch.float64, device="cuda")
        ys.append(s.shard_finish(total, xs, 1.0, 0.0, y).cpu().numpy())
        yab = torch.tensor(y0[s.row_begin:s.row_end], device="cuda")
        yabs.append(s.shard_finish(total, xs, W.ALPHA, W.BETA, yab).cpu().numpy())
        s.free()
    monkeypatch.delenv("NFFT4GP_AMD_SHARD_SPLIT")
    rec = {"y": np.concatenate(ys), "y_ab": np.concatenate(yabs)}
    ref = oracle_ref(name)
    e = {k: rel(rec[k], ref[k]) for k in rec}
    if bits == 64:
        full = W.make_op(amd, name, 0, bits)
        xd = torch.tensor(x, device="cuda")
        e["y_whole"] = rel(rec["y"], full.matsymv(xd).cpu().numpy())
        yab = full.matsymv(xd, W.ALPHA, W.BETA, torch.tensor(y0, device="cuda"))
        e["y_ab_whole"] = rel(rec["y_ab"], yab.cpu().numpy())
        full.free()
    print(f"{name} S {S} bits {bits}: " + ", ".join(f"{k} {v:.2e}" for k, v in e.items()))
    assert not np.isnan(rec["y"]).any(), "NaN survives beta = 0"
    assert max(e["y"], e["y_ab"]) <= (TOL_TIGHT if bits == 64 else TOL_CONTRACT), e
    if bits == 64:
        assert max(e["y_whole"], e["y_ab_whole"]) <= 1e-12, e

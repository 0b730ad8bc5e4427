"""gp_fit (the library's Adam on Nfft4GPGpProblemLoss) and gp_model (solve once, keep a FittedModel).

Base case: n = 1500, four 1-D windows, Gaussian, y = sum_c sin(2 pi x_c) + 0.1 noise, 4 fixed Rademacher probes,
30 Lanczos steps per loss, the operator's deterministic matvec on."""
import numpy as np
import pytest

import preconditioned_additive_gaussian_processes_with_fourier_acceleration_amd as amd

pytestmark = pytest.mark.gpu

N, D, NVECS, MAXITS, STEPS, LR = 1500, 4, 4, 30, 3, 0.01


def inv_softplus(v):
    return float(np.log(np.expm1(v)))


HYPER0 = np.array([inv_softplus(1.0), inv_softplus(0.1), inv_softplus(0.05)])  # f, l, mu after the softplus


@pytest.fixture(scope="module")
def base(torch_cuda):
    rng = np.random.default_rng(2024)
    X = rng.random((N, D))
    y = np.sin(2 * np.pi * X).sum(axis=1) + 0.1 * rng.standard_normal(N)
    R = np.where(rng.random((N, NVECS)) < 0.5, -1.0, 1.0)
    win = np.arange(D, dtype=np.int32)
    op = amd.NFFTAdditiveKernel(X, win, D, 1)
    op.set_deterministic(True)
    out = dict(X=X, y=y, R=R, win=win, op=op, torch=torch_cuda)
    yield out
    op.free()


def fit(b, **kw):
    return amd.gp_fit(b["X"], b["win"], D, 1, b["y"], HYPER0, STEPS, lr=LR, tol=1e-12, op=b["op"], maxits=MAXITS,
                      nvecs=NVECS, rademacher=b["R"], **kw)


def hand_rolled(b):
    """Adam in Python over the existing gp_loss: the same library calls in the same order"""
    x, m, v = HYPER0.copy(), np.zeros(3), np.zeros(3)
    xs, losses, gnorms = [x.copy()], [], []
    for t in range(STEPS):
        loss, g = amd.gp_loss(b["X"], b["win"], D, 1, b["y"], x, maxits=MAXITS, nvecs=NVECS, rademacher=b["R"],
                              op=b["op"])
        m = 0.9 * m + (1 - 0.9) * g
        v = 0.999 * v + (1 - 0.999) * g * g
        x = x - LR * (m / (1 - 0.9 ** (t + 1.0))) / (np.sqrt(v / (1 - 0.999 ** (t + 1.0))) + 1e-8)
        xs.append(x.copy())
        losses.append(loss)
        gnorms.append(float(np.sqrt(np.sum(g * g))))
    return np.array(xs), np.array(losses), np.array(gnorms)


def test_gp_fit_matches_a_hand_rolled_loop(base):
    """Both run the same library calls in the same order: histories equal to 1e-10 relative."""
    hyper, loss, gnorm, flag = fit(base)
    hx, hl, hg = hand_rolled(base)
    assert flag == 1 and hyper.shape == (STEPS + 1, 3) and loss.shape == (STEPS,) and gnorm.shape == (STEPS,)
    assert np.array_equal(hyper[0], HYPER0)
    for name, a, r in (("hyper", hyper, hx), ("loss", loss, hl), ("grad norm", gnorm, hg)):
        err = float(np.max(np.abs(a - r) / np.abs(r)))
        print(f"gp_fit vs hand-rolled loop, {name}: {err:.2e} relative")
        assert err <= 1e-10, (name, err)
    assert np.all(np.isfinite(loss)) and np.any(hyper[-1] != HYPER0)


def test_mask_freezes_a_hyperparameter(base):
    hyper, loss, gnorm, flag = fit(base, mask=[1, 0, 1])
    assert flag == 1
    assert np.all(hyper[:, 1] == HYPER0[1])
    assert np.all(hyper[-1, [0, 2]] != HYPER0[[0, 2]])


def test_fit_then_serve(base):
    """gp_fit for 3 steps from l ~ 0.1, gp_model, then 300 test points inside the training range against the existing
    gp_predict at the same hyperparameters: two NFFT approximations of one dense product (each e_train, the matvec's
    own distance from the dense product at the training points, with a margin of 2) plus the FGMRES tolerance:
    |difference| <= (4 e_train + 1e-7) max|mean|."""
    torch = base["torch"]
    X, y, win, op = base["X"], base["y"], base["win"], base["op"]
    hyper = fit(base)[0][-1]
    model = amd.gp_model(X, win, D, 1, y, hyper, op=op)
    rng = np.random.default_rng(7)
    lo, hi = X.min(axis=0), X.max(axis=0)
    Xp = lo + (hi - lo) * rng.random((300, D))
    mean = model.predict(Xp)
    assert model.n_outside == 0
    ref, _ = amd.gp_predict(X, Xp, win, D, 1, y, hyper)
    # e_train at the fitted hyperparameters (gp_model left op set up with them), as in test_gpu_model's check 3
    f, l, mu = model.f, model.l, model.mu
    a = rng.standard_normal(N)
    dense = np.zeros(N)
    for c in range(D):
        r = X[:, c][:, None] - X[:, c][None, :]
        dense += np.exp(-r * r / (2 * l * l)) @ a
    dense *= f * f / D
    mv = op.matsymv(torch.tensor(a, device="cuda")).cpu().numpy() - f * f * mu * a
    e_train = np.max(np.abs(mv - dense)) / np.max(np.abs(dense))
    diff = np.max(np.abs(mean - ref))
    bound = (4 * e_train + 1e-7) * np.max(np.abs(ref))
    print(f"fit then serve: f {f:.4f} l {l:.4f} mu {mu:.4f}; |model - gp_predict| {diff:.3e}, bound {bound:.3e} "
          f"(e_train {e_train:.3e}, max|mean| {np.max(np.abs(ref)):.3f})")
    truth = np.sin(2 * np.pi * Xp).sum(axis=1)
    rmse = float(np.sqrt(np.mean((mean - truth) ** 2)))
    rmse0 = float(np.sqrt(np.mean((np.mean(y) - truth) ** 2)))
    print(f"fit then serve: RMSE {rmse:.4f} against {rmse0:.4f} for the training mean")
    assert diff <= bound, (diff, bound)
    assert rmse < rmse0
    model.free()

"""CPU-side checks of the two-slice smoothing moments (``include/mmf.h``: ``MmfPfSmoothPairArgs`` /
``mmf_pf_smooth_pair_moments``) and of the EM refit built on them: the entry point refuses bad arguments on the host,
before any HIP call; the Python switches refuse what they cannot do; the M-step's known answers; the fp64 reference of the
GPU tests (``_smooth_cases.reference``) is held to its own identities, with the difference ``X - F`` in either precision,
and to the exact linear-Gaussian EM step.  (The struct's layout: ``test_abi_cpu.py``, for every struct of the binding.)"""
import ctypes
import inspect
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2

_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "weights", "logd", "workspace",
             "residual_mean", "residual_second_moment")


def _args(**over):
    from multimodalfilter_amd import _abi

    return sc.host_args(_abi.MmfPfSmoothPairArgs, _POINTERS, **{**dict(T=4, N=2, M=64, d=3), **over})


def test_pair_moments_refuse_bad_arguments_on_the_host():
    """Nulls and negative sizes -> ``MMF_EINVAL``; ``d``, ``M`` or ``N`` beyond the limits -> ``MMF_ETOOLARGE``; no
    trajectories or no transition (``T < 2``) -> a successful no-op.  All decided before any HIP call: the pointers are host
    memory and never dereferenced, and the stream is null."""
    lib = sc.lib()
    call = lambda **over: lib.mmf_pf_smooth_pair_moments(ctypes.byref(_args(**over)), None)
    assert lib.mmf_pf_smooth_pair_moments(None, None) == EINVAL
    for field in ("states_steps", "loglik_steps", "scale_tril", "weights", "pred_steps", "logd", "workspace", "residual_mean",
                  "residual_second_moment"):
        assert call(**{field: None}) == EINVAL, field
    assert call(d=0) == EINVAL and call(d=-1) == EINVAL and call(d=5) == ETOOLARGE
    assert call(M=0) == EINVAL and call(M=-3) == EINVAL and call(M=65537) == ETOOLARGE
    assert call(T=-1) == EINVAL and call(N=-1) == EINVAL and call(N=65536) == ETOOLARGE
    assert call(d=5, states_steps=None) == EINVAL  # an invalid call is invalid whatever its size
    assert call(N=0) == 0 and call(T=0) == 0 and call(T=1) == 0  # T < 2: no transition, nothing is written
    assert call(N=0, M=65536, d=4) == 0 and call(N=0, M=65537) == ETOOLARGE  # (the limits hold for the no-ops too)
    assert call(N=0, logw_in_steps=None) == 0  # the optional one
    # without a second step there is nothing to read or write beyond the history
    nothing = dict(pred_steps=None, logd=None, workspace=None, residual_mean=None, residual_second_moment=None)
    assert call(T=0, **nothing) == 0 and call(T=1, **nothing) == 0
    assert call(T=2, N=0, pred_steps=None) == EINVAL and call(T=2, N=0, workspace=None) == EINVAL


def test_workspace_size_is_the_documented_one():
    lib = sc.lib()
    size = lib.mmf_pf_smooth_pair_workspace_floats
    for T, N, M, d in [(5, 3, 300, 3), (2, 1, 1, 1), (40, 8, 512, 4), (5, 3, 64, 2), (5, 3, 65, 2)]:
        assert size(T, N, M, d) == (T - 1) * N * ((M + 63) // 64) * (1 + d + d * (d + 1) // 2), (T, N, M, d)
    assert size(1, 3, 300, 3) == 0 and size(0, 3, 300, 3) == 0 and size(5, 0, 300, 3) == 0
    assert size(5, 3, 300, 5) == 0 and size(5, 3, 65537, 3) == 0 and size(5, 3, 0, 3) == 0


def test_smooth_and_run_filter_refuse_transition_moments_with_another_method():
    """The two-slice moments belong to ``method="marginal"``.  The switch is the filter's ``record_transition_moments`` (a
    ``record_*`` attribute, default off: ``smooth``'s own parameter list is what it was); with it set another method is a
    ``ValueError`` before the history is looked at (there is none here) and, in ``run_filter``, before the run (the
    trajectories are not even read)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.record_history = True
    assert pf.record_transition_moments is False
    assert list(inspect.signature(pf.smooth).parameters) == ["lag", "method", "num_draws"]
    with pytest.raises(AssertionError, match="history"):  # switch off: every method goes on to the history, as before
        pf.smooth(method="ancestry")
    pf.record_transition_moments = True
    for method in ("ancestry", "simulation"):
        with pytest.raises(ValueError, match="record_transition_moments"):
            pf.smooth(method=method)
    with pytest.raises(ValueError, match="bogus"):
        pf.smooth(method="bogus")
    with pytest.raises(ValueError, match="fixed-lag"):  # the older refusals come first, as they did
        pf.smooth(lag=2, method="marginal")
    with pytest.raises(AssertionError, match="history"):  # the marginal method takes it and goes on to the history
        pf.smooth(method="marginal")
    assert pf.last_smoothed is None
    pf.record_transition_moments = False
    p = inspect.signature(evaluation.run_filter).parameters["smooth_transition_moments"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is False
    for method in ("ancestry", "simulation"):
        with pytest.raises(ValueError, match="smooth_transition_moments"):
            evaluation.run_filter(pf, None, smooth_method=method, smooth_transition_moments=True)
    assert pf.record_history is True and pf.record_belief is False and pf.record_transition_moments is False  # nothing was switched


def test_process_noise_m_step_known_answers():
    from multimodalfilter_amd.evaluation import process_noise_m_step

    rng = np.random.default_rng(3)
    A = rng.normal(size=(5, 2, 3, 3))
    m2 = torch.from_numpy(A @ A.transpose(0, 1, 3, 2) + 0.1 * np.eye(3))
    rec = SimpleNamespace(residual_second_moment=m2)
    for start in (0, 2):
        Q = m2[start:].mean(dim=(0, 1))
        L = process_noise_m_step(rec, start=start)
        assert L.shape == (3, 3) and L.dtype == m2.dtype and torch.equal(L, torch.tril(L)) and bool((torch.diagonal(L) > 0).all())
        assert float((L @ L.t() - Q).abs().max()) <= 1e-12
        Ld = process_noise_m_step(rec, diagonal=True, start=start)
        assert torch.equal(Ld, torch.diag(torch.diagonal(Ld)))
        assert float((torch.diagonal(Ld) ** 2 - torch.diagonal(Q)).abs().max()) <= 1e-12
    # a constant record: the factor is that of the one matrix; float32 records give float32 factors
    one = torch.tensor([[4.0, 2.0], [2.0, 5.0]])
    L = process_noise_m_step(SimpleNamespace(residual_second_moment=one.expand(3, 2, 2, 2)))
    assert L.dtype == torch.float32 and torch.allclose(L, torch.tensor([[2.0, 0.0], [1.0, 2.0]]), rtol=0, atol=1e-6)
    Ld = process_noise_m_step(SimpleNamespace(residual_second_moment=one.expand(3, 2, 2, 2)), diagonal=True)
    assert torch.allclose(Ld, torch.diag(torch.tensor([2.0, 5.0 ** 0.5])), rtol=0, atol=1e-6)
    # refusals name the first offending (t, n), t counted from the record's step 0
    bad = m2.clone()
    bad[3, 1, 0, 2] = float("nan")
    bad[4, 0, 1, 1] = float("inf")
    with pytest.raises(ValueError, match=r"non-finite.*\(3, 1\)"):
        process_noise_m_step(SimpleNamespace(residual_second_moment=bad))
    with pytest.raises(ValueError, match=r"non-finite.*\(3, 1\)"):
        process_noise_m_step(SimpleNamespace(residual_second_moment=bad), start=2, diagonal=True)
    neg = -m2.clone()
    with pytest.raises(ValueError, match=r"not positive definite.*\(0, 0\)"):
        process_noise_m_step(SimpleNamespace(residual_second_moment=neg))
    with pytest.raises(ValueError, match=r"not positive definite.*\(1, 0\)"):
        process_noise_m_step(SimpleNamespace(residual_second_moment=neg), start=1, diagonal=True)
    flat = torch.zeros((2, 2, 3, 3), dtype=torch.float64)  # rank 0: no Cholesky factor
    with pytest.raises(ValueError, match=r"not positive definite.*\(0, 0\)"):
        process_noise_m_step(SimpleNamespace(residual_second_moment=flat))
    with pytest.raises(ValueError, match="residual_second_moment"):
        process_noise_m_step(SimpleNamespace(covariance=m2))  # a record without the moments
    with pytest.raises(ValueError, match="no transitions"):
        process_noise_m_step(rec, start=5)


def test_model_noise_setters_and_fit_refusal():
    """``set_scale_tril`` copies in place (the parameter object stays), the diagonal-only model refuses off-diagonal mass,
    and ``fit_process_noise`` refuses a model without the method before any run."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import base, evaluation

    door = mmf.door_models.DoorParticleFilter().eval()   # the diagonal-only dynamics
    push = mmf.push_models.PushParticleFilter().eval()
    assert door.dynamics_model.diagonal_noise is True and push.dynamics_model.diagonal_noise is False
    for f in (door, push):
        dyn = f.dynamics_model
        d = dyn.state_dim
        store = dyn.Q_scale_tril_diag if dyn.diagonal_noise else dyn.Q_scale_tril
        where = store.data_ptr()
        L = torch.diag(torch.linspace(0.01, 0.03, d))
        dyn.set_scale_tril(L.double())
        assert store.data_ptr() == where and store.requires_grad is False and torch.equal(dyn.scale_tril(), L)
        low = L.clone()
        low[d - 1, 0] = 0.004
        if dyn.diagonal_noise:
            with pytest.raises(ValueError, match="diagonal"):
                dyn.set_scale_tril(low)
        else:
            dyn.set_scale_tril(low)
            assert torch.equal(dyn.scale_tril(), low)
        for wrong, what in ((low.t(), "lower-triangular"), (-L, "positive diagonal"), (L[:-1], "factor"),
                            (L * float("nan"), "finite")):
            with pytest.raises(ValueError, match=what):
                dyn.set_scale_tril(wrong)

    class Fixed(base.DynamicsModel):
        def forward(self, *, initial_states, controls):
            return initial_states, None

    with pytest.raises(TypeError, match="set_scale_tril"):
        evaluation.fit_process_noise(SimpleNamespace(dynamics_model=Fixed(state_dim=2)), None)
    with pytest.raises(TypeError, match="smooth_method"):
        evaluation.fit_process_noise(push, None, smooth_method="ancestry")


@pytest.mark.parametrize("M,d,full,ll_scale", [(37, 2, False, 0.5), (150, 3, True, 0.5), (150, 4, True, 50.0)])
def test_reference_row_marginal_is_the_marginal_smoothers_weight(M, d, full, ll_scale):
    """``sum_j xi[i, j] = W_{t|T}[i]`` and ``sum_ij xi = 1`` to 1e-12 inside the two-slice reference; its ``W_{t|T}`` are those
    of the same reference with the difference ``X - F`` formed in fp64 (what the marginal smoother's kernels are held to) up
    to the fp32 rounding of that difference, and, with dead particles, zero where theirs are."""
    L = sc.tril(d, full)
    X, F, ll, lw = sc.make_case(5, 3, M, d, (1e-3, 1e-2, 0.3), ll_scale, L, seed=7 + M + d)
    ll[:, 1, ::3] = -np.inf
    X[:, 1, ::3] = np.inf
    F[:, 1, ::3] = np.inf
    ref = sc.reference(X, F, ll, lw, L)
    assert np.abs(ref["total"] - 1.0).max() <= 1e-12
    assert np.abs(ref["row_marginal"] - ref["weights"][:-1]).max() <= 1e-12
    assert np.abs(ref["weights"].sum(-1) - 1.0).max() <= 1e-12
    assert np.isfinite(ref["residual_mean"]).all() and np.isfinite(ref["residual_second_moment"]).all()
    S = sc.reference(X.astype(np.float64), F.astype(np.float64), ll, lw, L)["weights"]  # (as the marginal GPU test calls it)
    assert (S[:, 1, ::3] == 0).all() and (ref["weights"][:, 1, ::3] == 0).all()
    # the fp32 difference is off by <= 2^-24 |x| ~ 1e-7, i.e. <= 1e-5 whitened at noise 0.01, against distances of a few
    assert np.abs(ref["weights"] - S).max() <= 1e-3 * S.max()
    sym = ref["residual_second_moment"]
    assert np.abs(sym - sym.transpose(0, 1, 3, 2)).max() <= 1e-18
    assert (np.linalg.eigvalsh(sym) >= -1e-18).all()


_LG = dict(d=3, N=8, M=512, T=40, q_true=0.05, r=0.3, p0=0.1)


@pytest.mark.parametrize("q0", [0.15, 0.02])
def test_one_em_step_matches_the_exact_linear_gaussian_step(q0):
    """A random walk ``q = 0.05`` observed through ``z = x + 0.3 eps`` (d = 3, N = 8, T = 40), filtered by a bootstrap
    filter of M = 512 particles under the wrong noise ``q0``, all in fp64: the M-step from the particle two-slice moments,
    ``sqrt(mean diag Q)``, lands within 2 % of the exact Kalman / RTS EM step (a study of three seeds each measured
    0.5 % at the worst) and moves from ``q0`` towards 0.05."""
    c = SimpleNamespace(**_LG)
    rng = np.random.default_rng(101)
    m0 = rng.normal(size=(c.N, c.d))
    x = m0 + np.sqrt(c.p0) * rng.normal(size=(c.N, c.d))
    truth = np.zeros((c.T, c.N, c.d))
    for t in range(c.T):
        x = x + c.q_true * rng.normal(size=(c.N, c.d))
        truth[t] = x
    z = truth + c.r * rng.normal(size=truth.shape)
    X, F, ll = sc.bootstrap_filter_history(z, m0, c.p0, q0, c.r, c.M, seed=202)
    ref = sc.reference(X, F, ll, None, q0 * np.eye(c.d))
    q_pf = float(np.sqrt(np.mean(np.diagonal(ref["residual_second_moment"], axis1=-2, axis2=-1))))
    q_exact = sc.rts_em_step(z, m0, c.p0, q0, c.r)
    print(f"q0 {q0}: particle EM step {q_pf:.5f}, exact RTS EM step {q_exact:.5f}, ratio - 1 = {q_pf / q_exact - 1.0:+.2e}")
    assert abs(q_pf / q_exact - 1.0) <= 0.02
    assert (q_pf < q0) if q0 > c.q_true else (q_pf > q0)
    assert abs(q_pf - c.q_true) < abs(q0 - c.q_true)

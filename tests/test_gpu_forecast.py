"""k-step-ahead forecasts on the GPU: ``mmf_pf_predictive`` (``csrc/pf_predictive.hip``) against the fp64 definition of
``tests/_forecast_cases.py`` on its whole family and its bit-for-bit identities (two calls, a row alone, with and without a
truth, every subset of outputs); ``ParticleFilter.belief_forecast`` on a real door filter against a step-by-step composition;
the extended Kalman filter's forecasts against the closed form of a linear-Gaussian model; ``evaluation.forecast_filter``.

The bar: ``REL_TOL`` -- ``rel_err_elementwise(got, fp64, floor=1e-3)`` for ``log_score``, ``pit``, ``spread`` and ``crps``,
``rel_err`` for ``mean`` and ``covariance`` -- with NaN exactly where the definition puts it.  Every figure is printed before
it is asserted."""
import itertools

import numpy as np
import pytest
import torch

import _forecast_cases as fk
import _rts_cases as rc
import _smooth_cases as sc
from _summary_gpu import N, _same_bits, assert_repeatable, assert_subsets_match_full, guarded_call
from _tol import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

OUTPUTS = fk.OUTPUTS
NO_TRUTH = tuple(k for k in OUTPUTS if k not in fk.NEED_TRUTH)


def _run(case, want=None, rows=None):
    """``_abi.pf_predictive`` on a case (or on ``rows`` of it) with every output between guard rows; the outputs not in
    ``want`` are handed over as null and their buffers must come back untouched -> ``dict`` of device tensors (``None`` for
    those)."""
    from multimodalfilter_amd import _abi

    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    X, la, lb, y = (sc.to_device(pick(case[k])) for k in ("states", "log_a", "log_b", "truth"))
    L = sc.to_device(case["scale_tril"])
    if want is None:
        want = OUTPUTS if y is not None else NO_TRUTH
    R, M, d = X.shape
    tails = {"mean": (d,), "covariance": (d, d), "log_score": (), "pit": (d,), "spread": (d,), "crps": (d,)}
    return guarded_call(lambda out: _abi.pf_predictive(X, la, lb, L, y, **out), R, tails, want, OUTPUTS, f"M={M} d={d} R={R}")


def _hold(ref, got, what, worst=None):
    """The outputs against the reference (those the case has); returns the errors."""
    errs = {k: fk.compare(N(got[k]), ref[k], k, what) for k in OUTPUTS if ref[k] is not None}
    line = f"{what}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" (bar {REL_TOL:.0e})"
    if worst is None:
        print(line)
    for k, e in errs.items():
        assert e < REL_TOL, line
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), e)
    return errs


# ------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("M", fk.ALL_MS)
def test_kernel_holds_the_definition_on_the_family(M):
    worst, cases = {}, 0
    for M_, d, R, variant, scale in fk.family():
        if M_ != M:
            continue
        case, ref = fk.family_case(M, d, R, variant, scale)
        _hold(ref, _run(case), f"M={M} d={d} R={R} {variant} scale={scale}", worst)
        cases += 1
    print(f"M={M}: {cases} cases, worst " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()) + f" (bar {REL_TOL:.0e})")


def test_kernel_at_the_particle_limit():
    """32 workgroups per row, 16 j-tiles each."""
    case = fk.make_case(fk.MAX_M, 1, 1, "plain", 0.3)
    _hold(fk.reference(case), _run(case), f"M={fk.MAX_M} d=1")


def test_a_truth_fifty_sigmas_away_has_a_finite_log_score():
    for M in (1, 65, 513):
        for scale in fk.SCALES:
            case = fk.make_case(M, 3, 3, "far_truth", scale)
            got = _run(case)
            assert bool(torch.isfinite(got["log_score"]).all()) and bool((got["log_score"] < -0.5 * fk.FAR ** 2).all()), (M, scale)
            assert bool((got["pit"] == 1).all())  # (beyond every component)
            _hold(fk.reference(case), got, f"far truth M={M} scale={scale}")


def test_equal_centres_give_the_single_gaussian():
    from multimodalfilter_amd import evaluation

    for M in (2, 65, 513):
        for d in fk.DIMS:
            case, ref = fk.family_case(M, d, 3, "equal_centres", 0.3) if M <= fk.SMALL else (fk.make_case(M, d, 3, "equal_centres", 0.3), None)
            got = _run(case)
            L = torch.from_numpy(case["scale_tril"]).double()
            live = ~np.isnan(case["states"][:, :, 0])
            centre = torch.from_numpy(np.stack([case["states"][r][live[r]][0] for r in range(3)])).double()
            Q, y = (L @ L.t()).expand(3, d, d), torch.from_numpy(case["truth"]).double()
            want = {"mean": centre, "covariance": Q, "crps": evaluation.gaussian_crps(centre, Q, y),
                    "log_score": evaluation.gaussian_log_density(centre, Q, y)}
            errs = {k: fk.compare(N(got[k]), v.numpy(), k) for k, v in want.items()}
            print(f"equal centres M={M} d={d}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
            assert max(errs.values()) < REL_TOL, (M, d, errs)


# ------------------------------------------------------------------------------------------ 2. bit-for-bit identities
@pytest.mark.parametrize("M", [1, 65, 257, fk.I_BLOCK, fk.I_BLOCK + 1, fk.J_TILE + 1, fk.BIG_M])
def test_two_calls_a_row_alone_and_no_truth_give_the_same_bits(M):
    for d, variant, scale in ((1, "plain", 0.3), (3, "dead_row", 0.02), (4, "dead_particles", 3.0)):
        case = fk.make_case(M, d, 3, variant, scale)
        got = assert_repeatable(_run, case, OUTPUTS, range(3), (M, d, variant))
        blind = _run(dict(case, truth=None))
        for k in NO_TRUTH:
            assert _same_bits(blind[k], got[k]), (M, d, variant, k)


@pytest.mark.parametrize("M", [65, fk.I_BLOCK + 1])
def test_every_subset_of_outputs_writes_only_what_was_asked_for_with_the_same_bits(M):
    """All 63 non-empty subsets with a truth, the 7 of ``mean``, ``covariance`` and ``spread`` without one (the untouched
    buffers are checked inside ``_run``)."""
    case = fk.make_case(M, 3, 3, "plain", 0.3)
    full = assert_subsets_match_full(_run, case, OUTPUTS, what=(M,))
    blind = dict(case, truth=None)
    for n in range(1, len(NO_TRUTH) + 1):
        for want in itertools.combinations(NO_TRUTH, n):
            got = _run(blind, want)
            for k in want:
                assert _same_bits(got[k], full[k]), (M, want, k)


# ------------------------------------------------------------------------------------------ 3. ParticleFilter.belief_forecast
class _Counting:
    """A noise source that hands the draws of another one through and keeps their shapes."""

    def __init__(self, inner):
        self.inner, self.gaussians, self.uniforms = inner, [], []

    def gaussian(self, shape, *, like):
        self.gaussians.append(tuple(shape))
        return self.inner.gaussian(shape, like=like)

    def uniform(self, shape, *, like):
        self.uniforms.append(tuple(shape))
        return self.inner.uniform(shape, like=like)

    def draw_steps(self, *args, **kwargs):
        return self.inner.draw_steps(*args, **kwargs)


def _case_of(F, log_a, log_b, L, truth):
    flat = lambda x, tail: None if x is None else x.detach().cpu().numpy().reshape((-1,) + tail)
    n, N_, M, d = F.shape
    return dict(states=flat(F, (M, d)), log_a=flat(log_a, (M,)), log_b=flat(log_b, (M,)), scale_tril=N(L), truth=flat(truth, (d,)))


@pytest.mark.parametrize("M", [65, 513])
def test_belief_forecast_on_a_real_filter(M):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi
    from multimodalfilter_amd.utils import ReplayNoise, tree_map

    dev = sc.dev()
    T, N_, H = 6, 2, 3
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorParticleFilter", N_, M, T, dev)
    truth = traj["states"][1:]

    def forward():
        f.record_history = True
        f.noise = mmf.NoiseSource(31)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        return f.forward_loop(observations=obs, controls=ctrl)

    est = forward().clone()
    h = f.last_history
    kept = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in", "ancestors") if getattr(h, k) is not None}
    f.smooth(method="marginal")
    smoothed, smoothed_weights = f.last_smoothed, f.last_smoothed.weights.clone()
    f.belief_scores(truth)
    scores, scores_crps = f.last_scores, f.last_scores.crps.clone()

    g = torch.Generator().manual_seed(9)
    blocks = [torch.randn(((T - k) * N_, M, d), generator=g) for k in range(1, H)]
    f.noise = _Counting(ReplayNoise(gaussians=[b.clone() for b in blocks]))
    mean = f.belief_forecast(H, truth)
    torch.cuda.synchronize()
    rec = f.last_forecast
    assert f.noise.gaussians == [((T - 1) * N_, M, d), ((T - 2) * N_, M, d)] and f.noise.uniforms == []
    assert set(vars(rec)) == {"mean", "covariance", "spread", "error", "log_score", "pit", "crps", "horizon"} and rec.horizon == H
    assert rec.mean is mean and mean.shape == (H, T, N_, d) and rec.covariance.shape == (H, T, N_, d, d)
    assert rec.log_score.shape == (H, T, N_) and all(getattr(rec, k).shape == (H, T, N_, d) for k in ("spread", "error", "pit", "crps"))
    # NaN exactly where t + h > T - 1
    for k in ("mean", "covariance", "spread", "error", "log_score", "pit", "crps"):
        x = getattr(rec, k)
        for lead in range(1, H + 1):
            assert bool(torch.isfinite(x[lead - 1, :T - lead]).all()) and bool(torch.isnan(x[lead - 1, T - lead:]).all()), (k, lead)
    # lead 1: the kernel on the smoothers' own predictions
    pred, tril = f._smoothing_transition(h, "marginal")
    lead1 = torch.empty((T - 1, N_, d), device=dev)
    _abi.pf_predictive(pred, h.log_weights_in[:T - 1], h.log_likelihoods[:T - 1], tril, mean=lead1)
    assert torch.equal(lead1, mean[0, :T - 1])
    # every lead: a step-by-step composition, then the fp64 definition
    dyn = f.dynamics_model
    X = h.states
    for k in range(1, H + 1):
        n = T - k
        ctx = dyn.encode_controls(tree_map(ctrl, lambda c: c[k:T].reshape((n * N_,) + tuple(c.shape[2:]))))
        F = dyn.propagate_encoded(X[:n].reshape(n * N_, M, d).contiguous(), ctx, None).reshape(n, N_, M, d)
        case = _case_of(F, h.log_weights_in[:n], h.log_likelihoods[:n], tril, truth[k:])
        got = {name: getattr(rec, name)[k - 1, :n].reshape((n * N_,) + tuple(getattr(rec, name).shape[3:])) for name in OUTPUTS}
        _hold(fk.reference(case), got, f"M={M} lead {k}")
        assert torch.equal(rec.error[k - 1, :n], mean[k - 1, :n] - truth[k:])
        if k < H:
            X = F + (blocks[k - 1].to(dev) @ tril.t()).reshape(n, N_, M, d)
    assert bool((rec.crps >= 0)[torch.isfinite(rec.crps)].all()) and bool(((rec.pit >= 0) & (rec.pit <= 1))[torch.isfinite(rec.pit)].all())
    # the same blocks give the same forecasts; without the pair pass and without a truth the rest has the same bits
    f.noise = ReplayNoise(gaussians=[b.clone() for b in blocks])
    again = f.belief_forecast(H, truth)
    assert torch.equal(again.view(torch.int32), mean.view(torch.int32)) and f.last_forecast is not rec
    assert torch.equal(f.last_forecast.crps.view(torch.int32), rec.crps.view(torch.int32))
    f.noise = ReplayNoise(gaussians=[b.clone() for b in blocks])
    f.belief_forecast(H, crps=False)
    assert set(vars(f.last_forecast)) == {"mean", "covariance", "horizon"}
    assert torch.equal(f.last_forecast.covariance.view(torch.int32), rec.covariance.view(torch.int32))
    # one lead draws nothing; horizons beyond the data are NaN and draw only what a later lead reads
    f.noise = _Counting(mmf.NoiseSource(5))
    one = f.belief_forecast(1, truth)
    assert f.noise.gaussians == [] and f.noise.uniforms == [] and torch.equal(one[0].view(torch.int32), mean[0].view(torch.int32))
    f.noise = _Counting(mmf.CounterNoise(5))
    far = f.belief_forecast(T + 2, truth)
    assert far.shape == (T + 2, T, N_, d) and bool(torch.isnan(far[T - 1:]).all()) and bool(torch.isfinite(far[T - 2, 0]).all())
    assert f.noise.gaussians == [((T - k) * N_, M, d) for k in range(1, T - 1)]
    assert torch.equal(far[0].view(torch.int32), mean[0].view(torch.int32))
    # nothing else moved
    assert f.last_history is h and f.last_smoothed is smoothed and f.last_scores is scores
    assert torch.equal(smoothed.weights, smoothed_weights) and torch.equal(scores.crps, scores_crps)
    for k, x in kept.items():
        assert torch.equal(getattr(h, k), x), k
    assert torch.equal(forward(), est)


# ------------------------------------------------------------------------------------------ 4. the extended Kalman filter
def test_ekf_lead_one_is_the_smoothers_prediction_bit_for_bit():
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    T, N_ = 6, 3
    torch.manual_seed(3)
    f = mmf.door_models.DoorKalmanFilter().to(dev).eval()
    from multimodalfilter_amd import synthetic
    from oracle import models as om

    d = om.TASKS["door"].state_dim
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N_, seed=17).items()}
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N_, d, d)
    f.record_history = True
    f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
    est = f.forward_loop(observations={k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}, controls=traj["controls"][1:])
    h = f.last_history
    means, covs = h.means.clone(), h.covariances.clone()
    f.smooth()
    smoothed = f.last_smoothed
    mu_pred, A, tril = f._smoothing_transition(h)
    mean = f.belief_forecast(3, traj["states"][1:])
    rec = f.last_forecast
    assert set(vars(rec)) == {"mean", "covariance", "error", "horizon"} and rec.horizon == 3 and rec.mean is mean
    assert torch.equal(mean[0, :T - 1], mu_pred)
    want = A @ h.covariances[:T - 1] @ A.transpose(-1, -2) + tril @ tril.t()
    assert rel_err(rec.covariance[0, :T - 1], want) < 1e-6
    for lead in (1, 2, 3):
        assert bool(torch.isfinite(mean[lead - 1, :T - lead]).all()) and bool(torch.isnan(mean[lead - 1, T - lead:]).all())
        assert bool(torch.isnan(rec.covariance[lead - 1, T - lead:]).all())
        assert torch.equal(rec.error[lead - 1, :T - lead], mean[lead - 1, :T - lead] - traj["states"][1:][lead:])
        sc.assert_symmetric_psd(0.5 * (rec.covariance[lead - 1, :T - lead] + rec.covariance[lead - 1, :T - lead].transpose(-1, -2)), lead)
    assert f.last_history is h and f.last_smoothed is smoothed and torch.equal(h.means, means) and torch.equal(h.covariances, covs)
    assert torch.equal(h.means, est)


@pytest.mark.parametrize("d", rc.LG_DIMS)
def test_ekf_forecasts_of_a_linear_gaussian_model_against_the_closed_form(d):
    """``x' = A(u) x + u b + w``: the forecast at lead ``h`` from ``(m, P)`` is ``Phi m + sum_k Psi_k u_k b`` with covariance
    ``Phi P Phi^T + sum_k Psi_k Q Psi_k^T``, ``Psi_k = A(u_{t+h}) .. A(u_{t+k+1})`` and ``Phi = Psi_0``: products written out
    in fp64, no recursion over beliefs."""
    from multimodalfilter_amd import filters

    dev = sc.dev()
    c = rc.lg_model(d)
    dyn, sensor = rc.lg_filter_models(d, dev)
    f = filters.VirtualSensorExtendedKalmanFilter(dynamics_model=dyn, virtual_sensor_model=sensor).to(dev).eval()
    y, u = rc._t(c["y"], torch.float32).to(dev), rc._t(c["u"], torch.float32).to(dev)
    f.record_history = True
    f.initialize_beliefs(mean=rc._t(c["m_init"], torch.float32).to(dev),
                         covariance=rc._t(c["P_init"], torch.float32).to(dev)[None].expand(rc.LG_N, d, d))
    f.forward_loop(observations=y, controls=u)
    h = f.last_history
    T, N_, H = rc.LG_T, rc.LG_N, 4
    mean = f.belief_forecast(H)
    rec = f.last_forecast
    assert set(vars(rec)) == {"mean", "covariance", "horizon"}
    A0, A1, b, L, u64 = (rc._t(c[k], torch.float64) for k in ("A0", "A1", "b", "L", "u"))
    Q = L @ L.t()
    m64, P64 = h.means.double().cpu(), h.covariances.double().cpu()
    for lead in range(1, H + 1):
        want_m, want_P = torch.zeros((T - lead, N_, d), dtype=torch.float64), torch.zeros((T - lead, N_, d, d), dtype=torch.float64)
        for t in range(T - lead):
            for n in range(N_):
                At = [A0 + u64[t + k, n, 0] * A1 for k in range(1, lead + 1)]  # A(u_{t+1}) .. A(u_{t+lead})
                psi = [torch.eye(d, dtype=torch.float64)]                      # Psi_lead, .., Psi_0
                for A in reversed(At):
                    psi.append(psi[-1] @ A)
                psi = psi[::-1]                                                # psi[k] = A(u_{t+lead}) .. A(u_{t+k+1})
                want_m[t, n] = psi[0] @ m64[t, n] + sum(psi[k] @ (u64[t + k, n, 0] * b) for k in range(1, lead + 1))
                want_P[t, n] = psi[0] @ P64[t, n] @ psi[0].t() + sum(psi[k] @ Q @ psi[k].t() for k in range(1, lead + 1))
        e_m, e_P = rel_err(mean[lead - 1, :T - lead], want_m, dims=1), rel_err(rec.covariance[lead - 1, :T - lead], want_P)
        print(f"d={d} lead {lead}: mean {e_m:.3e}, covariance {e_P:.3e} (bar {REL_TOL:.0e})")
        assert e_m < REL_TOL and e_P < REL_TOL
        assert bool(torch.isnan(mean[lead - 1, T - lead:]).all())
    # state-dependent process noise is refused as the smoother refuses it
    dyn, sensor = rc.lg_filter_models(d, dev, state_dependent_noise=True)
    g = filters.VirtualSensorExtendedKalmanFilter(dynamics_model=dyn, virtual_sensor_model=sensor).to(dev).eval()
    g.last_history = h
    with pytest.raises(ValueError, match="^belief_forecast needs one process-noise scale_tril"):
        g.belief_forecast(2)


# ------------------------------------------------------------------------------------------ 5. evaluation.forecast_filter
def test_forecast_filter_returns_both_records_and_puts_the_switches_back():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N_, M, T, H = 3, 64, 6, 3
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorCrossmodalParticleFilter", N_, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    plain = evaluation.run_filter(f, traj)
    f.noise = mmf.CounterNoise(7)
    est, rec = evaluation.forecast_filter(f, traj, H)
    assert f.record_history is False and f.record_belief is False and torch.equal(est, plain)
    assert rec is f.last_forecast and rec.horizon == H and rec.crps.shape == (H, T, N_, d) and rec.log_score.shape == (H, T, N_)
    h = f.last_history
    assert torch.equal(rec.error[0, :T - 1], rec.mean[0, :T - 1] - traj["states"][2:])
    summary = evaluation.forecast_summary(rec, start=0)
    assert set(summary) == {"rmse", "crps", "log_score", "pit_mean", "count"} and summary["count"].tolist() == [(T - k) * N_ for k in (1, 2, 3)]
    assert summary["rmse"].shape == (H, d) and summary["log_score"].shape == (H,) and bool(torch.isfinite(summary["crps"]).all())
    assert torch.allclose(summary["crps"][0], rec.crps[0, :T - 1].double().mean((0, 1)).float(), rtol=1e-6)
    f.noise = mmf.CounterNoise(7)
    _, fast = evaluation.forecast_filter(f, traj, H, crps=False)
    assert set(vars(fast)) == {"mean", "covariance", "error", "log_score", "pit", "horizon"}
    assert torch.equal(fast.log_score.view(torch.int32), rec.log_score.view(torch.int32)) and h is not None

    # an extended Kalman filter: the closed forms of its Gaussian forecasts
    torch.manual_seed(3)
    kf = mmf.door_models.DoorKalmanFilter().to(dev).eval()
    plain = evaluation.run_filter(kf, traj)
    est, rec = evaluation.forecast_filter(kf, traj, H)
    assert kf.record_history is False and torch.equal(est, plain) and rec is kf.last_forecast
    assert set(vars(rec)) == {"mean", "covariance", "error", "log_score", "pit", "crps", "horizon"}
    truth = traj["states"][1:]
    for lead in range(1, H + 1):
        m, P, y = rec.mean[lead - 1, :T - lead], rec.covariance[lead - 1, :T - lead], truth[lead:]
        assert torch.equal(rec.crps[lead - 1, :T - lead], evaluation.gaussian_crps(m, P, y))
        assert torch.equal(rec.log_score[lead - 1, :T - lead], evaluation.gaussian_log_density(m, P, y))
        assert bool(((rec.pit[lead - 1, :T - lead] >= 0) & (rec.pit[lead - 1, :T - lead] <= 1)).all())
        for k in ("crps", "log_score", "pit"):
            assert bool(torch.isnan(getattr(rec, k)[lead - 1, T - lead:]).all()), (k, lead)
    assert set(evaluation.forecast_summary(rec, start=0)) == {"rmse", "crps", "log_score", "pit_mean", "count"}
    _, rec = evaluation.forecast_filter(kf, traj, H, crps=False)
    assert set(vars(rec)) == {"mean", "covariance", "error", "log_score", "pit", "horizon"}

    # refused before the run: an unscented filter, a fused Kalman filter, an LSTM baseline ({}: the trajectories are not read)
    ukf = mmf.filters.VirtualSensorUnscentedKalmanFilter(dynamics_model=mmf.door_models.DoorDynamicsModel(),
                                                         virtual_sensor_model=kf.virtual_sensor_model).to(dev).eval()
    with pytest.raises(ValueError, match="forecast_filter: VirtualSensorUnscentedKalmanFilter keeps no history"):
        evaluation.forecast_filter(ukf, {}, H)
    with pytest.raises(ValueError, match="^belief_forecast needs a history"):
        ukf.belief_forecast(H)
    with pytest.raises(ValueError, match="forecast_filter: DoorCrossmodalKalmanFilter keeps no history to forecast from"):
        evaluation.forecast_filter(mmf.door_models.DoorCrossmodalKalmanFilter().to(dev).eval(), {}, H)
    with pytest.raises(ValueError, match="forecast_filter: DoorLSTMFilter has no belief to roll out"):
        evaluation.forecast_filter(mmf.door_models.DoorLSTMFilter().to(dev).eval(), {}, H)

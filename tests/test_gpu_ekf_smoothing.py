"""RTS smoothing of the extended Kalman filters on the GPU: ``mmf_ekf_smooth`` (``csrc/ekf_smooth.hip``) against fp64 on the
family of ``tests/_rts_cases.py``, its bit-for-bit identities, ``VirtualSensorExtendedKalmanFilter.smooth`` end to end --
against the dense conditioning of a linear-Gaussian model and, for the built-in models, against the fp64 recursion on
Jacobians the test evaluates itself -- and ``evaluation.run_filter`` / ``fit_process_noise`` on a Kalman filter.

The error rule of the project: ``rel_err(got, fp64) < max(1e-4, 3 x rel_err(fp32 yardstick, fp64))``, every figure printed
before it is asserted."""
import itertools

import pytest
import torch

import _rts_cases as rc
from _tol import REL_TOL, rel_err

pytestmark = pytest.mark.gpu


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


def _hold(name, got, want, yard):
    """The error rule on one output; empty outputs (``T == 1`` has no transition) have nothing to compare."""
    if want.numel() == 0:
        assert got.numel() == 0, name
        return
    err, own = rel_err(got, want), rel_err(yard, want)
    bar = max(REL_TOL, 3.0 * own)
    print(f"{name}: err {err:.3e}  yardstick {own:.3e}  bar {bar:.3e}")
    assert err < bar, (name, err, bar)


class _Guarded:
    """A float32 device array of ``rows`` leading slices between ``GUARD_ROWS`` guard slices holding the sentinel."""

    def __init__(self, rows, tail, dev):
        self.full = torch.full((rows + 2 * rc.GUARD_ROWS,) + tuple(tail), rc.SENTINEL, dtype=torch.float32, device=dev)
        self.view = self.full[rc.GUARD_ROWS:rc.GUARD_ROWS + rows]

    def guards_intact(self):
        g = rc.GUARD_ROWS
        return bool((self.full[:g] == rc.SENTINEL).all()) and bool((self.full[self.full.shape[0] - g:] == rc.SENTINEL).all())

    def untouched(self):
        return bool((self.full == rc.SENTINEL).all())


def _run_kernel(T, N, d, lag, moments, dev):
    """``_abi.ekf_smooth`` on ``family_case(T, N, d)`` with every output and the workspace between guard rows."""
    from multimodalfilter_amd import _abi

    c = rc.family_case(T, N, d)
    mu, Sigma, A, pred, L = (rc._t(c[k], torch.float32).to(dev) for k in ("mu", "Sigma", "A", "mu_pred", "L"))
    Tm = max(T - 1, 0)
    out = {"mean": _Guarded(T, (N, d), dev), "cov": _Guarded(T, (N, d, d), dev), "gain": _Guarded(Tm, (N, d, d), dev),
           "Sigma_pred": _Guarded(Tm, (N, d, d), dev), "resid_mean": _Guarded(Tm, (N, d), dev),
           "resid_m2": _Guarded(Tm, (N, d, d), dev)}
    _abi.ekf_smooth(mu, Sigma, A, pred, L, lag, out["mean"].view, out["cov"].view, out["gain"].view, out["Sigma_pred"].view,
                    out["resid_mean"].view if moments else None, out["resid_m2"].view if moments else None)
    torch.cuda.synchronize()
    for k, g in out.items():
        assert g.guards_intact(), f"{k}: a guard row was written (T={T} N={N} d={d} lag={lag})"
    return out


@pytest.mark.parametrize("N,d,T", list(itertools.product(rc.NS, rc.DIMS, rc.TS)))
def test_kernel_against_fp64_on_the_family(N, d, T):
    """Every lag of ``LAGS`` at one shape: smoothed means, covariances and gains, and for the full smoother the two-slice
    moments, against the fp64 ``rts_reference``; guard rows around every output survive; with null moment pointers the
    moment buffers are not touched."""
    dev = _dev()
    for lag in rc.LAGS:
        want = rc.family_reference(T, N, d, lag, torch.float64)
        yard = rc.family_reference(T, N, d, lag, torch.float32)
        out = _run_kernel(T, N, d, rc.lag_of(lag, T), False, dev)
        assert out["resid_mean"].untouched() and out["resid_m2"].untouched(), "moments written through null pointers"
        for k in ("mean", "cov", "gain"):
            _hold(f"T={T} N={N} d={d} lag={lag} {k}", out[k].view, want[k], yard[k])
        if lag is None:
            out = _run_kernel(T, N, d, None, True, dev)
            for k in ("mean", "cov", "gain", "resid_mean", "resid_m2"):
                _hold(f"T={T} N={N} d={d} moments {k}", out[k].view, want[k], yard[k])


def _one_step_with_null_transition_arrays(mu, Sigma, L):
    """The header's promise for ``T == 1``: ``A``, ``mu_pred``, ``gain`` and ``Sigma_pred`` may be null -- the struct is filled
    here by hand, for the full smoother and a lag -- and the call copies ``(mu, Sigma)``."""
    import ctypes

    from multimodalfilter_amd import _abi

    for lag in (-1, 2):
        out_mu, out_S = torch.full_like(mu, rc.SENTINEL), torch.full_like(Sigma, rc.SENTINEL)
        a = _abi.MmfEkfSmoothArgs()
        a.T, a.N, a.d, a.lag = 1, mu.shape[1], mu.shape[2], lag
        a.mu, a.Sigma, a.q_tril, a.mu_s, a.Sigma_s = _abi.vp(mu), _abi.vp(Sigma), _abi.vp(L), _abi.vp(out_mu), _abi.vp(out_S)
        assert a.A is None and a.mu_pred is None and a.gain is None and a.Sigma_pred is None and a.resid_mean is None
        assert _abi.load().mmf_ekf_smooth(ctypes.byref(a), _abi.stream_of(mu)) == 0
        torch.cuda.synchronize()
        assert torch.equal(out_mu, mu) and torch.equal(out_S, Sigma), lag


@pytest.mark.parametrize("N,d", list(itertools.product(rc.NS, rc.DIMS)))
def test_kernel_identities_hold_bit_for_bit(N, d):
    """``lag = 0`` returns ``(mu, Sigma)``; ``lag >= T - 1`` -- the fixed-lag kernel -- gives the bits of the full sweep, which
    gives the same bits with and without the moments; ``T = 1`` copies the filtered belief."""
    dev = _dev()
    for T in rc.TS:
        c = rc.family_case(T, N, d)
        mu, Sigma = rc._t(c["mu"], torch.float32).to(dev), rc._t(c["Sigma"], torch.float32).to(dev)
        zero = _run_kernel(T, N, d, 0, False, dev)
        assert torch.equal(zero["mean"].view, mu) and torch.equal(zero["cov"].view, Sigma), T
        full = _run_kernel(T, N, d, None, False, dev)
        with_moments = _run_kernel(T, N, d, None, True, dev)
        for k in ("mean", "cov", "gain"):
            assert torch.equal(full[k].view, with_moments[k].view), (T, k)
        for lag in (max(T - 1, 0), T + 3, 0x7FFFFFFF):
            lagged = _run_kernel(T, N, d, lag, False, dev)
            for k in ("mean", "cov", "gain"):
                assert torch.equal(lagged[k].view, full[k].view), (T, lag, k)
        if T == 1:
            assert torch.equal(full["mean"].view, mu) and torch.equal(full["cov"].view, Sigma)
            _one_step_with_null_transition_arrays(mu, Sigma, rc._t(c["L"], torch.float32).to(dev))
        if T > 2:  # a proper lag is not the full smoother (the comparison above is not vacuous)
            assert not torch.equal(_run_kernel(T, N, d, 1, False, dev)["mean"].view, full["mean"].view)


# ------------------------------------------------------------------------------ end to end, a linear-Gaussian user model
@pytest.mark.parametrize("d", rc.LG_DIMS)
def test_smooth_of_a_linear_gaussian_user_model_against_dense_conditioning(d):
    """A ``base.DynamicsModel`` in torch ops with a control-dependent transition matrix and a row-wise virtual sensor, run
    through the Python loop of steps: ``smooth()``, ``smooth(2)`` and the two-slice moments against the joint Gaussian
    conditioned densely in fp64 (no recursion); the yardstick is the same conditioning in float32.  A smoother that pairs
    ``means[t]`` with ``controls[t]`` instead of ``controls[t + 1]`` misses this by orders of magnitude
    (``test_rts_cases_cpu.py``)."""
    from multimodalfilter_amd import filters

    dev = _dev()
    c = rc.lg_model(d)
    dyn, sensor = rc.lg_filter_models(d, dev)
    f = filters.VirtualSensorExtendedKalmanFilter(dynamics_model=dyn, virtual_sensor_model=sensor).to(dev).eval()
    y, u = rc._t(c["y"], torch.float32).to(dev), rc._t(c["u"], torch.float32).to(dev)
    m0 = rc._t(c["m_init"], torch.float32).to(dev)
    P0 = rc._t(c["P_init"], torch.float32).to(dev)[None].expand(rc.LG_N, d, d)

    f.initialize_beliefs(mean=m0, covariance=P0)
    plain = f.forward_loop(observations=y, controls=u)
    assert f.last_history is None
    f.record_history = True
    f.initialize_beliefs(mean=m0, covariance=P0)
    est = f.forward_loop(observations=y, controls=u)
    assert torch.equal(est, plain)
    h = f.last_history
    assert h.means.shape == (rc.LG_T, rc.LG_N, d) and h.covariances.shape == (rc.LG_T, rc.LG_N, d, d) and h.controls is u
    assert torch.equal(h.means, est) and torch.equal(h.covariances[-1], f.belief_covariance)

    for lag in (None, 2, 0):
        want, yard = rc.dense_smoother(d, torch.float64, lag), rc.dense_smoother(d, torch.float32, lag)
        mean = f.smooth(lag)
        rec = f.last_smoothed
        assert rec.lag == lag and rec.method == "rts" and not hasattr(rec, "residual_mean")
        assert rec.gain.shape == (rc.LG_T - 1, rc.LG_N, d, d)
        _hold(f"d={d} lag={lag} mean", mean, want["mean"], yard["mean"])
        _hold(f"d={d} lag={lag} cov", rec.covariance, want["cov"], yard["cov"])
        if lag == 0:
            assert torch.equal(mean, est) and torch.equal(rec.covariance, h.covariances)
    f.record_transition_moments = True
    want, yard = rc.dense_smoother(d, torch.float64), rc.dense_smoother(d, torch.float32)
    mean = f.smooth()
    rec = f.last_smoothed
    _hold(f"d={d} moments mean", mean, want["mean"], yard["mean"])
    _hold(f"d={d} residual_mean", rec.residual_mean, want["resid_mean"], yard["resid_mean"])
    _hold(f"d={d} residual_second_moment", rec.residual_second_moment, want["resid_m2"], yard["resid_m2"])
    with pytest.raises(ValueError, match="record_transition_moments"):
        f.smooth(1)


# ------------------------------------------------------------------------------ end to end, the built-in models
def _task_filter(cls, dev, T=12, N=5, seed=17):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic
    from oracle import models as om

    d = om.TASKS["door"].state_dim
    torch.manual_seed(3)
    f = mmf.model_types("door")[cls]().to(dev).eval()
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=seed).items()}
    return f, d, traj


def _filter_and_smooth(f, d, traj, record=True):
    N = traj["states"].shape[1]
    cov = (torch.eye(d, device=traj["states"].device) * 0.1)[None].expand(N, d, d)
    f.record_history = record
    f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
    est = f.forward_loop(observations={k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")},
                         controls=traj["controls"][1:])
    f.record_history = False
    return est


@pytest.mark.parametrize("cls", ["DoorKalmanFilter", "DoorMeasurementCrossmodalKalmanFilter"])
def test_smooth_of_the_builtin_filters_against_the_fp64_recursion(cls):
    """``T = 12``, ``N = 5`` synthetic trajectories.  The reference is ``rts_reference`` in fp64 on the recorded history and on
    Jacobians / predictions the test evaluates ITSELF, step by step, with ``means[t]`` and ``controls[t + 1]`` indexed
    explicitly.  The smoothed output has the same bits under both forms of the forward loop, and recording the history
    changes no bit of the estimates."""
    from multimodalfilter_amd import engine

    dev = _dev()
    T, N = 12, 5
    f, d, traj = _task_filter(cls, dev, T, N)
    plain = _filter_and_smooth(f, d, traj, record=False)
    assert f.last_history is None
    out = {}
    for form in (False, True):
        with engine.persistent_forms(ekf=form):
            est = _filter_and_smooth(f, d, traj)
            assert torch.equal(est, plain), "recording the history changed the estimates"
            h = f.last_history
            f.record_transition_moments = True
            mean = f.smooth()
            f.record_transition_moments = False
            out[form] = (mean, f.last_smoothed, h)
    for k in ("covariance", "gain", "residual_mean", "residual_second_moment"):
        assert torch.equal(getattr(out[False][1], k), getattr(out[True][1], k)), k
    assert torch.equal(out[False][0], out[True][0])

    mean, rec, h = out[True]
    controls = traj["controls"][1:]
    assert h.controls is not None and h.means.shape == (T, N, d) and h.covariances.shape == (T, N, d, d)
    dyn = f.dynamics_model
    As, preds = [], []
    with torch.no_grad():
        for t in range(T - 1):
            x, J, L = dyn.predict_with_jacobian(h.means[t].contiguous(), dyn.encode_controls(controls[t + 1].contiguous()))
            As.append(J.clone())
            preds.append(x.clone())
    A, pred = torch.stack(As).cpu(), torch.stack(preds).cpu()
    args = (h.means.cpu(), h.covariances.cpu(), A, pred, L.cpu())
    want, yard = rc.rts_reference(*args, None, torch.float64), rc.rts_reference(*args, None, torch.float32)
    _hold(f"{cls} mean", mean, want["mean"], yard["mean"])
    _hold(f"{cls} covariance", rec.covariance, want["cov"], yard["cov"])
    _hold(f"{cls} gain", rec.gain, want["gain"], yard["gain"])
    _hold(f"{cls} residual_mean", rec.residual_mean, want["resid_mean"], yard["resid_mean"])
    _hold(f"{cls} residual_second_moment", rec.residual_second_moment, want["resid_m2"], yard["resid_m2"])
    lagged = f.smooth(3)
    want3, yard3 = rc.rts_reference(*args, 3, torch.float64), rc.rts_reference(*args, 3, torch.float32)
    _hold(f"{cls} lag 3 mean", lagged, want3["mean"], yard3["mean"])
    _hold(f"{cls} lag 3 covariance", f.last_smoothed.covariance, want3["cov"], yard3["cov"])
    assert float((mean - plain).abs().max()) > 0.0 and torch.equal(mean[-1], plain[-1])  # smoothing moved all but the last step


# ------------------------------------------------------------------------------ evaluation
def test_run_filter_and_fit_process_noise_on_a_kalman_filter():
    from multimodalfilter_amd import evaluation, filters
    import multimodalfilter_amd as mmf

    dev = _dev()
    T, N = 12, 5
    f, d, traj = _task_filter("DoorKalmanFilter", dev, T, N)
    filtered = evaluation.run_filter(f, traj)
    est, rec = evaluation.run_filter(f, traj, smooth_lag=None, return_belief=True)
    assert rec is f.last_smoothed and rec.method == "rts" and rec.lag is None and not hasattr(rec, "residual_mean")
    assert est.shape == (T, N, d) and rec.covariance.shape == (T, N, d, d) and rec.gain.shape == (T - 1, N, d, d)
    assert torch.equal(est[-1], filtered[-1]) and not torch.equal(est, filtered)
    assert torch.equal(evaluation.run_filter(f, traj, smooth_method="rts"), est)  # naming the method smooths, as "marginal" does
    assert torch.equal(evaluation.run_filter(f, traj, smooth_lag=0), filtered)
    assert f.record_history is False and f.record_belief is False and f.record_transition_moments is False

    est2, rec = evaluation.run_filter(f, traj, smooth_lag=None, return_belief=True, smooth_transition_moments=True)
    assert torch.equal(est2, est) and rec.residual_second_moment.shape == (T - 1, N, d, d)
    L = evaluation.process_noise_m_step(rec, diagonal=f.dynamics_model.diagonal_noise)
    assert L.shape == (d, d) and bool(torch.isfinite(L).all()) and bool((torch.diagonal(L) > 0).all())
    assert f.record_transition_moments is False
    with pytest.raises(ValueError, match="record_transition_moments"):  # the moments are the full smoother's
        evaluation.run_filter(f, traj, smooth_lag=2, smooth_transition_moments=True)
    assert f.record_history is False and f.record_transition_moments is False

    dyn = f.dynamics_model
    first = dyn.scale_tril().detach().clone()
    factors = evaluation.fit_process_noise(f, traj, iterations=2)
    assert len(factors) == 3 and torch.equal(factors[0], first)
    for Lk in factors:
        assert Lk.shape == (d, d) and bool(torch.isfinite(Lk).all()) and torch.equal(Lk, torch.tril(Lk))
        assert bool((torch.diagonal(Lk) > 0).all())
    assert not torch.equal(factors[1], factors[0]) and not torch.equal(factors[2], factors[1])
    assert torch.equal(dyn.scale_tril(), factors[-1])
    assert f.record_history is False and f.record_belief is False and f.record_transition_moments is False

    ukf = filters.VirtualSensorUnscentedKalmanFilter(dynamics_model=f.dynamics_model,
                                                     virtual_sensor_model=f.virtual_sensor_model).eval()
    with pytest.raises(NotImplementedError, match="no smoother"):
        evaluation.run_filter(ukf, traj, smooth_lag=None)
    fused = mmf.model_types("door")["DoorCrossmodalKalmanFilter"]().to(dev).eval()
    with pytest.raises(AssertionError, match="keeps no history to smooth"):
        evaluation.run_filter(fused, traj, smooth_lag=None)

"""Marginal (forward-filter backward-smoothing) particle smoothing on the GPU (``include/mmf.h``: ``mmf_pf_smooth_marginal``;
``ParticleFilter.smooth(method="marginal")`` / ``evaluation.run_filter(smooth_method=)``).

The kernels are held to an fp64 restatement of the definition (``_smooth_cases.reference`` with the difference ``X - F`` in
fp64: ``_reference64`` below) at the project's bar (``_tol.REL_TOL`` through ``rel_err``, per trajectory so that a narrow cloud
is measured against its own scale); the weights to the bar against the norm of their row, the ESS to 1e-4 relative.  The
forward side is held to the loop it stands for, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _smooth_cases as sc
from _tol import REL_TOL, rel_err

CHUNK = 256  # rows / columns the pair kernels stage at a time (csrc/pf_smooth_math.h: kPairChunk)


def _reference64(X, F, ll, lw, L):
    """The shared definition with the difference ``X_{t+1}[j] - F_t[i]`` formed in fp64, as these kernels are held to it."""
    return sc.reference(X.astype(np.float64), F.astype(np.float64), ll, lw, L)


def _run(X, F, ll, lw, L, want_cov=True, want_ess=True):
    g = sc.gpu_marginal(X, F, ll, lw, L, want_cov=want_cov, want_ess=want_ess, want_logd=False)
    return g["weights"], g["mean"], g["cov"], g["ess"]


def _check(got, want, what):
    """Weights within the bar of their row's norm, means and covariances within the bar per trajectory, ESS to 1e-4 relative,
    ``cov`` symmetric bit for bit and PSD to ``-1e-4 x trace``.  Prints the figures before asserting."""
    weights, mean, cov, ess = got
    wweights, wmean, wcov, wess = want["weights"], want["mean"], want["cov"], want["ess"]
    N = wmean.shape[1]
    e_w = max(rel_err(weights[:, n], wweights[:, n], dims=1) for n in range(N))
    e_mean = max(rel_err(mean[:, n], wmean[:, n], dims=1) for n in range(N))
    e_cov = max(rel_err(cov[:, n], wcov[:, n], dims=2) for n in range(N))
    e_ess = float(np.abs(ess.double().cpu().numpy() / wess - 1.0).max())
    print(f"{what}: weights {e_w:.2e} mean {e_mean:.2e} cov {e_cov:.2e} ess {e_ess:.2e} (ess min {wess.min():.1f} max {wess.max():.1f})")
    for x in (weights, mean, cov, ess):
        assert bool(torch.isfinite(x).all()), what
    assert e_w <= REL_TOL, (what, e_w)
    assert e_mean <= REL_TOL, (what, e_mean)
    assert e_cov <= REL_TOL, (what, e_cov)
    assert e_ess <= 1e-4, (what, e_ess)
    assert float((weights.double().sum(-1) - 1.0).abs().max()) <= 1e-5, what
    sc.assert_symmetric_psd(cov, what)


# ------------------------------------------------------------------------------------------ 1. kernels against fp64
_WIDTHS = (1e-3, 1e-2, 0.3)


@pytest.mark.parametrize("ll_scale", [0.5, 50.0])
@pytest.mark.parametrize("d", [1, 2, 3, 4])
@pytest.mark.parametrize("M", [1, 37, 300, 2 * CHUNK + 88])
def test_marginal_kernels_match_fp64(M, d, ll_scale):
    """Three trajectories of widths 1e-3 / 1e-2 / 0.3 per call, T = 5; the process noise once diagonal and once a full lower
    triangle.  M = 300 runs one whole chunk and a part of one, M = 600 two and a part; at scale 50 a particle or two hold
    the filter's weight at every step, scale 0.5 keeps hundreds alive."""
    T, N = 5, 3
    for full in (False, True):
        L = sc.tril(d, full)
        X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, ll_scale, L, seed=1000 * M + 10 * d + int(ll_scale) + full)
        _check(_run(X, F, ll, lw, L), _reference64(X, F, ll, lw, L), f"M={M} d={d} scale={ll_scale} full={full}")


# ------------------------------------------------------------------------------------------ 2. edges
def test_single_step_and_single_particle():
    L = sc.tril(3, True)
    X, F, ll, lw = sc.make_case(1, 3, 300, 3, _WIDTHS, 0.5, L, seed=1)
    got = _run(X, F, ll, lw, L)
    _check(got, _reference64(X, F, ll, lw, L), "T=1")
    assert rel_err(got[0][0], sc.softmax_rows(ll[0].astype(np.float64) + lw[0]), dims=1) <= REL_TOL  # the filter's weights
    L = sc.tril(2, False)
    X, F, ll, lw = sc.make_case(5, 2, 1, 2, _WIDTHS, 0.5, L, seed=2)
    got = _run(X, F, ll, lw, L)
    _check(got, _reference64(X, F, ll, lw, L), "M=1")
    assert torch.equal(got[1].cpu(), torch.from_numpy(X[:, :, 0]))  # the one particle is the mean
    assert float(got[2].abs().max()) == 0.0 and bool((got[0] == 1).all()) and bool((got[3] == 1).all())


def test_dead_particles_and_a_single_heavy_particle():
    """-inf log-likelihoods on half a row at every step, ``inf`` in the dead rows of ``X`` and ``F``: a finite result equal to
    the reference over the rest, zero weight on the dead.  One particle with all the weight at the last step: step T - 2 is
    re-weighted by the transition into that particle alone."""
    T, N, M, d = 5, 3, 300, 3
    L = sc.tril(d, True)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=11)
    ll[:, 1, ::2] = -np.inf
    X[:, 1, ::2] = np.inf
    F[:, 1, ::2] = np.inf
    got = _run(X, F, ll, lw, L)
    _check(got, _reference64(X, F, ll, lw, L), "half dead")
    assert float(got[0][:, 1, ::2].abs().max()) == 0.0 and bool((got[0][:, 1, 1::2] > 0).any())
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=12)
    ll[-1, :, 17] = 60.0  # the others keep exp(-60) ~ 1e-26 of it
    got = _run(X, F, ll, lw, L)
    want = _reference64(X, F, ll, lw, L)
    _check(got, want, "one heavy particle")
    assert float(got[0][-1, :, 17].min()) >= 1.0 - 1e-6 and float(want["ess"][-1].max()) <= 1.0 + 1e-9
    # by the definition, with one column: W_{T-2|T}[i] is proportional to W_{T-2}[i] N(X_{T-1}[17]; F_{T-2}[i], L L^T)
    z = (X[-1, :, 17].astype(np.float64)[:, None, :] - F[-1].astype(np.float64)) @ np.linalg.inv(L.astype(np.float64)).T
    direct = sc.softmax_rows(ll[-2].astype(np.float64) + lw[-2] - 0.5 * (z * z).sum(-1))
    assert rel_err(got[0][-2], direct, dims=1) <= REL_TOL


@pytest.mark.parametrize("M", [300, 2 * CHUNK + 88])
def test_two_calls_and_split_batches_give_the_same_bits(M):
    """Fixed-order reductions: two calls on the same inputs return the same bits, and the call on N = 3 trajectories returns
    what three calls on one trajectory each do.  Outputs that are not asked for change nothing."""
    L = sc.tril(3, True)
    X, F, ll, lw = sc.make_case(5, 3, M, 3, _WIDTHS, 0.5, L, seed=3 + M)
    a, b = _run(X, F, ll, lw, L), _run(X, F, ll, lw, L)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for n in range(3):
        one = _run(X[:, n:n + 1], F[:, n:n + 1], ll[:, n:n + 1], lw[:, n:n + 1], L)
        for x, y in zip(a, one):
            assert torch.equal(x[:, n:n + 1], y), n
    bare = _run(X, F, ll, lw, L, want_cov=False, want_ess=False)
    assert torch.equal(bare[0], a[0]) and torch.equal(bare[1], a[1])
    uniform = _run(X, F, ll, None, L)  # null incoming log-weights are uniform ones
    zeros = _run(X, F, ll, np.zeros_like(lw), L)
    for x, y in zip(uniform, zeros):
        assert torch.equal(x, y)


def test_a_bad_noise_factor_gives_nan_and_no_fault():
    """A zero, negative or non-finite diagonal entry of ``L``: every result is NaN (T = 1, where ``L`` is not used, included)."""
    L = sc.tril(3, True)
    X, F, ll, lw = sc.make_case(3, 2, 70, 3, _WIDTHS, 0.5, L, seed=21)
    for T in (3, 1):
        for bad in (0.0, -0.02, math.inf, math.nan):
            Lb = L.copy()
            Lb[1, 1] = bad
            got = _run(X[:T], F[:T - 1], ll[:T], lw[:T], Lb)
            for x in got:
                assert bool(torch.isnan(x).all()), (T, bad)


# ------------------------------------------------------------------------------------------ 3. known limits
def test_a_flat_transition_gives_the_filter_and_the_last_step_is_the_filters():
    """``L = 1e3 I``: every transition density is the same to 1e-6, so the smoothed moments are the lag-0 filter moments
    (``mmf_pf_smooth`` at lag 0 on the same history).  Any ``L``: the last step's weights are the softmax of the last step."""
    from multimodalfilter_amd import _abi

    dev = sc.dev()
    T, N, M, d = 5, 3, 300, 3
    L = sc.tril(d, True)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=31)
    G = sc.to_device
    fmean, fcov = torch.empty((T, N, d), device=dev), torch.empty((T, N, d, d), device=dev)
    _abi.pf_smooth(G(X), G(ll), G(lw), None, None, 0, fmean, fcov, None)
    flat = _run(X, F, ll, lw, (1e3 * np.eye(d)).astype(np.float32))
    sharp = _run(X, F, ll, lw, L)
    e_mean = max(rel_err(flat[1][:, n], fmean[:, n], dims=1) for n in range(N))
    e_cov = max(rel_err(flat[2][:, n], fcov[:, n], dims=2) for n in range(N))
    last = sc.softmax_rows(ll[-1].astype(np.float64) + lw[-1])
    e_last = max(rel_err(flat[0][-1], last, dims=1), rel_err(sharp[0][-1], last, dims=1))
    moved = rel_err(sharp[1][0], fmean[0], dims=1)
    print(f"flat transition against the filter: mean {e_mean:.2e} cov {e_cov:.2e}; last step's weights {e_last:.2e}; "
          f"the sharp transition moves step 0's mean by {moved:.2e}")
    assert e_mean <= REL_TOL and e_cov <= REL_TOL and e_last <= REL_TOL
    assert moved > 10 * REL_TOL  # (the comparison above is not vacuous: smoothing does change these means)


# ------------------------------------------------------------------------------------------ 4. whole filters
_CONFIGS = {"plain": {}, "soft": {"soft_resample_alpha": 0.5}, "ess": {"resample_ess_threshold": 0.5}, "noresample": {"resample": False}}


@functools.lru_cache(maxsize=None)
def _filter_runs(cls, config, M):
    """One filter, three runs on the same randomness: with ``record_indices`` (what the loop did before this history field
    existed), with ``record_history`` through the native loop and with ``record_history`` step by step."""
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    N, T = 4, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter(cls, N, M, T, dev)
    for k, v in _CONFIGS[config].items():
        setattr(f, k, v)

    def run(indices, history, native):
        f.record_indices, f.record_history, f.use_native_loop = indices, history, native
        f.noise = mmf.CounterNoise(99)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        torch.cuda.synchronize()
        clone = lambda x: None if x is None else x.clone()
        return dict(est=est.clone(), states=f.particle_states.clone(), logw=f.particle_log_weights.clone(), history=f.last_history,
                    idx=clone(f.last_resample_indices) if indices else None, ll=clone(f.last_log_likelihoods) if indices else None)

    out = dict(indices=run(True, False, True), native=run(False, True, True), steps=run(False, True, False),
               filter=f, ctrl=ctrl, N=N, T=T, M=M, d=d)
    f.use_native_loop, f.record_indices, f.record_history = True, False, False
    return out


_FILTER_CASES = [(cls, c, M) for cls in ("DoorParticleFilter", "PushParticleFilter") for c in _CONFIGS for M in (64, 300)]


@pytest.mark.parametrize("cls,config,M", _FILTER_CASES)
def test_filter_marginal_smoothing_matches_the_reference_and_the_loop_is_unchanged(cls, config, M):
    """``forward_loop`` with ``record_history``: estimates, belief on return and the history's tensors have the bits of the
    run with ``record_indices``; the history has ONE new field, ``controls``, the object the loop was given -- natively and
    step by step.  ``smooth(method="marginal")`` then equals the fp64 reference on that history, with the predictions
    ``F_t`` the test obtains itself through ``dynamics_model.propagate_encoded(..., None)``."""
    r = _filter_runs(cls, config, M)
    f, ind, T, N, d = r["filter"], r["indices"], r["T"], r["N"], r["d"]
    for name in ("native", "steps"):
        run, h = r[name], r[name]["history"]
        for k in ("est", "states", "logw"):
            assert torch.equal(run[k], ind[k]), (name, k)
        assert set(vars(h)) == {"states", "log_likelihoods", "log_weights_in", "ancestors", "resampled", "controls"}, name
        assert h.controls is r["ctrl"], name  # a reference, not a copy
        assert torch.equal(h.log_likelihoods, ind["ll"]), name
        assert (h.ancestors is None and ind["idx"] is None) if config == "noresample" else torch.equal(h.ancestors, ind["idx"]), name
    for k in ("states", "log_likelihoods", "log_weights_in"):
        assert torch.equal(getattr(r["native"]["history"], k), getattr(r["steps"]["history"], k)), k
    assert ind["history"] is None
    h = r["native"]["history"]
    dyn = f.dynamics_model
    with torch.no_grad():
        ctx = dyn.encode_controls(h.controls[1:].reshape((T - 1) * N, -1))
        F = dyn.propagate_encoded(h.states[:-1].reshape((T - 1) * N, M, d), ctx, None).reshape(T - 1, N, M, d)
    C = lambda x: x.detach().cpu().numpy()
    want = _reference64(C(h.states), C(F), C(h.log_likelihoods), C(h.log_weights_in), C(dyn.scale_tril()))
    f.last_history = h
    mean = f.smooth(method="marginal")
    rec = f.last_smoothed
    assert rec.method == "marginal" and rec.lag is None and set(vars(rec)) == {"covariance", "ess", "weights", "lag", "method"}
    assert mean.shape == (T, N, d) and rec.weights.shape == (T, N, M) and rec.ess.shape == (T, N)
    _check((rec.weights, mean, rec.covariance, rec.ess), want, f"{cls} {config} M={M}")
    f.smooth()  # the ancestry path's record is what it was
    assert set(vars(f.last_smoothed)) == {"covariance", "unique", "lag"} and f.last_smoothed.lag is None


def test_run_filter_returns_the_marginal_record():
    """``evaluation.run_filter(smooth_method="marginal", return_belief=True)``: the smoothed means and the record, equal to
    ``smooth(method="marginal")`` on the history the run left; the calibration metrics accept the record."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N, M, T = 4, 300, 8
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorParticleFilter", N, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    est, rec = evaluation.run_filter(f, traj, smooth_method="marginal", return_belief=True)
    assert f.record_history is False and f.record_belief is False  # switched back
    assert est.shape == (T, N, d) and rec.method == "marginal" and rec.covariance.shape == (T, N, d, d) and rec.ess.shape == (T, N)
    again = f.smooth(method="marginal")
    assert torch.equal(est, again) and torch.equal(rec.covariance, f.last_smoothed.covariance)
    assert bool((rec.ess >= 1.0 - 1e-4).all()) and bool((rec.ess <= M * (1.0 + 1e-4)).all())
    f.noise = mmf.CounterNoise(7)
    only = evaluation.run_filter(f, traj, smooth_lag=None, smooth_method="marginal")
    assert torch.is_tensor(only) and torch.equal(only, est)
    with pytest.raises(ValueError, match="fixed-lag"):
        evaluation.run_filter(f, traj, smooth_lag=2, smooth_method="marginal")
    assert f.record_history is False
    truth = traj["states"][1:]
    nll = evaluation.gaussian_nll(est, rec.covariance, truth, start=0)
    nees = evaluation.nees(est, rec.covariance, truth, start=0)
    assert nll.shape == (N,) and nees.shape == (T, N) and bool(torch.isfinite(nll).all()) and bool((nees >= 0).all())


# ------------------------------------------------------------------------------------------ 5. linear-Gaussian known answer
def test_marginal_is_no_worse_than_ancestry_against_the_exact_smoother():
    """The random-walk states of ``synthetic.make_trajectories`` (x' = x + 0.05 eps) observed through ``z = x + 0.3 eps``,
    filtered with the model that generated them (user models: the step-by-step history and the generic prediction path):
    N = 8, M = 512, T = 40.  Over steps 0 .. T - 10 and all trajectories the marginal smoother's RMSE to the exact RTS
    smoother is not larger than the ancestry smoother's.  A direction, no ratio (an fp64 restatement: 0.034 against 0.060)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    dev = sc.dev()
    d, N, M, T = 3, 8, 512, 40
    q, r = 0.05, 0.3
    truth = synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=23)["states"]
    z = truth[1:] + r * torch.randn((T, N, d), generator=torch.Generator().manual_seed(29))
    dyn, meas = sc.linear_gaussian_models(d, q, r, dev)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.record_history = True
    f.noise = mmf.NoiseSource(31)
    f.initialize_beliefs(mean=truth[0].to(dev), covariance=(0.1 * torch.eye(d))[None].expand(N, d, d).to(dev))
    est = f.forward_loop(observations={"z": z.to(dev)}, controls=torch.zeros((T, N, 7), device=dev))
    assert f.last_history.states.shape == (T, N, M, d) and f.last_history.controls.shape == (T, N, 7)
    ancestry = f.smooth()
    unique = f.last_smoothed.unique.float()
    marginal = f.smooth(method="marginal")
    rec = f.last_smoothed
    exact = torch.from_numpy(sc.rts(z.double().numpy(), truth[0].double().numpy(), 0.1, q, r))
    rmse = lambda x: float((x.double().cpu()[:T - 9] - exact[:T - 9]).pow(2).sum(-1).mean().sqrt())
    print(f"RMSE to the exact smoother over steps 0 .. T-10: marginal {rmse(marginal):.5f}, ancestry {rmse(ancestry):.5f}, "
          f"filter {rmse(est):.5f}; mean ess[0] {float(rec.ess[0].mean()):.1f}, mean unique[0] {float(unique[0].mean()):.1f}")
    assert bool(torch.isfinite(marginal).all()) and bool(torch.isfinite(rec.covariance).all())
    assert rmse(marginal) <= rmse(ancestry)


def test_state_dependent_noise_is_refused():
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    d, N, M, T = 2, 2, 64, 3
    dyn, meas = sc.linear_gaussian_models(d, 0.05, 0.3, dev, state_dependent=True)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.record_history = True
    f.noise = mmf.NoiseSource(5)
    f.initialize_beliefs(mean=torch.zeros((N, d), device=dev), covariance=(0.1 * torch.eye(d))[None].expand(N, d, d).to(dev))
    f.forward_loop(observations={"z": torch.zeros((T, N, d), device=dev)}, controls=torch.zeros((T, N, 7), device=dev))
    with pytest.raises(ValueError, match="state-dependent"):
        f.smooth(method="marginal")

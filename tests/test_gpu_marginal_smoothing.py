"""Marginal (forward-filter backward-smoothing) particle smoothing on the GPU (``include/mmf.h``: ``mmf_pf_smooth_marginal``;
``ParticleFilter.smooth(method="marginal")`` / ``evaluation.run_filter(smooth_method=)``).

The kernels are held to an fp64 restatement of the definition (``_reference`` below) at the project's bar (``_tol.REL_TOL``
through ``rel_err``, per trajectory so that a narrow cloud is measured against its own scale); the weights to the bar against
the norm of their row, the ESS to 1e-4 relative.  The forward side is held to the loop it stands for, bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import models as om

from _tol import REL_TOL, rel_err

CHUNK = 256  # rows / columns the pair kernels stage at a time (csrc/pf_smooth_math.h: kPairChunk)


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------------------ the fp64 reference
def _softmax_rows(a):
    """``softmax`` over the last axis in fp64; ``-inf`` gives exactly 0."""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _moments(X, W):
    """Mean, covariance and ``1 / sum W^2`` of ``X (..., M, d)`` under ``W (..., M)`` in fp64; rows of zero weight are not read."""
    X = np.where((W > 0)[..., None], np.asarray(X, dtype=np.float64), 0.0)
    mean = np.einsum("...m,...md->...d", W, X)
    dx = np.where((W > 0)[..., None], X - mean[..., None, :], 0.0)
    return mean, np.einsum("...m,...mi,...mj->...ij", W, dx, dx), 1.0 / (W * W).sum(-1)


def _reference(X, F, ll, lw, L):
    """Definition of ``mmf_pf_smooth_marginal`` in fp64 numpy: ``X (T, N, M, d)``, ``F (T - 1, N, M, d)``, ``ll (T, N, M)``,
    ``lw (T, N, M)`` or None, ``L (d, d)`` -> weights, mean, cov, ess.  Particles of zero weight are left out of every sum."""
    T, N, M, d = X.shape
    a = ll.astype(np.float64) + (0.0 if lw is None else lw.astype(np.float64))
    W = _softmax_rows(a)
    Linv = np.linalg.inv(np.tril(np.asarray(L, dtype=np.float64)))
    S = np.zeros((T, N, M))
    S[T - 1] = W[T - 1]
    for n in range(N):
        for t in range(T - 2, -1, -1):
            rows, cols = np.flatnonzero(W[t, n] > 0), np.flatnonzero(S[t + 1, n] > 0)
            diff = X[t + 1, n][cols].astype(np.float64)[None, :, :] - F[t, n][rows].astype(np.float64)[:, None, :]
            z = diff @ Linv.T
            term = np.log(W[t, n][rows])[:, None] - 0.5 * (z * z).sum(-1)
            top = term.max(0)
            logD = top + np.log(np.exp(term - top).sum(0))
            w = (S[t + 1, n][cols][None, :] * np.exp(term - logD[None, :])).sum(1)
            S[t, n][rows] = w / w.sum()
    return (S,) + _moments(X, S)


def _systematic(w, u):
    """Ancestors of systematic resampling (numpy, fp64): positions ``(u + k) / M`` in the CDF of ``w``."""
    M = len(w)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    return np.minimum(np.searchsorted(cdf, (u + np.arange(M)) / M, side="right"), M - 1)


def _tril(d, full, scale=0.02, seed=5):
    """The process noise of the kernel cases: 0.01 .. 0.04 wide, diagonal or a full lower triangle."""
    L = np.diag(scale * np.array([1.0, 0.5, 2.0, 1.5])[:d])
    if full:
        L = L + np.tril(0.4 * scale * np.random.default_rng(seed).normal(size=(d, d)), -1)
    return L.astype(np.float32)


def _make_case(T, N, M, d, widths, ll_scale, L, seed):
    """A run a filter could have left: step 0 is a cloud of the trajectory's width around an O(1) centre; every later set is
    drawn around the predictions ``F_t = X_t + drift_t`` of ancestors resampled systematically from the step's own weights
    (so the transition densities are not all negligible), with noise ``L``."""
    rng = np.random.default_rng(seed)
    widths = np.resize(np.asarray(widths, dtype=np.float64), N)
    X = np.zeros((T, N, M, d), dtype=np.float32)
    F = np.zeros((max(T - 1, 0), N, M, d), dtype=np.float32)
    ll = (ll_scale * rng.normal(size=(T, N, M))).astype(np.float32)
    lw = 0.3 * rng.normal(size=(T, N, M))
    lw = (lw - np.log(np.exp(lw).sum(-1, keepdims=True))).astype(np.float32)
    X[0] = rng.normal(size=(N, 1, d)) + widths[:, None, None] * rng.normal(size=(N, M, d))
    for t in range(T - 1):
        F[t] = X[t] + 0.05 * rng.normal(size=(N, 1, d))
        for n in range(N):
            a = ll[t, n].astype(np.float64) + lw[t, n]
            A = _systematic(np.exp(a - a.max()), rng.uniform())
            X[t + 1, n] = F[t, n][A] + rng.normal(size=(M, d)) @ L.astype(np.float64).T
    return X, F, ll, lw


def _run(X, F, ll, lw, L, want_cov=True, want_ess=True):
    from multimodalfilter_amd import _abi

    dev = _dev()
    T, N, M, d = X.shape
    G = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float32).to(dev)
    weights = torch.full((T, N, M), math.nan, device=dev)
    mean = torch.full((T, N, d), math.nan, device=dev)
    cov = torch.full((T, N, d, d), math.nan, device=dev) if want_cov else None
    ess = torch.full((T, N), math.nan, device=dev) if want_ess else None
    _abi.pf_smooth_marginal(G(X), G(F) if T > 1 else None, G(ll), G(lw), G(L), weights, mean, cov, ess)
    torch.cuda.synchronize()
    return weights, mean, cov, ess


def _check(got, want, what):
    """Weights within the bar of their row's norm, means and covariances within the bar per trajectory, ESS to 1e-4 relative,
    ``cov`` symmetric bit for bit and PSD to ``-1e-4 x trace``.  Prints the figures before asserting."""
    weights, mean, cov, ess = got
    wweights, wmean, wcov, wess = want
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
    assert torch.equal(cov, cov.transpose(-1, -2)), what
    c = cov.double().cpu()
    floor = -1e-4 * torch.diagonal(c, dim1=-2, dim2=-1).sum(-1)
    assert bool((torch.linalg.eigvalsh(c).min(-1).values >= floor - 1e-30).all()), what


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
        L = _tril(d, full)
        X, F, ll, lw = _make_case(T, N, M, d, _WIDTHS, ll_scale, L, seed=1000 * M + 10 * d + int(ll_scale) + full)
        _check(_run(X, F, ll, lw, L), _reference(X, F, ll, lw, L), f"M={M} d={d} scale={ll_scale} full={full}")


# ------------------------------------------------------------------------------------------ 2. edges
def test_single_step_and_single_particle():
    L = _tril(3, True)
    X, F, ll, lw = _make_case(1, 3, 300, 3, _WIDTHS, 0.5, L, seed=1)
    got = _run(X, F, ll, lw, L)
    _check(got, _reference(X, F, ll, lw, L), "T=1")
    assert rel_err(got[0][0], _softmax_rows(ll[0].astype(np.float64) + lw[0]), dims=1) <= REL_TOL  # the filter's weights
    L = _tril(2, False)
    X, F, ll, lw = _make_case(5, 2, 1, 2, _WIDTHS, 0.5, L, seed=2)
    got = _run(X, F, ll, lw, L)
    _check(got, _reference(X, F, ll, lw, L), "M=1")
    assert torch.equal(got[1].cpu(), torch.from_numpy(X[:, :, 0]))  # the one particle is the mean
    assert float(got[2].abs().max()) == 0.0 and bool((got[0] == 1).all()) and bool((got[3] == 1).all())


def test_dead_particles_and_a_single_heavy_particle():
    """-inf log-likelihoods on half a row at every step, ``inf`` in the dead rows of ``X`` and ``F``: a finite result equal to
    the reference over the rest, zero weight on the dead.  One particle with all the weight at the last step: step T - 2 is
    re-weighted by the transition into that particle alone."""
    T, N, M, d = 5, 3, 300, 3
    L = _tril(d, True)
    X, F, ll, lw = _make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=11)
    ll[:, 1, ::2] = -np.inf
    X[:, 1, ::2] = np.inf
    F[:, 1, ::2] = np.inf
    got = _run(X, F, ll, lw, L)
    _check(got, _reference(X, F, ll, lw, L), "half dead")
    assert float(got[0][:, 1, ::2].abs().max()) == 0.0 and bool((got[0][:, 1, 1::2] > 0).any())
    X, F, ll, lw = _make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=12)
    ll[-1, :, 17] = 60.0  # the others keep exp(-60) ~ 1e-26 of it
    got = _run(X, F, ll, lw, L)
    want = _reference(X, F, ll, lw, L)
    _check(got, want, "one heavy particle")
    assert float(got[0][-1, :, 17].min()) >= 1.0 - 1e-6 and float(want[3][-1].max()) <= 1.0 + 1e-9
    # by the definition, with one column: W_{T-2|T}[i] is proportional to W_{T-2}[i] N(X_{T-1}[17]; F_{T-2}[i], L L^T)
    z = (X[-1, :, 17].astype(np.float64)[:, None, :] - F[-1].astype(np.float64)) @ np.linalg.inv(L.astype(np.float64)).T
    direct = _softmax_rows(ll[-2].astype(np.float64) + lw[-2] - 0.5 * (z * z).sum(-1))
    assert rel_err(got[0][-2], direct, dims=1) <= REL_TOL


@pytest.mark.parametrize("M", [300, 2 * CHUNK + 88])
def test_two_calls_and_split_batches_give_the_same_bits(M):
    """Fixed-order reductions: two calls on the same inputs return the same bits, and the call on N = 3 trajectories returns
    what three calls on one trajectory each do.  Outputs that are not asked for change nothing."""
    L = _tril(3, True)
    X, F, ll, lw = _make_case(5, 3, M, 3, _WIDTHS, 0.5, L, seed=3 + M)
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
    L = _tril(3, True)
    X, F, ll, lw = _make_case(3, 2, 70, 3, _WIDTHS, 0.5, L, seed=21)
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

    dev = _dev()
    T, N, M, d = 5, 3, 300, 3
    L = _tril(d, True)
    X, F, ll, lw = _make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=31)
    G = lambda x: torch.as_tensor(x, dtype=torch.float32).contiguous().to(dev)
    fmean, fcov = torch.empty((T, N, d), device=dev), torch.empty((T, N, d, d), device=dev)
    _abi.pf_smooth(G(X), G(ll), G(lw), None, None, 0, fmean, fcov, None)
    flat = _run(X, F, ll, lw, (1e3 * np.eye(d)).astype(np.float32))
    sharp = _run(X, F, ll, lw, L)
    e_mean = max(rel_err(flat[1][:, n], fmean[:, n], dims=1) for n in range(N))
    e_cov = max(rel_err(flat[2][:, n], fcov[:, n], dims=2) for n in range(N))
    last = _softmax_rows(ll[-1].astype(np.float64) + lw[-1])
    e_last = max(rel_err(flat[0][-1], last, dims=1), rel_err(sharp[0][-1], last, dims=1))
    moved = rel_err(sharp[1][0], fmean[0], dims=1)
    print(f"flat transition against the filter: mean {e_mean:.2e} cov {e_cov:.2e}; last step's weights {e_last:.2e}; "
          f"the sharp transition moves step 0's mean by {moved:.2e}")
    assert e_mean <= REL_TOL and e_cov <= REL_TOL and e_last <= REL_TOL
    assert moved > 10 * REL_TOL  # (the comparison above is not vacuous: smoothing does change these means)


# ------------------------------------------------------------------------------------------ 4. whole filters
_CONFIGS = {"plain": {}, "soft": {"soft_resample_alpha": 0.5}, "ess": {"resample_ess_threshold": 0.5}, "noresample": {"resample": False}}


def _filter(cls, N, M, T, dev):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    tname = "door" if cls.startswith("Door") else "push"
    d = om.TASKS[tname].state_dim
    torch.manual_seed(3)
    f = mmf.model_types(tname)[cls]().to(dev).eval()
    f.num_particles = M
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=17).items()}
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cal = traj["states"][0][:, None, :] + 0.3 * torch.randn((N, 256, d), device=dev)
    synthetic.calibrate_measurement_heads(f, {k: v[0] for k, v in obs.items()}, cal, target_std=1.2)
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
    return f, d, traj, obs, traj["controls"][1:], cov


@functools.lru_cache(maxsize=None)
def _filter_runs(cls, config, M):
    """One filter, three runs on the same randomness: with ``record_indices`` (what the loop did before this history field
    existed), with ``record_history`` through the native loop and with ``record_history`` step by step."""
    import multimodalfilter_amd as mmf

    dev = _dev()
    N, T = 4, 6
    f, d, traj, obs, ctrl, cov = _filter(cls, N, M, T, dev)
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
    want = _reference(C(h.states), C(F), C(h.log_likelihoods), C(h.log_weights_in), C(dyn.scale_tril()))
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

    dev = _dev()
    N, M, T = 4, 300, 8
    f, d, traj, obs, ctrl, cov = _filter("DoorParticleFilter", N, M, T, dev)
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
def _rts(z, m0, p0, q, r):
    """Exact Kalman filter and Rauch-Tung-Striebel smoother of ``x' = x + q eps``, ``z = x + r eps`` in fp64: every state
    dimension is a scalar problem with the same variances.  ``z (T, ...)``, prior ``N(m0, p0)`` before the first step."""
    T = z.shape[0]
    mf, pf, mp, pp = np.zeros_like(z), np.zeros(T), np.zeros_like(z), np.zeros(T)
    m, p = m0, p0
    for t in range(T):
        mp[t], pp[t] = m, p + q * q
        k = pp[t] / (pp[t] + r * r)
        m, p = mp[t] + k * (z[t] - mp[t]), (1.0 - k) * pp[t]
        mf[t], pf[t] = m, p
    ms = mf.copy()
    for t in range(T - 2, -1, -1):
        ms[t] = mf[t] + pf[t] / pp[t + 1] * (ms[t + 1] - mp[t + 1])
    return ms


def _linear_gaussian_models(d, q, r, dev, state_dependent=False):
    from multimodalfilter_amd import base

    class RandomWalk(base.DynamicsModel):
        def __init__(self):
            super().__init__(state_dim=d)
            self.L = (q * torch.eye(d)).to(dev)

        def forward(self, *, initial_states, controls):
            L = self.L[None].expand(initial_states.shape[0], d, d)
            if state_dependent:
                L = L * (1.0 + initial_states[:, :1, None].abs())
            return initial_states, L

    class GaussianLik(base.ParticleFilterMeasurementModel):
        def __init__(self):
            super().__init__(state_dim=d)

        def forward(self, *, states, observations):
            e = observations["z"][:, None, :] - states
            return -0.5 * (e * e).sum(-1) / (r * r)

    return RandomWalk(), GaussianLik()


def test_marginal_is_no_worse_than_ancestry_against_the_exact_smoother():
    """The random-walk states of ``synthetic.make_trajectories`` (x' = x + 0.05 eps) observed through ``z = x + 0.3 eps``,
    filtered with the model that generated them (user models: the step-by-step history and the generic prediction path):
    N = 8, M = 512, T = 40.  Over steps 0 .. T - 10 and all trajectories the marginal smoother's RMSE to the exact RTS
    smoother is not larger than the ancestry smoother's.  A direction, no ratio (an fp64 restatement: 0.034 against 0.060)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    dev = _dev()
    d, N, M, T = 3, 8, 512, 40
    q, r = 0.05, 0.3
    truth = synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=23)["states"]
    z = truth[1:] + r * torch.randn((T, N, d), generator=torch.Generator().manual_seed(29))
    dyn, meas = _linear_gaussian_models(d, q, r, dev)
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
    exact = torch.from_numpy(_rts(z.double().numpy(), truth[0].double().numpy(), 0.1, q, r))
    rmse = lambda x: float((x.double().cpu()[:T - 9] - exact[:T - 9]).pow(2).sum(-1).mean().sqrt())
    print(f"RMSE to the exact smoother over steps 0 .. T-10: marginal {rmse(marginal):.5f}, ancestry {rmse(ancestry):.5f}, "
          f"filter {rmse(est):.5f}; mean ess[0] {float(rec.ess[0].mean()):.1f}, mean unique[0] {float(unique[0].mean()):.1f}")
    assert bool(torch.isfinite(marginal).all()) and bool(torch.isfinite(rec.covariance).all())
    assert rmse(marginal) <= rmse(ancestry)


def test_state_dependent_noise_is_refused():
    import multimodalfilter_amd as mmf

    dev = _dev()
    d, N, M, T = 2, 2, 64, 3
    dyn, meas = _linear_gaussian_models(d, 0.05, 0.3, dev, state_dependent=True)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.record_history = True
    f.noise = mmf.NoiseSource(5)
    f.initialize_beliefs(mean=torch.zeros((N, d), device=dev), covariance=(0.1 * torch.eye(d))[None].expand(N, d, d).to(dev))
    f.forward_loop(observations={"z": torch.zeros((T, N, d), device=dev)}, controls=torch.zeros((T, N, 7), device=dev))
    with pytest.raises(ValueError, match="state-dependent"):
        f.smooth(method="marginal")

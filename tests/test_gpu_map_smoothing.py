"""MAP path smoothing on the GPU (``include/mmf.h``: ``mmf_pf_smooth_map``; ``ParticleFilter.smooth(method="map")`` /
``evaluation.run_filter(smooth_method="map")`` / ``evaluation.path_log_density``), through the C entry and through the filter.

The kernel is held to the fp64 definition of ``_map_cases`` step by step, every step restated from the GPU's OWN previous row
(no accumulated error): ``v`` to ``V_BAR = 1e-5``, ``log_posterior`` to ``LP_BAR = 1e-6`` of the fp64 density of the GPU's own
path, the argmax decisions to ``REGRET = 0`` -- the bars ``test_map_smoothing_cpu.py`` derives from the fp32 yardstick (worst
``v`` 1.94e-6, ``log_posterior`` 1.25e-7, regret 0).  ``step_max``, ``indices`` and ``path`` are exact by construction and held
bit for bit.  The GPU's own worst over the cases of ``_map_cases.GPU_CASES``, as measured on one MI355X: ``v`` 1.94e-6 (case
by case the yardstick's figure to the digits printed), ``log_posterior`` 1.84e-7, regret 0; on the door filter's own history
7.5e-7, 5.0e-8 and 0 (``profiles/map_smooth/README.md``)."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _map_cases as mc
import _smooth_cases as sc


def _run(X, F, ll, lw, L):
    """``_abi.pf_smooth_map`` on numpy inputs -> its six outputs as numpy arrays (NaN / -7 filled before the call).  The
    incoming log-weights of the steps after the first are NaN: they are not read."""
    from multimodalfilter_amd import _abi

    dev = sc.dev()
    T, N, M, d = X.shape
    if lw is not None:
        lw = lw.copy()
        lw[1:] = np.nan
    out = dict(v=torch.full((T, N, M), math.nan, device=dev), step_max=torch.full((T, N), math.nan, device=dev),
               psi=torch.full((T, N, M), -7, dtype=torch.int32, device=dev), indices=torch.full((T, N), -7, dtype=torch.int32, device=dev),
               path=torch.full((T, N, d), math.nan, device=dev), log_posterior=torch.full((N,), math.nan, device=dev))
    _abi.pf_smooth_map(sc.to_device(X), sc.to_device(F) if T > 1 else None, sc.to_device(ll), sc.to_device(lw), sc.to_device(L),
                       out["indices"], out["path"], out["log_posterior"], out["v"], out["step_max"], out["psi"])
    torch.cuda.synchronize()
    return {k: x.cpu().numpy() for k, x in out.items()}


def _check(got, X, F, ll, lw0, L, what):
    """Everything a run is held to against fp64; prints the figures before asserting."""
    T, N, M, d = X.shape
    r = mc.check_run(got, X, F, ll, lw0, L)
    print(f"{what}: v {r['v']:.3e} log_posterior {r['lp']:.3e} regret {r['regret']:.3e} end to end {r['end']:.3e}")
    assert r["v"] <= mc.V_BAR, (what, r)
    assert r["regret"] <= mc.REGRET and r["psi_ok"], (what, r)
    assert r["lp"] <= mc.LP_BAR, (what, r)
    assert r["end"] <= T * mc.REGRET + mc.REF_EPS, (what, r)
    assert np.array_equal(got["step_max"], got["v"].max(-1)), what  # exact: bit for bit
    for n in range(N):  # the backtrack of the GPU's own psi, exactly
        idx, path = mc.backtrack(got["v"][T - 1, n], got["psi"][:, n], X[:, n])
        assert np.array_equal(got["indices"][:, n], idx), (what, n)
        assert np.array_equal(got["path"][:, n], path, equal_nan=True), (what, n)
    dead = ll == -np.inf
    assert bool((got["v"][dead] == -np.inf).all()) and bool((got["psi"][dead] == -1).all()), what
    return r


# ------------------------------------------------------------------------------------------ 1. the kernel against fp64
@functools.lru_cache(maxsize=None)
def _case(name):
    X, F, ll, lw, L = mc.build_case(name)
    return X, F, ll, lw, L, _run(X, F, ll, lw, L)


@pytest.mark.parametrize("name", list(mc.GPU_CASES))
def test_map_kernel_matches_fp64(name):
    X, F, ll, lw, L, got = _case(name)
    T, N, M, d = X.shape
    _check(got, X, F, ll, None if lw is None else lw[0], L, name)
    alive = got["indices"][0] >= 0
    if name == "dead_step":
        assert list(alive) == [True, False, True]
        assert bool((got["indices"][:, 1] == -1).all()) and bool(np.isnan(got["path"][:, 1]).all())
        assert got["log_posterior"][1] == -np.inf and bool((got["v"][3:, 1] == -np.inf).all())
        keep = [0, 2]  # the neighbours are what they are without it
        alone = _run(X[:, keep], F[:, keep], ll[:, keep], lw[:, keep], L)
        for k in got:
            assert np.array_equal(got[k][:, keep] if got[k].ndim > 1 else got[k][keep], alone[k]), k
    else:
        assert bool(alive.all()) and bool(np.isfinite(got["path"]).all()) and bool(np.isfinite(got["log_posterior"]).all())
    if name in ("dead_some", "dead_tile"):
        assert not bool((ll[np.arange(T)[:, None], np.arange(N)[None, :], got["indices"]] == -np.inf).any())


def test_a_planted_path_is_found():
    X, F, ll, lw, L, chain = mc.planted_case()
    got = _run(X, F, ll, lw, L)
    _check(got, X, F, ll, lw[0], L, "planted")
    assert np.array_equal(got["indices"], chain)


@pytest.mark.parametrize("M", [65, 257])
def test_ties_go_to_the_lower_index(M):
    """The copies of particle ``a`` sit in another group and column tile (``M = 65``: 63 and 64) and in another chunk
    (``M = 257``: 70 and 256): equal values, and the lower index wins every decision and the last maximum."""
    X, F, ll, lw, L, a = mc.tie_case(M)
    got = _run(X, F, ll, lw, L)
    _check(got, X, F, ll, lw[0], L, f"ties M={M}")
    assert bool((got["indices"] == a).all())
    for k in (min(70, M - 2), M - 1):
        assert np.array_equal(got["v"][:, :, k], got["v"][:, :, a])
        assert not bool((got["psi"] == k).any())


@pytest.mark.parametrize("name", ["M257", "dead_step"])
def test_two_calls_and_split_batches_give_the_same_bits(name):
    X, F, ll, lw, L, got = _case(name)
    again = _run(X, F, ll, lw, L)
    for k in got:
        assert np.array_equal(got[k], again[k], equal_nan=True), k
    one = _run(X[:, :1], F[:, :1], ll[:, :1], lw[:, :1], L)  # trajectory 0 of the N = 3 call against the N = 1 call on it
    for k in got:
        assert np.array_equal(got[k][:, :1] if got[k].ndim > 1 else got[k][:1], one[k], equal_nan=True), k
    zeros = lw.copy()
    zeros[0] = 0.0
    a, b = _run(X, F, ll, None, L), _run(X, F, ll, zeros, L)  # null incoming log-weights are zeros
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k


def test_a_bad_noise_factor_gives_nan_and_no_fault():
    """A zero, negative or non-finite diagonal entry of ``L``: every floating output NaN, every index -1 (``T = 1`` included)."""
    X, F, ll, lw, L = mc.build_case("M65")
    for T in (3, 1):
        for bad in (0.0, -0.02, math.inf, math.nan):
            Lb = L.copy()
            Lb[1, 1] = bad
            got = _run(X[:T], F[:T - 1], ll[:T], lw[:T], Lb)
            for k in ("v", "step_max", "path", "log_posterior"):
                assert bool(np.isnan(got[k]).all()), (T, bad, k)
            assert bool((got["indices"] == -1).all()) and bool((got["psi"] == -1).all()), (T, bad)


# ------------------------------------------------------------------------------------------ 2. through the filter
@functools.lru_cache(maxsize=None)
def _filter_run(cls="DoorParticleFilter", N=3, M=64, T=6):
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    f, d, traj, obs, ctrl, cov = sc.small_filter(cls, N, M, T, dev)

    def forward():
        f.record_history = True
        f.noise = mmf.NoiseSource(31)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        torch.cuda.synchronize()
        return est

    return f, forward, (T, N, M, d)


def _history_numpy(f):
    h = f.last_history
    with torch.no_grad():
        pred, tril = f._smoothing_transition(h, "map")
    C = lambda x: x.detach().cpu().numpy()
    return C(h.states), C(pred), C(h.log_likelihoods), C(h.log_weights_in), C(tril)


def test_filter_map_path_is_optimal_and_leaves_the_filter_alone():
    """``smooth(method="map")`` on a small real filter: the record, the path against fp64 on the filter's own history, and at
    least the density of every path backward simulation drew and of every ancestral line.  The noise stream and every output
    of ``forward_loop`` are what they are without the call."""
    from multimodalfilter_amd import evaluation

    f, forward, (T, N, M, d) = _filter_run()
    est = forward().clone()
    h = f.last_history
    before = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in", "ancestors") if getattr(h, k) is not None}
    belief = (f.particle_states.clone(), f.particle_log_weights.clone())
    path = f.smooth(method="map")
    rec = f.last_smoothed
    assert set(vars(rec)) == {"indices", "log_posterior", "lag", "method"} and rec.method == "map" and rec.lag is None
    assert path.shape == (T, N, d) and rec.indices.shape == (T, N) and rec.indices.dtype == torch.int32
    assert rec.log_posterior.shape == (N,) and rec.log_posterior.dtype == torch.float32
    after_map = f.noise.uniform((4, 5), like=h.states).clone()  # where the stream stands after smoothing ...
    assert torch.equal(forward(), est)
    assert torch.equal(f.noise.uniform((4, 5), like=h.states), after_map)  # ... is where it stands without it
    f.last_history = h
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k
    assert f.last_history is h
    # the path is rows of the history, its density is the record's, and it is the optimum of the fp64 definition
    rows = torch.gather(h.states, 2, rec.indices.long()[:, :, None, None].expand(T, N, 1, d))[:, :, 0]
    assert torch.equal(path, rows)
    own = evaluation.path_log_density(f, rec.indices)
    assert mc.scalar_error(rec.log_posterior.cpu().numpy(), own.cpu().numpy()) <= mc.LP_BAR
    X, F, ll, lw, L = _history_numpy(f)
    best = mc.viterbi_reference(X, F, ll, lw[0], L)["log_posterior"]
    assert float((best - own.cpu().numpy()).max()) <= T * mc.REGRET + mc.REF_EPS
    # every ancestral line of the last step's particles
    lines = torch.empty((T, N, M), dtype=torch.int64, device=h.states.device)
    lines[T - 1] = torch.arange(M, device=h.states.device)
    for t in range(T - 1, 0, -1):
        lines[t - 1] = lines[t] if h.ancestors is None else torch.gather(h.ancestors[t - 1].long(), 1, lines[t])
    ancestral = evaluation.path_log_density(f, lines)
    # the paths backward simulation draws (this one does advance the noise stream)
    f.smooth(method="simulation", num_draws=32)
    drawn = evaluation.path_log_density(f, f.last_smoothed.indices)
    assert drawn.shape == (N, 32) and ancestral.shape == (N, M) and bool(torch.isfinite(drawn).all())
    slack32 = mc.LP_BAR * rec.log_posterior.double().abs().clamp_min(1.0)  # what the fp32 log_posterior is held to
    print(f"MAP log_posterior {rec.log_posterior.tolist()}, best drawn {drawn.max(-1).values.tolist()}, best ancestral line "
          f"{ancestral.max(-1).values.tolist()}")
    for other in (drawn, ancestral):
        assert bool((own[:, None] >= other - (T * mc.REGRET + mc.REF_EPS)).all())
        assert bool((rec.log_posterior.double()[:, None] >= other - (T * mc.REGRET + mc.REF_EPS) - slack32[:, None]).all())
    assert torch.equal(f.particle_states, belief[0]) and torch.equal(f.particle_log_weights, belief[1])


def test_filter_map_smoothing_matches_fp64_on_its_history():
    f, forward, (T, N, M, d) = _filter_run()
    forward()
    X, F, ll, lw, L = _history_numpy(f)
    got = _run(X, F, ll, lw, L)
    _check(got, X, F, ll, lw[0], L, "DoorParticleFilter history")
    path = f.smooth(method="map")
    assert np.array_equal(f.last_smoothed.indices.cpu().numpy(), got["indices"]) and np.array_equal(path.cpu().numpy(), got["path"])
    assert np.array_equal(f.last_smoothed.log_posterior.cpu().numpy(), got["log_posterior"])


def test_run_filter_returns_the_map_path_and_record():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N, M, T = 3, 64, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorParticleFilter", N, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    path, rec = evaluation.run_filter(f, traj, smooth_method="map", return_belief=True)
    assert f.record_history is False and f.record_belief is False  # switched back
    assert path.shape == (T, N, d) and rec.method == "map" and rec.lag is None and not hasattr(rec, "covariance")
    assert rec.indices.shape == (T, N) and rec.log_posterior.shape == (N,) and bool(torch.isfinite(rec.log_posterior).all())
    again = f.smooth(method="map")
    assert torch.equal(path, again) and torch.equal(rec.indices, f.last_smoothed.indices)
    f.noise = mmf.CounterNoise(7)
    only = evaluation.run_filter(f, traj, smooth_lag=None, smooth_method="map")
    assert torch.is_tensor(only) and torch.equal(only, path)
    with pytest.raises(ValueError, match="fixed-lag"):
        evaluation.run_filter(f, traj, smooth_lag=2, smooth_method="map")
    assert f.record_history is False

"""CPU-side checks of MAP path smoothing (``include/mmf.h``: ``MmfPfSmoothMapArgs`` / ``mmf_pf_smooth_map``;
``ParticleFilter.smooth(method="map")``; ``evaluation.path_log_density``): the fp64 reference of ``_map_cases`` against a brute
force over all ``M^T`` paths, a planted path, the tie rule and an all-dead step; the entry point's refusals on the host,
before any HIP call; the Python switches' refusals; ``path_log_density`` against the reference; and the measurement of the
fp32 yardstick that the GPU tests' bars come from.

Measured over ``_map_cases.GPU_CASES`` (the last test prints them): the yardstick's worst one-step error of ``v`` against
fp64, ``|v32 - v64| / max(1, |v64|)`` with both rows rescaled by their own maximum, is 1.94e-6 (the "sharp" case, log-likelihoods
of +-150; at most 4.8e-7 on every other case), its worst ``log_posterior`` error against the fp64 density of its own path
1.25e-7, and its worst argmax regret 0: it takes the fp64-best pair at every decision.  Hence ``V_BAR = 1e-5``,
``LP_BAR = 1e-6`` and ``REGRET = 0`` (three times the measured figure, ``V_BAR`` and ``LP_BAR`` rounded up to the ladder)."""
import ctypes

import numpy as np
import pytest

import _map_cases as mc
import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2

_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "v", "step_max", "backpointers",
             "indices", "path", "log_posterior")
_OUTPUTS = _POINTERS[5:]


@pytest.fixture(autouse=True, scope="module")
def _the_entry_these_tests_describe():
    """The reference, the yardstick and the bars of this module are the definition of ONE entry point: without the binding
    and the method there is nothing they are the reference of."""
    from multimodalfilter_amd import _abi

    assert hasattr(_abi, "MmfPfSmoothMapArgs") and callable(getattr(_abi, "pf_smooth_map", None))


# ------------------------------------------------------------------------------------------ 1. the reference
def _small(T, M, d, dead, N=2):
    L = sc.tril(d, True)
    X, F, ll, lw = sc.make_case(T, N, M, d, (1e-2, 0.3), 0.5, L, seed=10 * T + M)
    if dead:
        ll[:, :, 1] = -np.inf
        X[:, :, 1] = np.nan
        F[:, :, 1] = np.nan
    return X, F, ll, lw[0], L


@pytest.mark.parametrize("dead", [False, True])
@pytest.mark.parametrize("T,M,d", [(1, 5, 2), (2, 4, 1), (4, 4, 3), (6, 3, 4)])
def test_the_reference_finds_the_brute_force_optimum(T, M, d, dead):
    X, F, ll, lw0, L = _small(T, M, d, dead)
    ref = mc.viterbi_reference(X, F, ll, lw0, L)
    indices, logpost = mc.brute_force(X, F, ll, lw0, L)
    assert np.array_equal(ref["indices"], indices)
    assert float(np.abs(ref["log_posterior"] - logpost).max()) <= mc.REF_EPS
    assert float(np.abs(mc.path_density(X, F, ll, lw0, L, ref["indices"]) - logpost).max()) <= mc.REF_EPS  # both forms of the definition
    assert np.array_equal(ref["step_max"], ref["v"].max(-1)) and bool((ref["psi"][0] == -1).all())
    for t in range(T):
        for n in range(X.shape[1]):
            assert np.array_equal(ref["path"][t, n], X[t, n, ref["indices"][t, n]])
    if dead:
        assert bool((ref["v"][:, :, 1] == -np.inf).all()) and bool((ref["psi"][:, :, 1] == -1).all())
        assert bool((ref["indices"] != 1).all()) and bool(np.isfinite(ref["path"]).all())


def test_the_reference_finds_a_planted_path():
    """The chain's fp64 margin over every other path exceeds 10: the best path that avoids the chain at step ``t`` -- any
    path other than the chain is one of those for some ``t`` -- is the optimum of the case with that particle dead."""
    X, F, ll, lw, L, chain = mc.planted_case()
    T, N = chain.shape
    ref = mc.viterbi_reference(X, F, ll, lw[0], L)
    assert np.array_equal(ref["indices"], chain)
    for t in range(T):
        without = ll.copy()
        for n in range(N):
            without[t, n, chain[t, n]] = -np.inf
        other = mc.viterbi_reference(X, F, without, lw[0], L)["log_posterior"]
        assert float((ref["log_posterior"] - other).min()) > 10.0, t


@pytest.mark.parametrize("M", [65, 257])
def test_ties_go_to_the_lower_index(M):
    X, F, ll, lw, L, a = mc.tie_case(M)
    for run in (mc.viterbi_reference, mc.yardstick32):
        got = run(X, F, ll, lw[0], L)
        assert bool((got["indices"] == a).all()), run.__name__
        copies = [k for k in range(M) if k != a and np.array_equal(X[:, :, k], X[:, :, a])]
        assert len(copies) == 2 and copies[-1] == M - 1
        for k in copies:  # the copies are worth exactly as much, and every column that leaves from one of them says `a`
            assert np.array_equal(got["v"][:, :, k], got["v"][:, :, a]), run.__name__
        assert not np.isin(got["psi"], copies).any(), run.__name__


def test_a_step_with_every_particle_dead():
    """Trajectory 1 of three has no particle alive at step 3: ``indices = -1``, a NaN ``path``, ``log_posterior = -inf``,
    ``v = -inf`` from that step on; its neighbours are what they are without it."""
    X, F, ll, lw, L = mc.build_case("dead_step")
    for run in (mc.viterbi_reference, mc.yardstick32):
        got = run(X, F, ll, lw[0], L)
        assert bool((got["indices"][:, 1] == -1).all()) and bool(np.isnan(got["path"][:, 1]).all())
        assert got["log_posterior"][1] == -np.inf and bool((got["v"][3:, 1] == -np.inf).all())
        assert bool((got["psi"][3:, 1] == -1).all()) and bool((got["step_max"][3:, 1] == -np.inf).all())
        keep = [0, 2]
        alone = run(X[:, keep], F[:, keep], ll[:, keep], lw[0][keep], L)
        for k in ("v", "psi", "indices", "path", "step_max"):
            assert np.array_equal(got[k][:, keep], alone[k]), (run.__name__, k)
        assert np.array_equal(got["log_posterior"][keep], alone["log_posterior"]) and bool(np.isfinite(alone["log_posterior"]).all())


# ------------------------------------------------------------------------------------------ 2. the entry point's host checks
def _args(alias=None, **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it (T N M d = 16); ``alias``: output field ->
    (field whose buffer it is pointed at, byte offset)."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfSmoothMapArgs, _POINTERS, **{**dict(T=2, N=2, M=2, d=2), **over})
    for field, (target, offset) in (alias or {}).items():
        setattr(a, field, ctypes.c_void_p(ctypes.addressof(a._buffers[_POINTERS.index(target)]) + offset))
    return a


def test_map_refuses_bad_arguments_on_the_host():
    """Nulls and negative sizes -> ``MMF_EINVAL``; ``d``, ``M`` or ``N`` beyond the limits -> ``MMF_ETOOLARGE``; an output on
    top of an input or of another output -> ``MMF_EINVAL``; no trajectories or no steps -> a successful no-op.  All decided
    before any HIP call: the pointers are host memory and never dereferenced, and the stream is null."""
    lib = sc.lib()
    call = lambda alias=None, **over: lib.mmf_pf_smooth_map(ctypes.byref(_args(alias, **over)), None)
    assert lib.mmf_pf_smooth_map(None, None) == EINVAL
    for field in ("states_steps", "loglik_steps", "scale_tril", "pred_steps") + _OUTPUTS:
        assert call(**{field: None}) == EINVAL, field
    assert call(d=0) == EINVAL and call(d=-1) == EINVAL and call(d=5) == ETOOLARGE
    assert call(M=0) == EINVAL and call(M=-3) == EINVAL and call(M=65537) == ETOOLARGE
    assert call(T=-1) == EINVAL and call(N=-1) == EINVAL and call(N=65536) == ETOOLARGE
    assert call(d=5, states_steps=None) == EINVAL  # an invalid call is invalid whatever its size
    assert call(N=0) == 0 and call(T=0) == 0
    assert call(N=0, M=65536, d=4) == 0 and call(N=0, M=65537) == ETOOLARGE  # (the limits hold for the no-ops too)
    assert call(N=0, logw_in_steps=None) == 0  # the optional one
    # without a second step there is no transition, so no predictions are needed
    assert call(T=0, pred_steps=None) == 0 and call(T=1, N=0, pred_steps=None) == 0 and call(T=2, N=0, pred_steps=None) == EINVAL
    # an output on top of an input, of another output, or only partly on top of one
    for out, target in (("v", "states_steps"), ("path", "pred_steps"), ("step_max", "loglik_steps"), ("backpointers", "logw_in_steps"),
                        ("log_posterior", "scale_tril"), ("indices", "path"), ("step_max", "v"), ("log_posterior", "backpointers")):
        assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"v": ("states_steps", 60)}) == EINVAL and call({"log_posterior": ("v", 28)}) == EINVAL
    assert call({"v": ("states_steps", 0)}, N=0) == 0  # (empty ranges overlap nothing)
    assert call({"v": ("states_steps", 0)}, M=65537) == ETOOLARGE


# ------------------------------------------------------------------------------------------ 3. the Python switches
def test_smooth_map_refusals_on_a_cpu_filter():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.record_history = True
    with pytest.raises(ValueError, match="fixed-lag"):
        pf.smooth(lag=1, method="map")
    with pytest.raises(ValueError, match="num_draws"):
        pf.smooth(method="map", num_draws=8)
    with pytest.raises(AssertionError, match="history"):
        pf.smooth(method="map")
    pf.record_transition_moments = True
    with pytest.raises(ValueError, match="record_transition_moments"):
        pf.smooth(method="map")
    pf.record_transition_moments = False
    with pytest.raises(ValueError, match="smooth_draws"):
        evaluation.run_filter(pf, {}, smooth_method="map", smooth_draws=8)
    with pytest.raises(ValueError, match="smooth_transition_moments"):
        evaluation.run_filter(pf, {}, smooth_method="map", smooth_transition_moments=True)
    assert pf.last_smoothed is None
    with pytest.raises(ValueError, match="history"):
        evaluation.path_log_density(pf, np.zeros((2, 2), dtype=np.int64))


def test_state_dependent_noise_is_refused():
    f = sc.cpu_filter_with_history(state_dependent=True).f
    with pytest.raises(ValueError, match="state-dependent"):
        f.smooth(method="map")
    assert f.last_smoothed is None


def test_path_log_density_is_the_definition():
    import torch

    from multimodalfilter_amd import evaluation

    made = sc.cpu_filter_with_history()
    f, X, F, ll, lw, L = made.f, made.X, made.X[:-1].copy(), made.ll, made.lw, made.L
    T, N, M, _ = X.shape
    ref = mc.viterbi_reference(X, F, ll, lw[0], L)
    got = evaluation.path_log_density(f, ref["indices"])
    assert got.dtype == torch.float64 and got.shape == (N,)
    assert float(np.abs(got.numpy() - ref["log_posterior"]).max()) <= mc.REF_EPS
    rng = np.random.default_rng(3)
    idx = rng.integers(0, M, size=(T, N, 5))
    idx[2, 1, 3] = -1
    idx[0, 0, 0] = -1
    got = evaluation.path_log_density(f, torch.from_numpy(idx).to(torch.int32)).numpy()
    want = np.stack([mc.path_density(X, F, ll, lw[0], L, idx[:, :, s]) for s in range(5)], axis=1)
    assert got.shape == (N, 5) and got[1, 3] == -np.inf and got[0, 0] == -np.inf and np.isfinite(got).sum() == 8
    assert np.array_equal(np.isfinite(got), np.isfinite(want))
    fin = np.isfinite(want)
    assert float(np.abs(got[fin] - want[fin]).max()) <= mc.REF_EPS
    assert bool((got <= ref["log_posterior"][:, None] + mc.REF_EPS).all())  # no path beats the optimum
    for bad in (np.full((T, N), M), np.full((T, N), -2), np.zeros((T, N + 1), dtype=np.int64), np.zeros((T, N))):
        with pytest.raises(ValueError):
            evaluation.path_log_density(f, bad)


# ------------------------------------------------------------------------------------------ 4. the yardstick and the bars
def test_the_bars_are_three_times_the_yardstick():
    """The fp32 yardstick over the GPU tests' cases, each step restated in fp64 from the yardstick's own previous row: the
    figures of the module docstring, and the bars of ``_map_cases`` by the rule."""
    worst = dict(v=0.0, lp=0.0, regret=0.0, end=0.0)
    for name in mc.GPU_CASES:
        X, F, ll, lw, L = mc.build_case(name)
        lw0 = None if lw is None else lw[0]
        r = mc.check_run(mc.yardstick32(X, F, ll, lw0, L), X, F, ll, lw0, L)
        print(f"{name}: v {r['v']:.3e} log_posterior {r['lp']:.3e} regret {r['regret']:.3e} end to end {r['end']:.3e}")
        assert r["psi_ok"], name
        worst = {k: max(worst[k], r[k]) for k in worst}
    print(f"worst: v {worst['v']:.3e} log_posterior {worst['lp']:.3e} regret {worst['regret']:.3e} end to end {worst['end']:.3e}")
    assert mc.V_BAR == mc.ladder(worst["v"]) and mc.LP_BAR == mc.ladder(worst["lp"])
    assert mc.REGRET == 3.0 * worst["regret"]
    assert worst["v"] <= 1.05 * mc.YARDSTICK_V and worst["lp"] <= 1.05 * mc.YARDSTICK_LP  # (the recorded figures)
    assert worst["end"] <= mc.REF_EPS

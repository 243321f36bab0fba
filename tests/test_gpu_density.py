"""Particle-posterior density on the GPU: ``mmf_pf_density`` (``csrc/pf_density.hip``) against the fp64 definition of
``tests/_density_cases.py`` on its whole family, the far tail that a fixed shift loses, its bit-for-bit identities (two
calls, a row alone, with and without a truth, every subset of the outputs), its internal consistency, the particle limit, and
``ParticleFilter.belief_density`` / ``evaluation.run_filter(return_density=)`` end to end on small real filters.

The bar of ``log_density``, ``log_score`` and ``entropy``: ``|got - fp64| <= REL_TOL max(1, |fp64|)`` (``_density_cases.log_err``)
with ``-inf`` and NaN exactly where the definition puts them; ``bandwidth``: ``rel_err_elementwise < REL_TOL``; the mode is the
first maximum of the kernel's own ``log_density``, a bit copy of that particle, and within the bar of the reference's maximum
(``_density_cases.check_mode``).  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _density_cases as dc
import _quantile_cases as qc
import _score_cases as sk
import _smooth_cases as sc
import _summary_gpu as sg
from _summary_gpu import N, _filter_run, _same_bits
from _tol import REL_TOL

pytestmark = pytest.mark.gpu

OUTPUTS = dc.OUTPUTS


def _run(case, want=OUTPUTS, rows=None):
    """``_abi.pf_density`` on a case (or on ``rows`` of it) with every output between guard rows; the outputs not in ``want``
    are handed over as null and their buffers must come back untouched -> ``dict`` of device tensors (``None`` for those).
    Without a truth ``log_score`` is never asked for."""
    from multimodalfilter_amd import _abi

    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    X, la, lb, y = (sc.to_device(pick(case[k])) for k in ("states", "log_a", "log_b", "truth"))
    if y is None:
        want = tuple(k for k in want if k != "log_score")
    R, M, d = X.shape

    def call(out):
        out["bandwidth_out"] = out.pop("bandwidth")
        _abi.pf_density(X, la, lb, y, rule=case["rule"], bandwidth=case["bandwidth"], min_bandwidth=case["min_bandwidth"], **out)

    tails = {"log_density": (M,), "log_score": (), "entropy": (), "mode": (d,), "bandwidth": (d,), "mode_index": ()}
    return sg.guarded_call(call, R, tails, want, OUTPUTS, f"M={M} d={d} R={R}", {"mode_index": torch.int32})


def _hold(case, ref, got, what):
    """Every output against the reference (those the case has); returns the errors."""
    errs = {"log_density": dc.log_err(N(got["log_density"]), ref["log_density"], f"{what} log_density"),
            "entropy": dc.log_err(N(got["entropy"]), ref["entropy"], f"{what} entropy"),
            "bandwidth": dc.bandwidth_err(N(got["bandwidth"]), ref["bandwidth"], f"{what} bandwidth")}
    if ref["log_score"] is not None:
        errs["log_score"] = dc.log_err(N(got["log_score"]), ref["log_score"], f"{what} log_score")
    errs["mode"] = dc.check_mode(case["states"], qc.weights64(case), N(got["log_density"]), N(got["mode_index"]), N(got["mode"]),
                                 ref["log_density"], what)
    print(f"{what}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" (bar {REL_TOL:.0e})")
    for k, e in errs.items():
        assert e <= REL_TOL, (what, k, e)
    return errs


# ------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("M", sk.ALL_MS)
def test_kernel_holds_the_definition_on_the_family(M):
    cases = 0
    for case_id in dc.family():
        if case_id[0] != M:
            continue
        case, ref = dc.family_case(*case_id)
        _hold(case, ref, _run(case), "M=%d d=%d R=%d %s %s" % case_id)
        cases += 1
    assert cases >= len(dc.VARIANTS)


def test_kernel_at_the_particle_limit():
    """32 workgroups per row, 16 j-tiles each."""
    case = dc.make_case(dc.MAX_M, 1, 1, "plain", "silverman")
    _hold(case, dc.reference(case), _run(case), f"M={dc.MAX_M} d=1")


# ------------------------------------------------------------------------------------------ 2. the far tail
def _uniform_case(X, truth, rule):
    d = X.shape[-1]
    return dict(states=X.astype(np.float32), log_a=None, log_b=None, truth=np.asarray(truth, np.float32), rule=rule,
                bandwidth=dc.FIXED[:d] if rule == "fixed" else None, min_bandwidth=(dc.MIN_BANDWIDTH,) * d)


@pytest.mark.parametrize("M", [257, 1025])
def test_a_truth_fifty_sigma_off_has_a_finite_log_score(M):
    """What a fixed shift by ``max a`` returns as ``-inf``: every exponent is below ``-1000``."""
    rng = np.random.default_rng(M)
    for d in sk.DIMS:
        X = rng.standard_normal((3, M, d))
        truth = X.mean(1) + 50.0 * X.std(1) * np.where(np.arange(d) % 2 == 0, 1.0, -1.0)
        for rule in dc.RULES:
            case = _uniform_case(X, truth, rule)
            ref = dc.reference(case)
            got = _run(case)
            assert np.isfinite(N(got["log_score"])).all() and (ref["log_score"] < -400.0).all(), (d, rule, ref["log_score"])
            _hold(case, ref, got, f"50 sigma M={M} d={d} {rule}")


def test_a_collapsed_set_has_a_finite_log_score_one_unit_away():
    """64 identical particles: ``h`` is the floor 1e-6 under the rules, and the truth 1.0 away is 1e6 bandwidths off."""
    for d in sk.DIMS:
        X = np.tile(np.linspace(0.25, 1.0, d, dtype=np.float32), (2, 64, 1))
        truth = X[:, 0, :].copy()
        truth[:, 0] += 1.0
        for rule in dc.RULES:
            case = _uniform_case(X, truth, rule)
            ref = dc.reference(case)
            got = _run(case)
            assert np.isfinite(N(got["log_score"])).all(), (d, rule, N(got["log_score"]))
            if rule != "fixed":
                assert (N(got["bandwidth"]) == np.float32(dc.MIN_BANDWIDTH)).all() and (ref["log_score"] < -4e11).all()
            _hold(case, ref, got, f"collapsed d={d} {rule}")


# ------------------------------------------------------------------------------------------ 3. bit-for-bit identities
BIT_MS = [1, 65, 257, 512, 513, 1025, 4096]
PARTICLE_OUTPUTS = tuple(k for k in OUTPUTS if k != "log_score")


@pytest.mark.parametrize("M", BIT_MS)
def test_two_calls_a_row_alone_and_a_missing_truth_give_the_same_bits(M):
    for d, variant, rule in ((1, "plain", "silverman"), (3, "dead_row", "scott"), (4, "moderate", "fixed")):
        case = dc.make_case(M, d, 3, variant, rule)
        got = sg.assert_repeatable(_run, case, OUTPUTS, range(3), (M, d, variant))
        blind = _run(dict(case, truth=None))
        assert blind["log_score"] is None
        for k in PARTICLE_OUTPUTS:
            assert _same_bits(blind[k], got[k]), (M, d, variant, k)


@pytest.mark.parametrize("M", BIT_MS)
def test_every_subset_of_the_outputs_writes_the_bits_of_the_full_call_and_nothing_else(M):
    """All 63 non-empty subsets (the untouched buffers are checked inside ``_run``)."""
    sg.assert_subsets_match_full(_run, dc.make_case(M, 3, 3, "plain", "silverman"), OUTPUTS, what=(M,))


# ------------------------------------------------------------------------------------------ 4. consistency
@pytest.mark.parametrize("M", [2, 65, 513, 1025])
def test_the_log_score_at_a_particle_is_that_particles_log_density(M):
    for d, variant, rule in ((1, "plain", "silverman"), (2, "moderate", "scott"), (3, "uniform", "fixed"), (4, "moderate", "silverman")):
        case = dict(dc.make_case(M, d, 3, variant, rule))
        W = qc.weights64(case)
        at = [int(np.flatnonzero(W[r] > 0)[(7 * r + 3) % int((W[r] > 0).sum())]) for r in range(3)]
        case["truth"] = np.stack([case["states"][r, at[r]] for r in range(3)])
        got = _run(case)
        score, own = N(got["log_score"]).astype(np.float64), N(got["log_density"])[np.arange(3), at].astype(np.float64)
        err = float((np.abs(score - own) / np.maximum(1.0, np.abs(own))).max())
        print(f"M={M} d={d} {variant} {rule}: log_score against the particle's own log_density {err:.3e}")
        assert err <= REL_TOL
        # the entropy, recomputed in fp64 from the kernel's own log_density and the weights
        live = W > 0
        Wn = W / W.sum(-1, keepdims=True)
        want = -np.where(live, Wn * np.where(live, N(got["log_density"]).astype(np.float64), 0.0), 0.0).sum(-1)
        e_err = dc.log_err(N(got["entropy"]), want, "entropy")
        print(f"M={M} d={d} {variant} {rule}: entropy against its own log_density {e_err:.3e}")
        assert e_err <= REL_TOL


# ------------------------------------------------------------------------------------------ 5. through the filter
def _case_of(states, log_a, log_b, truth, rule="silverman", bandwidth=None, min_bandwidth=dc.MIN_BANDWIDTH):
    d = states.shape[-1]
    return sg._case_of(states, log_a, log_b, truth, rule=rule, bandwidth=bandwidth, min_bandwidth=(min_bandwidth,) * d)


def _hold_record(rec, case, shape, what):
    T, N_, M, d = shape
    got = {"log_density": rec.log_density.reshape(T * N_, M), "entropy": rec.entropy.reshape(T * N_),
           "bandwidth": rec.bandwidth.reshape(T * N_, d), "mode": rec.mode.reshape(T * N_, d),
           "mode_index": rec.mode_index.reshape(T * N_),
           "log_score": rec.log_score.reshape(T * N_) if hasattr(rec, "log_score") else None}
    _hold(case, dc.reference(case), got, what)


@pytest.mark.parametrize("M", [64, 300])
def test_belief_density_on_a_real_filter(M):
    """``of="filtered"``, ``of="smoothed"`` after the marginal smoother and after backward simulation equal the fp64
    definition evaluated on the records' own arrays.  Nothing else moves: the estimates, the history, the smoothed record,
    the quantile and score records and the noise stream are what they are without the calls."""
    from multimodalfilter_amd.utils import ReplayNoise

    f, forward, traj, shape = _filter_run("DoorCrossmodalParticleFilter", M, owner="density")
    T, N_, _, d = shape
    est = forward().clone()
    h = f.last_history
    truth = traj["states"][1:]
    before = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in", "ancestors") if getattr(h, k) is not None}
    f.belief_quantiles((0.5,), truth=truth)
    f.belief_scores(truth)
    quantiles, scores = f.last_quantiles, f.last_scores
    kept = quantiles.quantiles.clone(), scores.crps.clone()
    f.last_density = None
    mode = f.belief_density(truth)
    rec = f.last_density
    assert set(vars(rec)) == {"mode", "mode_index", "log_density", "entropy", "bandwidth", "of", "rule", "log_score"}
    assert rec.of == "filtered" and rec.rule == "silverman" and type(rec.rule) is str
    assert rec.mode is mode and mode.shape == (T, N_, d) and rec.mode_index.shape == (T, N_) and rec.mode_index.dtype == torch.int32
    assert rec.log_density.shape == (T, N_, M) and rec.entropy.shape == (T, N_) and rec.bandwidth.shape == (T, N_, d)
    picked = torch.gather(h.states, 2, rec.mode_index.long()[..., None, None].expand(T, N_, 1, d))[:, :, 0]
    assert torch.equal(mode, picked)
    _hold_record(rec, _case_of(h.states, h.log_weights_in, h.log_likelihoods, truth), shape, f"M={M} filtered")
    # without a truth: no log_score, everything else the same bits
    f.belief_density()
    blind = f.last_density
    assert not hasattr(blind, "log_score") and torch.equal(blind.mode, mode) and _same_bits(blind.log_density, rec.log_density)
    assert _same_bits(blind.entropy, rec.entropy) and torch.equal(blind.mode_index, rec.mode_index)
    # Scott's rule with a floor per dimension, and fixed bandwidths
    f.belief_density(truth, bandwidth="scott", min_bandwidth=(1e-3, 1e-4, 1e-5))
    case = _case_of(h.states, h.log_weights_in, h.log_likelihoods, truth, "scott")
    case["min_bandwidth"] = (1e-3, 1e-4, 1e-5)
    assert f.last_density.rule == "scott"
    _hold_record(f.last_density, case, shape, f"M={M} filtered, scott")
    fixed = (0.05, 0.2, 0.1)
    f.belief_density(truth, bandwidth=fixed)
    assert f.last_density.rule == "fixed" and bool((f.last_density.bandwidth == torch.tensor(fixed, device=mode.device)).all())
    _hold_record(f.last_density, _case_of(h.states, h.log_weights_in, h.log_likelihoods, truth, "fixed", fixed), shape, f"M={M} filtered, fixed")
    assert f.last_quantiles is quantiles and torch.equal(quantiles.quantiles, kept[0])
    assert f.last_scores is scores and torch.equal(scores.crps, kept[1])
    after = f.noise.uniform((4, 5), like=h.states).clone()  # where the noise stream stands after the calls ...
    assert torch.equal(forward(), est)
    assert torch.equal(f.noise.uniform((4, 5), like=h.states), after)  # ... is where it stands without them
    f.last_history = h
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k

    # the marginal smoother's weights over the history's states
    mean = f.smooth(method="marginal").clone()
    s = f.last_smoothed
    weights = s.weights.clone()
    f.belief_density(truth, of="smoothed")
    assert f.last_smoothed is s and torch.equal(s.weights, weights) and f.last_density.of == "smoothed"
    _hold_record(f.last_density, _case_of(h.states, torch.log(weights), None, truth), shape, f"M={M} marginal")
    assert torch.equal(f.smooth(method="marginal"), mean)

    # backward simulation: 16 equally weighted draws per step
    S = 16
    f.noise = ReplayNoise(uniforms=[torch.rand((T, N_, S), generator=torch.Generator().manual_seed(5))])
    f.smooth(method="simulation", num_draws=S)
    s = f.last_smoothed
    assert bool(torch.isfinite(s.trajectories).all())
    f.belief_density(truth, of="smoothed")
    _hold_record(f.last_density, _case_of(s.trajectories, None, None, truth), (T, N_, S, d), f"M={M} simulation")
    assert f.last_smoothed is s and f.last_history is h and f.last_quantiles is quantiles and f.last_scores is scores
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k
    for method in ("ancestry", "map"):
        f.smooth(method=method)
        kept_density = f.last_density
        with pytest.raises(ValueError, match="of='smoothed'"):
            f.belief_density(truth, of="smoothed")
        assert f.last_density is kept_density


# ------------------------------------------------------------------------------------------ 6. run_filter(return_density=)
def test_run_filter_places_the_density_record_between_the_scores_and_the_quantiles():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N_, M, T = 3, 64, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorCrossmodalParticleFilter", N_, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    plain = evaluation.run_filter(f, traj)
    f.noise = mmf.CounterNoise(7)
    off = evaluation.run_filter(f, traj, return_density=False)
    assert isinstance(off, torch.Tensor) and torch.equal(off, plain)
    f.noise = mmf.CounterNoise(7)
    others = evaluation.run_filter(f, traj, return_belief=True, return_scores=True, return_quantiles=(0.5,))
    f.noise = mmf.CounterNoise(7)
    same = evaluation.run_filter(f, traj, return_belief=True, return_scores=True, return_quantiles=(0.5,), return_density=False)
    assert len(same) == len(others) == 4 and torch.equal(same[0], others[0]) and torch.equal(same[1].covariance, others[1].covariance)
    assert _same_bits(same[2].crps, others[2].crps) and _same_bits(same[2].energy, others[2].energy)
    assert _same_bits(same[3].quantiles, others[3].quantiles) and _same_bits(same[3].pit, others[3].pit)
    f.noise = mmf.CounterNoise(7)
    est, rec = evaluation.run_filter(f, traj, return_density=True)
    assert f.record_history is False and f.record_belief is False  # put back
    assert torch.equal(est, plain)
    assert rec is f.last_density and rec.of == "filtered" and rec.rule == "silverman" and rec.log_score.shape == (T, N_)
    h = f.last_history
    _hold_record(rec, _case_of(h.states, h.log_weights_in, h.log_likelihoods, traj["states"][1:]), (T, N_, M, d), "run_filter")
    summary = evaluation.density_summary(rec, start=0)
    assert set(summary) == {"log_score", "entropy"}
    assert abs(summary["entropy"] - float(rec.entropy.double().mean())) <= 1e-9 * max(1.0, abs(summary["entropy"]))
    f.noise = mmf.CounterNoise(7)
    out = evaluation.run_filter(f, traj, return_belief=True, return_scores=True, return_density=True, density_bandwidth="scott",
                                return_quantiles=(0.5,))
    assert len(out) == 5 and out[1] is f.last_belief and out[2] is f.last_scores and out[3] is f.last_density
    assert out[4] is f.last_quantiles and out[3].rule == "scott" and torch.equal(out[0], plain)
    assert _same_bits(out[2].crps, others[2].crps) and _same_bits(out[4].quantiles, others[3].quantiles)
    f.noise = mmf.CounterNoise(7)
    out = evaluation.run_filter(f, traj, smooth_method="marginal", return_density=True, density_bandwidth=(0.05, 0.2, 0.1),
                                return_quantiles=(0.5,))
    assert len(out) == 3 and out[1] is f.last_density and out[1].of == "smoothed" and out[1].rule == "fixed"
    assert out[2] is f.last_quantiles and out[2].of == "smoothed" and f.record_history is False and f.record_belief is False
    f.noise = mmf.NoiseSource(7)  # (backward simulation draws (T, N, S) uniforms, which a CounterNoise does not)
    out = evaluation.run_filter(f, traj, smooth_method="simulation", smooth_draws=8, return_belief=True, return_density=True)
    assert len(out) == 3 and out[1] is f.last_smoothed and out[2].of == "smoothed" and out[2].log_density.shape == (T, N_, 8)


def test_run_filter_gives_a_kalman_filter_the_closed_forms():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation, synthetic
    from oracle import models as om

    dev = sc.dev()
    N_, T = 3, 6
    d = om.TASKS["door"].state_dim
    torch.manual_seed(3)
    f = mmf.door_models.DoorKalmanFilter().to(dev).eval()
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N_, seed=17).items()}
    truth = traj["states"][1:]
    plain = evaluation.run_filter(f, traj)
    est, belief = evaluation.run_filter(f, traj, return_belief=True)
    assert torch.equal(est, plain)
    est2, rec = evaluation.run_filter(f, traj, return_density=True)
    assert f.record_belief is False and torch.equal(est2, plain)
    assert set(vars(rec)) == {"log_score", "entropy", "mode", "of"} and rec.of == "filtered" and torch.equal(rec.mode, plain)
    assert torch.equal(rec.log_score, evaluation.gaussian_log_density(est, belief.covariance, truth)) and rec.log_score.shape == (T, N_)
    assert torch.equal(rec.entropy, evaluation.gaussian_entropy(belief.covariance))
    nll = evaluation.gaussian_nll(est, belief.covariance, truth, start=0)
    assert torch.allclose(-rec.log_score.mean(0), nll, rtol=1e-5, atol=1e-5)
    assert set(evaluation.density_summary(rec, start=0)) == {"log_score", "entropy"}
    out = evaluation.run_filter(f, traj, return_belief=True, return_innovations=True, return_scores=True, return_density=True)
    assert len(out) == 5 and out[2] is f.last_innovations and hasattr(out[3], "crps") and torch.equal(out[4].log_score, rec.log_score)
    # smoothed: the smoothed means under the smoothed covariance
    sm, srec = evaluation.run_filter(f, traj, smooth_lag=None, return_belief=True)
    sm2, rec2 = evaluation.run_filter(f, traj, smooth_lag=None, return_density=True)
    assert torch.equal(sm, sm2) and rec2.of == "smoothed"
    assert torch.equal(rec2.log_score, evaluation.gaussian_log_density(sm, srec.covariance, truth))
    lstm = mmf.door_models.DoorLSTMFilter().to(dev).eval()
    with pytest.raises(ValueError, match="return_density"):
        evaluation.run_filter(lstm, traj, return_density=True)

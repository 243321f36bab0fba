"""Per-modality attribution on the GPU: ``mmf_pf_modalities`` (``csrc/pf_modalities.hip``) against the fp64 definition of
``tests/_modality_cases.py`` on its whole family and at the particle limit, its bit-for-bit identities (two calls, a row
alone, every subset of the outputs), the exact cases, and ``ParticleFilter.belief_modalities`` /
``evaluation.run_filter(return_modalities=)`` end to end on small real filters.

The bars are those of ``_modality_cases.compare``, every one ``< REL_TOL``; every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _modality_cases as mc
import _smooth_cases as sc
from _density_cases import log_err
from _score_cases import compare as rel_compare
from _summary_gpu import N, _filter_run, assert_repeatable, assert_subsets_match_full, guarded_call
from _tol import REL_TOL

pytestmark = pytest.mark.gpu

OUTPUTS = mc.OUTPUTS


def _run(case, want=OUTPUTS, rows=None):
    """``_abi.pf_modalities`` on a case (or on ``rows`` of it) with every output between guard rows; the outputs not in
    ``want`` are handed over as null and their buffers must come back untouched -> ``dict`` of device tensors (``None`` for
    those)."""
    from multimodalfilter_amd import _abi

    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    X, lw, beta = (sc.to_device(pick(case[k])) for k in ("states", "log_w", "beta"))
    l = sc.to_device(case["loglik"] if rows is None else case["loglik"][:, rows])
    R, M, d = X.shape
    K = l.shape[0]
    return guarded_call(lambda out: _abi.pf_modalities(X, lw, [l[k] for k in range(K)], beta, **out), R, mc.shapes(R, K, d),
                        want, OUTPUTS, f"M={M} d={d} R={R} K={K}")


def _hold(case, ref, got, what):
    errs = mc.compare(case, got, ref, what)
    print(f"{what}: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()) + f" (bar {REL_TOL:.0e})")
    for k, e in errs.items():
        assert e < REL_TOL, (what, k, e)
    return errs


# ------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("M", mc.MS)
def test_kernel_holds_the_definition_on_the_family(M):
    worst = {}
    for M_, d, R, K, variant in mc.family():
        if M_ != M:
            continue
        case, ref = mc.family_case(M, d, R, K, variant)
        what = f"M={M} d={d} R={R} K={K} {variant}"
        errs = mc.compare(case, _run(case), ref, what)
        for k, e in errs.items():
            assert e < REL_TOL, (what, k, e)
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"M={M}: worst " + ", ".join(f"{k} {e:.3e}" for k, e in worst.items()) + f" (bar {REL_TOL:.0e})")


def test_kernel_at_the_particle_limit():
    """512 threads, eight batches of four particles each, the widest shape."""
    case = mc.make_case(mc.MAX_M, 4, 1, 4, "plain")
    _hold(case, mc.reference(case), _run(case), f"M={mc.MAX_M} d=4 K=4")


# ------------------------------------------------------------------------------------------ 2. bit-for-bit identities
@pytest.mark.parametrize("M", [1, 65, 257, 513, mc.THREADS * mc.RUN_PT, mc.THREADS * mc.RUN_PT + 1, 2 * mc.THREADS * mc.RUN_PT + 1])
def test_two_calls_and_a_row_alone_give_the_same_bits(M):
    for d, K, variant in ((1, 1, "plain"), (3, 2, "dead_row"), (4, 4, "blackout"), (2, 3, "nan_loglik")):
        assert_repeatable(_run, mc.make_case(M, d, 3, K, variant), OUTPUTS, range(3), (M, d, K, variant))


@pytest.mark.parametrize("M", [65, 257, mc.THREADS * mc.RUN_PT + 1])
def test_every_subset_of_the_outputs_writes_the_bits_of_the_full_call_and_nothing_else(M):
    """(the untouched buffers and the guard rows are checked inside ``_run``)"""
    assert_subsets_match_full(_run, mc.make_case(M, 3, 3, 3, "blackout"), OUTPUTS, what=(M,))


# ------------------------------------------------------------------------------------------ 3. the exact cases
@pytest.mark.parametrize("M", [2, 65, 1000])
def test_one_modality_is_the_whole_fusion(M):
    for d in (1, 3):
        for variant in ("plain", "no_beta", "uniform"):
            case = mc.make_case(M, d, 3, 1, variant)
            got = {k: N(v).astype(np.float64) for k, v in _run(case).items()}
            what = (M, d, variant)
            b = 0.0 if case["beta"] is None else case["beta"][:, 0].astype(np.float64)
            print(what, "rho - 1", np.abs(got["responsibility"] - 1).max(), "divergence", np.abs(got["divergence"]).max())
            assert rel_compare(got["responsibility"], np.ones((3, 1)), "rho") < REL_TOL, what
            assert log_err(got["divergence"], np.zeros((3, 1)), "divergence") < REL_TOL, what
            assert log_err(got["log_evidence"][:, 0] + b, got["log_evidence"][:, 1], "log_evidence") < REL_TOL, what
            assert rel_compare(got["ess"][:, 0], got["ess"][:, 1], "ess") < REL_TOL and bool((got["overlap"] == 1).all()), what
            if case["beta"] is None:                                  # then u and v are the same floats
                assert bool((got["divergence"] == 0).all()) and bool((got["responsibility"] == 1).all()), what
                assert bool((got["log_evidence"][:, 0] == got["log_evidence"][:, 1]).all()), what
                assert bool((got["mean"][:, 0] == got["mean"][:, 1]).all()) and bool((got["ess"][:, 0] == got["ess"][:, 1]).all()), what


@pytest.mark.parametrize("M", [2, 65, 1000])
def test_identical_modalities_share_by_beta_alone(M):
    for K in (2, 4):
        case = mc.make_case(M, 3, 3, K, "identical")
        got = {k: N(v).astype(np.float64) for k, v in _run(case).items()}
        b = case["beta"].astype(np.float64)
        soft = np.exp(b - np.log(np.exp(b).sum(-1, keepdims=True)))
        errs = dict(rho=rel_compare(got["responsibility"], soft, "rho"), overlap=rel_compare(got["overlap"], np.ones((3, K, K)), "overlap"),
                    divergence=log_err(got["divergence"], np.zeros((3, K)), "divergence"))
        print(f"M={M} K={K} identical: " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
        assert max(errs.values()) < REL_TOL, (M, K, errs)
        assert bool((got["overlap"] == got["overlap"].transpose(0, 2, 1)).all())


@pytest.mark.parametrize("M", [2, 65, 1000])
def test_disjoint_modalities_do_not_overlap_at_all(M):
    for K in (2, 3):
        case = mc.make_case(M, 2, 3, K, "disjoint")
        got = _run(case)
        _hold(case, mc.reference(case), got, f"M={M} K={K} disjoint")
        ov = N(got["overlap"])
        assert bool((ov[:, 0, 1] == 0).all()) and bool((ov[:, 1, 0] == 0).all()), (M, K, ov)
        assert bool((ov.view(np.uint32) == ov.transpose(0, 2, 1).copy().view(np.uint32)).all())
        if K == 2:
            rho, div = N(got["responsibility"]).astype(np.float64), N(got["divergence"]).astype(np.float64)
            assert log_err(div, -np.log(rho), "divergence = -log rho") < REL_TOL, (M, div, rho)


def _minus_infinity_case(M, K):
    """The plain case with ``beta_0 = -inf`` in every row (a weight model that knows of a blackout) and, in row 1, every
    ``beta_k = -inf``: no modality with a share there."""
    case = dict(mc.make_case(M, 3, 3, K, "plain"))
    beta = case["beta"].copy()
    beta[:, 0] = -np.inf
    beta[1] = -np.inf
    case["beta"] = beta
    return case


@pytest.mark.parametrize("M", [2, 65, 1000])
def test_a_modality_log_weight_of_minus_infinity_takes_no_share(M):
    for K in (1, 2, 3):
        case = _minus_infinity_case(M, K)
        ref = mc.reference(case)
        got = _run(case)
        _hold(case, ref, got, f"M={M} K={K} beta = -inf")
        rho, le = N(got["responsibility"]), N(got["log_evidence"])
        assert bool((rho[:, 0] == 0).all()) and bool((rho[1] == 0).all()), (M, K, rho)
        assert bool(np.isfinite(le[:, :K]).all()) and le[1, K] == -np.inf, (M, K, le)   # each sensor's own evidence stays
        assert bool(np.isnan(N(got["divergence"])[1]).all()) and bool(np.isnan(N(got["mean"])[1, K]).all())
        if K > 1:
            assert np.allclose(rho[[0, 2]].sum(-1), 1.0, rtol=0, atol=1e-5)


# ------------------------------------------------------------------------------------------ 4. through the filter
def _record_case(h, rec):
    """The record's own inputs as a case of ``T N`` rows."""
    T, N_, M, d = h.states.shape
    K = rec.log_likelihoods.shape[0]
    C = lambda x: x.detach().cpu().numpy()
    return dict(states=C(h.states).reshape(T * N_, M, d), log_w=C(h.log_weights_in).reshape(T * N_, M),
                loglik=C(rec.log_likelihoods).reshape(K, T * N_, M), beta=None if rec.log_weights is None else C(rec.log_weights).reshape(T * N_, K))


def _hold_filter(kind, M):
    f, forward, traj, (T, N_, _, d) = _filter_run(kind, M, owner="modalities")
    f.record_belief = True
    try:
        est = forward().clone()
    finally:
        f.record_belief = False
    h, belief = f.last_history, f.last_belief
    assert h.observations is not None and tuple(h.enabled_models) == (True, True)
    kept = (f.last_smoothed, f.last_quantiles, f.last_scores, f.last_density, f.last_modes)
    before = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in")}
    f.last_modalities = None
    rho = f.belief_modalities()
    torch.cuda.synchronize()
    rec = f.last_modalities
    K = 2
    assert set(vars(rec)) == {"responsibility", "log_evidence", "ess", "mean", "divergence", "overlap", "log_likelihoods", "log_weights",
                              "modalities"}
    assert rec.responsibility is rho and rec.modalities == (0, 1) and rho.shape == (T, N_, K)
    assert rec.log_evidence.shape == rec.ess.shape == (T, N_, K + 1) and rec.mean.shape == (T, N_, K + 1, d)
    assert rec.divergence.shape == (T, N_, K) and rec.overlap.shape == (T, N_, K, K)
    assert rec.log_likelihoods.shape == (K, T, N_, M) and rec.log_weights.shape == (T, N_, K)
    now = (f.last_smoothed, f.last_quantiles, f.last_scores, f.last_density, f.last_modes)
    assert f.last_history is h and all(a is b for a, b in zip(now, kept))
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k

    # the definition on the record's own inputs
    case = _record_case(h, rec)
    got = {k: getattr(rec, k).reshape((T * N_,) + tuple(getattr(rec, k).shape[2:])) for k in OUTPUTS}
    _hold(case, mc.reference(case), got, f"{kind} M={M}")

    # the re-evaluated l_k are what the filter fused
    s = case["beta"].T[:, :, None].astype(np.float64) + case["loglik"].astype(np.float64)
    fused = mc._lse(np.where(np.isnan(s), -np.inf, s), 0)
    e_fused = log_err(fused, N(h.log_likelihoods).reshape(T * N_, M).astype(np.float64), "logsumexp_k(beta + l_k)")
    # the fused entries are the filter's own estimate and belief record
    top = np.nanmax(np.abs(N(h.states).reshape(T * N_, -1)), axis=-1)      # the largest live |coordinate| of every row
    e_mean = float((np.abs(N(rec.mean[:, :, K]) - N(est)).reshape(T * N_, d).max(-1) / top).max())
    e_le = log_err(N(rec.log_evidence[..., K]), N(belief.log_evidence).astype(np.float64), "log_evidence")
    e_ess = rel_compare(N(rec.ess[..., K]), N(belief.ess).astype(np.float64), "ess")
    mix = (rec.responsibility.double()[..., None] * rec.mean.double()[:, :, :K]).sum(2)
    e_mix = float(((mix - rec.mean.double()[:, :, K]).abs().reshape(T * N_, d).max(-1).values.cpu().numpy() / top).max())
    print(f"{kind} M={M}: fused log-likelihood {e_fused:.3e}, mean against the estimate {e_mean:.3e}, log_evidence {e_le:.3e}, "
          f"ess {e_ess:.3e}, sum rho_k mean_k against the fused mean {e_mix:.3e} (bar {REL_TOL:.0e})")
    assert e_fused <= REL_TOL and e_mean < REL_TOL and e_le < REL_TOL and e_ess < REL_TOL and e_mix < REL_TOL
    assert bool(((rho.sum(-1) - 1).abs() < 1e-5).all())
    return f, forward, est


@pytest.mark.parametrize("M", [64, 300])
def test_belief_modalities_on_a_real_filter(M):
    f, forward, est = _hold_filter("DoorCrossmodalParticleFilter", M)
    h = f.last_history
    after = f.noise.uniform((4, 5), like=h.states).clone()  # where the noise stream stands after the call ...
    assert torch.equal(forward(), est)
    assert torch.equal(f.noise.uniform((4, 5), like=h.states), after)  # ... is where it stands without it


def test_belief_modalities_reports_a_range_flag_raised_while_it_encodes_again():
    """The status word is checked around the whole call: a report of the observation encoders, which run before the
    measurement networks, is not cleared away on the way into them."""
    from multimodalfilter_amd import _abi, engine

    f, forward, traj, _ = _filter_run("DoorCrossmodalParticleFilter", 64, owner="modalities")
    forward()
    meas = f.measurement_model
    encode = meas.encode_observations

    def flagged(observations):
        ctx = encode(observations)
        engine.range_flag(ctx["modality_log_weights"].device).bitwise_or_(_abi.FLAG_RANGE)  # (what an f16x3 encoder launch does)
        return ctx

    meas.encode_observations = flagged
    try:
        with pytest.raises(_abi.MmfError, match="f16x3 operand range"):
            f.belief_modalities()
    finally:
        del meas.encode_observations
    f.belief_modalities()                                          # and the flag was consumed: the next call is clean


def test_belief_modalities_on_the_push_filter():
    _hold_filter("PushCrossmodalParticleFilter", 64)


def test_one_enabled_modality_and_a_changed_mask():
    f, forward, traj, (T, N_, M, d) = _filter_run("DoorCrossmodalParticleFilter", 64, owner="modalities-mask")
    meas = f.measurement_model
    try:
        meas.enabled_models = [True, False]
        est = forward()
        h = f.last_history
        assert h.enabled_models == (True, False)
        rho = f.belief_modalities()
        rec = f.last_modalities
        assert rec.modalities == (0,) and rho.shape == (T, N_, 1) and rec.mean.shape == (T, N_, 2, d) and rec.overlap.shape == (T, N_, 1, 1)
        assert rec.log_likelihoods.shape == (1, T, N_, M) and rec.log_weights.shape == (T, N_, 1)
        case = _record_case(h, rec)
        got = {k: getattr(rec, k).reshape((T * N_,) + tuple(getattr(rec, k).shape[2:])) for k in OUTPUTS}
        _hold(case, mc.reference(case), got, "enabled [True, False]")
        assert rel_compare(N(rho), np.ones((T, N_, 1)), "rho") < REL_TOL
        top = np.nanmax(np.abs(N(h.states).reshape(T * N_, -1)), axis=-1)
        assert float((np.abs(N(rec.mean[:, :, 1]) - N(est)).reshape(T * N_, d).max(-1) / top).max()) < REL_TOL
        meas.enabled_models = [True, True]
        with pytest.raises(ValueError, match="enabled_models"):
            f.belief_modalities()
        assert f.last_modalities is rec
        meas.enabled_models = [True, False]
        assert torch.equal(f.belief_modalities(), rho)
    finally:
        meas.enabled_models = [True, True]


# ------------------------------------------------------------------------------------------ 5. run_filter(return_modalities=)
def test_run_filter_places_the_modalities_record_between_the_modes_and_the_quantiles():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N_, M, T = 3, 64, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorCrossmodalParticleFilter", N_, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    plain = evaluation.run_filter(f, traj)
    f.noise = mmf.CounterNoise(7)
    off = evaluation.run_filter(f, traj, return_modalities=False)
    assert isinstance(off, torch.Tensor) and torch.equal(off, plain)
    f.noise = mmf.CounterNoise(7)
    est, rec = evaluation.run_filter(f, traj, return_modalities=True)
    assert f.record_history is False and f.record_belief is False  # put back
    assert torch.equal(est, plain) and rec is f.last_modalities and rec.responsibility.shape == (T, N_, 2)
    f.noise = mmf.CounterNoise(7)
    out = evaluation.run_filter(f, traj, return_belief=True, return_modes=2, return_modalities=True, return_quantiles=(0.5,))
    assert len(out) == 5 and out[1] is f.last_belief and out[2] is f.last_modes and out[3] is f.last_modalities and out[4] is f.last_quantiles
    assert torch.equal(out[0], plain) and torch.equal(out[3].responsibility, rec.responsibility)
    summary = evaluation.modality_summary(rec, start=0)
    assert summary["responsibility"].shape == summary["dominant"].shape == summary["prior"].shape == (2,)
    assert abs(float(summary["responsibility"].sum()) - 1) < 1e-5 and abs(float(summary["dominant"].sum()) - 1) < 1e-6
    errors = evaluation.modality_errors(rec, traj["states"][1:])
    assert errors.shape == (T, N_, 3)
    assert torch.allclose(errors[..., 2], torch.linalg.vector_norm(est - traj["states"][1:], dim=-1), rtol=0, atol=1e-3)
    # a Kalman filter and an LSTM baseline are refused before they run
    for ctor in (mmf.door_models.DoorCrossmodalKalmanFilter, mmf.door_models.DoorLSTMFilter):
        g = ctor().to(dev).eval()
        with pytest.raises(ValueError, match="return_modalities needs a crossmodal particle filter"):
            evaluation.run_filter(g, traj, return_modalities=True)


def _same_record(a, b, what):
    """Two records field by field: tensors ``torch.equal`` on their bytes (a NaN beyond the count of modes is equal to
    itself), everything else ``==``."""
    assert set(vars(a)) == set(vars(b)), what
    for k, x in vars(a).items():
        y = getattr(b, k)
        if isinstance(x, torch.Tensor):
            assert x.dtype == y.dtype and x.shape == y.shape, (what, k)
            assert torch.equal(x.contiguous().view(torch.uint8), y.contiguous().view(torch.uint8)), (what, k)
        else:
            assert x == y, (what, k)


@pytest.mark.parametrize("smooth_method", [None, "marginal"])
def test_run_filter_hands_every_summary_the_arguments_of_the_direct_call(smooth_method):
    """All the records at once, in order, and each what the direct ``belief_*`` call leaves on the same filter afterwards."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N_, M, T = 3, 64, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorCrossmodalParticleFilter", N_, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    probs = (0.1, 0.5, 0.9)
    smooth = {} if smooth_method is None else {"smooth_method": smooth_method}
    out = evaluation.run_filter(f, traj, return_belief=True, return_scores=True, return_density=True, return_modes=2,
                                return_modalities=True, return_quantiles=probs, **smooth)
    torch.cuda.synchronize()
    assert type(out) is tuple and len(out) == 7                     # (the estimates and the six records a particle filter has)
    est, belief, scores, density, modes, modalities, quantiles = out
    assert f.record_history is False and f.record_belief is False
    assert est.shape == (T, N_, d) and belief is (f.last_belief if smooth_method is None else f.last_smoothed)
    assert scores is f.last_scores and density is f.last_density and modes is f.last_modes
    assert modalities is f.last_modalities and quantiles is f.last_quantiles
    of = "filtered" if smooth_method is None else "smoothed"
    truth = traj["states"][1:]
    f.belief_scores(truth, of=of)
    _same_record(scores, f.last_scores, "scores")
    f.belief_density(truth, of=of)
    _same_record(density, f.last_density, "density")
    f.belief_modes(of, max_modes=2)
    _same_record(modes, f.last_modes, "modes")
    f.belief_modalities()
    _same_record(modalities, f.last_modalities, "modalities")
    f.belief_quantiles(probs, of=of, truth=truth)
    _same_record(quantiles, f.last_quantiles, "quantiles")
    assert scores is not f.last_scores and quantiles is not f.last_quantiles and scores.of == density.of == modes.of == quantiles.of == of

"""``evaluation.run_filter`` as a host function, on stand-in filters (``_filter_stubs.py``): the order in which two wrong
arguments are answered, the order of what is returned, the arguments every ``belief_*`` call is given and the ``record_*``
switches around the run; and the five record summaries (``score_summary``, ``distance_summary``, ``density_summary``,
``modality_summary``, ``mode_summary``) against their definitions written out, bit for bit, on records with NaN and both
infinities scattered in."""
import itertools
import math

import pytest
import torch

from _filter_stubs import _Kalman, _Particles, _Recorded

T, N, D = 5, 2, 3


def _fixed():
    g = torch.Generator().manual_seed(5)
    states = torch.randn((T + 1, N, D), generator=g)
    traj = dict(states=states, image=torch.zeros((T + 1, N, 1)), gripper_pos=torch.zeros((T + 1, N, 1)),
                gripper_sensors=torch.zeros((T + 1, N, 1)), controls=torch.zeros((T + 1, N, 1)))
    est, smoothed = (states[1:] + s * torch.randn((T, N, D), generator=g) for s in (0.3, 0.1))
    A, B = (torch.randn((T, N, D, D), generator=g) for _ in range(2))
    cov, smoothed_cov = (X @ X.transpose(-1, -2) + 0.1 * torch.eye(D) for X in (A, B))
    return traj, (est, cov, smoothed, smoothed_cov)


TRAJ, (EST, COV, SMOOTHED, SMOOTHED_COV) = _fixed()
TRUTH = TRAJ["states"][1:]
KINDS = ("crossmodal", "particles", "kalman", "gaussian", "point")


def _filter(kind, prior=False):
    """``crossmodal``, ``particles`` (one measurement model, no transition moments) and ``kalman`` log their calls;
    ``gaussian`` has ``record_belief`` and nothing else, ``point`` not even that."""
    fixed = (EST, COV, SMOOTHED, SMOOTHED_COV)
    if kind == "crossmodal":
        return _Particles(*fixed, prior=prior)
    if kind == "particles":
        return _Particles(*fixed, prior=prior, crossmodal=False)
    if kind == "kalman":
        return _Kalman(*fixed, prior=prior)
    return _Recorded(EST, COV if kind == "gaussian" else None)


# ------------------------------------------------------------------------------------------ 1. the order of the refusals
_SETS = ("crossmodal", "particles")                     # the kinds whose summaries read a weighted particle set per step
_BELIEF = ("crossmodal", "particles", "kalman", "gaussian")
# single faults in the order in which run_filter answers them: (kinds, keyword arguments, exception, start of the message
# with {name} the filter's type, whether the trajectories are read before it).  An option without its return_* argument
# names that argument's off value, and a fault of the smoothing method names the method, so that no later fault's
# arguments cure it.
_FAULTS = [
    (("crossmodal", "particles", "gaussian", "point"), dict(return_innovations=True), ValueError,
     "run_filter: return_innovations needs a Kalman filter; {name} has no record_innovations", False),
    (KINDS, dict(smooth_transition_moments=True, smooth_method="map"), ValueError,
     "run_filter: smooth_transition_moments are the two-slice moments", False),
    (KINDS, dict(smooth_draws=8), ValueError, "run_filter: smooth_draws is the number of paths", False),
    (KINDS, dict(score_scale=(1.0, 1.0, 1.0), return_scores=False), ValueError, "run_filter: score_scale is the scale of return_scores'", False),
    (KINDS, dict(return_scores=True, score_scale=(1.0, 0.0, 1.0)), ValueError,
     "run_filter: score_scale must be None or d positive finite floats, got", False),
    (_SETS, dict(return_scores=True, smooth_method="map"), ValueError, "run_filter: return_scores reads a weighted particle set", False),
    (KINDS, dict(density_bandwidth="scott", return_density=False), ValueError, "run_filter: density_bandwidth is the bandwidth of", False),
    (("point",), dict(return_density=True), ValueError, "run_filter: return_density needs a belief; {name} returns a point", False),
    (_BELIEF, dict(return_density=True, density_bandwidth=(1.0, 0.0, 1.0)), ValueError,
     "run_filter: density_bandwidth must be 'silverman', 'scott' or d positive finite floats", False),
    (_SETS, dict(return_density=True, smooth_method="map"), ValueError, "run_filter: return_density reads a weighted particle set", False),
    (KINDS, dict(modes_link_radius=2.0, return_modes=None), ValueError, "run_filter: modes_link_radius is the link radius of", False),
    (("point",), dict(return_modes=2), ValueError, "run_filter: return_modes needs a belief; {name} returns a point", False),
    (_BELIEF, dict(return_modes=9), ValueError, "run_filter: return_modes must be None or the number of modes to report, 1 .. 8, got 9", False),
    (_BELIEF, dict(return_modes=2, modes_link_radius=-1.0), ValueError,
     "run_filter: modes_link_radius must be a positive finite float, got -1.0", False),
    (_SETS, dict(return_modes=2, smooth_method="map"), ValueError, "run_filter: return_modes reads a weighted particle set", False),
    (("particles", "kalman", "gaussian", "point"), dict(return_modalities=True), ValueError,
     "run_filter: return_modalities needs a crossmodal particle filter (belief_modalities over a "
     "CrossmodalParticleFilterMeasurementModel); {name} is none: it fuses no modalities", False),
    (("kalman", "gaussian", "point"), dict(return_quantiles=(0.5,)), ValueError,
     "run_filter: return_quantiles needs a particle filter; {name} has no belief_quantiles", False),
    (_SETS, dict(return_quantiles=(0.5,), smooth_method="map"), ValueError, "run_filter: return_quantiles reads a weighted particle set", False),
    # (on a particle filter these two name a smoothing method that leaves weighted sets: with "map" of a fault above, the
    # record they ask for would be refused before that fault's)
    (_SETS, dict(return_scores=True, score_scale=(1.0, 1.0), smooth_method="marginal"), ValueError,
     "run_filter: score_scale must be None or d = 3 positive finite floats, got (1.0, 1.0)", True),
    (("kalman", "gaussian", "point"), dict(return_scores=True, score_scale=(1.0, 1.0)), ValueError,
     "run_filter: score_scale must be None or d = 3 positive finite floats, got (1.0, 1.0)", True),
    (_SETS, dict(return_density=True, density_bandwidth=(1.0, 1.0), smooth_method="marginal"), ValueError,
     "run_filter: density_bandwidth must be 'silverman', 'scott' or d = 3 positive finite floats, got (1.0, 1.0)", True),
    (("kalman", "gaussian"), dict(return_density=True, density_bandwidth=(1.0, 1.0)), ValueError,
     "run_filter: density_bandwidth must be 'silverman', 'scott' or d = 3 positive finite floats, got (1.0, 1.0)", True),
    (("point",), dict(return_belief=True), AssertionError, "{name} keeps no belief to record", True),
    (("gaussian", "point"), dict(smooth_lag=3), AssertionError, "{name} keeps no history to smooth", True),
    (("particles",), dict(smooth_method="marginal", smooth_transition_moments=True), AssertionError,
     "{name} computes no transition moments", True),
]


def _refused(kind, kwargs, error, message, reads_traj):
    from multimodalfilter_amd import evaluation

    f = _filter(kind)
    with pytest.raises(error) as caught:
        evaluation.run_filter(f, TRAJ if reads_traj else {}, **kwargs)
    want = message.format(name=type(f).__name__)
    assert type(caught.value) is error and str(caught.value).startswith(want), (kind, kwargs, str(caught.value), want)


def test_every_fault_alone_is_refused_with_its_message():
    assert {k for kinds, *_ in _FAULTS for k in kinds} == set(KINDS)
    for kinds, kwargs, error, message, reads_traj in _FAULTS:
        for kind in kinds:
            _refused(kind, kwargs, error, message, reads_traj)


def test_of_two_faults_the_earlier_one_is_answered():
    """Every pair on one kind of filter whose arguments do not disagree; the trajectories are ``{}`` wherever the earlier
    fault is to be found before they are read."""
    pairs = 0
    for (i, first), (j, second) in itertools.combinations(enumerate(_FAULTS), 2):
        if any(k in second[1] and second[1][k] != v for k, v in first[1].items()):
            continue
        for kind in set(first[0]) & set(second[0]):
            _refused(kind, {**first[1], **second[1]}, *first[2:])
            pairs += 1
    print(f"{pairs} pairs of {len(_FAULTS)} faults")
    assert pairs >= 200


def test_the_range_of_return_modes_is_checked_before_the_link_radius():
    """(the two faults of the table name different ``return_modes``, so their pair is not in it)"""
    for kind in _BELIEF:
        _refused(kind, dict(return_modes=9, modes_link_radius=-1.0), ValueError, "run_filter: return_modes must be None or", False)


def test_the_fused_kalman_filters_get_their_own_reason():
    import multimodalfilter_amd as mmf

    f = mmf.door_models.DoorCrossmodalKalmanFilter().eval()
    from multimodalfilter_amd import evaluation

    with pytest.raises(ValueError, match="^run_filter: return_modalities needs a crossmodal particle filter.*is none: the Kalman "
                                         "filters fuse their sub-filters per state dimension"):
        evaluation.run_filter(f, {}, return_modalities=True, return_quantiles=(0.5,))


def test_the_parsers_accept_what_float_accepts():
    """``score_scale`` goes through ``float(v)``: a ``bool`` and a numeric string pass, unlike in ``belief_scores``."""
    from multimodalfilter_amd import evaluation

    f = _filter("crossmodal")
    evaluation.run_filter(f, TRAJ, return_scores=True, score_scale=(True, "2", 0.5))
    assert f.called("belief_scores")[0][1]["scale"] == (1.0, 2.0, 0.5)
    evaluation.run_filter(f, TRAJ, return_density=True, density_bandwidth=(True, "2", 0.5))
    assert f.called("belief_density")[0][1]["bandwidth"] == (1.0, 2.0, 0.5)
    for bad in ("abc", 2.0, None, (), (1.0, math.nan, 1.0), (1.0, math.inf, 1.0), (1.0, "x", 1.0)):
        with pytest.raises(ValueError, match="^run_filter: density_bandwidth must be 'silverman', 'scott' or d positive finite floats$"):
            evaluation.run_filter(f, {}, return_density=True, density_bandwidth=bad)
    for bad in ("abc", 2.0, (), (1.0, math.nan, 1.0), (1.0, "x", 1.0)):
        with pytest.raises(ValueError, match="^run_filter: score_scale must be None or d positive finite floats, got"):
            evaluation.run_filter(f, {}, return_scores=True, score_scale=bad)
    for given in ("silverman", "scott"):                       # the default is told apart by identity
        with pytest.raises(ValueError, match="without\\s+return_density"):
            evaluation.run_filter(f, {}, density_bandwidth=given)
    with pytest.raises(ValueError, match="without return_modes"):
        evaluation.run_filter(f, {}, modes_link_radius=3.0)
    with pytest.raises(ValueError, match="smooth_draws"):
        evaluation.run_filter(f, {}, smooth_draws=64)


# ------------------------------------------------------------------------------------------ 2. the happy path
_VALUES = dict(return_belief=True, return_innovations=True, return_scores=True, return_density=True, return_modes=2,
               return_modalities=True, return_quantiles=(0.1, 0.5, 0.9))          # in the order of what is returned
_SUPPORTED = {"crossmodal": ("return_belief", "return_scores", "return_density", "return_modes", "return_modalities", "return_quantiles"),
              "kalman": ("return_belief", "return_innovations", "return_scores", "return_density", "return_modes")}
_BELIEF_CALLS = ("belief_scores", "belief_density", "belief_modes", "belief_modalities", "belief_quantiles")


def _check_run(kind, asked, smooth_method, prior):
    from multimodalfilter_amd import evaluation

    f = _filter(kind, prior)
    before = f.switches()
    assert set(before.values()) == {prior}
    smooths = smooth_method is not None
    kwargs = {k: _VALUES[k] for k in asked}
    if smooths:
        kwargs["smooth_method"] = smooth_method
    out = evaluation.run_filter(f, TRAJ, **kwargs)
    what = (kind, asked, smooth_method, prior)
    est, of = (SMOOTHED, "smoothed") if smooths else (EST, "filtered")
    assert f.switches() == before, what

    # the switches during the run, and put back before anything else is called
    particles = kind == "crossmodal"
    summaries = [k for k in asked if k not in ("return_belief", "return_innovations")]
    during = dict(before)
    if "return_belief" in asked or (not particles and {"return_scores", "return_density"} & set(asked)):
        during["record_belief"] = True
    if smooths or (particles and summaries):
        during["record_history"] = True
    if "return_innovations" in asked:
        during["record_innovations"] = True
    (_, _, seen), = f.called("forward_loop")
    assert seen == during, what
    assert [c[0] for c in f.calls[:2]] == ["initialize_beliefs", "forward_loop"], what
    for name, arguments, seen in f.calls[2:]:
        assert seen == before, (what, name)
    if smooths:
        assert f.calls[2][:2] == ("smooth", dict(lag=None, method=smooth_method)), what
    else:
        assert not f.called("smooth"), what

    # what is returned, in order
    if not asked:
        assert out is est, what
    else:
        assert type(out) is tuple and len(out) == 1 + len(asked) and out[0] is est, what
    got = dict(zip(asked, out[1:])) if asked else {}
    assert list(got) == [k for k in _VALUES if k in asked]
    if "return_belief" in got:
        assert got["return_belief"] is (f.last_smoothed if smooths else f.last_belief) and got["return_belief"] is not None, what
    if "return_innovations" in got:
        assert got["return_innovations"] is f.last_innovations and f.last_innovations is not None, what

    # every belief_* call once, in order, with its arguments; or the closed forms of the Gaussian belief
    want_calls = [n for n, k in zip(_BELIEF_CALLS, list(_VALUES)[2:]) if k in asked] if particles else []
    assert [c[0] for c in f.calls[3 if smooths else 2:]] == want_calls, what
    calls = {name: arguments for name, arguments, _ in f.calls}
    if particles:
        for name, key in zip(_BELIEF_CALLS, list(_VALUES)[2:]):
            if key in asked:
                assert got[key] is getattr(f, "last_" + key[len("return_"):]), (what, key)
        if "return_scores" in asked:
            a = calls["belief_scores"]
            assert torch.equal(a["truth"], TRUTH) and a["of"] == of and a["scale"] is None, what
        if "return_density" in asked:
            a = calls["belief_density"]
            assert torch.equal(a["truth"], TRUTH) and a["of"] == of and a["bandwidth"] is evaluation._DEFAULT_BANDWIDTH, what
        if "return_modes" in asked:
            a = calls["belief_modes"]
            assert a == dict(of=of, max_modes=2, link_radius=3.0) and type(a["max_modes"]) is int and type(a["link_radius"]) is float, what
        if "return_modalities" in asked:
            assert calls["belief_modalities"] == {}, what                      # always of the filtered sets
        if "return_quantiles" in asked:
            a = calls["belief_quantiles"]
            assert a["probs"] == (0.1, 0.5, 0.9) and a["of"] == of and torch.equal(a["truth"], TRUTH), what
    else:
        cov = SMOOTHED_COV if smooths else COV
        if "return_scores" in asked:
            rec = got["return_scores"]
            assert set(vars(rec)) == {"crps", "of", "scale"} and rec.of == of and rec.scale == (1.0, 1.0, 1.0), what
            assert torch.equal(rec.crps, evaluation.gaussian_crps(est, cov, TRUTH)), what
        if "return_density" in asked:
            rec = got["return_density"]
            assert set(vars(rec)) == {"log_score", "entropy", "mode", "of"} and rec.of == of and rec.mode is est, what
            assert torch.equal(rec.log_score, evaluation.gaussian_log_density(est, cov, TRUTH)), what
            assert torch.equal(rec.entropy, evaluation.gaussian_entropy(cov)), what
        if "return_modes" in asked:
            rec = got["return_modes"]
            assert rec.of == of and rec.max_modes == 2 and torch.equal(rec.modes[:, :, 0], est), what
            assert bool(torch.isnan(rec.modes[:, :, 1]).all()) and bool((rec.count == 1).all()), what


@pytest.mark.parametrize("kind", sorted(_SUPPORTED))
def test_every_subset_of_the_records_in_order_with_the_switches_put_back(kind):
    names = _SUPPORTED[kind]
    runs = 0
    for n in range(len(names) + 1):
        for asked in itertools.combinations(names, n):
            for smooth_method in (None, "marginal"):
                _check_run(kind, asked, smooth_method, prior=False)
                runs += 1
    _check_run(kind, names, None, prior=True)
    _check_run(kind, names, "marginal", prior=True)
    assert runs == 2 << len(names)


def test_a_point_estimate_and_a_scale():
    from multimodalfilter_amd import evaluation

    point = _filter("point")
    assert evaluation.run_filter(point, TRAJ) is EST
    out = evaluation.run_filter(point, TRAJ, return_scores=True, score_scale=(2.0, 1.0, 0.5))
    assert type(out) is tuple and len(out) == 2 and out[0] is EST
    e = EST - TRUTH
    assert set(vars(out[1])) == {"crps", "energy", "of", "scale"} and out[1].of == "filtered" and out[1].scale == (2.0, 1.0, 0.5)
    assert torch.equal(out[1].crps, e.abs())
    assert torch.equal(out[1].energy, torch.linalg.vector_norm(e / torch.tensor((2.0, 1.0, 0.5)), dim=-1))


def test_what_counts_as_smoothing():
    """A lag smooths with the filter's default method; a named method other than ``"ancestry"`` is the full smoother; a named
    ``"ancestry"`` without a lag smooths nothing.  ``smooth_draws`` and the transition-moment switch reach ``smooth``."""
    from multimodalfilter_amd import evaluation

    for prior in (False, True):
        f = _filter("crossmodal", prior)
        assert evaluation.run_filter(f, TRAJ, smooth_method="ancestry") is EST and not f.called("smooth")
        (_, _, seen), = f.called("forward_loop")
        assert seen["record_history"] is prior

        f = _filter("crossmodal", prior)
        out = evaluation.run_filter(f, TRAJ, smooth_lag=0, return_belief=True)
        assert out[0] is SMOOTHED and out[1] is f.last_smoothed
        assert f.called("smooth")[0][1] == dict(lag=0, method="ancestry")
        f.default_smooth_method = "rts"
        assert evaluation.run_filter(f, TRAJ, smooth_lag=None) is SMOOTHED and f.called("smooth")[1][1] == dict(lag=None, method="rts")

        f = _filter("crossmodal", prior)
        out = evaluation.run_filter(f, TRAJ, smooth_method="simulation", smooth_draws=8, return_quantiles=(0.5,))
        assert f.called("smooth")[0][1] == dict(lag=None, method="simulation", num_draws=8)
        assert f.called("belief_quantiles")[0][1]["of"] == "smoothed" and out[1] is f.last_quantiles

        f = _filter("crossmodal", prior)
        evaluation.run_filter(f, TRAJ, smooth_method="marginal", smooth_transition_moments=True, return_modalities=True)
        (_, _, seen), = f.called("smooth")
        assert seen == dict(record_belief=prior, record_history=prior, record_transition_moments=True)
        (_, _, seen), = f.called("forward_loop")
        assert seen == dict(record_belief=prior, record_history=True, record_transition_moments=prior)
        assert f.called("belief_modalities")[0][2] == f.switches() == dict.fromkeys(seen, prior)


@pytest.mark.parametrize("fail", ["forward_loop", "smooth"])
def test_the_switches_are_put_back_when_the_run_or_the_smoother_raises(fail):
    from multimodalfilter_amd import evaluation

    for kind in sorted(_SUPPORTED):
        for prior in (False, True):
            f = _filter(kind, prior)
            before = f.switches()
            f.fail = fail
            kwargs = {k: _VALUES[k] for k in _SUPPORTED[kind]}
            if kind == "crossmodal":
                kwargs["smooth_transition_moments"] = True
            with pytest.raises(RuntimeError, match=f"{fail} fails"):
                evaluation.run_filter(f, TRAJ, smooth_method="marginal", **kwargs)
            assert f.switches() == before and set(before.values()) == {prior}, (kind, prior)
            (_, _, seen), = f.called(fail)
            if fail == "forward_loop" or kind == "crossmodal":
                assert True in seen.values()                              # (it was raised with a switch set)
            assert not any(f.called(name) for name in _BELIEF_CALLS)


def test_compare_filters_puts_the_history_switch_back():
    from multimodalfilter_amd import evaluation

    class Comparable(_Particles):
        def belief_distance(self, other, *, of, other_of, scale):
            self._log("belief_distance", other=other, of=of, other_of=other_of, scale=scale)
            self.last_distance = object()

    for method, of in ((None, "filtered"), ("marginal", "smoothed")):
        a, b = (Comparable(EST, COV, SMOOTHED, SMOOTHED_COV) for _ in range(2))
        est = SMOOTHED if method else EST
        got = evaluation.compare_filters(a, b, TRAJ, smooth_method=method)
        assert got[0] is est and got[1] is est and got[2] is a.last_distance
        for f in (a, b):
            assert f.called("forward_loop")[0][2]["record_history"] is True and f.switches()["record_history"] is False
        assert a.called("belief_distance")[0][1:] == (dict(other=b, of=of, other_of=of, scale=None), a.switches())
        b.fail = "forward_loop"
        with pytest.raises(RuntimeError):
            evaluation.compare_filters(a, b, TRAJ, smooth_method=method)
        assert a.record_history is False and b.record_history is False


# ------------------------------------------------------------------------------------------ 3. the summaries, bit for bit
def _scattered(shape, seed, share=0.25):
    """Standard normals with NaN, ``+inf`` and ``-inf`` in about ``share`` of the entries."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    u = torch.rand(shape, generator=g)
    for k, bad in enumerate((math.nan, math.inf, -math.inf)):
        x = torch.where((u >= k * share / 3) & (u < (k + 1) * share / 3), torch.full_like(x, bad), x)
        x.view(-1)[-1 - k] = bad                                   # (each at least once, after either start)
    assert all(bool(m.any()) for m in (torch.isnan(x), x == math.inf, x == -math.inf))
    return x


def _mean_of_the_finite(x, start, tail):
    """The definition every summary names: the steps from ``start``, all leading axes as one, the sum in float64 of the
    finite entries over their number, per entry of the ``tail`` trailing axes -> float64."""
    x = x[start:].to(torch.float64)
    x = x.reshape((-1,) + tuple(x.shape[x.dim() - tail:]))
    finite = torch.isfinite(x)
    total = torch.where(finite, x, torch.zeros_like(x)).sum(dim=0)
    out = total / finite.sum(dim=0)
    assert bool(torch.isfinite(out).all())                       # (every entry has a finite step: no 0 / 0 in these records)
    return out


_STARTS = (0, 2)
_R = (9, 4)                                                     # (T, N) of the records


def test_score_and_distance_summaries_are_the_means_of_the_finite_entries():
    from multimodalfilter_amd import base, evaluation

    crps, energy, spread = _scattered(_R + (D,), 1), _scattered(_R, 2), _scattered(_R + (D + 1,), 3)
    for start in _STARTS:
        got = evaluation.score_summary(base.belief_record(crps=crps, energy=energy, spread=spread), start=start)
        assert set(got) == {"crps", "energy", "spread"} and type(got["energy"]) is float
        assert torch.equal(got["crps"], _mean_of_the_finite(crps, start, 1).to(torch.float32)) and got["crps"].dtype == torch.float32
        assert torch.equal(got["spread"], _mean_of_the_finite(spread, start, 1).to(torch.float32))
        assert got["energy"] == float(_mean_of_the_finite(energy, start, 0).to(torch.float32))       # (rounded through float32)
        assert set(evaluation.score_summary(base.belief_record(crps=crps), start=start)) == {"crps"}
        w, c, ks = (_scattered(_R + (D,), seed) for seed in (4, 5, 6))
        got = evaluation.distance_summary(base.belief_record(wasserstein=w, cramer=c, ks=ks, energy=energy), start=start)
        assert set(got) == {"wasserstein", "cramer", "ks", "energy"} and type(got["energy"]) is float
        for k, x in (("wasserstein", w), ("cramer", c), ("ks", ks)):
            assert torch.equal(got[k], _mean_of_the_finite(x, start, 1).to(torch.float32)) and got[k].dtype == torch.float32, k
        assert got["energy"] == float(_mean_of_the_finite(energy, start, 0).to(torch.float32))


def test_density_summary_is_the_float64_mean_of_the_finite_entries():
    from multimodalfilter_amd import base, evaluation

    log_score, entropy = _scattered(_R, 7), _scattered(_R, 8)
    for start in _STARTS:
        got = evaluation.density_summary(base.belief_record(log_score=log_score, entropy=entropy), start=start)
        want = {"log_score": float(_mean_of_the_finite(log_score, start, 0)), "entropy": float(_mean_of_the_finite(entropy, start, 0))}
        assert got == want                                        # (not rounded through float32)
        assert want["entropy"] != float(torch.tensor(want["entropy"], dtype=torch.float32))
        assert evaluation.density_summary(base.belief_record(entropy=entropy), start=start) == {"entropy": want["entropy"]}


def test_modality_summary_against_its_definition():
    from multimodalfilter_amd import base, evaluation

    K = 3
    rho, le, div = _scattered(_R + (K,), 9, share=0.1), _scattered(_R + (K + 1,), 10), _scattered(_R + (K,), 11)
    overlap, beta = _scattered(_R + (K, K), 12), _scattered(_R + (K,), 13, share=0.15)
    beta = torch.where(beta == math.inf, torch.full_like(beta, -math.inf), beta)  # (softmax of +inf is NaN for the whole row)
    for start in _STARTS:
        rec = base.belief_record(responsibility=rho, log_evidence=le, divergence=div, overlap=overlap, log_weights=beta)
        got = evaluation.modality_summary(rec, start=start)
        assert set(got) == {"responsibility", "dominant", "log_evidence", "divergence", "overlap", "prior"}
        want = {"responsibility": _mean_of_the_finite(rho, start, 1), "log_evidence": _mean_of_the_finite(le, start, 1),
                "divergence": _mean_of_the_finite(div, start, 1), "overlap": _mean_of_the_finite(overlap, start, 2),
                "prior": _mean_of_the_finite(torch.softmax(beta.to(torch.float64), dim=-1), start, 1)}
        rows = [r for r in rho[start:].reshape(-1, K) if bool(torch.isfinite(r).all())]  # the steps with a live particle
        assert 0 < len(rows) < rho[start:].numel() // K
        wins = [sum(1 for r in rows if int(torch.argmax(r)) == k) for k in range(K)]    # (argmax: the lowest index among equals)
        want["dominant"] = torch.tensor([w / len(rows) for w in wins], dtype=torch.float64)
        assert got["overlap"].shape == (K, K) and got["log_evidence"].shape == (K + 1,)
        for k, x in want.items():
            assert got[k].dtype == torch.float32 and torch.equal(got[k], x.to(torch.float32)), (start, k)
        del rec.log_weights
        assert torch.equal(evaluation.modality_summary(rec, start=start)["prior"], torch.full((K,), 1.0 / K))


def test_mode_summary_against_its_definition():
    from multimodalfilter_amd import base, evaluation

    K = 3
    g = torch.Generator().manual_seed(14)
    modes = _scattered(_R + (K, D), 15, share=0.3)
    modes[1, 0] = math.nan                                                          # a step that reports no mode
    count = torch.randint(0, K + 1, _R, generator=g, dtype=torch.int32)
    mass = torch.rand(_R + (K,), generator=g)
    true = torch.randn(_R + (D,), generator=g)
    rec = base.belief_record(modes=modes, mass=mass, count=count)
    for start in _STARTS:
        got = evaluation.mode_summary(rec, true, start=start)
        assert set(got) == {"count", "top_mass", "multimodal", "top_rmse", "best_rmse"} and all(type(v) is float for v in got.values())
        c = count[start:].to(torch.float64).reshape(-1)
        assert got["count"] == float(c.mean()) and got["multimodal"] == float((c > 1).to(torch.float64).mean())
        assert got["top_mass"] == float(mass[start:, :, 0].to(torch.float64).mean())
        err = torch.linalg.vector_norm(modes - true[:, :, None, :], dim=-1)          # (T, N, K): NaN where a mode is not reported
        best = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err).min(dim=-1).values
        best = torch.where(torch.isnan(err).all(dim=-1), torch.full_like(best, math.nan), best)
        assert math.isnan(float(best[1, 0])) and bool((best == math.inf).any())
        for k, e in (("top", err[..., 0]), ("best", best)):
            e = e.to(torch.float64)
            assert got[k + "_rmse"] == float(torch.sqrt(_mean_of_the_finite(e * e, start, 0))), (start, k)   # the root in float64
        assert evaluation.mode_summary(rec, start=start) == {k: got[k] for k in ("count", "top_mass", "multimodal")}
        errors = evaluation.mode_errors(rec, true)
        for k, e in (("top", err[..., 0]), ("best", best)):
            assert torch.equal(torch.nan_to_num(errors[k], nan=-1.0), torch.nan_to_num(e, nan=-1.0)), k


def test_the_truth_of_the_errors_is_checked_with_one_message():
    from multimodalfilter_amd import base, evaluation

    modes, mean = torch.zeros((4, 2, 3, D)), torch.zeros((4, 2, 3, D))
    for who, call in (("mode_errors", lambda t: evaluation.mode_errors(base.belief_record(modes=modes), t)),
                      ("modality_errors", lambda t: evaluation.modality_errors(base.belief_record(mean=mean), t))):
        for bad, got in ((torch.zeros((4, 2)), "(4, 2)"), (torch.zeros((5, 2, D)), "(5, 2, 3)"), (torch.zeros((4, 2, D + 1)), "(4, 2, 4)"),
                         ([[0.0]], "list"), (None, "NoneType")):
            with pytest.raises(ValueError) as caught:
                call(bad)
            assert str(caught.value) == f"{who}: true must be a (T, N, d) = (4, 2, 3) tensor, got {got}"
    for bad in ((1.0, 1.0), (1.0, 0.0, 1.0), "abc", 2.0, (1.0, "x", 1.0)):
        with pytest.raises(ValueError) as caught:
            evaluation.mode_errors(base.belief_record(modes=modes), torch.zeros((4, 2, D)), scale=bad)
        assert str(caught.value) == "mode_errors: scale must be None or d = 3 positive finite floats"
    got = evaluation.mode_errors(base.belief_record(modes=modes + 2.0), torch.zeros((4, 2, D)), scale=(True, "2", 0.5))
    assert torch.allclose(got["top"], torch.full((4, 2), math.sqrt(4.0 + 1.0 + 16.0)), rtol=1e-6, atol=0)   # (2 / 1, 2 / 2, 2 / 0.5)

"""CPU-side checks of the k-step-ahead forecasts (``include/mmf.h``: ``MmfPfPredictiveArgs`` / ``mmf_pf_predictive``;
``ParticleFilter.belief_forecast`` / ``VirtualSensorExtendedKalmanFilter.belief_forecast``; ``evaluation.forecast_filter`` /
``forecast_summary``): the family of ``_forecast_cases`` is certified against the fp32 formulation, the fp64 reference obeys
the identities of a Gaussian mixture, and the entry point's and the Python layers' refusals are reached on the host before
any HIP call or device work."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import _filter_stubs as stubs
import _forecast_cases as fk
import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("centres", "log_a", "log_b", "scale_tril", "truth")
_OUTPUTS = fk.OUTPUTS
_POINTERS = _INPUTS + _OUTPUTS + ("workspace",)


@pytest.fixture(autouse=True, scope="module")
def _the_entry_these_tests_describe():
    """The family and the reference of this module define ONE entry point: without the binding, the methods and the
    evaluation functions there is nothing they are the reference of."""
    from multimodalfilter_amd import _abi, evaluation, filters

    assert hasattr(_abi, "MmfPfPredictiveArgs") and callable(getattr(_abi, "pf_predictive", None))
    assert callable(getattr(_abi, "pf_predictive_workspace_bytes", None))
    assert callable(getattr(filters.ParticleFilter, "belief_forecast", None))
    assert callable(getattr(filters.VirtualSensorExtendedKalmanFilter, "belief_forecast", None))
    assert callable(getattr(evaluation, "forecast_filter", None)) and callable(getattr(evaluation, "forecast_summary", None))


# ------------------------------------------------------------------------------------------ 1. the family is certified
@pytest.mark.parametrize("M", fk.ALL_MS)
def test_the_fp32_formulation_is_within_the_cap_on_the_family(M):
    """A condition on the INPUTS: where fp32 torch ops cannot hold ``CAP = REL_TOL / 3`` against fp64, the kernel could not
    be asked for ``REL_TOL`` either.  Every case is held to it, none is skipped."""
    worst, cases = {}, 0
    for M_, d, R, variant, scale in fk.family():
        if M_ != M:
            continue
        case, ref = fk.family_case(M, d, R, variant, scale)
        got = fk.torch_formulation(case)
        what = f"M={M} d={d} R={R} {variant} scale={scale}"
        for name in fk.OUTPUTS:
            if ref[name] is None:
                assert got[name] is None and case["truth"] is None and name in fk.NEED_TRUTH
                continue
            e = fk.compare(got[name].numpy(), ref[name], name, what)
            assert e < fk.CAP, (what, name, e)
            worst[name] = max(worst.get(name, 0.0), e)
        cases += 1
    assert cases >= 1
    print(f"M={M}: {cases} cases, worst fp32 formulation against fp64 " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items())
          + f" (cap {fk.CAP:.0e})")


def test_the_family_covers_what_the_definition_distinguishes():
    seen = set(fk.family())
    assert {m for m, *_ in seen} == set(fk.ALL_MS) and len([1 for m, *_ in seen if m == fk.BIG_M]) == 1
    for edge in (fk.I_BLOCK, fk.J_TILE):
        assert {edge - 1, edge, edge + 1} <= set(fk.MS)
    for M in fk.MS:
        assert {v for m, _, _, v, _ in seen if m == M} == set(fk.VARIANTS + fk.SPECIALS)
        assert {d for m, d, _, v, _ in seen if m == M and v == "plain"} == set(fk.DIMS)
        if M <= fk.SMALL:
            assert {(d, R, v, s) for m, d, R, v, s in seen if m == M} >= {
                (d, R, v, s) for d in fk.DIMS for R in fk.RS for v in fk.VARIANTS for s in fk.SCALES}
        else:
            assert {s for m, _, _, _, s in seen if m == M} == set(fk.SCALES)
    for scale in fk.SCALES:
        L = fk.scale_tril(4, scale)
        assert np.array_equal(L, np.tril(L)) and (np.tril(L, -1) != 0).sum() == 6 and (np.diag(L) > 0).all()  # full, not diagonal
    # NaN exactly where the definition puts it
    case, ref = fk.family_case(65, 3, 3, "dead_row", 0.3)
    for name in fk.OUTPUTS:
        assert np.isnan(ref[name][1]).all() and np.isfinite(np.delete(ref[name], 1, 0)).all(), name
    case, ref = fk.family_case(65, 3, 3, "nan_truth", 0.3)
    k = int(np.flatnonzero(np.isnan(case["truth"][1]))[0])
    assert np.isnan(ref["log_score"][1]) and np.isfinite(np.delete(ref["log_score"], 1)).all()
    for name in ("crps", "pit"):
        assert np.isnan(ref[name][1, k]) and np.isfinite(np.delete(ref[name][1], k)).all() and np.isfinite(ref[name][[0, 2]]).all()
    for name in ("mean", "covariance", "spread"):
        assert np.isfinite(ref[name]).all()
    case, ref = fk.family_case(65, 3, 3, "no_truth", 0.3)
    assert all(ref[name] is None for name in fk.NEED_TRUTH) and np.isfinite(ref["spread"]).all()
    for variant in ("plain", "dead_particles"):
        case, _ = fk.family_case(65, 3, 3, variant, 0.3)
        assert np.isnan(case["states"]).any() and np.isinf(case["log_b"]).any()  # dead particles carry NaN rows
    case, _ = fk.family_case(2, 3, 3, "dead_particles", 0.3)
    assert np.isnan(case["states"][:, 1]).all() and np.isfinite(case["states"][:, 0]).all()


# ------------------------------------------------------------------------------------------ 2. identities of the reference
def _gaussian(mean, cov, truth):
    from multimodalfilter_amd import evaluation

    m, c, y = (torch.from_numpy(np.array(a, np.float64)) for a in (mean, cov, truth))
    return evaluation.gaussian_crps(m, c, y).numpy(), evaluation.gaussian_log_density(m, c, y).numpy()


@pytest.mark.parametrize("scale", fk.SCALES)
def test_one_component_is_the_gaussian_closed_form(scale):
    for d in fk.DIMS:
        for variant in ("plain", "uniform", "far_truth"):
            case, ref = fk.family_case(1, d, 3, variant, scale)
            L = case["scale_tril"].astype(np.float64)
            Q = np.broadcast_to(L @ L.T, (3, d, d))
            centre = case["states"][:, 0, :].astype(np.float64)
            crps, log_density = _gaussian(centre, Q, case["truth"])
            assert np.allclose(ref["mean"], centre, rtol=1e-15, atol=0) and np.allclose(ref["covariance"], Q, rtol=1e-14, atol=0)
            assert np.allclose(ref["crps"], crps, rtol=1e-9, atol=1e-13 * scale)
            assert np.allclose(ref["log_score"], log_density, rtol=1e-11, atol=1e-11)
            assert np.allclose(ref["spread"], 2.0 * np.sqrt(np.diag(Q[0])) / math.sqrt(math.pi), rtol=1e-14, atol=0)


@pytest.mark.parametrize("M", [2, 65, 257])
def test_equal_centres_are_the_single_gaussian_and_the_scores_are_in_range(M):
    for d in fk.DIMS:
        for scale in fk.SCALES:
            case, ref = fk.family_case(M, d, 3, "equal_centres", scale)
            L = case["scale_tril"].astype(np.float64)
            Q = np.broadcast_to(L @ L.T, (3, d, d))
            live = ~np.isnan(case["states"][:, :, 0])
            centre = np.stack([case["states"][r][live[r]][0] for r in range(3)]).astype(np.float64)
            crps, log_density = _gaussian(centre, Q, case["truth"])
            assert np.allclose(ref["mean"], centre, rtol=1e-14, atol=0)
            assert np.allclose(ref["covariance"], Q, rtol=1e-12, atol=1e-30)
            assert np.allclose(ref["crps"], crps, rtol=1e-8, atol=1e-12 * scale)
            assert np.allclose(ref["log_score"], log_density, rtol=1e-10, atol=1e-10)
            for variant in ("plain", "uniform", "only_a", "dead_particles", "far_truth"):
                case, ref = fk.family_case(M, d, 3, variant, scale)
                assert bool((ref["crps"] >= 0).all()) and bool((ref["spread"] > 0).all())
                assert bool(((ref["pit"] >= 0) & (ref["pit"] <= 1 + 1e-14)).all())  # (the weights sum to 1 to a few ulps)
                assert np.isfinite(ref["log_score"]).all()  # (50 sigma away included)
                # every component twice with half its weight: the same mixture, the same figures
                W = np.concatenate([fk.sm.weights64(case)] * 2, axis=1) * 0.5
                twice = fk.reference_rows(np.concatenate([case["states"]] * 2, axis=1), W, case["scale_tril"], case["truth"])
                for name in fk.OUTPUTS:
                    assert np.allclose(twice[name], ref[name], rtol=1e-9, atol=1e-13), (name, variant)


def test_spread_against_a_quadrature_of_the_mixture_cdf():
    """An independent route to the CRPS in one dimension: ``int (F(x) - 1[x >= y])^2 dx`` of the mixture's CDF."""
    case, ref = fk.family_case(63, 1, 3, "plain", 0.3)
    sigma = float(abs(case["scale_tril"][0, 0]))
    W = fk.sm.weights64(case)
    for r in range(3):
        live = W[r] > 0
        x, w, y = case["states"][r, live, 0].astype(np.float64), W[r][live] / W[r][live].sum(), float(case["truth"][r, 0])
        lo, hi = min(x.min() - 10 * sigma, y) - 1e-9, max(x.max() + 10 * sigma, y) + 1e-9
        cdf = lambda g: fk.normal_cdf((g[:, None] - x[None, :]) / sigma) @ w
        left, right = np.linspace(lo, y, 200001), np.linspace(y, hi, 200001)
        trapezoid = lambda f, g: float((0.5 * (f[1:] + f[:-1]) * np.diff(g)).sum())
        want = trapezoid(cdf(left) ** 2, left) + trapezoid((cdf(right) - 1.0) ** 2, right)
        assert abs(ref["crps"][r, 0] - want) <= 1e-7 * max(1.0, want), (r, ref["crps"][r, 0], want)


# ------------------------------------------------------------------------------------------ 3. the entry point's host checks
def _args(alias=None, **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfPredictiveArgs, _POINTERS, **{**dict(R=2, M=2, d=2, workspace_bytes=64), **over})
    return sc.alias_host_args(a, _POINTERS, alias)


def test_the_header_the_binding_and_the_struct_agree():
    from multimodalfilter_amd import _abi

    fields = [name for name, _ in _abi.MmfPfPredictiveArgs._fields_]
    assert fields == ["R", "M", "d", *_POINTERS, "workspace_bytes"]
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mmf.h")).read()
    body = text[text.index("typedef struct MmfPfPredictiveArgs"):text.index("} MmfPfPredictiveArgs;")]
    assert re.findall(r"(\w+)\s*[;,]", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == fields  # the same fields in the same order
    assert "int mmf_pf_predictive(const MmfPfPredictiveArgs* args" in text and "size_t mmf_pf_predictive_workspace_bytes(int R, int M, int d);" in text
    section = text[text.rfind("/* ----", 0, text.index("typedef struct MmfPfPredictiveArgs")):text.index("typedef struct MmfPfPredictiveArgs")]
    assert "torchfilter" in section and "ABI 42" in section
    res, args = _abi.SIGNATURES["mmf_pf_predictive"]
    assert res is ctypes.c_int and args[0]._type_ is _abi.MmfPfPredictiveArgs and args[1] is ctypes.c_void_p
    assert _abi.SIGNATURES["mmf_pf_predictive_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int] * 3)
    assert _abi.ABI_VERSION == 42 and _abi.PREDICTIVE_MAX_M == 16384 == fk.MAX_M


def test_predictive_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == 42
    call = lambda alias=None, **over: lib.mmf_pf_predictive(ctypes.byref(_args(alias, **over)), None)
    assert lib.mmf_pf_predictive(None, None) == EINVAL
    assert lib.mmf_pf_predictive(ctypes.byref(_abi.MmfPfPredictiveArgs()), None) == EINVAL  # all zero
    assert call(centres=None) == EINVAL and call(scale_tril=None) == EINVAL
    assert call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(M=0) == EINVAL and call(M=-2) == EINVAL and call(R=-1) == EINVAL
    assert call(**{k: None for k in _OUTPUTS}) == EINVAL                                    # nothing requested
    for name in fk.NEED_TRUTH:                                                              # a score without a truth
        assert call(truth=None, **{k: None for k in fk.NEED_TRUTH if k != name}) == EINVAL, name
    for out in _OUTPUTS:
        for target in _INPUTS + tuple(o for o in _OUTPUTS if o != out):
            assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"mean": ("centres", 28)}) == EINVAL and call({"crps": ("spread", 4)}) == EINVAL  # partly on top
    assert call({"covariance": ("scale_tril", 12)}) == EINVAL
    assert call(M=16385) == ETOOLARGE and call(M=1 << 20) == ETOOLARGE
    assert call(M=16385, centres=None) == EINVAL                     # an invalid call is invalid whatever its size
    assert call(R=1 << 27, M=16384) == ETOOLARGE                     # R * workgroups per row beyond a 32-bit grid
    W = _abi.pf_predictive_workspace_bytes
    assert (W(0, 513, 2), W(1, 513, 2), W(1, 512, 2), W(3, 16384, 4)) == (0, 2 * 9 * 8, 0, 3 * 32 * 9 * 8)
    assert W(1, 513, 0) == 0 and W(1, 0, 2) == 0
    # successful no-ops: no rows (the arrays are empty, so nothing is needed and nothing overlaps)
    assert call(R=0) == 0 and call(R=0, M=16384, d=4) == 0 and call(R=0, M=16385) == ETOOLARGE
    assert call(R=0, log_a=None, log_b=None) == 0 and call(R=0, truth=None, log_score=None, pit=None, crps=None) == 0
    assert call(R=0, workspace=None, workspace_bytes=0, M=4096) == 0
    assert call({"crps": ("centres", 0)}, R=0) == 0


def test_predictive_workspace_refusals_on_the_host():
    """With ``M > 512`` the arrays no longer fit the 16-float host buffers, but every check below is decided on pointer
    values alone, before any HIP call.  The workspace is the pair pass's: without ``spread`` and ``crps`` none is asked for."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    R, M, d = 1, 513, 1
    need = _abi.pf_predictive_workspace_bytes(R, M, d)
    big = [(ctypes.c_float * (R * M * (d + 1) + 64))() for _ in _POINTERS]

    def call(**over):
        a = _abi.MmfPfPredictiveArgs()
        for name, b in zip(_POINTERS, big):
            setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
        a.R, a.M, a.d, a.workspace_bytes = R, M, d, need
        for k, v in over.items():
            setattr(a, k, v)
        a._keep = big
        return lib.mmf_pf_predictive(ctypes.byref(a), None)

    base = ctypes.addressof(big[_POINTERS.index("workspace")])
    assert need == 2 * 9 * 8
    assert call(workspace=None) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    assert call(workspace=ctypes.c_void_p(base + 4)) == EINVAL       # not 8-byte aligned
    for target in _INPUTS + _OUTPUTS:
        assert call(workspace=ctypes.cast(big[_POINTERS.index(target)], ctypes.c_void_p)) == EINVAL, target
    assert call(R=0) == 0 and call(R=0, workspace=None, workspace_bytes=0, spread=None, crps=None) == 0


def test_the_binding_refuses_cpu_tensors():
    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_predictive(x, None, None, torch.eye(3), torch.zeros((2, 3)), mean=torch.zeros((2, 3)), crps=torch.zeros((2, 3)))
    with pytest.raises(AssertionError):
        _abi.pf_predictive(x, None, None, torch.eye(2), None, mean=torch.zeros((2, 3)))


# ------------------------------------------------------------------------------------------ 4. the Python refusals
class _CountingNoise:
    """Counts the draws a filter asks for; serves none."""

    def __init__(self):
        self.gaussians, self.uniforms = [], []

    def gaussian(self, shape, *, like):
        self.gaussians.append(tuple(shape))
        return torch.zeros(tuple(shape))

    def uniform(self, shape, *, like):
        self.uniforms.append(tuple(shape))
        return torch.zeros(tuple(shape))


def test_belief_forecast_refusals_come_before_any_device_work():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_forecast is None
    with pytest.raises(ValueError, match="^belief_forecast needs a history: set record_history and run forward_loop"):
        pf.belief_forecast(3)
    with pytest.raises(TypeError):
        pf.belief_forecast()  # the horizon is required
    sig = inspect.signature(pf.belief_forecast).parameters
    assert list(sig) == ["horizon", "truth", "crps"] and sig["truth"].default is None
    assert sig["crps"].kind is inspect.Parameter.KEYWORD_ONLY and sig["crps"].default is True

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    f.noise = _CountingNoise()
    truth = torch.zeros((T, N, d))
    before = (f.last_history, f.last_smoothed, f.last_scores)
    for bad in (0, -1, 1.0, 2.5, "3", None, True, (2,)):
        with pytest.raises(ValueError, match="belief_forecast: horizon must be an int >= 1"):
            f.belief_forecast(bad, truth)
    for bad in (torch.zeros((T, N)), torch.zeros((T + 1, N, d)), torch.zeros((T, N, d + 1)), np.zeros((T, N, d))):
        with pytest.raises(ValueError, match="belief_forecast: truth must be None or a"):
            f.belief_forecast(2, bad)
    f.train()
    with pytest.raises(RuntimeError, match="belief_forecast: the training"):
        f.belief_forecast(2, truth)
    f.eval()
    big = base.history_record(states=torch.zeros((1, 1, fk.MAX_M + 1, 1)), log_likelihoods=torch.zeros((1, 1, fk.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="belief_forecast: 16385 particles per set; mmf_pf_predictive serves at most 16384"):
        f.belief_forecast(1)
    f.last_history = before[0]
    assert f.last_forecast is None and (f.last_history, f.last_smoothed, f.last_scores) == before
    assert f.noise.gaussians == [] and f.noise.uniforms == []
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    with pytest.raises(_abi.MmfError):
        f.belief_forecast(2, truth)
    assert f.last_forecast is None and f.noise.gaussians == []  # (lead 1 draws nothing, and lead 1 is where it stopped)
    # state-dependent process noise is refused as the smoothers refuse it
    dyn, meas = sc.linear_gaussian_models(d, 0.05, 0.3, torch.device("cpu"), state_dependent=True)
    g = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M).eval()
    g.last_history = f.last_history
    with pytest.raises(ValueError, match="^belief_forecast needs one process-noise scale_tril"):
        g.belief_forecast(2)
    # one recorded step: every lead is beyond the data, nothing is launched and nothing is drawn
    one = sc.cpu_filter_with_history(T=1).f
    one.noise = _CountingNoise()
    mean = one.belief_forecast(3, torch.zeros((1, N, d)))
    rec = one.last_forecast
    assert mean is rec.mean and mean.shape == (3, 1, N, d) and bool(torch.isnan(mean).all()) and rec.horizon == 3
    assert set(vars(rec)) == {"mean", "covariance", "spread", "error", "log_score", "pit", "crps", "horizon"}
    assert rec.covariance.shape == (3, 1, N, d, d) and rec.log_score.shape == (3, 1, N) and one.noise.gaussians == []
    one.belief_forecast(2, crps=False)
    assert set(vars(one.last_forecast)) == {"mean", "covariance", "horizon"}


def test_the_kalman_filters_answer_as_the_issue_says():
    """The extended filters have the method and ask for a history; the unscented filter inherits it and, keeping no history,
    answers the same; the fused Kalman filters and the LSTM baselines have no such method."""
    import multimodalfilter_amd as mmf

    extended = 0
    for name, cls in mmf.model_types("door").items():
        f = cls().eval()
        if isinstance(f, mmf.filters.VirtualSensorExtendedKalmanFilter):
            extended += 1
            assert f.last_forecast is None
            with pytest.raises(ValueError, match="^belief_forecast needs a history"):
                f.belief_forecast(2)
            with pytest.raises(ValueError, match="horizon must be an int >= 1"):
                f.belief_forecast(0)
        elif not isinstance(f, mmf.filters.ParticleFilter):
            assert not hasattr(f, "belief_forecast"), name
    assert extended >= 1
    ukf = mmf.filters.VirtualSensorUnscentedKalmanFilter
    assert ukf.belief_forecast is mmf.filters.VirtualSensorExtendedKalmanFilter.belief_forecast
    assert list(inspect.signature(ukf.belief_forecast).parameters) == ["self", "horizon", "truth"]


def _traj(T, N, d, g):
    states = torch.randn((T + 1, N, d), generator=g)
    return dict(states=states, image=torch.zeros((T + 1, N, 1)), gripper_pos=torch.zeros((T + 1, N, 1)),
                gripper_sensors=torch.zeros((T + 1, N, 1)), controls=torch.zeros((T + 1, N, 1)))


class _Forecasting(stubs._Particles):
    """... with ``belief_forecast`` as well."""

    last_forecast = None

    def belief_forecast(self, horizon, truth=None, *, crps=True):
        self._log("belief_forecast", horizon=horizon, truth=truth, crps=crps)
        self.last_forecast = object()


def test_forecast_filter_refuses_before_the_run_and_puts_the_switch_back():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    g = torch.Generator().manual_seed(3)
    T, N, d = 5, 2, 3
    traj = _traj(T, N, d, g)
    est = traj["states"][1:] + 0.1
    cov = torch.eye(d).expand(T, N, d, d)
    sig = inspect.signature(evaluation.forecast_filter).parameters
    assert list(sig) == ["filter_model", "traj", "horizon", "crps", "initial_cov_scale", "measurement_initialize"]
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("crps", "initial_cov_scale", "measurement_initialize"))
    assert (sig["crps"].default, sig["initial_cov_scale"].default, sig["measurement_initialize"].default) == (True, 0.1, False)
    # refused before the run: the stand-ins log every call, and the trajectories ({}) are never read
    kalman = stubs._Kalman(est, cov, est, cov)                 # record_belief and record_history, no belief_forecast
    point = stubs._Recorded(est)                               # a point estimator like the LSTM baselines
    with pytest.raises(ValueError, match="forecast_filter: _Kalman keeps no history to forecast from"):
        evaluation.forecast_filter(kalman, {}, 3)
    with pytest.raises(ValueError, match="forecast_filter: _Recorded has no belief to roll out"):
        evaluation.forecast_filter(point, {}, 3)
    assert kalman.calls == []
    refused = 0
    for name, cls in mmf.model_types("door").items():
        f = cls().eval()
        extended = isinstance(f, mmf.filters.VirtualSensorExtendedKalmanFilter)
        if isinstance(f, mmf.filters.ParticleFilter) or (extended and not isinstance(f, mmf.filters.VirtualSensorUnscentedKalmanFilter)):
            continue
        with pytest.raises(ValueError, match="forecast_filter: .* (keeps no history to forecast from|has no belief to roll out)"):
            evaluation.forecast_filter(f, {}, 3)  # (before the run: the trajectories are never read)
        refused += 1
    assert refused >= 2  # the fused Kalman filters and the LSTM baselines
    f = _Forecasting(est, cov, est, cov)
    for bad in (0, 2.0, True, None):
        with pytest.raises(ValueError, match="forecast_filter: horizon must be an int >= 1"):
            evaluation.forecast_filter(f, {}, bad)
    assert f.calls == []
    # the run: record_history set for the loop and put back, also when the loop fails
    out, rec = evaluation.forecast_filter(f, traj, 3, crps=False)
    assert out is est and rec is f.last_forecast and f.record_history is False
    (_, _, during), = f.called("forward_loop")
    assert during["record_history"] is True and during["record_belief"] is False
    (_, arguments, after), = f.called("belief_forecast")
    assert arguments["horizon"] == 3 and arguments["crps"] is False and torch.equal(arguments["truth"], traj["states"][1:])
    assert after["record_history"] is False
    f = _Forecasting(est, cov, est, cov, prior=True)
    f.fail = "forward_loop"
    with pytest.raises(RuntimeError, match="forward_loop fails"):
        evaluation.forecast_filter(f, traj, 3)
    assert f.record_history is True and f.called("belief_forecast") == []  # (put back to what it held)


def test_run_filter_is_untouched():
    from multimodalfilter_amd import evaluation

    assert list(inspect.signature(evaluation.run_filter).parameters) == [
        "filter_model", "traj", "initial_cov_scale", "measurement_initialize", "return_belief", "smooth_lag", "smooth_method",
        "smooth_draws", "smooth_transition_moments", "return_innovations", "return_density", "density_bandwidth", "return_modes",
        "modes_link_radius", "return_modalities", "return_quantiles", "return_scores", "score_scale"]


def test_forecast_summary_against_hand_computed_values():
    from multimodalfilter_amd import base, evaluation

    nan = math.nan
    H, T, N, d = 2, 3, 1, 2
    error = torch.tensor([[[[1.0, 2.0]], [[3.0, 0.0]], [[nan, nan]]],
                          [[[2.0, 2.0]], [[nan, nan]], [[nan, nan]]]])
    crps = torch.tensor([[[[0.5, 1.0]], [[1.5, nan]], [[nan, nan]]],
                         [[[4.0, 6.0]], [[nan, nan]], [[nan, nan]]]])
    log_score = torch.tensor([[[-1.0], [-3.0], [nan]], [[-5.0], [nan], [nan]]])
    pit = torch.tensor([[[[0.2, 0.4]], [[0.6, 0.8]], [[nan, nan]]], [[[0.1, 0.9]], [[nan, nan]], [[nan, nan]]]])
    assert error.shape == (H, T, N, d) and log_score.shape == (H, T, N)
    rec = base.belief_record(mean=error, covariance=None, error=error, crps=crps, log_score=log_score, pit=pit, horizon=H)
    got = evaluation.forecast_summary(rec, start=0)
    assert set(got) == {"rmse", "crps", "log_score", "pit_mean", "count"}
    assert torch.allclose(got["rmse"], torch.tensor([[math.sqrt(5.0), math.sqrt(2.0)], [2.0, 2.0]]))
    assert torch.equal(got["crps"], torch.tensor([[1.0, 1.0], [4.0, 6.0]]))  # (a NaN entry is left out of its own mean)
    assert torch.equal(got["log_score"], torch.tensor([-2.0, -5.0])) and got["log_score"].shape == (H,)
    assert torch.allclose(got["pit_mean"], torch.tensor([[0.4, 0.6], [0.1, 0.9]]))
    assert got["count"].tolist() == [2, 1]
    got = evaluation.forecast_summary(rec, start=1)
    assert got["count"].tolist() == [1, 0] and torch.allclose(got["rmse"][0], torch.tensor([3.0, 0.0]))
    assert bool(torch.isnan(got["rmse"][1]).all()) and bool(torch.isnan(got["log_score"][1]))
    got = evaluation.forecast_summary(base.belief_record(mean=error, error=error, horizon=H), start=0)
    assert set(got) == {"rmse", "count"}
    assert inspect.signature(evaluation.forecast_summary).parameters["start"].default == evaluation.START_TRUNCATION
    for bad in (base.belief_record(crps=crps), base.belief_record(mean=error, covariance=None, horizon=H),
                base.belief_record(error=error)):
        with pytest.raises(ValueError, match="forecast_summary: the record is no forecast record"):
            evaluation.forecast_summary(bad)

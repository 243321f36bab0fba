"""Evaluation harness: the role of ``/root/reference/crossmodal/eval_helpers.py:70-217`` on
device-resident ``(T, N, ...)`` batches, plus the multi-GPU reduction of its error statistic.
"""
import contextlib
import math
import numbers
from collections import namedtuple
from typing import Dict

import numpy as np
import torch

from . import base, base_models, filters, pf_summaries
from .base_models import CrossmodalParticleFilterMeasurementModel
from .pf_smoothing import _DEFAULT_DRAWS
from .task_models import DOOR, PUSH

START_TRUNCATION = 30


class _DefaultMethod(str):
    """The default of ``run_filter(smooth_method=)``: ``"ancestry"``, told apart by identity from an ``"ancestry"`` the
    caller passed, since a filter may name another default (``default_smooth_method``)."""


_DEFAULT_METHOD = _DefaultMethod("ancestry")
_DEFAULT_BANDWIDTH = _DefaultMethod("silverman")  # likewise the default of ``run_filter(density_bandwidth=)``


class _DefaultRadius(float):
    """The default of ``run_filter(modes_link_radius=)``, told apart by identity from a ``3.0`` the caller passed."""


_DEFAULT_RADIUS = _DefaultRadius(3.0)

# what a filter without the switch is told (an AssertionError: the caller asked the wrong kind of filter)
_WITHOUT_SWITCH = {"record_belief": "keeps no belief to record", "record_history": "keeps no history to smooth",
                   "record_transition_moments": "computes no transition moments"}


@contextlib.contextmanager
def _switched(filter_model, name):
    """Runs its body with the filter's ``record_*`` switch ``name`` set and puts back what it held, on every path."""
    assert hasattr(filter_model, name), f"{type(filter_model).__name__} {_WITHOUT_SWITCH.get(name, 'has no ' + name)}"
    was = getattr(filter_model, name)
    setattr(filter_model, name, True)
    try:
        yield
    finally:
        setattr(filter_model, name, was)


def _floats(values):
    """``values`` as a tuple of floats, or ``None`` where it is no sequence of what ``float()`` takes.  That is more than
    ``ParticleFilter._positive_floats`` takes -- a ``bool``, a numeric string -- and every caller keeps its own message."""
    try:
        return tuple(float(v) for v in values)
    except (TypeError, ValueError):
        return None


def _positive(values) -> bool:
    return bool(values) and all(0.0 < v < math.inf for v in values)


# ---- the records run_filter appends: one description each (_Record), in the order in which they are checked and returned
_Record = namedtuple("_Record", "argument asked kind weighted switch make option default unused check sized",
                     defaults=(None,) * 5)
_Record.__doc__ = """``argument``: the ``return_*`` argument that asks for the record, and ``asked(value)``: whether it does.
``option``: its companion argument, ``default`` that argument's default, compared by identity, and ``unused``: what a caller
who passes the option without the argument is told (``None``: no option).  ``kind(filter_model)``: ``"particles"``,
``"gaussian"`` or ``"point"``, or the ``ValueError`` of a filter that cannot give the record.  ``check(value, option)``: the
value checks that need no trajectory; returns the option as the record is made with.  ``sized``: the message of an option
that is a tuple of another length than the state dimension (``None``: no such option).  ``weighted``: the particle kind reads
a weighted set per step -- the smoothed sets when the call smooths, which only ``"marginal"`` and ``"simulation"`` leave.
``switch``: per kind, the ``record_*`` switch the run needs.  ``make(kind, run, value, option)``: the record, after the run."""
_Run = namedtuple("_Run", "filter est truth of smoothed")  # what make() reads: est and of are the smoother's where smoothed


def _belief_of(run):
    """The belief record that goes with the returned means: the smoothed one when the call smooths."""
    return run.filter.last_smoothed if run.smoothed else run.filter.last_belief


def _is_given(value) -> bool:
    return value is not None


def _belief_kind(what, point=None):
    """A particle filter has ``belief_<what>``, a Kalman filter ``record_belief``; a filter with neither (an LSTM baseline) is
    the kind ``point``, or refused."""
    def kind(filter_model):
        if hasattr(filter_model, "belief_" + what):
            return "particles"
        if hasattr(filter_model, "record_belief"):
            return "gaussian"
        if point is None:
            raise ValueError(f"run_filter: return_{what} needs a belief; {type(filter_model).__name__} returns a point "
                             f"estimate, which has no {what} (no belief_{what}, no record_belief)")
        return point
    return kind


def _innovations_kind(filter_model):
    if not hasattr(filter_model, "record_innovations"):
        raise ValueError(f"run_filter: return_innovations needs a Kalman filter; {type(filter_model).__name__} has no "
                         "record_innovations (a particle filter reports log_evidence through return_belief)")
    return "gaussian"


def _modalities_kind(filter_model):
    if not (hasattr(filter_model, "belief_modalities")
            and isinstance(getattr(filter_model, "measurement_model", None), CrossmodalParticleFilterMeasurementModel)):
        what = ("the Kalman filters fuse their sub-filters per state dimension, and the attribution of that fusion is a "
                "separate change"
                if isinstance(filter_model, (base_models._FusedKalmanFilters, filters.VirtualSensorExtendedKalmanFilter))
                else "it fuses no modalities")
        raise ValueError(f"run_filter: return_modalities needs a crossmodal particle filter (belief_modalities over a "
                         f"CrossmodalParticleFilterMeasurementModel); {type(filter_model).__name__} is none: {what}")
    return "particles"


def _quantiles_kind(filter_model):
    if not hasattr(filter_model, "belief_quantiles"):
        raise ValueError(f"run_filter: return_quantiles needs a particle filter; {type(filter_model).__name__} has no "
                         "belief_quantiles (a Gaussian belief's quantiles are closed form: mean and covariance)")
    return "particles"


def _check_score_scale(value, scale):
    if scale is None:
        return None
    floats = _floats(scale)
    if not _positive(floats):
        raise ValueError(f"run_filter: score_scale must be None or d positive finite floats, got {scale if floats is None else floats!r}")
    return floats


def _check_density_bandwidth(value, bandwidth):
    if isinstance(bandwidth, str) and bandwidth in ("silverman", "scott"):
        return bandwidth
    floats = _floats("" if isinstance(bandwidth, str) else bandwidth)
    if not _positive(floats):
        raise ValueError("run_filter: density_bandwidth must be 'silverman', 'scott' or d positive finite floats")
    return floats


def _check_modes(count, radius):
    if isinstance(count, bool) or not isinstance(count, numbers.Integral) or not 1 <= count <= 8:
        raise ValueError(f"run_filter: return_modes must be None or the number of modes to report, 1 .. 8, got {count!r}")
    if isinstance(radius, bool) or not isinstance(radius, numbers.Real) or not 0.0 < float(radius) < math.inf:
        raise ValueError(f"run_filter: modes_link_radius must be a positive finite float, got {radius!r}")
    return float(radius)


def _make_innovations(kind, run, value, option):
    return run.filter.last_innovations


def _make_scores(kind, run, value, scale):
    if kind == "particles":
        run.filter.belief_scores(run.truth, of=run.of, scale=scale)
        return run.filter.last_scores
    s = (1.0,) * run.truth.shape[-1] if scale is None else scale
    with torch.no_grad():
        if kind == "gaussian":
            return base.belief_record(crps=gaussian_crps(run.est, _belief_of(run).covariance, run.truth), of=run.of, scale=s)
        e = run.est - run.truth  # a point mass
        energy = torch.linalg.vector_norm(e / torch.tensor(s, dtype=e.dtype, device=e.device), dim=-1)
        return base.belief_record(crps=e.abs(), energy=energy, of=run.of, scale=s)


def _make_density(kind, run, value, bandwidth):
    if kind == "particles":
        run.filter.belief_density(run.truth, of=run.of, bandwidth=bandwidth)
        return run.filter.last_density
    with torch.no_grad():
        cov = _belief_of(run).covariance
        return base.belief_record(log_score=gaussian_log_density(run.est, cov, run.truth), entropy=gaussian_entropy(cov),
                                  mode=run.est, of=run.of)


def _make_modes(kind, run, count, radius):
    K = int(count)
    if kind == "particles":
        run.filter.belief_modes(run.of, max_modes=K, link_radius=radius)
        return run.filter.last_modes
    est = run.est
    with torch.no_grad():  # the one mode a Gaussian has
        at = torch.full(est.shape[:2] + (K, est.shape[-1]), math.nan, dtype=est.dtype, device=est.device)
        at[:, :, 0] = est
        mass = torch.zeros(est.shape[:2] + (K,), dtype=est.dtype, device=est.device)
        mass[:, :, 0] = 1.0
        count = torch.ones(est.shape[:2], dtype=torch.int32, device=est.device)
        return base.belief_record(modes=at, mean=at.clone(), mass=mass, count=count, of=run.of, max_modes=K)


def _make_modalities(kind, run, value, option):
    run.filter.belief_modalities()  # always of the filtered sets: a smoothed weight is not a prior times a likelihood
    return run.filter.last_modalities


def _make_quantiles(kind, run, probs, option):
    run.filter.belief_quantiles(probs, of=run.of, truth=run.truth)
    return run.filter.last_quantiles


_HISTORY = {"particles": "record_history"}
_RECORDS = (
    _Record(argument="return_innovations", asked=bool, kind=_innovations_kind, weighted=False,
            switch={"gaussian": "record_innovations"}, make=_make_innovations),
    _Record(argument="return_scores", asked=bool, option="score_scale", default=None,
            unused="run_filter: score_scale is the scale of return_scores' energy score; without return_scores it has no use",
            kind=_belief_kind("scores", point="point"), check=_check_score_scale,
            sized="run_filter: score_scale must be None or d = {d} positive finite floats, got {got!r}",
            weighted=True, switch={**_HISTORY, "gaussian": "record_belief", "point": None}, make=_make_scores),
    _Record(argument="return_density", asked=bool, option="density_bandwidth", default=_DEFAULT_BANDWIDTH,
            unused="run_filter: density_bandwidth is the bandwidth of return_density's kernel density; without "
                   "return_density it has no use",
            kind=_belief_kind("density"), check=_check_density_bandwidth,
            sized="run_filter: density_bandwidth must be 'silverman', 'scott' or d = {d} positive finite floats, got {got!r}",
            weighted=True, switch={**_HISTORY, "gaussian": "record_belief"}, make=_make_density),
    _Record(argument="return_modes", asked=_is_given, option="modes_link_radius", default=_DEFAULT_RADIUS,
            unused="run_filter: modes_link_radius is the link radius of return_modes' quick shift; without return_modes "
                   "it has no use",
            kind=_belief_kind("modes"), check=_check_modes, weighted=True, switch={**_HISTORY, "gaussian": None}, make=_make_modes),
    _Record(argument="return_modalities", asked=bool, kind=_modalities_kind, weighted=False, switch=_HISTORY, make=_make_modalities),
    _Record(argument="return_quantiles", asked=_is_given, kind=_quantiles_kind, weighted=True, switch=_HISTORY, make=_make_quantiles),
)


def _plan(record, filter_model, arguments, unweighted=None):
    """The checks of one record that need no trajectory, in their order -> ``(record, kind, value, option)``, or ``None``
    where the record is not asked for.  ``unweighted``: the smoothing method where the call smooths with one that leaves no
    weighted set per step."""
    value, option = arguments[record.argument], arguments.get(record.option, record.default)
    asked = record.asked(value)
    if option is not record.default and not asked:
        raise ValueError(record.unused)
    if not asked:
        return None
    kind = record.kind(filter_model)
    if record.check is not None:
        option = record.check(value, option)
    if record.weighted and kind == "particles" and unweighted is not None:
        raise ValueError(f"run_filter: {record.argument} reads a weighted particle set per step; smooth_method={unweighted!r} "
                         "leaves none (ancestry keeps no per-step weights, a MAP path is not a distribution): smooth with "
                         "'marginal' or 'simulation', or do not smooth")
    return record, kind, value, option


def run_filter(filter_model, traj: Dict[str, torch.Tensor], *, initial_cov_scale: float = 0.1,
               measurement_initialize: bool = False, return_belief: bool = False, smooth_lag=False,
               smooth_method: str = _DEFAULT_METHOD, smooth_draws: int = _DEFAULT_DRAWS, smooth_transition_moments: bool = False,
               return_innovations: bool = False, return_density: bool = False, density_bandwidth=_DEFAULT_BANDWIDTH,
               return_modes=None, modes_link_radius: float = _DEFAULT_RADIUS, return_modalities: bool = False,
               return_quantiles=None, return_scores: bool = False, score_scale=None):
    """Initialise the belief at ``states[0]`` with covariance ``0.1 I`` (or from the first
    observation, ``eval_helpers.py:116-131``) and filter ``[1:]`` (``:139-142``).  Returns the estimates ``(T, N, d)`` alone,
    or one tuple: the estimates, then whatever of belief, innovations, scores, density, modes, modalities and quantiles was
    asked for, in this order.

    The run and the smoother.
    ``return_belief``: run with ``record_belief`` set and return ``filter_model.last_belief`` -- the per-step posterior
    covariances (and the particle filter's ESS / log-evidence) for the calibration metrics below.
    ``smooth_lag``: ``False`` (the default) leaves all of this as it is; an integer or ``None`` (the full smoother) runs a
    particle filter with ``record_history`` set and returns ``filter_model.smooth(smooth_lag)`` -- the whole recorded
    trajectory is at hand, so ``E[x_t | y_1..t+lag]`` is the better estimate -- and, with ``return_belief``, the smoothed
    record ``filter_model.last_smoothed`` (``covariance``, ``unique``, ``lag``) in place of the filter's.
    ``smooth_method``: passed to ``smooth(method=)``; left at its default it is the filter's ``default_smooth_method`` --
    ``"rts"`` for the extended Kalman filters (``VirtualSensorExtendedKalmanFilter.smooth``: ``covariance``, ``gain``,
    ``lag``), ``"ancestry"`` for every filter that names none, the particle filter included; ``"marginal"`` smooths also where ``smooth_lag`` is left at ``False``
    (it is the full smoother: ``smooth_lag`` must be ``False`` or ``None``) and leaves ``covariance``, ``ess``, ``weights``;
    ``"simulation"`` likewise, with ``smooth_draws`` joint paths per trajectory (``smooth(num_draws=)``, default 64; passing it with
    another method is the ``ValueError`` it is there), and leaves ``covariance``, ``trajectories``, ``indices``, ``num_draws``;
    ``"map"`` likewise returns the most probable particle PATH ``(T, N, d)`` and leaves ``indices``, ``log_posterior`` and no
    ``covariance`` (a path is not a distribution: ``gaussian_nll`` / ``nees`` / ``coverage`` do not apply).
    ``smooth_transition_moments``: smooths with the filter's ``record_transition_moments`` set -- with
    ``smooth_method="marginal"`` or ``"rts"`` alone; the record gains ``residual_mean`` and ``residual_second_moment``
    (``process_noise_m_step``).

    The appended records (``_RECORDS`` describes each once).  For all of them: the truth is ``traj["states"][1:]``.  A filter
    that cannot give the record, an option without its ``return_*`` argument, a bad option and a smoothing method that does
    not fit are refused before the run, in the order of the records; the trajectories are not read before that.  Every
    ``record_*`` switch the run needs is put back on every path, before the record is made.  A particle filter runs with
    ``record_history`` set and its ``belief_*`` method is called with ``of="smoothed"`` exactly when the call smooths, which
    then must be with ``"marginal"`` or ``"simulation"``: ``"ancestry"`` with a lag, ``"map"`` and ``"rts"`` leave no weighted
    set per step.  A filter with a belief covariance (the Kalman filters) gets the closed forms of its Gaussian belief, of the
    returned means and the covariance that goes with them -- the smoothed one when the call smooths.  With the argument left
    at its default every return value and every bit is as without it.
    ``return_innovations``: runs a Kalman filter with ``record_innovations`` set and appends ``filter_model.last_innovations``
    -- ``nis``, ``log_likelihood``, ``accepted`` per step (``innovation_summary``).  A filter without the switch (the particle
    filters, the LSTM baselines) is refused.
    ``return_scores``: strictly proper scores of the belief, the one scale on which the three kinds of filter can be ranked as
    distributions (``score_summary``).  Particles: ``belief_scores(truth, of=, scale=score_scale)`` -- ``crps (T, N, d)``,
    ``energy (T, N)``, ``spread (T, N, d + 1)``.  Gaussian, with ``record_belief`` set: ``crps = gaussian_crps(...)`` and no
    ``energy``, which has no closed form.  A filter with neither (the LSTM baselines) gets the scores of a point mass: ``crps =
    |estimate - true|``, ``energy = |(estimate - true) / s|``.  ``score_scale``: ``None`` or ``d`` positive finite floats ``s``
    for the Euclidean norm of ``energy``.
    ``return_density``: the logarithmic score of the belief at the truth, its entropy and its mode (``density_summary``).
    Particles: ``belief_density(truth, of=, bandwidth=density_bandwidth)``.  Gaussian, with ``record_belief`` set: ``log_score =
    gaussian_log_density(...)``, ``entropy = gaussian_entropy(...)`` and ``mode``, the returned means.  A point estimate has no
    density: refused.  ``density_bandwidth``: ``"silverman"`` (the default), ``"scott"`` or ``d`` positive finite floats.
    ``return_modes``: an integer ``K`` (1 .. 8): how many hypotheses the belief holds per step, where they are and what each
    weighs (``mode_errors``, ``mode_summary``).  Particles: ``belief_modes(of, max_modes=K, link_radius=modes_link_radius)``
    (default 3.0 bandwidths).  Gaussian: the one mode a Gaussian has -- ``modes (T, N, K, d)`` and ``mean`` with the returned
    means at rank 0 and NaN beyond, ``mass`` 1 and 0, ``count`` 1.  A point estimate is refused.
    ``return_modalities``: which sensor decided each step: every modality's share of the fused posterior, its own evidence,
    mean, divergence and overlap (``modality_summary``, ``modality_errors``).  A crossmodal particle filter calls
    ``belief_modalities()``, always of the filtered sets, whatever the call smooths with -- a smoothed weight is not a prior
    times a likelihood.  Every other filter is refused: a particle filter with one measurement model fuses nothing, an LSTM
    baseline has no belief, and the Kalman filters fuse their sub-filters per state dimension, whose attribution is a separate
    change.
    ``return_quantiles``: a sequence of probabilities; a particle filter calls ``belief_quantiles(probs, of=, truth=)``:
    ``probs``, ``quantiles (T, N, Q, d)``, ``of``, ``pit (T, N, d)`` (``interval_coverage``, ``pit_histogram``).  A filter
    without ``belief_quantiles`` (the Kalman filters, whose quantiles are closed form, and the LSTM baselines) is refused."""
    # 1. check everything, in order, before the run
    arguments = dict(return_innovations=return_innovations, return_scores=return_scores, score_scale=score_scale,
                     return_density=return_density, density_bandwidth=density_bandwidth, return_modes=return_modes,
                     modes_link_radius=modes_link_radius, return_modalities=return_modalities, return_quantiles=return_quantiles)
    plans = [_plan(_RECORDS[0], filter_model, arguments)]  # (the innovations, which no smoother bears on, come first)
    named = smooth_method is not _DEFAULT_METHOD
    if not named:
        smooth_method = getattr(filter_model, "default_smooth_method", "ancestry")
    if smooth_transition_moments and smooth_method not in ("marginal", "rts"):
        raise ValueError(f"run_filter: smooth_transition_moments are the two-slice moments that smooth_method='marginal' (particle "
                         f"filters) and 'rts' (extended Kalman filters) compute; "
                         f"smooth_method={smooth_method!r} has none")
    if smooth_draws is not _DEFAULT_DRAWS and smooth_method != "simulation":
        raise ValueError(f"run_filter: smooth_draws is the number of paths smooth_method='simulation' draws; "
                         f"smooth_method={smooth_method!r} takes none")
    if named and smooth_method != "ancestry" and smooth_lag is False:
        smooth_lag = None  # a named smoother is the full one
    smoothing = smooth_lag is not False  # (0 is a lag)
    of = "smoothed" if smoothing else "filtered"
    unweighted = smooth_method if smoothing and smooth_method not in ("marginal", "simulation") else None
    plans += [_plan(record, filter_model, arguments, unweighted) for record in _RECORDS[1:]]
    plans = [plan for plan in plans if plan is not None]
    states = traj["states"]
    T1, N, d = states.shape
    for record, _, _, option in plans:
        if isinstance(option, tuple) and len(option) != d:
            raise ValueError(record.sized.format(d=d, got=option))
    obs = {k: traj[k] for k in ("image", "gripper_pos", "gripper_sensors")}
    # 2. set the switches (belief, history, innovations: the order in which a filter without one is told so)
    needed = {record.switch[kind] for record, kind, _, _ in plans}
    needed.update(["record_belief"] * bool(return_belief) + ["record_history"] * smoothing)
    with contextlib.ExitStack() as switches:
        for name in ("record_belief", "record_history", "record_innovations"):
            if name in needed:
                switches.enter_context(_switched(filter_model, name))
        # 3. initialise, run, and smooth
        with torch.no_grad():
            if measurement_initialize and hasattr(filter_model, "measurement_initialize_beliefs"):
                filter_model.measurement_initialize_beliefs({k: v[0] for k, v in obs.items()})
            else:
                cov = (torch.eye(d, device=states.device) * initial_cov_scale)[None].expand(N, d, d)
                filter_model.initialize_beliefs(mean=states[0], covariance=cov)
            est = filter_model.forward_loop(observations={k: v[1:] for k, v in obs.items()},
                                            controls=traj["controls"][1:])
    if smoothing:
        draws = {} if smooth_draws is _DEFAULT_DRAWS else {"num_draws": smooth_draws}  # (another method refuses it, as smooth() does)
        with _switched(filter_model, "record_transition_moments") if smooth_transition_moments else contextlib.nullcontext():
            est = filter_model.smooth(smooth_lag, method=smooth_method, **draws)
    # 4. make the records in order
    run = _Run(filter_model, est, states[1:], of, smoothing)
    out = [est, _belief_of(run)] if return_belief else [est]
    out += [record.make(kind, run, value, option) for record, kind, value, option in plans]
    return est if len(out) == 1 else tuple(out)


def compare_filters(filter_a, filter_b, traj: Dict[str, torch.Tensor], *, smooth_method=None, smooth_draws: int = _DEFAULT_DRAWS,
                    scale=None, **run_filter_kwargs):
    """Two particle filters on the same trajectories, and how far their posteriors are apart step by step: 300 particles
    against 4096, one arithmetic mode, resampling scheme or modality mask against another.  Both run through
    ``run_filter``'s initialisation (``run_filter_kwargs``: ``initial_cov_scale``, ``measurement_initialize``) with
    ``record_history`` set, and the switches are put back.  ``smooth_method=None`` compares the filtered sets;
    ``"marginal"`` or ``"simulation"`` (with ``smooth_draws`` paths) smooths both and compares the smoothed sets.  Returns
    ``(estimates_a, estimates_b, record)``: what ``run_filter`` returns for each -- the smoothed estimates when the call
    smooths -- and ``filter_a.last_distance`` as ``filter_a.belief_distance(filter_b, scale=scale)`` leaves it
    (``distance_summary``).  Each filter draws from its own ``noise``.  Anything that is not a particle filter is refused
    before either runs: a Gaussian belief or a point estimate has no particle set, and the closed forms are a separate
    change."""
    for name, f in (("filter_a", filter_a), ("filter_b", filter_b)):
        if not (hasattr(f, "belief_distance") and hasattr(f, "record_history")):
            raise ValueError(f"compare_filters: {name} must be a particle filter; {type(f).__name__} has no belief_distance (a "
                             "Gaussian belief or a point estimate has no particle set to compare)")
    if filter_a is filter_b:
        raise ValueError("compare_filters: filter_a and filter_b are one object, whose second run would replace the first's "
                         "history; compare one filter's own sets with belief_distance(of=, other_of=)")
    if smooth_method not in (None, "marginal", "simulation"):
        raise ValueError(f"compare_filters: smooth_method must be None, 'marginal' or 'simulation' (the smoothers that leave a "
                         f"weighted set per step), got {smooth_method!r}")
    if smooth_draws is not _DEFAULT_DRAWS and smooth_method != "simulation":
        raise ValueError(f"compare_filters: smooth_draws is the number of paths smooth_method='simulation' draws; "
                         f"smooth_method={smooth_method!r} takes none")
    extra = sorted(set(run_filter_kwargs) - {"initial_cov_scale", "measurement_initialize"})
    if extra:
        raise ValueError(f"compare_filters: run_filter_kwargs may name initial_cov_scale and measurement_initialize, got {extra}")
    smooth = {} if smooth_method is None else {"smooth_method": smooth_method}
    if smooth_draws is not _DEFAULT_DRAWS:
        smooth["smooth_draws"] = smooth_draws
    estimates = []
    for f in (filter_a, filter_b):
        with _switched(f, "record_history"):
            estimates.append(run_filter(f, traj, **smooth, **run_filter_kwargs))
    of = "filtered" if smooth_method is None else "smoothed"
    filter_a.belief_distance(filter_b, of=of, other_of=of, scale=scale)
    return estimates[0], estimates[1], filter_a.last_distance


def forecast_filter(filter_model, traj: Dict[str, torch.Tensor], horizon: int, *, crps: bool = True,
                    initial_cov_scale: float = 0.1, measurement_initialize: bool = False):
    """Runs a filter over the trajectories and forecasts every step ``1 .. horizon`` steps ahead: how good is the learned
    dynamics model on its own, ``h`` steps out, under the belief the filter really held?  The run goes through
    ``run_filter``'s initialisation with ``record_history`` set, and the switch is put back on every path; the truth is
    ``traj["states"][1:]``.  Returns ``(estimates, record)``: the filter's estimates ``(T, N, d)`` as ``run_filter`` returns
    them and ``filter_model.last_forecast`` (``forecast_summary``), every array with the forecast of step ``t + h`` made at
    ``t`` at ``[h - 1, t]`` and NaN where ``t + h > T - 1``.
    A particle filter calls ``belief_forecast(horizon, truth, crps=crps)``: ``mean``, ``covariance``, ``error``, ``log_score``,
    ``pit``, ``horizon`` and, with ``crps``, ``spread`` and ``crps`` of the predictive mixtures (``mmf_pf_predictive``).  An
    extended Kalman filter calls its ``belief_forecast(horizon, truth)`` and the record is completed with the closed forms of
    its Gaussian forecasts: ``log_score = gaussian_log_density(...)``, ``pit = Phi((y - mean) / sigma)`` and, with ``crps``,
    ``crps = gaussian_crps(...)``; there is no ``spread``.  Every other filter is refused before the run, the trajectories
    unread: the unscented and the fused Kalman filters keep no history to forecast from, and the LSTM baselines have no
    belief to roll out."""
    if isinstance(filter_model, filters.VirtualSensorUnscentedKalmanFilter):
        raise ValueError("forecast_filter: VirtualSensorUnscentedKalmanFilter keeps no history to forecast from (its "
                         "record_history cannot be set); forecast with the extended Kalman filter or a particle filter")
    if not (hasattr(filter_model, "belief_forecast") and hasattr(filter_model, "record_history")):
        why = ("keeps no history to forecast from" if hasattr(filter_model, "record_belief") else
               "has no belief to roll out through a dynamics model")
        raise ValueError(f"forecast_filter: {type(filter_model).__name__} {why}; forecast with a particle filter or "
                         "VirtualSensorExtendedKalmanFilter")
    if isinstance(horizon, bool) or not isinstance(horizon, numbers.Integral) or horizon < 1:
        raise ValueError(f"forecast_filter: horizon must be an int >= 1, got {horizon!r}")
    with _switched(filter_model, "record_history"):
        est = run_filter(filter_model, traj, initial_cov_scale=initial_cov_scale, measurement_initialize=measurement_initialize)
    truth = traj["states"][1:]
    if hasattr(filter_model, "belief_scores"):  # (a particle filter: what _belief_kind tells the kinds apart by)
        filter_model.belief_forecast(horizon, truth, crps=crps)
        return est, filter_model.last_forecast
    filter_model.belief_forecast(horizon, truth)
    rec = filter_model.last_forecast
    T = truth.shape[0]
    with torch.no_grad():
        y = truth.to(device=rec.mean.device, dtype=torch.float32)
        rec.log_score = torch.full_like(rec.mean[..., 0], math.nan)
        rec.pit = torch.full_like(rec.mean, math.nan)
        if crps:
            rec.crps = torch.full_like(rec.mean, math.nan)
        for h in range(1, min(int(horizon), T - 1) + 1):  # (the leads beyond the data hold NaN covariances: not factorised)
            mean, cov, true = rec.mean[h - 1, :T - h], rec.covariance[h - 1, :T - h], y[h:]
            rec.log_score[h - 1, :T - h] = gaussian_log_density(mean, cov, true)
            sigma = torch.sqrt(torch.diagonal(cov, dim1=-2, dim2=-1))
            rec.pit[h - 1, :T - h] = 0.5 * torch.erfc((mean - true) / (sigma * math.sqrt(2.0)))
            if crps:
                rec.crps[h - 1, :T - h] = gaussian_crps(mean, cov, true)
    return est, rec


def forecast_summary(record, start: int = START_TRUNCATION) -> Dict[str, torch.Tensor]:
    """Means of a forecast record (``last_forecast`` after ``belief_forecast`` with a truth; ``forecast_filter``) per lead,
    over the finite entries of the origins ``t >= start`` and the trajectories: ``rmse (H, d)`` of ``error``, ``count (H,)``
    the number of targets with a finite error behind each lead's figures and, where the record holds them, ``crps (H, d)``,
    ``log_score (H,)`` and ``pit_mean (H, d)`` (0.5 for a calibrated forecast).  The targets beyond the data and the steps
    without a live particle (NaN) are left out, like ``score_summary`` leaves them; a lead without any is NaN with count 0."""
    if getattr(record, "horizon", None) is None or getattr(record, "error", None) is None:
        raise ValueError("forecast_summary: the record is no forecast record with a truth (no horizon or no error); take it "
                         "from belief_forecast(horizon, truth) or forecast_filter")
    H = int(record.horizon)
    per_lead = lambda x, tail: torch.stack([_finite_mean(x[h], start, tail=tail) for h in range(H)]).to(torch.float32)
    out = {"rmse": torch.sqrt(per_lead(record.error.to(torch.float64) ** 2, 1)),
           "count": torch.isfinite(record.error[:, start:]).all(dim=-1).sum(dim=(1, 2))}
    if getattr(record, "crps", None) is not None:
        out["crps"] = per_lead(record.crps, 1)
    if getattr(record, "log_score", None) is not None:
        out["log_score"] = per_lead(record.log_score, 0)
    if getattr(record, "pit", None) is not None:
        out["pit_mean"] = per_lead(record.pit, 1)
    return out


def _finite_mean(x: torch.Tensor, start: int, tail: int = 0) -> torch.Tensor:
    """The mean of the finite entries of ``x[start:]`` over its leading axes, accumulated in float64; the ``tail`` trailing
    axes are kept -> float64.  What every record summary below means by a mean after the burn-in."""
    x = x[start:].to(torch.float64)
    x = x.reshape((-1,) + tuple(x.shape[x.dim() - tail:]))
    ok = torch.isfinite(x)
    return torch.where(ok, x, torch.zeros_like(x)).sum(dim=0) / ok.sum(dim=0)


def _check_truth(who: str, true, T: int, N: int, d: int) -> None:
    if not isinstance(true, torch.Tensor) or tuple(true.shape) != (T, N, d):
        raise ValueError(f"{who}: true must be a (T, N, d) = ({T}, {N}, {d}) tensor, got "
                         f"{tuple(true.shape) if isinstance(true, torch.Tensor) else type(true).__name__}")


def distance_summary(record, start: int = START_TRUNCATION) -> Dict[str, object]:
    """Means of a distance record (``ParticleFilter.last_distance``; ``compare_filters``) over the finite entries of the steps
    after the burn-in, over time and trajectories: ``wasserstein``, ``cramer``, ``ks`` ``(d,)`` and ``energy`` (a float).
    Steps at which a side had no live particle (NaN) are left out, like ``score_summary`` leaves them."""
    if getattr(record, "wasserstein", None) is None:
        raise ValueError("distance_summary: the record has no wasserstein; take it from belief_distance or compare_filters")
    out = {k: _finite_mean(getattr(record, k), start, tail=1).to(torch.float32) for k in ("wasserstein", "cramer", "ks")}
    out["energy"] = float(_finite_mean(record.energy[..., None], start, tail=1).to(torch.float32)[0])
    return out


def path_log_density(filter_model, indices) -> torch.Tensor:
    """The joint log-density of index paths through ``filter_model.last_history`` -- ``log_posterior`` of
    ``smooth(method="map")`` by its definition (``include/mmf.h``, "MAP path smoothing"): for ``indices (T, N)`` or
    ``(T, N, S)`` integers ``i_t`` into the particles of step ``t``,
    ``v_0[i_0] + sum_{t >= 1} (loglik_t[i_t] - 1/2 |L^-1 (X_t[i_t] - F_{t-1}[i_{t-1}])|^2 - c)`` with
    ``v_0 = loglik_0 + logw_in_0`` and ``c = sum_k log L_kk + (d / 2) log 2 pi`` -> ``(N,)`` or ``(N, S)`` float64.  Float64
    torch ops on the chosen pairs only, ``O(T N S d^2)`` beside one evaluation of the dynamics means: no ``M^2``.  A path
    with a ``-1`` anywhere (a dead draw of ``method="simulation"``, a dead trajectory of ``method="map"``) gets ``-inf``.
    It compares the MAP path with the paths ``smooth(method="simulation")`` drew (``last_smoothed.indices``) and with the
    filter's ancestral lines."""
    h = getattr(filter_model, "last_history", None)
    if h is None or getattr(h, "states", None) is None:
        raise ValueError("path_log_density needs a particle history: set record_history and run forward_loop first")
    idx = torch.as_tensor(indices)
    if idx.dtype in (torch.bool,) or idx.is_floating_point() or idx.is_complex():
        raise ValueError(f"path_log_density: indices must be integers, got {idx.dtype}")
    T, N, M, d = h.states.shape
    if idx.dim() not in (2, 3) or tuple(idx.shape[:2]) != (T, N):
        raise ValueError(f"path_log_density: indices must be (T, N) or (T, N, S) = ({T}, {N}[, S]), got {tuple(idx.shape)}")
    single = idx.dim() == 2
    idx = (idx[..., None] if single else idx).to(device=h.states.device, dtype=torch.int64)
    if bool(((idx < -1) | (idx >= M)).any()):
        raise ValueError(f"path_log_density: indices must lie in -1 .. {M - 1}")
    dead = (idx < 0).any(dim=0)
    g = idx.clamp_min(0)
    take = lambda rows, k: torch.gather(rows.to(torch.float64), 2, k[..., None].expand(k.shape + (d,)))
    with torch.no_grad():
        pred, tril = filter_model._smoothing_transition(h, "map")
        total = torch.gather(h.log_likelihoods.to(torch.float64), 2, g).sum(dim=0)
        if h.log_weights_in is not None:
            total = total + torch.gather(h.log_weights_in[0].to(torch.float64), 1, g[0])
        if T > 1:
            L = torch.tril(tril.to(torch.float64))
            e = take(h.states[1:], g[1:]) - take(pred, g[:-1])
            z = torch.linalg.solve_triangular(L, e[..., None], upper=False)[..., 0]
            c = torch.log(torch.diagonal(L)).sum() + 0.5 * d * math.log(2.0 * math.pi)
            total = total + (-0.5 * (z * z).sum(-1) - c).sum(dim=0)
        total = torch.where(dead, torch.full_like(total, -math.inf), total)
    return total[:, 0] if single else total


def innovation_summary(record, dim: int) -> Dict[str, torch.Tensor]:
    """What a Kalman filter's innovation record (``last_innovations``; ``run_filter(return_innovations=True)``) says about
    the model, without ground truth.  ``dim``: the state dimension ``d``.  Under a consistent filter the NIS is chi-squared
    with ``d`` degrees of freedom, so ``mean_nis`` should be close to ``d``.
    ``mean_nis``: the mean NIS over ALL measurements, rejected ones included; ``accepted_fraction``; ``log_likelihood``: the
    sum of the per-step log-likelihoods over the ACCEPTED measurements (``log p(y_{1:T})`` of the model where nothing was
    rejected).  One 0-d tensor each for a single filter, ``(K,)`` -- one entry per sub-filter -- for a fused record;
    ``nis_over_dim = mean_nis / dim``, close to 1 for a consistent filter.  Plain torch on the record's device."""
    dim = int(dim)
    if dim < 1:
        raise ValueError(f"innovation_summary: dim must be the state dimension (>= 1), got {dim}")
    for k in ("nis", "log_likelihood", "accepted"):
        if getattr(record, k, None) is None:
            raise ValueError(f"innovation_summary: the record has no {k}; run the filter with record_innovations set")
    nis, ll, acc = record.nis.to(torch.float64), record.log_likelihood.to(torch.float64), record.accepted.to(torch.bool)
    if getattr(record, "sub_filters", None) is not None:  # (..., K, N) -> (K, everything else)
        nis, ll, acc = (t.movedim(-2, 0).reshape(t.shape[-2], -1) for t in (nis, ll, acc))
        axis = 1
    else:
        nis, ll, acc = (t.reshape(-1) for t in (nis, ll, acc))
        axis = 0
    if nis.shape[axis] == 0:
        raise ValueError("innovation_summary: the record holds no measurement")
    mean_nis = nis.mean(dim=axis)
    return {"mean_nis": mean_nis, "nis_over_dim": mean_nis / dim, "accepted_fraction": acc.to(torch.float64).mean(dim=axis),
            "log_likelihood": torch.where(acc, ll, torch.zeros_like(ll)).sum(dim=axis)}


def process_noise_m_step(record, *, diagonal: bool = False, start: int = 0) -> torch.Tensor:
    """The M-step of EM for the process noise from a smoothed record with transition moments
    (``smooth(method="marginal")`` of a particle filter or ``smooth()`` of an extended Kalman filter, ``method="rts"``, with
    ``record_transition_moments`` set): ``Q = mean over steps >= start and all trajectories of
    residual_second_moment`` -- the raw second moment, since the model's noise has mean zero -- and the ``(d, d)``
    ``scale_tril = cholesky(Q)``; ``diagonal``: ``diag(sqrt(diag Q))``, for a model that holds a diagonal only.  Plain torch,
    on the record's device (CPU tensors included).  A non-finite entry, or a ``Q`` that is not positive definite, is a
    ``ValueError`` naming the first offending ``(t, n)``."""
    m2 = getattr(record, "residual_second_moment", None)
    if m2 is None:
        raise ValueError("process_noise_m_step: the record has no residual_second_moment; smooth with "
                         "the filter's record_transition_moments set (method='marginal' for a particle filter, the full "
                         "'rts' smoother for an extended Kalman filter)")
    if m2.dim() != 4 or m2.shape[-1] != m2.shape[-2]:
        raise ValueError(f"process_noise_m_step: residual_second_moment must be (T - 1, N, d, d), got {tuple(m2.shape)}")
    start = int(start)
    if start < 0 or start >= m2.shape[0] or m2.shape[1] == 0:
        raise ValueError(f"process_noise_m_step: no transitions at steps >= {start} ({m2.shape[0]} steps, {m2.shape[1]} trajectories)")
    m2 = m2[start:].detach()

    def first(bad):  # the first (t, n) in row-major order, t counted from the record's step 0
        k = int(torch.nonzero(bad.reshape(-1))[0])
        return start + k // bad.shape[1], k % bad.shape[1]

    bad = ~torch.isfinite(m2).all(-1).all(-1)
    if bool(bad.any()):
        raise ValueError("process_noise_m_step: non-finite residual_second_moment at (t, n) = (%d, %d)" % first(bad))
    Q = m2.to(torch.float64).mean(dim=(0, 1))
    Q = 0.5 * (Q + Q.t())
    if diagonal:
        var = torch.diagonal(Q)
        if not bool((var > 0).all()):
            zero = ~(torch.diagonal(m2, dim1=-2, dim2=-1) > 0).all(-1)
            where = first(zero) if bool(zero.any()) else (start, 0)
            raise ValueError("process_noise_m_step: the refitted noise is not positive definite; first degenerate "
                             "residual_second_moment at (t, n) = (%d, %d)" % where)
        return torch.diag(torch.sqrt(var)).to(m2.dtype)
    L, info = torch.linalg.cholesky_ex(Q)
    if int(info) != 0:
        each = torch.linalg.cholesky_ex(m2.to(torch.float64))[1] != 0
        where = first(each) if bool(each.any()) else (start, 0)
        raise ValueError("process_noise_m_step: the refitted noise is not positive definite; first degenerate "
                         "residual_second_moment at (t, n) = (%d, %d)" % where)
    return L.to(m2.dtype)


def _moments_method(filter_model) -> str:
    """The smoothing method whose record carries the two-slice transition moments: the Kalman smoother for a filter whose
    default it is, the particle filter's marginal smoother otherwise."""
    return "rts" if getattr(filter_model, "default_smooth_method", None) == "rts" else "marginal"


def fit_process_noise(filter_model, traj: Dict[str, torch.Tensor], *, iterations: int = 5, start: int = 0,
                      return_log_likelihood: bool = False, **run_filter_kwargs):
    """EM for the process noise of ``filter_model.dynamics_model`` on the trajectories ``traj``: every iteration runs
    ``run_filter(smooth_method="marginal", smooth_transition_moments=True, return_belief=True)`` (the E-step: the two-slice
    moments under the current noise; ``smooth_method="rts"`` for an extended Kalman filter), takes ``process_noise_m_step`` over the steps ``>= start`` and hands the factor to
    ``dynamics_model.set_scale_tril`` -- the diagonal form where the model's ``diagonal_noise`` is true.  Returns the list
    of ``(d, d)`` factors, the initial one first: ``iterations + 1`` entries.  ``run_filter_kwargs`` go to ``run_filter``
    (``initial_cov_scale``, ``measurement_initialize``); the smoothing switches are this function's own.  The filter's
    ``record_*`` switches are restored on every path; a model without ``set_scale_tril`` is a ``TypeError`` before any
    run.  The moments are those of THIS process's trajectories: summing them across ranks is out of scope.
    ``return_log_likelihood`` (Kalman filters): also returns, as a second list of ``iterations + 1`` floats, the total
    log-likelihood ``sum_t,n log p(y_t | y_1..t-1)`` of the filter under each factor of the first list (``innovation_summary``
    of the E-step's own run; one more filter run for the last factor) -- what EM must not decrease, up to the linearisation.
    A filter without ``record_innovations`` is refused before any run."""
    dyn = getattr(filter_model, "dynamics_model", None)
    if dyn is None or not callable(getattr(dyn, "set_scale_tril", None)) or not callable(getattr(dyn, "scale_tril", None)):
        raise TypeError(f"fit_process_noise: {type(dyn).__name__} has no set_scale_tril(L) / scale_tril(): the process noise "
                        "of this dynamics model cannot be refitted (base.DynamicsModel documents the optional method)")
    if return_log_likelihood and not hasattr(filter_model, "record_innovations"):
        raise ValueError(f"fit_process_noise: return_log_likelihood needs a Kalman filter; {type(filter_model).__name__} has no "
                         "record_innovations")
    for k in ("smooth_method", "smooth_transition_moments", "return_belief", "smooth_lag", "smooth_draws", "return_innovations"):
        if k in run_filter_kwargs:
            raise TypeError(f"fit_process_noise: {k} is set by fit_process_noise itself")
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"fit_process_noise: iterations must be >= 0, got {iterations}")
    diagonal = bool(getattr(dyn, "diagonal_noise", False))
    out, logliks = [dyn.scale_tril().detach().clone()], []
    total = lambda innovations: float(innovation_summary(innovations, traj["states"].shape[-1])["log_likelihood"].sum())
    for _ in range(iterations):
        got = run_filter(filter_model, traj, smooth_method=_moments_method(filter_model), smooth_transition_moments=True,
                         return_belief=True, return_innovations=return_log_likelihood, **run_filter_kwargs)
        record = got[1]
        if return_log_likelihood:
            logliks.append(total(got[2]))
        L = process_noise_m_step(record, diagonal=diagonal, start=start)
        dyn.set_scale_tril(L)
        out.append(dyn.scale_tril().detach().clone())
    if return_log_likelihood:  # (the last factor has had no E-step)
        logliks.append(total(run_filter(filter_model, traj, return_innovations=True, **run_filter_kwargs)[1]))
        return out, logliks
    return out


def _whitened_error(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor):
    """``(L^-1 e, L)`` with ``C = L L^T`` (Cholesky) and ``e = predicted - true``, batched over ``(T, N)``."""
    L = torch.linalg.cholesky(covariance)
    e = (predicted - true).to(covariance.dtype)
    return torch.linalg.solve_triangular(L, e[..., None], upper=False)[..., 0], L


def nees(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor,
         start: int = START_TRUNCATION) -> torch.Tensor:
    """Normalised estimation error squared ``e^T C^-1 e`` of every step after the burn-in: ``(T, N, d)``, ``(T, N, d, d)``,
    ``(T, N, d)`` -> ``(T - start, N)``.  Its mean is ``d`` for a calibrated filter (chi-square with ``d`` degrees)."""
    y, _ = _whitened_error(predicted[start:], covariance[start:], true[start:])
    return torch.sum(y * y, dim=-1)


def gaussian_nll(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor,
                 start: int = START_TRUNCATION) -> torch.Tensor:
    """Negative log-likelihood of the true state under ``N(predicted, covariance)``, mean over time after the burn-in:
    ``0.5 (e^T C^-1 e + log det C + d log 2 pi)`` -> ``(N,)``, one number per trajectory."""
    y, L = _whitened_error(predicted[start:], covariance[start:], true[start:])
    logdet = 2.0 * torch.sum(torch.log(torch.diagonal(L, dim1=-2, dim2=-1)), dim=-1)
    d = predicted.shape[-1]
    return torch.mean(0.5 * (torch.sum(y * y, dim=-1) + logdet + d * math.log(2.0 * math.pi)), dim=0)


def gaussian_log_density(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
    """The log density of the true state under ``N(predicted, covariance)``, per step: ``(T, N, d)``, ``(T, N, d, d)``,
    ``(T, N, d)`` -> ``(T, N)``, ``-0.5 (e^T C^-1 e + log det C + d log 2 pi)``: the logarithmic score of a Gaussian belief,
    the number ``ParticleFilter.belief_density`` leaves as ``log_score`` for a particle set.  ``gaussian_nll`` is its negated
    mean over the steps after the burn-in.  In the dtype of ``covariance``."""
    y, L = _whitened_error(predicted, covariance, true)
    logdet = 2.0 * torch.sum(torch.log(torch.diagonal(L, dim1=-2, dim2=-1)), dim=-1)
    d = predicted.shape[-1]
    return -0.5 * (torch.sum(y * y, dim=-1) + logdet + d * math.log(2.0 * math.pi))


def gaussian_entropy(covariance: torch.Tensor) -> torch.Tensor:
    """The differential entropy of ``N(., covariance)``: ``(T, N, d, d)`` -> ``(T, N)``, ``0.5 log det(2 pi e C)``; what
    ``ParticleFilter.belief_density`` estimates as ``entropy`` for a particle set."""
    L = torch.linalg.cholesky(covariance)
    logdet = 2.0 * torch.sum(torch.log(torch.diagonal(L, dim1=-2, dim2=-1)), dim=-1)
    d = covariance.shape[-1]
    return 0.5 * (logdet + d * (1.0 + math.log(2.0 * math.pi)))


def density_summary(record, start: int = START_TRUNCATION) -> Dict[str, float]:
    """Means of a density record (``ParticleFilter.last_density``; ``run_filter(return_density=True)``) over the finite
    entries of the steps after the burn-in, over time and trajectories: ``log_score`` (where the record holds one; higher is
    better, its negation is the NLL) and ``entropy``, two floats.  Steps without a live particle (NaN) and log scores of
    ``-inf`` are left out, like ``score_summary`` leaves them."""
    if getattr(record, "entropy", None) is None:
        raise ValueError("density_summary: the record has no entropy; take it from belief_density or run_filter(return_density=True)")
    out = {"entropy": float(_finite_mean(record.entropy, start))}
    if getattr(record, "log_score", None) is not None:
        out["log_score"] = float(_finite_mean(record.log_score, start))
    return out


def map_axes(record):
    """The cell centres of a maps record (``ParticleFilter.last_maps``): ``(x (T, N, Gx), y (T, N, Gy))`` float32 along
    ``record.dims[0]`` and ``record.dims[1]``, by the rasteriser's own formula (``include/mmf.h``, ``mmf_pf_raster``):
    ``density[t, n, j, i]`` sits at ``(x[t, n, i], y[t, n, j])``."""
    if getattr(record, "density", None) is None or getattr(record, "center", None) is None or getattr(record, "step", None) is None:
        raise ValueError("map_axes: the record has no density, center and step; take it from belief_maps")
    return pf_summaries.map_cell_centres(record.center, record.step, record.cells)


def map_summary(record, true=None, start: int = START_TRUNCATION) -> Dict[str, object]:
    """Means of a maps record (``ParticleFilter.last_maps``) over the finite entries of the steps after the burn-in, over time
    and trajectories: ``mass``, the share of the belief inside the window (a float); with ``true (T, N, d)`` also
    ``peak_error``, the distance in the two map dimensions between the centre of the highest-density cell (the first among
    equals) and the truth; with likelihood maps also ``agreement (K + 1,)``, the Bhattacharyya coefficient between the
    normalised density map and each normalised ``exp(l - max l)`` map, the fused one last: does what sensor ``k`` says lie
    where the belief is?  Steps with a NaN map are left out, like ``score_summary`` leaves them."""
    density = getattr(record, "density", None)
    if density is None or density.dim() != 4 or getattr(record, "mass", None) is None:
        raise ValueError("map_summary: the record has no density (T, N, Gy, Gx) and mass; take it from belief_maps")
    T, N, Gy, Gx = density.shape
    out = {"mass": float(_finite_mean(record.mass, start))}
    with torch.no_grad():
        flat = density.reshape(T, N, Gy * Gx).to(torch.float64)
        blank = ~torch.isfinite(flat).all(dim=-1)
        nan = torch.full((T, N), math.nan, dtype=torch.float64, device=density.device)
        if true is not None:
            if not isinstance(true, torch.Tensor) or true.dim() != 3 or tuple(true.shape[:2]) != (T, N) or true.shape[2] <= max(record.dims):
                raise ValueError(f"map_summary: true must be a (T, N, d) = ({T}, {N}, d) tensor with d > {max(record.dims)}, got "
                                 f"{tuple(true.shape) if isinstance(true, torch.Tensor) else type(true).__name__}")
            x, y = map_axes(record)
            peak = torch.argmax(torch.where(blank[..., None], torch.zeros_like(flat), flat), dim=-1)  # (the first maximum)
            at = torch.stack([torch.gather(x, 2, (peak % Gx)[..., None])[..., 0],
                              torch.gather(y, 2, (peak // Gx)[..., None])[..., 0]], dim=-1).to(torch.float64)
            y2 = true.to(device=density.device, dtype=torch.float64)[..., list(record.dims)]
            out["peak_error"] = float(_finite_mean(torch.where(blank, nan, torch.linalg.vector_norm(at - y2, dim=-1)), start))
        ll = getattr(record, "log_likelihood", None)
        if ll is not None:
            K1 = ll.shape[2]
            p = flat / flat.sum(dim=-1, keepdim=True)
            l = ll.reshape(T, N, K1, Gy * Gx).to(torch.float64)
            q = torch.exp(l - l.max(dim=-1, keepdim=True).values)
            q = q / q.sum(dim=-1, keepdim=True)
            bc = torch.sqrt(p[:, :, None, :] * q).sum(dim=-1)                                     # (T, N, K + 1)
            out["agreement"] = _finite_mean(torch.where(blank[..., None], nan[..., None], bc), start, tail=1).to(torch.float32)
    return out


def mode_errors(record, true: torch.Tensor, scale=None) -> Dict[str, torch.Tensor]:
    """Errors of a modes record (``ParticleFilter.last_modes``; ``run_filter(return_modes=K)``) against the true states
    ``(T, N, d)``: ``top (T, N)``, the Euclidean error of the heaviest mode; ``best (T, N)``, the least error over the
    reported modes -- the oracle error of the multi-hypothesis tracking literature: was the truth among the hypotheses? --
    and ``best_rank (T, N)`` int64, which mode that was.  ``scale``: ``None`` or ``d`` positive finite floats dividing the
    coordinates inside the norm.  A step that reports no mode gives NaN, NaN and ``-1``."""
    modes = getattr(record, "modes", None)
    if modes is None or modes.dim() != 4:
        raise ValueError("mode_errors: the record has no modes (T, N, K, d); take it from belief_modes or run_filter(return_modes=K)")
    T, N, K, d = modes.shape
    _check_truth("mode_errors", true, T, N, d)
    if scale is not None:
        scale = _floats(scale)
        if scale is None or len(scale) != d or not _positive(scale):
            raise ValueError(f"mode_errors: scale must be None or d = {d} positive finite floats")
    with torch.no_grad():
        e = modes - true.to(device=modes.device, dtype=modes.dtype)[:, :, None, :]
        if scale is not None:
            e = e / torch.tensor(scale, dtype=e.dtype, device=e.device)
        err = torch.linalg.vector_norm(e, dim=-1)                       # (T, N, K); NaN at a rank beyond the count
        there = ~torch.isnan(err)
        best, rank = torch.where(there, err, torch.full_like(err, math.inf)).min(dim=-1)
        none = ~there.any(dim=-1)
        nan = torch.full_like(best, math.nan)
        return {"top": err[..., 0], "best": torch.where(none, nan, best), "best_rank": torch.where(none, torch.full_like(rank, -1), rank)}


def mode_summary(record, true=None, start: int = START_TRUNCATION) -> Dict[str, float]:
    """Means of a modes record over the steps after the burn-in, over time and trajectories: ``count``, the number of modes;
    ``top_mass``, the mass of the heaviest; ``multimodal``, the share of steps with more than one mode.  With ``true (T, N,
    d)`` also ``top_rmse`` and ``best_rmse``, the root mean squares of ``mode_errors``' ``top`` and ``best`` over the steps that
    report a mode."""
    if getattr(record, "count", None) is None or getattr(record, "mass", None) is None:
        raise ValueError("mode_summary: the record has no count and mass; take it from belief_modes or run_filter(return_modes=K)")
    count = record.count[start:].to(torch.float64).reshape(-1)
    out = {"count": float(count.mean()), "top_mass": float(record.mass[start:, :, 0].to(torch.float64).mean()),
           "multimodal": float((count > 1).to(torch.float64).mean())}
    if true is not None:
        errors = mode_errors(record, true)
        for k in ("top", "best"):
            x = errors[k].to(torch.float64)
            out[k + "_rmse"] = float(torch.sqrt(_finite_mean(x * x, start)))
    return out


def modality_summary(record, start: int = START_TRUNCATION) -> Dict[str, torch.Tensor]:
    """Means of a modalities record (``ParticleFilter.last_modalities``; ``run_filter(return_modalities=True)``) over the
    steps after the burn-in, over time and trajectories, each over its finite entries: ``responsibility (K,)``, every
    modality's share of the fused posterior; ``dominant (K,)``, the share of steps where modality ``k`` has the largest
    responsibility (the lowest index among equals; steps without a live particle are left out); ``log_evidence (K + 1,)``,
    the fused one last; ``divergence (K,)``; ``overlap (K, K)``; and ``prior (K,)``, the mean of ``softmax_k beta`` -- what the
    weight model asked for, uniform without one -- to read ``responsibility`` against."""
    rho = getattr(record, "responsibility", None)
    if rho is None or getattr(record, "log_evidence", None) is None:
        raise ValueError("modality_summary: the record has no responsibility and log_evidence; take it from belief_modalities "
                         "or run_filter(return_modalities=True)")

    mean = lambda x, tail=1: _finite_mean(x, start, tail).to(torch.float32)
    K = rho.shape[-1]
    r = rho[start:].reshape(-1, K)
    ok = torch.isfinite(r).all(dim=-1)
    first = torch.argmax(torch.where(ok[:, None], r, torch.zeros_like(r)), dim=-1)  # (the first maximum: the lowest index)
    wins = torch.nn.functional.one_hot(first, K).to(torch.float64) * ok[:, None]
    beta = getattr(record, "log_weights", None)
    prior = (torch.full((K,), 1.0 / K, dtype=torch.float32, device=rho.device) if beta is None else
             mean(torch.softmax(beta.to(torch.float64), dim=-1)))
    return {"responsibility": mean(rho), "dominant": (wins.sum(dim=0) / ok.sum()).to(torch.float32),
            "log_evidence": mean(record.log_evidence), "divergence": mean(record.divergence),
            "overlap": mean(record.overlap, tail=2), "prior": prior}


def modality_errors(record, true: torch.Tensor) -> torch.Tensor:
    """Euclidean errors ``(T, N, K + 1)`` of a modalities record's ``mean (T, N, K + 1, d)`` against the true states
    ``(T, N, d)``: what each sensor alone would have estimated on the filter's particles, and, last, the fused estimate.  NaN
    where a modality carried no weight."""
    mean = getattr(record, "mean", None)
    if mean is None or mean.dim() != 4:
        raise ValueError("modality_errors: the record has no mean (T, N, K + 1, d); take it from belief_modalities or "
                         "run_filter(return_modalities=True)")
    T, N, _, d = mean.shape
    _check_truth("modality_errors", true, T, N, d)
    with torch.no_grad():
        return torch.linalg.vector_norm(mean - true.to(device=mean.device, dtype=mean.dtype)[:, :, None, :], dim=-1)


def coverage(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor, level: float = 0.95,
             start: int = START_TRUNCATION) -> torch.Tensor:
    """Share of the steps after the burn-in whose true state lies inside the ``level`` ellipsoid of the belief, i.e. whose
    NEES is at most the ``level`` quantile of the chi-square distribution with ``d`` degrees -> ``(N,)``; ``level`` for a
    calibrated filter.  The test is made on the CDF side, ``F_d(nees) <= level``: ``F_2(x) = 1 - exp(-x / 2)`` in closed
    form, otherwise the regularised lower incomplete gamma ``P(d / 2, x / 2)`` (``torch.special.gammainc``)."""
    assert 0.0 < level < 1.0
    x = nees(predicted, covariance, true, start)
    d = predicted.shape[-1]
    if d == 2:
        cdf = 1.0 - torch.exp(-0.5 * x)
    else:
        cdf = torch.special.gammainc(torch.full_like(x, 0.5 * d), 0.5 * x)
    return torch.mean((cdf <= level).to(x.dtype), dim=0)


def gaussian_crps(predicted: torch.Tensor, covariance: torch.Tensor, true: torch.Tensor) -> torch.Tensor:
    """The continuous ranked probability score of the Gaussian belief ``N(predicted, covariance)`` at the true state, per
    state dimension, in closed form on the covariance's diagonal: ``(T, N, d)``, ``(T, N, d, d)``, ``(T, N, d)`` -> ``(T, N,
    d)``, ``sigma [z (2 Phi(z) - 1) + 2 phi(z) - 1 / sqrt(pi)]`` with ``z = (y - mu) / sigma`` (Gneiting & Raftery 2007), and
    ``|y - mu|`` where ``sigma = 0``: a point mass.  The same number ``ParticleFilter.belief_scores`` takes on a weighted
    particle set, so the two kinds of belief are ranked on one scale.  In the dtype of ``covariance``."""
    var = torch.diagonal(covariance, dim1=-2, dim2=-1)
    sigma = torch.sqrt(var.clamp_min(0.0))
    e = (true - predicted).to(sigma.dtype)
    point = sigma == 0
    z = e / torch.where(point, torch.ones_like(sigma), sigma)
    phi = torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)
    closed = sigma * (z * torch.erf(z / math.sqrt(2.0)) + 2.0 * phi - 1.0 / math.sqrt(math.pi))
    return torch.where(point, e.abs(), closed)


def score_summary(record, start: int = START_TRUNCATION) -> Dict[str, object]:
    """Means of a score record (``ParticleFilter.last_scores``; ``run_filter(return_scores=True)``) over the finite entries
    of the steps after the burn-in, over time and trajectories: ``crps (d,)``, and, where the record holds them, ``energy``
    (a float) and ``spread (d + 1,)``.  Lower is better; ``crps`` is in each state dimension's own units.  Steps without a
    live particle (NaN) are left out, like the other metrics leave them."""
    if getattr(record, "crps", None) is None:
        raise ValueError("score_summary: the record has no crps; take it from belief_scores or run_filter(return_scores=True)")
    mean = lambda x: _finite_mean(x, start, tail=1).to(torch.float32)  # over every axis but the last
    out = {"crps": mean(record.crps)}
    if getattr(record, "energy", None) is not None:
        out["energy"] = float(mean(record.energy[..., None])[0])
    if getattr(record, "spread", None) is not None:
        out["spread"] = mean(record.spread)
    return out


def interval_coverage(lower: torch.Tensor, upper: torch.Tensor, true: torch.Tensor, start: int = START_TRUNCATION) -> torch.Tensor:
    """Share of the steps after the burn-in whose true state lies inside the credible interval, per trajectory and state
    dimension: ``(T, N, d)`` x3 -> ``(N, d)``, the mean over time of ``lower <= true <= upper``; the interval's level for a
    calibrated filter -- e.g. 0.95 for the ``0.025`` and ``0.975`` quantiles of ``ParticleFilter.belief_quantiles``.  The
    non-parametric counterpart of ``coverage``, which tests against the moment-matched ellipsoid.  A NaN bound (a step without
    a live particle) does not cover."""
    assert lower.shape == upper.shape == true.shape, (tuple(lower.shape), tuple(upper.shape), tuple(true.shape))
    inside = (lower[start:] <= true[start:]) & (true[start:] <= upper[start:])
    return torch.mean(inside.to(torch.float32), dim=0)


def pit_histogram(pit: torch.Tensor, bins: int = 10, start: int = START_TRUNCATION) -> torch.Tensor:
    """Histogram of the probability integral transform (``belief_quantiles(truth=)``'s ``pit (T, N, d)``) after the burn-in,
    over all steps and trajectories: ``(d, bins)`` shares of equal-width bins of ``[0, 1]`` that sum to 1 per dimension, with
    ``pit == 1`` in the last bin.  Flat (``1 / bins`` each) for a calibrated filter; a U shape says the belief is too narrow,
    a hump too wide, a slope biased.  NaN entries (steps without a live particle) are left out."""
    assert isinstance(bins, int) and bins >= 1
    p = pit[start:]
    d = p.shape[-1]
    p = p.reshape(-1, d)
    ok = ~torch.isnan(p)
    idx = torch.clamp(torch.floor(torch.nan_to_num(p, nan=0.0).to(torch.float64) * bins).to(torch.int64), 0, bins - 1)
    counts = torch.zeros((d, bins), dtype=torch.float64, device=p.device)
    counts.scatter_add_(1, idx.t().contiguous(), ok.t().to(torch.float64).contiguous())
    return (counts / counts.sum(dim=1, keepdim=True)).to(torch.float32)


def per_trajectory_mse(predicted: torch.Tensor, true: torch.Tensor,
                       start: int = START_TRUNCATION) -> torch.Tensor:
    """``(T, N, d)`` x2 -> ``(N, d)``: mean over time of the squared error after a burn-in
    (``eval_helpers.py:149-157``)."""
    err = predicted[start:] - true[start:]
    return torch.mean(err ** 2, dim=0)


def raw_rmse(per_batch_mse: torch.Tensor) -> np.ndarray:
    """``sqrt(mean_N)`` per state dimension (``eval_helpers.py:160``)."""
    return np.sqrt(np.mean(per_batch_mse.detach().cpu().numpy(), axis=0))


def task_metrics(task_name: str, rmse: np.ndarray) -> Dict[str, float]:
    """Unit conversion of ``eval_helpers.py:166-177`` (door) and ``:192-203`` (push)."""
    spec = DOOR if task_name == "door" else PUSH
    scaled = rmse * np.array(spec.rmse_scale)
    out = {"raw_rmse": [float(x) for x in rmse]}
    if task_name == "door":
        out["theta_rmse_deg"] = float(scaled[0] * 180.0 / np.pi)
        out["x_rmse_cm"] = float(scaled[1] * 100.0)
        out["y_rmse_cm"] = float(scaled[2] * 100.0)
    else:
        out["x_rmse_cm"] = float(scaled[0] * 100.0)
        out["y_rmse_cm"] = float(scaled[1] * 100.0)
    return out

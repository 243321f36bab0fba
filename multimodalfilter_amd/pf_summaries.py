"""The summaries of ``filters.ParticleFilter``: the ``belief_*`` readers of the particle sets a ``forward_loop`` recorded.
Each reads ``last_history`` / ``last_smoothed``, writes a ``last_*`` record of its own and touches nothing of the recursion."""
import math
import numbers
from typing import Optional

import torch

from . import _abi, base, engine
from .utils import tree_map

_MAP_CHUNK_STATES = 1 << 22  # grid states of one measurement launch of belief_maps(likelihoods=True): 64 MiB of them at d = 4


def map_cell_centres(center: torch.Tensor, step, cells):
    """The cell centres of belief maps (``include/mmf.h``, ``mmf_pf_raster``): ``center (..., 2)``, ``step`` and ``cells =
    (Gx, Gy)`` -> ``(u (..., Gx), v (..., Gy))`` float32, ``u_i = fmaf(float(i) - 0.5f (Gx - 1), step_x, c_x)``.  The product
    is exact in float64 and the sum is rounded once more on the way to float32: the middle cell of an odd count is the centre
    bit for bit."""
    axes = []
    for k, (s, g) in enumerate(zip(step, cells)):
        i = torch.arange(g, dtype=torch.float64, device=center.device) - 0.5 * (g - 1)
        axes.append((i * float(s) + center[..., k, None].to(torch.float64)).to(torch.float32))
    return axes[0], axes[1]


class ParticleSummaries:
    """The ``belief_*`` methods of the particle filter, a mixin like ``filters.InnovationSwitches``; the host class supplies
    ``last_history`` / ``last_smoothed``, the two models, ``noise`` and ``ParticleSmoothing._transition_means``.
    ``belief_quantiles(probs, of=, truth=)``: per-dimension weighted quantiles of the recorded sets (and the PIT of a true
    state) -> ``last_quantiles``; the non-parametric counterpart of the covariance (``mmf_pf_quantiles``).
    ``belief_scores(truth, of=, scale=)``: CRPS per dimension and the energy score of the recorded sets against the true
    states -> ``last_scores``; strictly proper, so calibration and sharpness in one number (``mmf_pf_scores``).
    ``belief_density(truth=, of=, bandwidth=, min_bandwidth=)``: the kernel density of the recorded sets -- the mode per step
    (returned), the log density at every particle, the entropy and, with a truth, the logarithmic score -> ``last_density``
    (``mmf_pf_density``).
    ``belief_modes(of=, max_modes=, link_radius=, bandwidth=, min_bandwidth=)``: the modes of the recorded sets by quick shift
    on that density -- how many, where, and the mass of each (returned: ``modes (T, N, K, d)``) -> ``last_modes``
    (``mmf_pf_modes``).
    ``belief_modalities()``: with a crossmodal measurement model, which sensor decided each step -- every enabled modality's
    evidence-weighted share of the fused posterior (returned: ``responsibility (T, N, K)``), its own evidence, effective
    sample size, mean, divergence from the fused posterior and overlap with the others -> ``last_modalities``
    (``mmf_pf_modalities``); ``forward_loop`` keeps a reference to the observations and the ``enabled_models`` of the run
    in the history for it.
    ``belief_distance(other=, of=, other_of=, scale=)``: two-sample distances between the recorded sets of two filters, or of
    one filter's filtered and smoothed sets -- 1-Wasserstein per dimension (returned), Cramer, Kolmogorov-Smirnov and the
    energy distance -> ``last_distance`` (``mmf_pf_distance``).
    ``belief_forecast(horizon, truth=, crps=)``: k-step-ahead forecasts from every recorded step -- the sets rolled out through
    the dynamics, the predictive Gaussian mixture of each lead with its mean (returned), covariance, log score, PIT and CRPS in
    closed form -> ``last_forecast`` (``mmf_pf_predictive``).
    ``belief_maps(center, span, dims=, cells=, of=, bandwidth=, min_bandwidth=, likelihoods=, observations=)``: the recorded
    beliefs as pictures -- the 2-D marginal of that density on a grid around ``center`` (returned: ``density (T, N, Gy, Gx)``)
    for the predicted, filtered or smoothed sets and, with ``likelihoods``, every sensor's and the fused log-likelihood on the
    same grid -> ``last_maps`` (``mmf_pf_raster``).
    """

    def _init_summaries(self):
        self.last_quantiles = None    # belief_quantiles(): per-dimension weighted quantiles (and the PIT) of the recorded sets
        self.last_scores = None       # belief_scores(): CRPS, energy score and sharpness of the recorded sets against the truth
        self.last_density = None      # belief_density(): mode, log density, entropy and log score of the recorded sets
        self.last_modes = None        # belief_modes(): the modes of the recorded sets, their masses, means and members
        self.last_modalities = None   # belief_modalities(): each modality's share, evidence and own posterior on the recorded sets
        self.last_distance = None     # belief_distance(): two-sample distances between the recorded sets of two posteriors
        self.last_forecast = None     # belief_forecast(): the k-step-ahead predictive mixtures of the recorded sets, scored
        self.last_maps = None         # belief_maps(): the recorded beliefs (and the likelihoods) rasterised on a grid

    def _recorded_sets(self, of: str, who: str):
        """``(states (T, N, M, d), log_a, log_b)`` of the weighted particle sets that ``who`` (``belief_quantiles``,
        ``belief_scores``, ``belief_density``) reads: ``of="filtered"`` the history's ``states`` under ``log_weights_in + log_likelihoods``;
        ``of="smoothed"`` the history's states under ``log(weights)`` after the marginal smoother, the drawn ``trajectories``
        with no weights after backward simulation.  Everything else is the ``ValueError`` of ``who``."""
        h = self.last_history
        if of == "filtered":
            if h is None or getattr(h, "states", None) is None:
                raise ValueError(f"{who} needs a history: set record_history and run forward_loop (evaluation mode) first")
            return h.states, h.log_weights_in, h.log_likelihoods
        s = self.last_smoothed
        if s is None:
            raise ValueError(f"{who}(of='smoothed') needs a smoothed record: call smooth(method='marginal') or "
                             "smooth(method='simulation') first")
        method = getattr(s, "method", "ancestry")
        if method == "marginal":
            if h is None or getattr(h, "states", None) is None or tuple(h.states.shape[:3]) != tuple(s.weights.shape):
                raise ValueError(f"{who}(of='smoothed'): the marginal smoother's weights belong to a history that "
                                 "is no longer there: run forward_loop with record_history and smooth again")
            with torch.no_grad():
                return h.states, torch.log(s.weights), None
        if method == "simulation":
            return s.trajectories, None, None
        if method == "map":
            raise ValueError(f"{who}(of='smoothed'): smooth(method='map') leaves one path, and a path is not a "
                             "distribution: smooth with method='marginal' or 'simulation'")
        raise ValueError(f"{who}(of='smoothed'): smooth(method={method!r}) keeps no per-step weights over the "
                         "recorded sets: smooth with method='marginal' or 'simulation'")

    def _summary_inputs(self, who: str, of: str, truth, serves: str, truth_is: str = "a", required: bool = False):
        """What ``who`` (``belief_quantiles``, ``belief_scores``, ``belief_density``) opens with, in this order: the ``of``
        check, the recorded sets, the particle cap (``serves``: how the error words it) and the shape of ``truth (T, N, d)``,
        which may be ``None`` unless ``required``.  Returns ``(states, log_a, log_b, y)``, ``y`` the truth as a contiguous
        float32 tensor on the sets' device, or ``None``."""
        if of not in ("filtered", "smoothed"):
            raise ValueError(f"{who}: of must be 'filtered' or 'smoothed', got {of!r}")
        states, log_a, log_b = self._recorded_sets(of, who)
        T, N, M, d = states.shape
        if M > _abi.SUMMARY_MAX_M:
            raise ValueError(f"{who}: {M} particles per set; {serves.format(_abi.SUMMARY_MAX_M)}")
        if (required or truth is not None) and (not isinstance(truth, torch.Tensor) or tuple(truth.shape) != (T, N, d)):
            raise ValueError(f"{who}: truth must be {truth_is} (T, N, d) = ({T}, {N}, {d}) tensor, got "
                             f"{tuple(truth.shape) if isinstance(truth, torch.Tensor) else type(truth).__name__}")
        with torch.no_grad():
            y = None if truth is None else truth.detach().to(device=states.device, dtype=torch.float32).contiguous()
        return states, log_a, log_b, y

    @staticmethod
    def _positive_floats(who: str, value, name: str, or_what: str, d: int):
        """``value`` as a tuple of ``d`` positive finite floats, or the ``ValueError`` of ``who``: ``name`` must be
        ``or_what`` or ``d`` positive finite floats."""
        real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and 0.0 < float(v) < math.inf
        try:
            vs = [] if isinstance(value, (str, bytes)) else [v for v in value]
        except TypeError:
            vs = []
        if len(vs) != d or not all(real(v) for v in vs):
            raise ValueError(f"{who}: {name} must be {or_what} or {d} positive finite floats, got {value!r}")
        return tuple(float(v) for v in vs)

    @classmethod
    def _density_bandwidths(cls, who: str, bandwidth, min_bandwidth, d: int):
        """``(rule, fixed, floor)`` of the ``bandwidth`` / ``min_bandwidth`` arguments of ``who`` (``belief_density``,
        ``belief_modes``): ``"silverman"`` or ``"scott"`` with the floor (a float or ``d`` floats), or ``d`` positive finite
        floats used as they are (``rule == "fixed"``); everything else is the ``ValueError`` of ``who``."""
        floats = lambda value, name, or_what: cls._positive_floats(who, value, name, or_what, d)
        if isinstance(bandwidth, str) and bandwidth in ("silverman", "scott"):
            rule, fixed = str(bandwidth), None
        else:
            rule, fixed = "fixed", floats(bandwidth, "bandwidth", "'silverman', 'scott'")
        if not isinstance(min_bandwidth, bool) and isinstance(min_bandwidth, numbers.Real):
            min_bandwidth = (min_bandwidth,) * d
        return rule, fixed, floats(min_bandwidth, "min_bandwidth", "a positive finite float")

    def belief_scores(self, truth: torch.Tensor, *, of: str = "filtered", scale=None) -> torch.Tensor:
        """Strictly proper scores of the recorded particle sets against the true states (``mmf_pf_scores``,
        ``include/mmf.h``): the continuous ranked probability score per state dimension, ``crps (T, N, d)`` -- returned --
        and its multivariate form, the energy score ``energy (T, N)``, both ``E|X - y| - 1/2 E|X - X'|`` over the weighted
        set, the second expectation over all ``M^2`` pairs of a set in HIP.  They reward calibration and sharpness
        together, are in the state's own units and reduce to the absolute / Euclidean error for a point mass
        (``evaluation.gaussian_crps`` is the closed form of a Gaussian belief).  ``spread (T, N, d + 1)`` is the sharpness
        term ``E|X - X'|`` alone, per dimension and, last, in the Euclidean norm.
        ``truth (T, N, d)`` is required.  ``of`` means what it means for ``belief_quantiles``: ``"filtered"`` reads
        ``last_history``, ``"smoothed"`` reads ``last_smoothed`` after ``smooth(method="marginal")`` or ``"simulation"``;
        ``"ancestry"`` and ``"map"`` records are refused.  ``scale``: ``None`` or ``d`` positive finite floats dividing the
        coordinates inside the Euclidean norm (``energy`` and ``spread[..., d]`` only), for states whose dimensions have
        different units.  Leaves ``last_scores``: ``crps``, ``energy``, ``spread``, ``of``, ``scale`` (a tuple).  Draws no
        noise and leaves ``last_history`` / ``last_smoothed`` / ``last_quantiles`` as they are.  A step without a live
        particle gives NaN; a NaN component of the truth gives NaN in its ``crps`` and in ``energy``."""
        states, log_a, log_b, y = self._summary_inputs("belief_scores", of, truth, "mmf_pf_scores serves at most {}", required=True)
        T, N, M, d = states.shape
        sc = (1.0,) * d if scale is None else self._positive_floats("belief_scores", scale, "scale", "None", d)
        dev = states.device
        with torch.no_grad():
            crps = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            energy = torch.empty((T, N), dtype=torch.float32, device=dev)
            spread = torch.empty((T, N, d + 1), dtype=torch.float32, device=dev)
            _abi.pf_scores(states, log_a, log_b, y, crps, energy, spread, sc)
        self.last_scores = base.belief_record(crps=crps, energy=energy, spread=spread, of=of, scale=sc)
        return crps

    def belief_forecast(self, horizon: int, truth: Optional[torch.Tensor] = None, *, crps: bool = True) -> torch.Tensor:
        """k-step-ahead forecasts from every recorded step, scored in closed form (``mmf_pf_predictive``, ``include/mmf.h``):
        where will the state be in ``h`` steps, and how sure is the filter?  With ``T`` recorded steps, origin ``t`` and lead
        ``h`` in ``1 .. horizon``, the target is step ``t + h <= T - 1``.  The roll-out starts from the filtered sets --
        ``last_history.states[t]`` under ``log_weights_in[t] + log_likelihoods[t]``, what ``of="filtered"`` means elsewhere --
        and for ``k = 1 .. h`` propagates them noise-free under the recorded controls, ``F(k) = f(X(k-1), u_{t+k})``, one call
        of the dynamics for all ``(T - k) N`` sets (K2 for the built-in models; a user model goes through ``dyn(...)`` as in the
        smoothers, state-dependent noise refused), then adds the process noise, ``X(k) = F(k) + eps(k) L^T``, for the leads
        that follow.  The weights never change.  The forecast at lead ``h`` is the mixture ``sum_i W_i N(x; F(h)_i, L L^T)``:
        the noise of the last step is not drawn but integrated, so lead 1 draws nothing.
        Returns ``mean (H, T, N, d)``: the forecast of ``x_{t+h}`` made at ``t`` sits at ``[h - 1, t]``, NaN where ``t + h >
        T - 1`` (``horizon >= T`` is allowed: the leads beyond the data are NaN).  Leaves ``last_forecast``: ``mean``,
        ``covariance (H, T, N, d, d)`` (the process noise of the last step included), ``horizon`` and, with ``crps`` (the
        ``O(M^2)`` pair pass), ``spread (H, T, N, d)``; with ``truth (T, N, d)`` also ``error`` = ``mean - truth[t + h]``,
        ``log_score (H, T, N)``, ``pit (H, T, N, d)`` and, with ``crps``, ``crps (H, T, N, d)`` -- strictly proper scores with
        no bandwidth, where ``belief_density`` needs a kernel density estimate.
        Noise: ``eps(k)`` is ONE ``self.noise.gaussian(((T - k) N, M, d))`` draw per ``k``, in the order ``k = 1 .. H - 1``
        and only while a later lead has a target (``k < min(H, T - 1)``): ``horizon = 1`` leaves the noise stream where it
        was, a ``ReplayNoise`` holding the blocks reproduces the forecasts, and ``CounterNoise`` serves.  Memory: two sets of
        ``(T, N, M, d)`` at a time.  Evaluation mode only; ``last_history``, ``last_smoothed`` and the other records are left
        as they are.  The Kalman filters have a ``belief_forecast`` of their own; the unscented and fused filters and the LSTM
        baselines keep no history and are not reached."""
        who = "belief_forecast"
        if isinstance(horizon, bool) or not isinstance(horizon, numbers.Integral) or horizon < 1:
            raise ValueError(f"{who}: horizon must be an int >= 1, got {horizon!r}")
        if self.training:
            raise RuntimeError(f"{who}: the training (autograd) paths keep no history; call .eval() first")
        states, log_a, log_b, y = self._summary_inputs(who, "filtered", truth, "mmf_pf_predictive serves at most {}", "None or a")
        T, N, M, d = states.shape
        H, dev, controls = int(horizon), states.device, self.last_history.controls
        blank = lambda *tail: torch.full((H, T, N) + tail, math.nan, dtype=torch.float32, device=dev)
        with torch.no_grad():
            out = {"mean": blank(d), "covariance": blank(d, d)}
            if crps:
                out["spread"] = blank(d)
            if y is not None:
                out.update(log_score=blank(), pit=blank(d))
                if crps:
                    out["crps"] = blank(d)
            X = states
            for k in range(1, min(H, T - 1) + 1):
                n = T - k
                F, tril = self._transition_means(X[:n], tree_map(controls, lambda c: c[k:T]), who)
                tril = tril.detach().to(device=dev, dtype=torch.float32).contiguous()
                _abi.pf_predictive(F, None if log_a is None else log_a[:n], None if log_b is None else log_b[:n], tril,
                                   None if y is None else y[k:], **{name: buf[k - 1, :n] for name, buf in out.items()})
                if k < min(H, T - 1):
                    eps = self.noise.gaussian((n * N, M, d), like=F)
                    X = F + (eps @ tril.t()).reshape(n, N, M, d)
            if y is not None:
                out["error"] = blank(d)
                for k in range(1, min(H, T - 1) + 1):
                    out["error"][k - 1, :T - k] = out["mean"][k - 1, :T - k] - y[k:]
        self.last_forecast = base.belief_record(horizon=H, **out)
        return out["mean"]

    def belief_density(self, truth: Optional[torch.Tensor] = None, *, of: str = "filtered", bandwidth="silverman",
                       min_bandwidth=1e-6) -> torch.Tensor:
        """The kernel density estimate of the recorded particle sets (``mmf_pf_density``, ``include/mmf.h``): a Gaussian
        product kernel on the weighted set, one bandwidth per state dimension, all ``M^2`` pairs of a set in HIP.  Returns
        ``mode (T, N, d)``: per step the particle where the density is highest -- the point estimate of a multimodal belief,
        a state the filter holds, where the mean lies between the modes.  Leaves ``last_density``: ``mode``, ``mode_index
        (T, N)`` int32, ``log_density (T, N, M)`` (``-inf`` at a dead particle), ``entropy (T, N)`` -- the resubstitution
        estimate ``-sum W log p(x)``, a sharpness figure that assumes no Gaussian --, ``bandwidth (T, N, d)``, ``of``,
        ``rule`` and, with ``truth (T, N, d)``, ``log_score (T, N)``: the log density at the true state, the logarithmic
        score (its negated mean is the NLL that ``evaluation.gaussian_nll`` is for a Gaussian belief).
        ``bandwidth``: ``"silverman"`` or ``"scott"`` -- the rule of thumb per step on the weighted standard deviation of
        each dimension and the effective sample size, not below ``min_bandwidth`` (a float or ``d`` floats) -- or ``d``
        positive finite floats used as they are (``rule == "fixed"``).  ``of`` means what it means for ``belief_scores``.
        Draws no noise and leaves ``last_history`` / ``last_smoothed`` / ``last_quantiles`` / ``last_scores`` as they are.  A
        step without a live particle gives NaN and ``mode_index = -1``; a NaN component of the truth gives NaN in its
        ``log_score`` only."""
        states, log_a, log_b, y = self._summary_inputs("belief_density", of, truth, "mmf_pf_density serves at most {}", "None or a")
        T, N, M, d = states.shape
        rule, fixed, floor = self._density_bandwidths("belief_density", bandwidth, min_bandwidth, d)
        dev = states.device
        with torch.no_grad():
            log_density = torch.empty((T, N, M), dtype=torch.float32, device=dev)
            log_score = None if y is None else torch.empty((T, N), dtype=torch.float32, device=dev)
            entropy = torch.empty((T, N), dtype=torch.float32, device=dev)
            mode = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            mode_index = torch.empty((T, N), dtype=torch.int32, device=dev)
            h = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            _abi.pf_density(states, log_a, log_b, y, rule=rule, bandwidth=fixed, min_bandwidth=floor, log_density=log_density,
                            log_score=log_score, entropy=entropy, mode=mode, mode_index=mode_index, bandwidth_out=h)
        extra = {} if log_score is None else {"log_score": log_score}
        self.last_density = base.belief_record(mode=mode, mode_index=mode_index, log_density=log_density, entropy=entropy,
                                               bandwidth=h, of=of, rule=rule, **extra)
        return mode

    def belief_modes(self, of: str = "filtered", *, max_modes: int = 4, link_radius: float = 3.0, bandwidth="silverman",
                     min_bandwidth=1e-6) -> torch.Tensor:
        """The modes of the recorded particle sets (``mmf_pf_modes``, ``include/mmf.h``): how many hypotheses the belief
        holds per step, where each one is and how much probability it carries -- "the door is open with probability 0.7".
        Quick shift on the kernel density of ``belief_density``: every particle links to its nearest neighbour of higher
        density within ``link_radius`` bandwidths, the roots of that forest are the modes and a tree's weight is the mode's
        mass; all ``M^2`` pairs of a set in HIP, deterministic, nothing iterated.  Returns ``modes (T, N, K, d)``, ``K =
        max_modes`` (1 .. 8): per step the ``min(count, K)`` heaviest modes, heaviest first, each a particle of the set; ranks
        beyond ``count`` are NaN.  Leaves ``last_modes``: ``modes``, ``index (T, N, K)`` int32 (``-1`` beyond ``count``),
        ``mass (T, N, K)`` (0 beyond), ``mean (T, N, K, d)`` -- the weighted mean of each mode's members --, ``count (T, N)``
        int32, ``labels`` and ``parent (T, N, M)`` int32 (every particle's mode and link, ``-1`` at a dead particle),
        ``bandwidth (T, N, d)``, ``of``, ``rule``, ``link_radius``, ``max_modes``.
        ``of``, ``bandwidth`` and ``min_bandwidth`` mean what they mean for ``belief_density``, whose log density and
        bandwidths are computed here (``mmf_pf_density``) without touching ``last_density``.  Draws no noise and leaves every
        other ``last_*`` record as it is.  A step without a live particle has ``count = 0``."""
        states, log_a, log_b, _ = self._summary_inputs("belief_modes", of, None, "mmf_pf_modes serves at most {}")
        T, N, M, d = states.shape
        if isinstance(max_modes, bool) or not isinstance(max_modes, numbers.Integral) or not 1 <= max_modes <= _abi.MODES_MAX:
            raise ValueError(f"belief_modes: max_modes must be an integer in 1 .. {_abi.MODES_MAX}, got {max_modes!r}")
        if isinstance(link_radius, bool) or not isinstance(link_radius, numbers.Real) or not 0.0 < float(link_radius) < math.inf:
            raise ValueError(f"belief_modes: link_radius must be a positive finite float (in bandwidths), got {link_radius!r}")
        rule, fixed, floor = self._density_bandwidths("belief_modes", bandwidth, min_bandwidth, d)
        K, tau = int(max_modes), float(link_radius)
        dev = states.device
        with torch.no_grad():
            log_density = torch.empty((T, N, M), dtype=torch.float32, device=dev)
            h = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            _abi.pf_density(states, log_a, log_b, None, rule=rule, bandwidth=fixed, min_bandwidth=floor, log_density=log_density,
                            bandwidth_out=h)
            ints = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
            parent, labels, count, index = ints(T, N, M), ints(T, N, M), ints(T, N), ints(T, N, K)
            modes = torch.empty((T, N, K, d), dtype=torch.float32, device=dev)
            mass = torch.empty((T, N, K), dtype=torch.float32, device=dev)
            mean = torch.empty((T, N, K, d), dtype=torch.float32, device=dev)
            _abi.pf_modes(states, log_a, log_b, log_density, h, link_radius=tau, max_modes=K, parent=parent, labels=labels,
                          count=count, index=index, modes=modes, mass=mass, mean=mean)
        self.last_modes = base.belief_record(modes=modes, index=index, mass=mass, mean=mean, count=count, labels=labels,
                                             parent=parent, bandwidth=h, of=of, rule=rule, link_radius=tau, max_modes=K)
        return modes

    @engine.checked_loop
    def belief_maps(self, center: torch.Tensor, span, *, dims=(0, 1), cells=64, of: str = "filtered", bandwidth="silverman",
                    min_bandwidth=1e-6, likelihoods: bool = False, observations=None) -> torch.Tensor:
        """The recorded beliefs as pictures (``mmf_pf_raster``, ``include/mmf.h``): per step a grid of ``cells`` over the two
        state dimensions ``dims`` around ``center``, holding the 2-D marginal of the kernel density of ``belief_density`` --
        what shows a multimodal belief as two hills where every other summary gives numbers.  Returns ``density (T, N, Gy,
        Gx)``, x fastest, rasterised in HIP with the exact-fp32 MFMA; no ``(M, G)`` factor array is formed.
        ``center (T, N, d)``: where each step's window sits -- the truth, or the estimates ``forward_loop`` returned.
        ``span``: two positive finite floats, the window's widths along ``dims[0]`` and ``dims[1]`` in the state's units; a
        cell is ``span / cells`` wide.  ``cells``: an int or ``(Gx, Gy)``, each in 2 .. 128; with an odd count the middle
        cell's centre is ``center`` bit for bit (``evaluation.map_axes`` gives every cell's).
        ``of``: ``"filtered"`` and ``"smoothed"`` mean what they mean for ``belief_density``; ``"predicted"`` is the history's
        ``states`` under ``log_weights_in`` alone, the belief before the step's measurement -- so three calls give prior,
        likelihood and posterior on one grid.  ``bandwidth`` and ``min_bandwidth`` are ``belief_density``'s, and so are the
        bandwidths (``mmf_pf_density`` asked for nothing else: it stops after the moments): the map is the marginal of the
        density ``belief_density`` reports.
        ``likelihoods=True`` adds ``log_likelihood (T, N, K + 1, Gy, Gx)``: the measurement networks evaluated on the grid
        -- ``dims`` at the cell centres, every other dimension at ``center``'s value --, unnormalised log-likelihoods and no
        densities.  Under a ``CrossmodalParticleFilterMeasurementModel`` the ``K`` enabled unimodal maps
        (``modality_log_likelihoods``, every network in one launch) and, last, the fused ``logsumexp_k(beta_k + l_k)``, from
        the observations and ``enabled_models`` the run left in the history, as ``belief_modalities`` reads them; under any
        other measurement model one map of ``measurement_model(states=grid, observations=observations)``, ``observations (T,
        N, ...)`` then being required (given, they are read under a crossmodal model too).  Rows go in chunks within K2's
        limits, and the status word is cleared on entry and checked on the way out: a grid state that leaves the f16x3 range
        raises here.
        Leaves ``last_maps``: ``density``, ``mass (T, N)`` -- ``sum density step_x step_y``, the share of the belief inside
        the window --, ``center (T, N, 2)``, ``step``, ``dims``, ``cells``, ``span`` (tuples), ``bandwidth (T, N, 2)``, ``of``,
        ``rule`` and, with ``likelihoods``, ``log_likelihood``, ``modalities`` (the enabled models' indices; ``(0,)`` without
        a fusion) and ``log_weights (T, N, K)`` (``beta``, or ``None``).  Draws no noise and leaves every other ``last_*``
        record as it is.  Evaluation mode only.  A step without a live particle or with a NaN in ``center[..., dims]``
        gives a NaN map."""
        from .base_models import CrossmodalParticleFilterMeasurementModel  # (base_models imports this module)

        who = "belief_maps"
        if self.training:
            raise RuntimeError(f"{who}: the training (autograd) paths keep no history; call .eval() first")
        if of not in ("predicted", "filtered", "smoothed"):
            raise ValueError(f"{who}: of must be 'predicted', 'filtered' or 'smoothed', got {of!r}")
        states, log_a, log_b, _ = self._summary_inputs(who, "filtered" if of == "predicted" else of, None,
                                                       "mmf_pf_raster serves at most {}")
        if of == "predicted":
            log_b = None  # (the belief before the step's measurement)
        T, N, M, d = states.shape
        whole = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Integral)
        real = lambda v: not isinstance(v, bool) and isinstance(v, numbers.Real) and 0.0 < float(v) < math.inf
        pair = lambda v: list(v) if isinstance(v, (tuple, list)) else []
        if d < 2:
            raise ValueError(f"{who}: a map needs two state dimensions, the state has {d}")
        if len(pair(dims)) != 2 or not all(whole(k) and 0 <= k < d for k in dims) or dims[0] == dims[1]:
            raise ValueError(f"{who}: dims must be two distinct state dimensions in 0 .. {d - 1}, got {dims!r}")
        grid = (cells, cells) if whole(cells) else tuple(pair(cells))
        if len(grid) != 2 or not all(whole(g) and 2 <= g <= _abi.RASTER_MAX_CELLS for g in grid):
            raise ValueError(f"{who}: cells must be an int or (Gx, Gy), each in 2 .. {_abi.RASTER_MAX_CELLS}, got {cells!r}")
        dims, (Gx, Gy) = (int(dims[0]), int(dims[1])), (int(grid[0]), int(grid[1]))
        step = ()
        if len(pair(span)) == 2 and all(real(s) for s in span):
            step = tuple(_abi.as_float32(float(s) / g) for s, g in zip(span, (Gx, Gy)))  # (the kernel's host floats)
        if len(step) != 2 or not all(real(s) for s in step):
            raise ValueError(f"{who}: span must be two positive finite floats (with span / cells positive and finite in "
                             f"float32), got {span!r}")
        if not isinstance(center, torch.Tensor) or tuple(center.shape) != (T, N, d):
            raise ValueError(f"{who}: center must be a (T, N, d) = ({T}, {N}, {d}) tensor, got "
                             f"{tuple(center.shape) if isinstance(center, torch.Tensor) else type(center).__name__}")
        rule, fixed, floor = self._density_bandwidths(who, bandwidth, min_bandwidth, d)
        meas, obs = self.measurement_model, None
        if likelihoods:
            crossmodal = isinstance(meas, CrossmodalParticleFilterMeasurementModel)
            h = self.last_history
            obs = observations
            if crossmodal:
                recorded = getattr(h, "enabled_models", None)
                if obs is None:
                    obs = getattr(h, "observations", None)
                if recorded is not None and tuple(meas.enabled_models) != tuple(recorded):
                    raise ValueError(f"{who}: enabled_models = {list(meas.enabled_models)} now, {list(recorded)} when the history "
                                     "was recorded: the maps would be another fusion's; run forward_loop again")
            if obs is None:
                raise ValueError(f"{who}(likelihoods=True): no observations to evaluate the measurement model on: "
                                 + ("the history holds none; " if crossmodal else f"{type(meas).__name__} leaves none in the history; ")
                                 + "pass observations=, the (T, N, ...) observations of the run")
            leaves = list(obs.values()) if isinstance(obs, dict) else [obs]
            if not all(isinstance(x, torch.Tensor) and tuple(x.shape[:2]) == (T, N) for x in leaves):
                raise ValueError(f"{who}: every tensor of observations must lead with (T, N) = ({T}, {N})")
        dev = states.device
        with torch.no_grad():
            c = center.detach().to(device=dev, dtype=torch.float32).contiguous()
            c2 = c[..., list(dims)].contiguous()
            h_all = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            _abi.pf_density(states, log_a, log_b, None, rule=rule, bandwidth=fixed, min_bandwidth=floor, bandwidth_out=h_all)
            h2 = h_all[..., list(dims)].contiguous()
            density = torch.empty((T, N, Gy, Gx), dtype=torch.float32, device=dev)
            _abi.pf_raster(states, log_a, log_b, c2, h2, density, dims=dims, step=step)
            mass = (density.to(torch.float64).sum(dim=(-1, -2)) * (step[0] * step[1])).to(torch.float32)
            extra = self._likelihood_maps(c, dims, step, (Gx, Gy), obs) if likelihoods else {}
        self.last_maps = base.belief_record(density=density, mass=mass, center=c2.view(T, N, 2), step=step, dims=dims,
                                            cells=(Gx, Gy), span=(float(span[0]), float(span[1])), bandwidth=h2.view(T, N, 2),
                                            of=of, rule=rule, **extra)
        return density

    def _likelihood_maps(self, center, dims, step, cells, observations):
        """The likelihood part of ``belief_maps``: ``center (T, N, d)`` float32 on the device and ``observations (T, N, ...)``
        -> the ``log_likelihood (T, N, K + 1, Gy, Gx)``, ``modalities`` and ``log_weights`` of the record.  The grid states
        hold ``dims`` at the cell centres and every other dimension at ``center``'s value; the rows go in chunks of at most
        ``_MAP_CHUNK_STATES`` grid states, within what a K2 launch takes."""
        from .base_models import CrossmodalParticleFilterMeasurementModel  # (base_models imports this module)

        meas = self.measurement_model
        crossmodal = isinstance(meas, CrossmodalParticleFilterMeasurementModel)
        T, N, d = center.shape
        (Gx, Gy), R = cells, T * N
        u, v = map_cell_centres(center[..., list(dims)], step, cells)
        flat = tree_map(observations, lambda x: x.reshape((R,) + tuple(x.shape[2:])))
        rows = max(1, min(_abi.MEASURE_MAX_PARTICLES, _MAP_CHUNK_STATES) // (Gx * Gy))
        maps, betas, enabled = [], [], (0,)
        for r0 in range(0, R, rows):
            r1 = min(R, r0 + rows)
            g = center.reshape(R, d)[r0:r1, None, None, :].repeat(1, Gy, Gx, 1)
            g[..., dims[0]] = u.view(R, Gx)[r0:r1, None, :]
            g[..., dims[1]] = v.view(R, Gy)[r0:r1, :, None]
            g = g.view(r1 - r0, Gy * Gx, d)
            o = tree_map(flat, lambda x: x[r0:r1])
            if crossmodal:
                logliks, beta, enabled = meas.modality_log_likelihoods(g, meas.encode_observations(o))
                ll = torch.stack(logliks, dim=1)                          # (rows, K, Gy Gx)
                fused = torch.logsumexp(ll if beta is None else ll + beta[:, :, None], dim=1, keepdim=True)
                maps.append(torch.cat([ll, fused], dim=1))
                betas.append(beta)
            else:
                maps.append(meas(states=g, observations=o).to(torch.float32).reshape(r1 - r0, 1, Gy * Gx))
        K1 = maps[0].shape[1]
        return dict(log_likelihood=torch.cat(maps).view(T, N, K1, Gy, Gx), modalities=tuple(enabled),
                    log_weights=torch.cat(betas).view(T, N, K1 - 1) if betas and betas[0] is not None else None)

    @engine.checked_loop
    def belief_modalities(self) -> torch.Tensor:
        """Which sensor decided each step of the recorded run (``mmf_pf_modalities``, ``include/mmf.h``): the crossmodal
        fusion ``logsumexp_k(beta_k + l_k)`` taken apart again.  Returns ``responsibility (T, N, K)``, ``K`` the enabled
        modalities: the evidence-weighted share ``rho_k`` of modality ``k`` in the fused posterior, ``W = sum_k rho_k W^k``
        with ``W^k`` the posterior that modality alone would have left on the same particles -- not ``beta``, which a
        modality with likelihoods of larger scale overrules.  Leaves ``last_modalities``: ``responsibility``,
        ``log_evidence (T, N, K + 1)`` -- how well each sensor alone explained the observation, the fused figure last --,
        ``ess (T, N, K + 1)``, ``mean (T, N, K + 1, d)`` -- what each sensor alone would have estimated --, ``divergence
        (T, N, K)``, ``KL(W^k || W)``, ``overlap (T, N, K, K)``, the Bhattacharyya coefficient between two sensors'
        posteriors (do they agree?), ``log_likelihoods (K, T, N, M)``, the unimodal ``l_k`` themselves (likelihood maps),
        ``log_weights (T, N, K)``, ``beta`` as the weight model gave it (``None`` without one), and ``modalities``, the
        enabled models' indices.
        Reads the filtered sets of ``last_history`` (``states`` under ``log_weights_in``; ``record_history`` and
        ``forward_loop`` first) and the observations and ``enabled_models`` that run left there: the observations are encoded
        again over the ``T N`` rows and every unimodal network is evaluated on the recorded particles in one launch
        (``CrossmodalParticleFilterMeasurementModel.modality_log_likelihoods``).  There is no ``of=``: a smoothed weight is
        not a prior times a likelihood.  Needs a crossmodal measurement model with the ``enabled_models`` of the run.  The
        status word is cleared on entry and checked on the way out, as ``forward_loop`` does it, so an activation of the
        encoders or of the networks that left the f16x3 range raises here (the weights may have changed since the run).  Draws no
        noise and leaves every other ``last_*`` record as it is.  A modality without weight on any live particle has
        responsibility 0 and NaN figures; a step without a live particle gives NaN."""
        from .base_models import CrossmodalParticleFilterMeasurementModel  # (base_models imports this module)

        who = "belief_modalities"
        h = self.last_history
        if h is None or getattr(h, "states", None) is None:
            raise ValueError(f"{who} needs a history: set record_history and run forward_loop (evaluation mode) first")
        meas = self.measurement_model
        if not isinstance(meas, CrossmodalParticleFilterMeasurementModel):
            raise ValueError(f"{who} attributes the fusion of a CrossmodalParticleFilterMeasurementModel; "
                             f"{type(meas).__name__} fuses nothing")
        recorded = getattr(h, "enabled_models", None)
        if getattr(h, "observations", None) is None or recorded is None:
            raise ValueError(f"{who}: the history holds no observations: it was not left by this filter's forward_loop")
        if tuple(meas.enabled_models) != tuple(recorded):
            raise ValueError(f"{who}: enabled_models = {list(meas.enabled_models)} now, {list(recorded)} when the history was "
                             "recorded: the recorded log-likelihoods are another fusion's; run forward_loop again")
        T, N, M, d = h.states.shape
        if M > _abi.SUMMARY_MAX_M:
            raise ValueError(f"{who}: {M} particles per set; mmf_pf_modalities serves at most {_abi.SUMMARY_MAX_M}")
        R = T * N
        dev = h.states.device
        with torch.no_grad():
            ctx = meas.encode_observations(tree_map(h.observations, lambda x: x.reshape((R,) + tuple(x.shape[2:]))))
            logliks, beta, enabled = meas.modality_log_likelihoods(h.states.view(R, M, d), ctx)
            K = len(logliks)
            new = lambda *tail: torch.empty((T, N) + tail, dtype=torch.float32, device=dev)
            out = dict(responsibility=new(K), log_evidence=new(K + 1), ess=new(K + 1), mean=new(K + 1, d), divergence=new(K),
                       overlap=new(K, K))
            _abi.pf_modalities(h.states, h.log_weights_in, [l.view(T, N, M) for l in logliks],
                               None if beta is None else beta.view(T, N, K), **out)
            log_likelihoods = torch.stack(logliks).view(K, T, N, M)
        self.last_modalities = base.belief_record(log_likelihoods=log_likelihoods, log_weights=None if beta is None else beta.view(T, N, K),
                                                  modalities=enabled, **out)
        return out["responsibility"]

    def belief_distance(self, other: Optional["ParticleFilter"] = None, *, of: str = "filtered", other_of: str = "filtered",
                        scale=None) -> torch.Tensor:
        """Two-sample distances between the recorded particle sets of this filter (set A, read with ``of``) and of ``other``
        (set B, read with ``other_of``; ``None``: this filter), step by step (``mmf_pf_distance``, ``include/mmf.h``): how far
        two posteriors are apart as distributions, where the means can only be subtracted.  ``f.belief_distance(of="filtered",
        other_of="smoothed")`` after ``smooth(method="marginal")`` is how far the future moved the belief; two filters run on
        the same data with 300 and 4096 particles, two arithmetic modes or two modality masks are compared the same way.
        Returns ``wasserstein (T, N, d)``, the 1-Wasserstein (earth mover's) distance per state dimension in the state's own
        units.  Leaves ``last_distance``: ``wasserstein``, ``cramer (T, N, d)`` -- the integral of the squared CDF difference,
        which has no cancellation and resolves two posteriors that are almost the same --, ``ks (T, N, d)`` -- the
        Kolmogorov-Smirnov statistic in [0, 1] --, all three on K1's integer fixed-point weights (identical sets give exactly
        0, a step's bits do not depend on the batch); ``energy (T, N)``, the multivariate energy distance, and ``terms
        (T, N, 3)``, ``E|X - Y|, E|X - X'|, E|Y - Y'|`` in the Euclidean norm, ``energy = sqrt(max(2 terms[0] - terms[1] -
        terms[2], 0))`` -- a cancelling difference: below about 1e-3 of the sets' own spread read ``cramer``; ``of``,
        ``other_of``, ``scale`` (a tuple) and ``particles = (M_a, M_b)``.
        ``of`` and ``other_of`` mean what ``of`` means for ``belief_quantiles``.  The two sides must agree in ``(T, N, d)``;
        their particle counts need not, and together may not exceed 16384.  ``scale``: as in ``belief_scores``, for the
        norm of ``energy`` and ``terms`` only.  Draws no noise and leaves every other record of both filters as it is.  A
        step at which either side has no live particle gives NaN."""
        from .filters import ParticleFilter  # (filters imports this module)

        who = "belief_distance"
        if other is None:
            other = self
        if not isinstance(other, ParticleFilter):
            raise ValueError(f"{who}: other must be a ParticleFilter or None, got {type(other).__name__} (a Gaussian or a "
                             "point estimate has no particle set)")
        for name, value in (("of", of), ("other_of", other_of)):
            if value not in ("filtered", "smoothed"):
                raise ValueError(f"{who}: {name} must be 'filtered' or 'smoothed', got {value!r}")
        xa, la_a, lb_a = self._recorded_sets(of, who)
        xb, la_b, lb_b = other._recorded_sets(other_of, who)
        T, N, Ma, d = xa.shape
        Mb = xb.shape[2]
        if (xb.shape[0], xb.shape[1], xb.shape[3]) != (T, N, d):
            raise ValueError(f"{who}: the two sides must agree in (T, N, d): this filter's {of} sets have (T, N, d) = "
                             f"({T}, {N}, {d}), the other's {other_of} sets ({xb.shape[0]}, {xb.shape[1]}, {xb.shape[3]})")
        if xb.device != xa.device:
            raise ValueError(f"{who}: the two sides are on different devices ({xa.device}, {xb.device})")
        if Ma + Mb > _abi.DISTANCE_MAX_M:
            raise ValueError(f"{who}: {Ma} + {Mb} particles per pair of sets; mmf_pf_distance sorts at most "
                             f"{_abi.DISTANCE_MAX_M} of both sets together in LDS")
        sc = (1.0,) * d if scale is None else self._positive_floats(who, scale, "scale", "None", d)
        dev = xa.device
        with torch.no_grad():
            new = lambda *tail: torch.empty((T, N) + tail, dtype=torch.float32, device=dev)
            out = dict(wasserstein=new(d), cramer=new(d), ks=new(d), energy=new(), terms=new(3))
            _abi.pf_distance(xa, la_a, lb_a, xb, la_b, lb_b, scale=sc, **out)
        self.last_distance = base.belief_record(of=of, other_of=other_of, scale=sc, particles=(Ma, Mb), **out)
        return out["wasserstein"]

    def belief_quantiles(self, probs, *, of: str = "filtered", truth: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-dimension weighted quantiles of the recorded particle sets (``mmf_pf_quantiles``, ``include/mmf.h``): the
        non-parametric counterpart of ``record_belief``'s covariance -- median, credible intervals -- for a belief that need
        not be Gaussian.  ``probs``: 1 .. 16 floats in ``[0, 1]``.  Returns ``(T, N, Q, d)``; every value is a particle's own
        coordinate (the inverted weighted CDF on K1's integer fixed-point weights: the same bits whatever the batch).
        ``of = "filtered"``: the pre-resampling weighted set of every step of ``last_history`` (``record_history`` and
        ``forward_loop`` first) -- ``states`` under ``log_weights_in + log_likelihoods``, the set the estimate is taken from.
        ``of = "smoothed"``: the sets of ``last_smoothed`` -- after ``smooth(method="marginal")`` the history's states under
        the smoothed ``weights``; after ``smooth(method="simulation")`` the ``num_draws`` drawn ``trajectories``, equally
        weighted.  ``"ancestry"`` keeps no per-step weights and ``"map"`` is a path, not a distribution: both are refused.
        ``truth (T, N, d)``: also the probability integral transform of the true state, ``pit (T, N, d)`` -- the weighted share
        of the particles at or below it, per dimension; under a calibrated filter it is uniform on ``[0, 1]``
        (``evaluation.pit_histogram``).  Leaves ``last_quantiles``: ``probs`` (a tuple), ``quantiles``, ``of`` and, with a
        truth, ``pit``.  Draws no noise and leaves ``last_history`` / ``last_smoothed`` as they are.  A step without a live
        particle gives NaN."""
        if of not in ("filtered", "smoothed"):  # (here as well as in _summary_inputs: it goes before the probs)
            raise ValueError(f"belief_quantiles: of must be 'filtered' or 'smoothed', got {of!r}")
        try:
            ps = [p for p in probs]
        except TypeError:
            raise ValueError(f"belief_quantiles: probs must be a sequence of floats in [0, 1], got {probs!r}") from None
        if not 1 <= len(ps) <= _abi.QUANTILES_MAX:
            raise ValueError(f"belief_quantiles: probs must hold 1 .. {_abi.QUANTILES_MAX} probabilities, got {len(ps)}")
        for p in ps:
            if isinstance(p, bool) or not isinstance(p, numbers.Real) or not 0.0 <= float(p) <= 1.0:  # (a NaN fails the range)
                raise ValueError(f"belief_quantiles: probs must be floats in [0, 1], got {p!r}")
        ps = tuple(float(p) for p in ps)
        states, log_a, log_b, query = self._summary_inputs("belief_quantiles", of, truth, "mmf_pf_quantiles sorts at most {} in LDS")
        T, N, M, d = states.shape
        dev = states.device
        with torch.no_grad():
            quantiles = torch.empty((T, N, len(ps), d), dtype=torch.float32, device=dev)
            pit = None if query is None else torch.empty((T, N, d), dtype=torch.float32, device=dev)
            _abi.pf_quantiles(states, log_a, log_b, ps, quantiles, query, pit)
        extra = {} if pit is None else {"pit": pit}
        self.last_quantiles = base.belief_record(probs=ps, quantiles=quantiles, of=of, **extra)
        return quantiles

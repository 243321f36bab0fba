"""``torchfilter.filters`` on MI355X: the particle filter and the virtual-sensor EKF.

API as the reference uses it -- ``ParticleFilter(dynamics_model=, measurement_model=,
num_particles=)`` with public mutable ``num_particles`` / ``dynamics_model`` /
``measurement_model`` (``/root/reference/crossmodal/door_models/pf.py:14-27``,
``train_helpers.py:46,94``); ``VirtualSensorExtendedKalmanFilter(dynamics_model=,
virtual_sensor_model=)`` with ``_belief_mean`` / ``_belief_covariance``
(``door_models/kf.py:14-28``, ``base_models/crossmodal_kf.py:180``) -- with the recursion
itself running in hand-written HIP: ``mmf_pf_init_particles`` for the initial belief, K1
(``mmf_pf_reweight_resample``) for reweight / normalise / estimate / resample / gather, K3
(``mmf_ekf_step``) for the Kalman algebra, and the native step loops
(``mmf_pf_forward_loop`` / ``mmf_ekf_forward_loop``) behind ``forward_loop``.
Step order follows upstream torchfilter.
"""
import math
import numbers
from typing import NamedTuple, Optional

import torch

from . import _abi, base, engine
from .engine import _timed, check_range, require_device, reserve_memory, use_autograd
from .pf_smoothing import ParticleSmoothing
from .pf_summaries import ParticleSummaries
from .utils import CounterBlock, CounterNoise, NoiseSource, tree_index, tree_leading_shape, tree_map

_MODES = {"none": 0, "systematic": 1, "multinomial": 2}


def dedup_workspace_words(N: int, M: int) -> int:
    """int32 elements of the run-table workspace (``include/mmf.h``: ``mmf_pf_dedup_workspace_words``)."""
    return N * M + 2 * N * (M + 1) + N


def dedup_eligible(*, T: int, M: int, d: int, mode: int, soft_alpha: float, adaptive: bool, recording: bool = False) -> bool:
    """Whether ``forward_loop`` hands the native loop a run-table workspace: the switch, a loop long enough to have a
    step that consumes a table (``T >= 2``), no ESS-triggered resampling, and the library's own rule
    (``mmf_pf_dedup_plan``: plain systematic resampling, ``M % 64 == 0``, ``d`` 2 or 3, K1's run variant fits LDS)."""
    if not engine.PF_DEDUP or adaptive or T < 2:
        return False
    return _abi.pf_dedup_plan(M, d, mode, soft_alpha, recording)


class _StepPolicy(NamedTuple):
    """What one step does with a belief of ``M`` particles (``ParticleFilter._step_policy``)."""
    resample: bool
    mode: int                   # 1 systematic / 2 multinomial; 0 on a step that does not resample
    M_out: int                  # the particle count the step leaves
    soft: bool                  # soft_resample_alpha < 1 on a step that resamples
    threshold: Optional[float]  # resample_ess_threshold on a resampling step that keeps the count, else None


# the optional parts of one native loop (``ParticleFilter._loop_form``)
_LoopForm = NamedTuple("_LoopForm", [(part, bool) for part in ("regularise", "dedup", "history", "per_step", "persistent")])


class ParticleFilter(base.Filter, ParticleSmoothing, ParticleSummaries):
    """Bootstrap particle filter (T1).  The recursion and its switches are here; ``smooth()`` is
    ``pf_smoothing.ParticleSmoothing``, the ``belief_*`` summaries of a recorded run are ``pf_summaries.ParticleSummaries``.

    ``resample=None`` resamples iff ``not self.training`` (upstream behaviour).
    ``soft_resample_alpha < 1`` (upstream option): ancestors are drawn from the
    mixture ``alpha w + (1 - alpha) / M`` and keep the importance weights ``w / mixture``
    (``mmf_pf_reweight_resample_soft``; inside the native loop too: ``MmfPfLoopArgs.soft_alpha``).
    ``resample_mode``: ``"systematic"`` (low variance, one uniform per trajectory; what
    ``north_star`` asks for) or ``"multinomial"`` (upstream's distribution, one uniform per
    particle).  Both use the fixed-point CDF of ``csrc/pf_resample.hip``.

    ``resample_ess_threshold`` in ``(0, 1]`` (``None``: off): ESS-triggered resampling -- on a step that resamples, a
    trajectory resamples only if its effective sample size is below ``threshold * M`` (``not (ess >= float32(threshold *
    M))``: a tie keeps) and otherwise keeps its particles and carries its normalised weights forward
    (``mmf_pf_reweight_resample_adaptive`` / ``mmf_pf_forward_loop_adaptive``, the persistent launch included).  The
    step's uniforms are drawn either way, so the noise stream does not depend on the decisions.  ``last_resampled``: the
    decisions, ``bool (N,)`` after ``forward`` and ``(T, N)`` after ``forward_loop`` (``None`` while the threshold is unset).
    A step that changes the particle count resamples every trajectory.

    Belief: ``particle_states (N, M, d)``, ``particle_log_weights (N, M)``.
    ``record_belief = True``: every step also leaves the second moment of the belief it took its estimate from -- the
    pre-resampling weighted set -- in ``last_belief``: ``covariance (N, d, d)`` about the weighted mean, ``ess (N)``,
    ``log_evidence (N)`` (``include/mmf.h``, K1); after ``forward_loop`` with a leading ``T`` axis, written by the native
    loops themselves (the persistent launch included).  Training (autograd) paths compute it with detached torch ops
    from the particle tensors, step by step: correct, not fast.
    ``record_history = True`` (evaluation only; setting it on a training-mode filter raises): ``forward_loop`` keeps what a
    smoother needs in ``last_history`` (``base.history_record``: the propagated sets, log-likelihoods, incoming log-weights
    and ancestors of every step, ``4 (d + 3)`` bytes per particle-step) -- the native loop writes it in place
    (``mmf_pf_forward_loop_history``: the loop of launches; the persistent launch is skipped, as with ``record_indices``),
    the step-by-step loop stacks the same tensors.  Every other output of the loop has the same bits either way.
    ``smooth(lag, method=, num_draws=)`` and ``record_transition_moments``: ``pf_smoothing.ParticleSmoothing``.
    ``belief_quantiles`` / ``_scores`` / ``_density`` / ``_modes`` / ``_modalities`` / ``_distance`` / ``_forecast`` / ``_maps``:
    ``pf_summaries.ParticleSummaries``.
    ``keep_training_sets = True`` (training mode only; evaluation ignores it, ``record_history`` is its record there): a
    ``forward_loop`` leaves ``last_training_sets = {"states" (T, N, M, d), "log_weights" (T, N, M)}``, every step's weighted set
    -- the one its estimate is taken from, before any resampling -- as differentiable tensors, so that a loss can be put on the
    belief as a distribution (``train.particle_set_nll``, ``train.particle_set_scores``, ``train.filter_loss(loss="nll" |
    "energy" | train.crps_loss())``).  From the native recursion they
    are views of the buffers it keeps anyway and their gradients return through ``mmf_pf_train_backward_sets``; the
    step-by-step paths stack them.  Off (the default): every launch and every bit as before.
    ``regularisation`` (``None``: off, the default -- every launch and every bit as before; evaluation only, a training-mode
    step with it set raises): the REGULARISED (post-resampling) particle filter of Musso, Oudjane & Le Gland.  A float ``> 0``
    is the ``scale`` of the bandwidth, ``1.0`` the rule of thumb: on every step that resamples, each survivor of a
    trajectory that resampled is drawn from the kernel density of the pre-resampling weighted set instead of being copied,
    ``x <- x[a] + h L eps`` with ``h = scale (4 / ((d + 2) ess))^(1 / (d + 4))`` (Silverman's factor on the ESS) and ``L`` the
    Cholesky factor of K1's weighted covariance plus ``diag(regularisation_floor^2)`` (``mmf_pf_regularise``,
    ``include/mmf.h``); ``regularisation_floor`` (``0.0``; a float or ``d`` floats) gives a collapsed direction a jitter of
    its own; ``regularisation_shrink = True`` shrinks the survivors towards the weighted mean first (Liu & West), which
    leaves mean and covariance of the set unchanged.  The jitter's normals come from ``regularisation_noise``
    (``NoiseSource(1)``: a stream of its own, so ``self.noise`` does not move with the switch; a ``CounterNoise`` on stream
    ``CounterNoise.JITTER`` is generated inside the kernel by the native loop; one with the ``(seed, stream)`` of
    ``self.noise`` is a ``ValueError`` -- it would correlate the jitter with the process noise).  ``last_regularisation``:
    ``bandwidth (N,)`` after ``forward`` / ``(T, N)`` after ``forward_loop`` (0 where a trajectory kept its set, NaN where its
    ESS was not finite), ``scale``, ``floor``, ``shrink``.  Ancestors, log-weights, estimates and belief records of a step are
    K1's, unchanged; the native loop takes its loop of launches (the persistent form and the run table are not eligible:
    jittered particles have no runs).  It composes with ``record_history`` / ``record_belief`` / ``resample_ess_threshold``
    (a kept trajectory is left bit for bit) / ``soft_resample_alpha`` / ``estimation_method="argmax"`` / both resampling
    modes / a changing particle count.  The history is what it was -- the propagated sets and K1's ancestors -- and all four
    smoothers remain valid on it: the ancestry trace follows the ancestors, which still name the particle a survivor
    descends from, and the pair-based ones (marginal, simulation, MAP) judge the model's transition density between the
    recorded sets, not how a set was produced.
    Randomness comes from ``self.noise`` (``utils.NoiseSource``), never from global RNG state.
    """

    def __init__(self, *, dynamics_model: base.DynamicsModel,
                 measurement_model: base.ParticleFilterMeasurementModel,
                 num_particles: int = 100, resample: Optional[bool] = None,
                 resample_mode: str = "systematic",
                 estimation_method: str = "weighted_average", soft_resample_alpha: float = 1.0,
                 resample_ess_threshold: Optional[float] = None):
        super().__init__(state_dim=dynamics_model.state_dim)
        assert 0.0 < soft_resample_alpha <= 1.0
        self.soft_resample_alpha = soft_resample_alpha
        self.resample_ess_threshold = resample_ess_threshold
        self.last_resampled = None
        assert isinstance(dynamics_model, base.DynamicsModel)
        assert isinstance(measurement_model, base.ParticleFilterMeasurementModel)
        assert measurement_model.state_dim == self.state_dim
        assert resample_mode in ("systematic", "multinomial")
        assert estimation_method in ("weighted_average", "argmax")
        self.dynamics_model = dynamics_model
        self.measurement_model = measurement_model
        self.num_particles = num_particles
        self.resample = resample
        self.resample_mode = resample_mode
        self.estimation_method = estimation_method
        self.noise = NoiseSource(0)
        # parity certificates: with record_indices set, every step (and the native loop, per step)
        # keeps its ancestors, the log-likelihoods K2 produced and the log-weights K1 started from
        self.record_indices = False
        self.last_resample_indices = None
        self.last_log_likelihoods = None
        self.last_log_weights_in = None
        self.record_belief = False    # per-step covariance / ESS / log-evidence -> last_belief
        self.last_belief = None
        self.record_history = False   # forward_loop keeps the per-step sets / weights / ancestors -> last_history, smooth()
        self.last_history = None
        self._init_smoothing()
        self._init_summaries()
        self.keep_training_sets = False   # a train-mode forward_loop leaves every step's weighted set, differentiable -> last_training_sets
        self.last_training_sets = None
        self._step_training_set = None
        self._step_history = None
        self.use_native_loop = True   # False: forward_loop keeps the step-by-step Python loop
        self.particle_states: torch.Tensor = None
        self.particle_log_weights: torch.Tensor = None
        self._spare_states = None
        self._dedup_words = None      # int32 run-table workspace of the native loop (engine.PF_DEDUP)
        self._regularisation = None   # scale of regularised resampling (None: off) -> last_regularisation
        if engine.PF_REGULARISATION is not None:  # env MMF_PF_REGULARISATION: the scale a new filter starts with (evaluation only)
            if not 0.0 < engine.PF_REGULARISATION < math.inf:
                raise ValueError(f"MMF_PF_REGULARISATION must be a finite float > 0, got {engine.PF_REGULARISATION!r}")
            self._regularisation = engine.PF_REGULARISATION
        self._regularisation_floor = 0.0
        self.regularisation_shrink = False
        self._regularisation_noise = NoiseSource(1)
        self.last_regularisation = None
        self._initialized = False

    @property
    def resample_ess_threshold(self) -> Optional[float]:
        return self._resample_ess_threshold

    @resample_ess_threshold.setter
    def resample_ess_threshold(self, value: Optional[float]) -> None:
        assert value is None or 0.0 < float(value) <= 1.0, "resample_ess_threshold must lie in (0, 1]"  # (a NaN fails too)
        self._resample_ess_threshold = None if value is None else float(value)

    @property
    def regularisation(self) -> Optional[float]:
        return self._regularisation

    @regularisation.setter
    def regularisation(self, value: Optional[float]) -> None:
        if value is not None:
            if isinstance(value, bool) or not isinstance(value, numbers.Real) or not (0.0 < float(value) < math.inf):
                raise ValueError(f"regularisation must be None or a finite float > 0 (the bandwidth's scale), got {value!r}")
            if self.training:
                raise RuntimeError("regularisation: the training (autograd) paths do not jitter; call .eval() first")
        self._regularisation = None if value is None else float(value)

    @property
    def regularisation_floor(self):
        return self._regularisation_floor

    @regularisation_floor.setter
    def regularisation_floor(self, value) -> None:
        _abi.regularise_floor(value, self.state_dim)  # a float or d floats, finite and >= 0; otherwise a ValueError
        self._regularisation_floor = float(value) if isinstance(value, numbers.Real) else tuple(float(v) for v in value)

    @property
    def regularisation_noise(self) -> NoiseSource:
        return self._regularisation_noise

    @regularisation_noise.setter
    def regularisation_noise(self, value: NoiseSource) -> None:
        self._check_regularisation_noise(value)
        self._regularisation_noise = value

    def _check_regularisation_noise(self, source=None) -> None:
        """A counter source of the jitter must not be the process noise's: the same ``(seed, stream)`` draws the same normals
        for particle ``m`` of step ``t`` twice."""
        source = self._regularisation_noise if source is None else source
        main = getattr(self, "noise", None)
        if (isinstance(source, CounterNoise) and isinstance(main, CounterNoise)
                and (source.seed, source.stream) == (main.seed, main.stream)):
            raise ValueError(f"regularisation_noise shares (seed, stream) = ({source.seed}, {source.stream}) with the filter's "
                             "noise: the jitter would repeat the process noise (use stream=CounterNoise.JITTER or another seed)")

    def _regularisation_args(self):
        """``None`` while the switch is off; otherwise ``(scale, floor as d floats, shrink)``, checked."""
        if self._regularisation is None:
            return None
        if self.training:
            raise RuntimeError("regularisation: the training (autograd) paths do not jitter; call .eval() first")
        self._check_regularisation_noise()
        return self._regularisation, _abi.regularise_floor(self._regularisation_floor, self.state_dim), bool(self.regularisation_shrink)

    @property
    def record_history(self) -> bool:
        return self._record_history

    @record_history.setter
    def record_history(self, value: bool) -> None:
        if value and self.training:
            raise RuntimeError("record_history: the training (autograd) paths keep no history; call .eval() first")
        self._record_history = bool(value)

    # ------------------------------------------------------------------ belief
    def initialize_beliefs(self, *, mean: torch.Tensor, covariance: torch.Tensor) -> None:
        N, d = mean.shape
        assert d == self.state_dim
        assert covariance.shape == (N, d, d)
        require_device(mean, "ParticleFilter.initialize_beliefs")
        M = self.num_particles
        eps = self.noise.gaussian((N, M, d), like=mean)
        if use_autograd(self) and (mean.requires_grad or covariance.requires_grad):
            # differentiable initialisation (training): torch ops
            L = torch.linalg.cholesky(covariance.to(torch.float32))
            self.particle_states = (mean[:, None, :] + torch.einsum("nij,nmj->nmi", L, eps)).contiguous()
            self.particle_log_weights = mean.new_full((N, M), -math.log(M))
        else:
            states = torch.empty((N, M, d), dtype=torch.float32, device=mean.device)
            logw = torch.empty((N, M), dtype=torch.float32, device=mean.device)
            not_pd = torch.zeros(1, dtype=torch.int32, device=mean.device)
            _abi.pf_init_particles(mean.detach().to(torch.float32).contiguous(),
                                   covariance.detach().to(torch.float32).contiguous(),
                                   eps.to(torch.float32).contiguous(), states, logw, not_pd)
            if engine.is_capturing():  # no host read inside a hipGraph capture: FLAG_NOT_PD in the status word, read after the replay
                engine.range_flag(mean.device).bitwise_or_(not_pd.ne(0).to(torch.int32) * _abi.FLAG_NOT_PD)
            elif int(not_pd.item()):
                raise ValueError("initialize_beliefs: covariance is not positive definite")
            self.particle_states, self.particle_log_weights = states, logw
        self._spare_states = None
        self._initialized = True

    def reserve(self, *, steps: int, batch: int, particles: int = None) -> int:
        """Plan memory for ``forward_loop`` over ``steps`` x ``batch`` trajectories: grows the
        allocator once so the loop itself never calls ``hipMalloc``.  Returns the bytes reserved."""
        M = self.num_particles if particles is None else particles
        d = self.state_dim
        dev = next(self.parameters()).device
        per_row = 64 * 4 * 12               # encoder contexts, image features, program outputs
        per_step = batch * M * 4 * (2 * d + 4)  # particle ping-pong, log-weights, log-lik, noise views
        # the image-encoder workspace is persistent: create it now, outside the reserved block
        if steps * batch > 0:
            engine._image_workspace(dev, min(steps * batch, engine._IMAGE_CHUNK), 2)
        # 8 steps' worth of particle buffers: initialize_beliefs() builds the new belief while the
        # previous run's belief and scratch are still alive (measured: 4x left the first loop at
        # a new length one 12 MB segment short = one stream-draining hipMalloc)
        # the run table of the native loop (engine.PF_DEDUP): rank (N, M), run_anc / run_start (N, M + 1), n_runs (N), int32
        per_step += 4 * dedup_workspace_words(batch, M)
        nbytes = steps * batch * per_row + 8 * per_step + (64 << 20)
        if self.record_history:  # states, log-likelihoods, incoming log-weights, ancestors of every step
            nbytes += steps * batch * M * 4 * (d + 3)
        if self._regularisation is not None:  # the jitter's (T, N, M, d) normals (a counter source on the jitter stream has none)
            nbytes += steps * batch * M * 4 * d
        reserve_memory(dev, nbytes)
        return nbytes

    def _adapt_particle_count(self) -> None:
        """Upstream torchfilter's particle-count adaptation for steps that do not resample
        (the reference flips 30 <-> 300 in ``train()``,
        ``/root/reference/crossmodal/door_models/pf.py:24-27``, so a train-mode step right after
        an eval-mode belief lands here): the first ``(M_new // M) * M`` slots are whole copies of
        the particle set, the rest a sample without replacement (one permutation shared by the
        batch -- drawn from ``self.noise``: the arg-sort of ``M`` uniforms -- where upstream calls
        ``torch.randperm``); log-weights are gathered alongside and re-normalised."""
        N, M, d = self.particle_states.shape
        Mo = int(self.num_particles)
        dev = self.particle_states.device
        copies = (Mo // M) * M
        parts = []
        if copies > 0:
            parts.append(torch.arange(M, device=dev).repeat(copies // M))
        if Mo - copies > 0:
            perm = torch.argsort(self.noise.uniform((M,), like=self.particle_states), stable=True)
            parts.append(perm[:Mo - copies])
        idx = torch.cat(parts)[None, :].expand(N, Mo)
        self.particle_states = torch.gather(self.particle_states, 1, idx[:, :, None].expand(N, Mo, d)).contiguous()
        lw = torch.gather(self.particle_log_weights, 1, idx)
        self.particle_log_weights = (lw - torch.logsumexp(lw, dim=1, keepdim=True)).contiguous()
        self._spare_states = None

    # ------------------------------------------------------------------ one step
    def _step_policy(self, M: int) -> _StepPolicy:
        """What a step does with a belief of ``M`` particles; the one place the switches are read for it.  A step that
        changes the particle count resamples everybody: the threshold is dropped."""
        resample = (not self.training) if self.resample is None else bool(self.resample)
        M_out, thr = int(self.num_particles), self.resample_ess_threshold
        return _StepPolicy(resample=resample, mode=_MODES[self.resample_mode] if resample else 0, M_out=M_out,
                           soft=resample and self.soft_resample_alpha < 1.0,
                           threshold=thr if resample and M_out == M else None)

    def _adapt_unless_resampling(self, policy: _StepPolicy, M: int):
        """A step that does not resample takes the belief to ``num_particles`` first -> the belief's ``(N, M, d)`` after that."""
        if not policy.resample and policy.M_out != M:
            self._adapt_particle_count()
        return self.particle_states.shape

    def _k1(self, *tensors_and_mode, threshold=None, resampled=None, **record):
        """K1 (``loglik, logw_in, states, u, estimate, out, logw_out, idx, mode``) through the wrapper, and so the C symbol, of
        this combination: a ``threshold`` (``_StepPolicy.threshold``) -> ``mmf_pf_reweight_resample_adaptive``; a ``record``
        (``cov=``, ``ess=``, ``log_evidence=``: the belief record or the jitter's scratch) -> ``_belief``; neither -> the plain one."""
        alpha = self.soft_resample_alpha if tensors_and_mode[-1] != 0 else 1.0
        if threshold is not None:
            _abi.pf_reweight_resample_adaptive(*tensors_and_mode, alpha, ess_threshold=threshold, resampled=resampled, **record)
        elif record:
            _abi.pf_reweight_resample_belief(*tensors_and_mode, alpha, **record)
        else:
            _abi.pf_reweight_resample(*tensors_and_mode, alpha)

    def _propagate(self, controls, ctrl_ctx, N, M, d):
        eps = self.noise.gaussian((N, M, d), like=self.particle_states)
        dyn = self.dynamics_model
        if hasattr(dyn, "propagate_encoded"):
            if ctrl_ctx is None:
                ctrl_ctx = dyn.encode_controls(controls)
            spare = self._spare_states
            if spare is not None and spare.shape != self.particle_states.shape:
                spare = None
            return dyn.propagate_encoded(self.particle_states, ctrl_ctx, eps, out=spare)
        # generic user model (torch ops on the device): same control for a trajectory's particles
        flat = self.particle_states.reshape(N * M, d)
        rep = tree_map(controls, lambda t: torch.repeat_interleave(t, repeats=M, dim=0))
        pred, tril = dyn(initial_states=flat, controls=rep)
        return (pred + torch.einsum("rij,rj->ri", tril, eps.reshape(N * M, d))).reshape(N, M, d).contiguous()

    def _measure(self, states, observations, obs_ctx):
        meas = self.measurement_model
        if hasattr(meas, "forward_encoded"):
            if obs_ctx is None:
                obs_ctx = meas.encode_observations(observations)
            return meas.forward_encoded(states, obs_ctx)
        return meas(states=states, observations=observations).to(torch.float32).contiguous()

    def _step(self, observations, controls, obs_ctx=None, ctrl_ctx=None) -> torch.Tensor:
        assert self._initialized, "Particle filter not initialized!"
        reg = self._regularisation_args()  # (raises on a training-mode filter, before anything is drawn or launched)
        M = self.particle_states.shape[1]
        policy = self._step_policy(M)
        if self.record_history and not policy.resample and policy.M_out != M:
            # (the adapted set is a re-indexing of the belief that no ancestor array records)
            raise RuntimeError("record_history: a step that adapts the particle count without resampling keeps no ancestry")
        N, M, d = self._adapt_unless_resampling(policy, M)

        self.last_regularisation = None
        with torch.no_grad():
            states = self._propagate(controls, ctrl_ctx, N, M, d)
            loglik = self._measure(states, observations, obs_ctx)
            assert loglik.shape == (N, M)
            if self.record_indices:
                self.last_log_likelihoods, self.last_log_weights_in = loglik, self.particle_log_weights
            keep_history = self.record_history
            lw_before = self.particle_log_weights

            estimate = torch.empty((N, d), dtype=torch.float32, device=states.device)
            rec = self._new_belief_record((N,), d, states.device) if self.record_belief else None
            rk = {} if rec is None else dict(cov=rec.covariance, ess=rec.ess, log_evidence=rec.log_evidence)
            # the decisions of this step: nobody on a step that does not resample, everybody where the particle count changes
            self.last_resampled = None if self.resample_ess_threshold is None else torch.full(
                (N,), policy.resample, dtype=torch.bool, device=states.device)
            if policy.resample:
                Mo, mode, thr = policy.M_out, policy.mode, policy.threshold
                u = self.noise.uniform((N,) if mode == 1 else (N, Mo), like=states)
                # two buffers ping-pong: dynamics wrote `states`; the old belief is free again
                out = self.particle_states
                if out.shape != (N, Mo, d) or out.data_ptr() == states.data_ptr():
                    out = torch.empty((N, Mo, d), dtype=torch.float32, device=states.device)
                logw_out = torch.empty((N, Mo), dtype=torch.float32, device=states.device)
                idx = (torch.empty((N, Mo), dtype=torch.int32, device=states.device)
                       if self.record_indices or keep_history else None)
                lw_in = self.particle_log_weights
                if reg is not None and rec is None:  # the jitter reads K1's covariance and ESS: the recording form, into scratch
                    rk = dict(cov=torch.empty((N, d, d), dtype=torch.float32, device=states.device),
                              ess=torch.empty((N,), dtype=torch.float32, device=states.device))
                took = torch.empty((N,), dtype=torch.int32, device=states.device) if thr is not None else None
                _timed("pf_reweight_resample", 0.0, N * M * 4.0 * (2 + d) + N * Mo * 4.0 * d, lambda: self._k1(
                    loglik, lw_in, states, u, estimate, out, logw_out, idx, mode, threshold=thr, resampled=took, **rk))
                if took is not None:
                    self.last_resampled = took.ne(0)
                if reg is not None:  # `estimate` is still K1's weighted mean here (argmax replaces it below)
                    scale, floor, shrink = reg
                    h = torch.empty((N,), dtype=torch.float32, device=states.device)
                    eps_j = self._regularisation_noise.gaussian((N, Mo, d), like=states)
                    _timed("pf_regularise", 0.0, N * Mo * 4.0 * 3 * d, lambda: _abi.pf_regularise(
                        out, rk["cov"], rk["ess"], scale=scale, floor=floor, shrink=shrink, mean=estimate,
                        resampled=took, noise=eps_j, bandwidth=h))
                    self.last_regularisation = base.belief_record(bandwidth=h, scale=scale, floor=tuple(floor), shrink=shrink)
                # (the history keeps `states`: it must not come back as the next step's output buffer)
                self._spare_states = None if keep_history else states
                self.last_resample_indices = idx if self.record_indices else None
                self._step_history = (states, loglik, lw_before, idx) if keep_history else None
            else:
                self._step_history = (states, loglik, lw_before, None) if keep_history else None
                out, logw_out = states, torch.empty_like(loglik)
                if keep_history:
                    self._spare_states = None  # the old belief is a slice of the history: the next step gets a new buffer
                elif states.data_ptr() != self.particle_states.data_ptr():
                    self._spare_states = self.particle_states  # the old belief is the next scratch
                self._k1(loglik, self.particle_log_weights, states, None, estimate, None, logw_out, None, 0, **rk)
            self.last_belief = rec
            if self.estimation_method == "argmax":
                # arg-max of the *pre-resampling* normalised weights
                tot = self.particle_log_weights + loglik
                best = torch.argmax(tot, dim=1)
                estimate = states[torch.arange(N, device=states.device), best]
            self.particle_states = out
            self.particle_log_weights = logw_out
        return estimate

    @staticmethod
    def _new_belief_record(lead, d, device):
        E = lambda *shape: torch.empty(tuple(lead) + shape, dtype=torch.float32, device=device)
        return base.belief_record(covariance=E(d, d), ess=E(), log_evidence=E())

    @staticmethod
    def _belief_record_torch(states, logw_in, loglik):
        """The belief record from the particle tensors with detached torch ops in fp64 (the training paths)."""
        with torch.no_grad():
            a = (logw_in + loglik).detach().double()
            lev = torch.logsumexp(a, dim=1)
            w = torch.exp(a - lev[:, None])
            x = states.detach().double()
            dx = x - torch.sum(w[:, :, None] * x, dim=1, keepdim=True)
            cov = torch.einsum("nm,nmi,nmj->nij", w, dx, dx)
            return base.belief_record(covariance=cov.float(), ess=(1.0 / torch.sum(w * w, dim=1)).float(),
                                      log_evidence=lev.float())

    def _step_autograd(self, observations, controls, dyn_bias=None, meas_ctx=None) -> torch.Tensor:
        """Differentiable torch formulation of the step (training backend "autograd"): gradients
        flow through the reparameterised noise and the log-weights; resampling, when requested,
        runs through K1 on detached tensors (it stops gradients upstream as well)."""
        assert self._initialized, "Particle filter not initialized!"
        if self._regularisation is not None:
            raise RuntimeError("regularisation: the training (autograd) paths do not jitter; call .eval() first")
        M = self.particle_states.shape[1]
        policy = self._step_policy(M)
        N, M, d = self._adapt_unless_resampling(policy, M)
        if engine.use_hip_backward() and hasattr(self.dynamics_model, "forward_particles"):
            # K6: the N*M-row network evaluates and differentiates in HIP
            pred = self.dynamics_model.forward_particles(states=self.particle_states, controls=controls,
                                                         bias=dyn_bias)
            eps = self.noise.gaussian((N, M, d), like=pred)
            states = pred + eps @ self.dynamics_model.scale_tril().t()
        else:
            flat = self.particle_states.reshape(N * M, d)
            rep = tree_map(controls, lambda t: torch.repeat_interleave(t, repeats=M, dim=0))
            pred, tril = self.dynamics_model(initial_states=flat, controls=rep)
            eps = self.noise.gaussian((N, M, d), like=pred).reshape(N * M, d)
            states = (pred + torch.einsum("rij,rj->ri", tril, eps)).reshape(N, M, d)
        if meas_ctx is not None:
            loglik = self.measurement_model.forward_encoded_autograd(states, meas_ctx)
        else:
            loglik = self.measurement_model(states=states, observations=observations)
        self.last_belief = (self._belief_record_torch(states, self.particle_log_weights, loglik)
                            if self.record_belief else None)
        if engine.use_hip_backward() and self.estimation_method == "weighted_average":
            # K6: reweight + normalise + estimate forward (K1 mode 0) and backward in HIP
            estimate, logw = engine.ReweightEstimateFunction.apply(loglik, self.particle_log_weights, states)
        else:
            logw = self.particle_log_weights + loglik
            logw = logw - torch.logsumexp(logw, dim=1, keepdim=True)
            if self.estimation_method == "weighted_average":
                estimate = torch.sum(torch.exp(logw)[:, :, None] * states, dim=1)
            else:
                estimate = states[torch.arange(N, device=states.device), torch.argmax(logw, dim=1)]
        self.particle_states, self.particle_log_weights = states, logw
        self._step_training_set = (states, logw) if self.keep_training_sets else None  # (before any resampling)
        self.last_resampled = (None if self.resample_ess_threshold is None else
                               torch.full((N,), policy.resample, dtype=torch.bool, device=states.device))
        if policy.resample:
            Mo, mode, soft, thr = policy.M_out, policy.mode, policy.soft, policy.threshold
            u = self.noise.uniform((N,) if mode == 1 else (N, Mo), like=states)
            out = torch.empty((N, Mo, d), dtype=torch.float32, device=states.device)
            logw_out = torch.empty((N, Mo), dtype=torch.float32, device=states.device)
            scratch = torch.empty((N, d), dtype=torch.float32, device=states.device)
            idx = torch.empty((N, Mo), dtype=torch.int32, device=states.device) if soft else None
            adaptive = thr is not None
            with torch.no_grad():
                # (with a threshold K1 supplies the ancestors and the decisions: the ESS of the normalised weights)
                took = torch.empty((N,), dtype=torch.int32, device=states.device) if adaptive else None
                self._k1(torch.zeros_like(logw), logw.detach().contiguous(), states.detach().contiguous(), u, scratch, out,
                         logw_out, idx, mode, threshold=thr, resampled=took)
                if adaptive:
                    self.last_resampled = took.ne(0)
            if soft:
                # upstream's soft resampling is differentiable: the ancestors come from K1, the
                # survivors' states and importance weights are re-derived with torch ops so that
                # gradients reach the pre-resampling weights and particles
                a = self.soft_resample_alpha
                gi = idx.long()
                mix = torch.logaddexp(logw + math.log(a), torch.full_like(logw, math.log((1.0 - a) / M)))
                new = torch.gather(logw - mix, 1, gi)
                out = torch.gather(states, 1, gi[:, :, None].expand(N, Mo, d))
                logw_out = new - torch.logsumexp(new, dim=1, keepdim=True)
            if adaptive:
                # per trajectory: a kept one is the no-resample step's belief, gradients through its weights included
                # (soft: its identity ancestors make `out` the same rows already; the weights are the ones to select)
                took = self.last_resampled
                out = torch.where(took[:, None, None], out, states)
                logw_out = torch.where(took[:, None], logw_out, logw)
            self.particle_states, self.particle_log_weights = out, logw_out
        return estimate

    # ------------------------------------------------------------------ the native loop
    def _loop_form(self, policy: _StepPolicy, reg, timer, T, N, M, d, nets) -> _LoopForm:
        """Which optional parts this run has: what ``pf_enqueue_steps`` and the five ``mmf_pf_forward_loop*`` entries
        (``csrc/pf_loop.hip``) decide from the same arguments.  ``regularise``: one jitter launch after every K1 of a loop
        that resamples, and no run table (jittered particles have no runs).  ``dedup``: the run-table workspace, the dynamics
        network once per distinct resampled ancestor (``dedup_eligible``).  ``history`` / ``per_step``: the per-step arrays of
        ``record_history`` / ``record_indices``, which only the loop of launches writes.  ``persistent``: a small problem as
        ONE launch for all T steps (``csrc/pf_persistent.inc``), same bits; a threshold or ``record_belief`` does not bar it."""
        dyn = self.dynamics_model
        history = bool(self.record_history)
        regularise = reg is not None and policy.resample
        alpha = _abi.as_float32(self.soft_resample_alpha) if policy.soft else 0.0  # (MmfPfLoopArgs.soft_alpha)
        dedup = not regularise and dedup_eligible(T=T, M=M, d=d, mode=policy.mode, soft_alpha=alpha,
                                                  adaptive=policy.threshold is not None, recording=self.record_belief)
        persistent = bool(engine.PF_PERSISTENT and policy.mode == 1 and timer is None and not self.record_indices
                          and not history and not regularise and alpha == 0.0 and self.estimation_method != "argmax"
                          and d in (2, 3) and dyn._net.n_res == 3 and all(net.n_res == 2 for net, _b, _l in nets)
                          and _abi.pf_persistent_plan(N, M, len(nets)) > 0)
        return _LoopForm(regularise=regularise, dedup=dedup, history=history, per_step=bool(self.record_indices) or history,
                         persistent=persistent)

    def _loop_args(self, policy: _StepPolicy, T, N, nets, logw_stride, ctrl_all):
        """The always-present fields of ``MmfPfLoopArgs``, the steps' noise (drawn here) among them -> ``(a, est, (states_a,
        states_b, logw_a, logw_b), keep)``; ``keep`` holds what only the struct points to until the launches are enqueued."""
        dyn, like, mode = self.dynamics_model, self.particle_states, policy.mode
        _, M, d = like.shape
        u_shape = None if mode == 0 else ((N,) if mode == 1 else (N, M))
        eps, u = self.noise.draw_steps(T, (N, M, d), u_shape, like=like)
        if isinstance(eps, CounterBlock) and eps.stream != 0:  # the dynamics kernel generates stream 0 only
            eps = eps.tensor(like=like)
        dev = like.device
        states_a = like.contiguous()
        states_b = self._spare_states if (self._spare_states is not None and self._spare_states.shape == states_a.shape
                                          and self._spare_states.data_ptr() != states_a.data_ptr()) else torch.empty_like(states_a)
        logw_a = self.particle_log_weights.contiguous()
        logw_b = torch.empty_like(logw_a)
        loglik = torch.empty_like(logw_a)
        est = torch.empty((T, N, d), dtype=torch.float32, device=dev)
        tril = dyn.scale_tril().contiguous()
        keep = [nets, eps, u, tril, loglik]
        P = _abi.vp
        a = _abi.MmfPfLoopArgs()
        a.T, a.N, a.M, a.d, a.n_meas, a.resample_mode = T, N, M, d, len(nets), mode
        a.precision = dyn._net.precision_code()
        a.n_res_dyn, a.n_res_meas, a.logw_stride = dyn._net.n_res, nets[0][0].n_res, logw_stride
        a.dyn_packed, a.dyn_bias = P(dyn._net.blob()), P(ctrl_all["bias"])
        for k, (net, bias, lw) in enumerate(nets):
            a.meas_packed[k], a.meas_bias[k], a.meas_logw[k] = P(net.blob()), P(bias), P(lw)
        if isinstance(eps, CounterBlock):   # counter-based noise: generated inside the dynamics kernel
            a.noise, a.noise_mode = None, 2
            a.noise_seed, a.noise_step0, a.noise_traj0 = eps.seed, eps.step0, eps.traj0
        else:
            a.noise = P(eps)
        a.scale_tril, a.uniforms = P(tril), P(u)
        a.states_a, a.states_b, a.logw_a, a.logw_b = P(states_a), P(states_b), P(logw_a), P(logw_b)
        a.loglik, a.estimates = P(loglik), P(est)
        a.range_flag = P(engine.range_flag(dev), torch.int32)
        if policy.soft:
            a.soft_alpha = float(self.soft_resample_alpha)  # survivors carry importance weights (mmf_pf_reweight_resample_soft)
        if self.estimation_method == "argmax":
            est_scratch = torch.empty((N, d), dtype=torch.float32, device=dev)
            keep.append(est_scratch)
            a.estimate_argmax, a.estimate_scratch = 1, P(est_scratch)
        return a, est, (states_a, states_b, logw_a, logw_b), keep

    def _loop_records(self, a, keep, form: _LoopForm, policy: _StepPolicy, T, states_a, logw_a):
        """The optional records, allocated and attached to ``a``: per-step log-likelihoods and ancestors, the history, the
        belief records, the decisions of ESS-triggered resampling -> ``(hist, history, took)``, ``None`` where there is none."""
        N, M, d = states_a.shape
        dev, P = states_a.device, _abi.vp
        history = hist = None
        if form.per_step:
            ll_steps = torch.empty((T, N, M), dtype=torch.float32, device=dev)
            idx_steps = torch.empty((T, N, M), dtype=torch.int32, device=dev) if policy.mode != 0 else None
            a.loglik_steps, a.indices_steps = P(ll_steps), P(idx_steps, torch.int32)
            if self.record_indices:
                self.last_log_weights_in = logw_a.clone()
                self.last_log_likelihoods = ll_steps
                if policy.mode != 0:
                    self.last_resample_indices = idx_steps
            if form.history:  # the loop writes the propagated sets and the incoming log-weights in place
                hist = base.history_record(states=torch.empty((T, N, M, d), dtype=torch.float32, device=dev),
                                           log_likelihoods=ll_steps,
                                           log_weights_in=torch.empty((T, N, M), dtype=torch.float32, device=dev),
                                           ancestors=idx_steps, resampled=None)
                logw_in0 = torch.empty_like(logw_a)
                keep.append(logw_in0)
                history = _abi.MmfPfHistory()
                history.states_steps, history.logw_in_steps, history.logw_in0 = P(hist.states), P(hist.log_weights_in), P(logw_in0)
        self.last_belief = None
        if self.record_belief:  # written by K1 in every form of the loop; does not change which form runs
            self.last_belief = rec = self._new_belief_record((T, N), d, dev)
            a.cov_steps, a.ess_steps, a.log_evidence_steps = P(rec.covariance), P(rec.ess), P(rec.log_evidence)
        # (only steps that resample have a decision to take)
        took = torch.empty((T, N), dtype=torch.int32, device=dev) if policy.threshold is not None else None
        return hist, history, took

    def _loop_regularise(self, reg, T, like, keep):
        """``MmfPfLoopRegularise`` from ``reg`` (``_regularisation_args``): the jitter normals (drawn here, after the process
        noise), K1's scratch where no belief record takes its covariance and ESS, the bandwidths -> ``last_regularisation``."""
        scale, floor, shrink = reg
        N, M, d = like.shape
        dev, P = like.device, _abi.vp
        regularise = _abi.MmfPfLoopRegularise()
        regularise.scale, regularise.shrink = scale, int(shrink)
        for i, v in enumerate(floor):
            regularise.floor[i] = v
        eps_j, _ = self._regularisation_noise.draw_steps(T, (N, M, d), None, like=like)  # the steps' draws, in their order
        if isinstance(eps_j, CounterBlock) and eps_j.stream != CounterNoise.JITTER:  # the kernel generates the jitter stream
            eps_j = eps_j.tensor(like=like)
        if isinstance(eps_j, CounterBlock):
            regularise.noise_mode = 2
            regularise.noise_seed, regularise.noise_step0, regularise.noise_traj0 = eps_j.seed, eps_j.step0, eps_j.traj0
        else:
            regularise.noise = P(eps_j)
        h_steps = torch.empty((T, N), dtype=torch.float32, device=dev)
        scratch = [None if self.record_belief else torch.empty((N, d, d), dtype=torch.float32, device=dev),
                   None if self.record_belief else torch.empty((N,), dtype=torch.float32, device=dev)]
        regularise.cov, regularise.ess = P(scratch[0]), P(scratch[1])
        regularise.bandwidth_steps = P(h_steps)
        keep += [eps_j, scratch]
        self.last_regularisation = base.belief_record(bandwidth=h_steps, scale=scale, floor=tuple(floor), shrink=shrink)
        return regularise

    def _loop_dedup(self, N, M, dev):
        """The run-table workspace of the native loop (``engine.PF_DEDUP``), kept on the filter from one loop to the next."""
        words = dedup_workspace_words(N, M)
        if self._dedup_words is None or self._dedup_words.numel() != words or self._dedup_words.device != dev:
            self._dedup_words = torch.empty(words, dtype=torch.int32, device=dev)
        return _abi.pf_dedup_workspace(self._dedup_words, N, M)

    def _loop_timing(self, timer, T, N, M, d, nets):
        """The kernel timer's side: ``(events, stride, file)``, the events ``pf_loop.hip`` records around the launches of
        every ``stride``-th step and ``file()``, which hands them to the timer with the kernels' names and work afterwards."""
        if timer is None:
            return None, 1, lambda: None
        dyn = self.dynamics_model
        names = ["particle_net_dynamics"] + ["particle_net_measure"] * len(nets) + ["pf_reweight_resample"]
        stride = max(1, int(timer.loop_stride))
        events = timer.loop_events(2 * len(names) * len(range(stride // 2, T, stride)))  # pf_loop.hip samples t % stride == stride // 2
        R = N * M
        work = [(2.0 * R * engine.particle_net_macs(d, dyn._net.n_res, dyn._net.n_out), R * 4.0 * 3 * d)]
        work += [(2.0 * R * engine.particle_net_macs(d, net.n_res, net.n_out), R * 4.0 * (d + 1 + (k > 0)))
                 for k, (net, _, _) in enumerate(nets)]
        work.append((0.0, R * 4.0 * (2 + 2 * d)))
        return events, stride, lambda: timer.add_loop_records(names, work, events)

    def _native_loop(self, obs_all, ctrl_all, T, N):
        """All ``T`` steps through ``mmf_pf_forward_loop`` (one C call, no per-step Python) when
        both models are fused networks; ``None`` -> the caller runs the step-by-step loop."""
        dyn, meas = self.dynamics_model, self.measurement_model
        if obs_all is None or ctrl_all is None or not hasattr(dyn, "_net") or not hasattr(meas, "fused_measurements"):
            return None
        if not self.use_native_loop:
            return None
        plan = meas.fused_measurements(obs_all)
        if plan is None or T == 0:
            return None
        nets, logw_stride = plan
        Nb, M, d = self.particle_states.shape
        policy = self._step_policy(M)
        if Nb != N or policy.M_out != M or len(nets) > _abi.LOOP_MAX_MEAS:
            return None
        assert self._initialized, "Particle filter not initialized!"
        like = self.particle_states
        reg = self._regularisation_args()  # (raises before anything is drawn or launched)
        self.last_regularisation = None
        timer = engine.kernel_timer()
        form = self._loop_form(policy, reg, timer, T, N, M, d, nets)
        a, est, (states_a, states_b, logw_a, logw_b), keep = self._loop_args(policy, T, N, nets, logw_stride, ctrl_all)
        hist, history, took = self._loop_records(a, keep, form, policy, T, states_a, logw_a)
        regularise = self._loop_regularise(reg, T, like, keep) if form.regularise else None
        dedup = self._loop_dedup(N, M, like.device) if form.dedup else None
        events, stride, file_timer_records = self._loop_timing(timer, T, N, M, d, nets)
        # the persistent launch needs ALL its workgroups resident; if it gives up (another process on this GPU) the belief
        # is restored and the loop re-run as launches, for this call and for the rest of the process (engine.run_persistent)
        loc = engine.run_persistent(a, lambda: _abi.pf_forward_loop(a, like, events, stride, ess_threshold=policy.threshold,
                                                                    resampled_steps=took, dedup=dedup, history=history,
                                                                    regularise=regularise),
                                    device=like.device,
                                    n_sync_words=_abi.pf_persistent_sync_words(N, M, d, len(nets)) if form.persistent else 0,
                                    restore=(states_a, logw_a))
        file_timer_records()
        self.particle_states = states_b if loc & 1 else states_a
        self._spare_states = states_a if loc & 1 else states_b
        self.particle_log_weights = logw_b if loc & 2 else logw_a
        if self.resample_ess_threshold is None:
            self.last_resampled = None
        else:
            self.last_resampled = took.ne(0) if took is not None else torch.zeros((T, N), dtype=torch.bool, device=like.device)
        if hist is not None:
            hist.resampled = self.last_resampled
        self.last_history = hist
        del keep
        return est

    def _native_train_loop(self, dyn_all, meas_all, T, N):
        """K6, whole recursion (``engine.PfTrainLoopFunction``): all ``T`` train-mode steps forward in one C
        call, backward in one; ``None`` -> the caller's step-by-step autograd loop (user models, resampling
        while training, ``argmax`` estimates, a belief of another particle count)."""
        dyn, meas = self.dynamics_model, self.measurement_model
        policy = self._step_policy(int(self.num_particles))  # (a belief of another count is turned away below)
        if (dyn_all is None or meas_all is None or not hasattr(dyn, "_net") or not hasattr(meas, "train_plan")
                or policy.resample or self.estimation_method != "weighted_average" or T == 0 or not self.use_native_loop
                or self.record_belief):  # (the training recursion keeps no per-step record: the step loop computes it)
            return None
        assert self._initialized, "Particle filter not initialized!"
        Nb, M, d = self.particle_states.shape
        if Nb != N or policy.M_out != M:
            return None
        plan = meas.train_plan(meas_all)
        if plan is None:
            return None
        nets, biases, beta, K_all = plan
        if len(nets) > _abi.LOOP_MAX_MEAS:
            return None
        # the native recursion returns no gradient for the process-noise factor (the reference's models freeze Q)
        # and takes ONE depth for all measurement networks: a trainable / state-dependent Q or networks of
        # different depths keep the step-by-step autograd loop, which differentiates `eps @ scale_tril^T`
        if dyn.scale_tril().requires_grad or len({net.n_res for net, _col in nets}) != 1:
            return None
        eps, _ = self.noise.draw_steps(T, (N, M, d), None, like=self.particle_states)
        if isinstance(eps, CounterBlock):  # the training recursion reads its noise from a tensor
            blk = eps
            eps = torch.empty((T, N, M, d), dtype=torch.float32, device=self.particle_states.device)
            for t in range(T):
                _abi.philox_normals(blk.seed, blk.step0 + t, blk.traj0, eps[t])
        params = list(dyn._net._sources())
        for net, _col in nets:
            params += net._sources()
        empty = torch.empty(0, dtype=torch.float32, device=self.particle_states.device)
        if self.keep_training_sets:  # the recursion's own buffers as two more (differentiable) outputs
            est, states, logw, set_states, set_logw = engine.PfTrainLoopFunction.apply(
                (dyn._net, nets, K_all, True), T, N, M, self.particle_states, self.particle_log_weights, eps,
                dyn.scale_tril(), dyn_all, beta if beta is not None else empty, *biases, *params)
            self.last_training_sets = {"states": set_states, "log_weights": set_logw}
        else:
            est, states, logw = engine.PfTrainLoopFunction.apply(
                (dyn._net, nets, K_all), T, N, M, self.particle_states, self.particle_log_weights, eps,
                dyn.scale_tril(), dyn_all, beta if beta is not None else empty, *biases, *params)
        self.particle_states, self.particle_log_weights = states, logw
        self._spare_states = None
        return est

    def _loop_of_steps(self, T, step, N):
        """``forward_loop`` step by step: ``step(t, rows of step t in the T*N flattened arrays)``; the per-step records
        (``last_belief``, ``last_resampled``) are stacked along a leading ``T`` axis."""
        out, beliefs, took, hist, sets, jitter = [], [], [], [], [], []
        self._step_training_set = None
        self.last_regularisation = None
        for t in range(T):
            out.append(step(t, slice(t * N, (t + 1) * N)))
            beliefs.append(self.last_belief)
            took.append(self.last_resampled)
            jitter.append(self.last_regularisation)
            hist.append(self._step_history)
            sets.append(self._step_training_set)
        if sets and sets[0] is not None:  # (training steps with keep_training_sets: the sets before any resampling)
            self.last_training_sets = {"states": torch.stack([s for s, _ in sets]), "log_weights": torch.stack([w for _, w in sets])}
        self._step_training_set = None
        if self.record_belief:
            self.last_belief = base.stack_belief_records(beliefs)
        if took and took[0] is not None:
            self.last_resampled = torch.stack(took, dim=0)
        if jitter and all(j is not None for j in jitter):  # (every step of a loop resamples, or none does)
            self.last_regularisation = base.belief_record(bandwidth=torch.stack([j.bandwidth for j in jitter]), scale=jitter[0].scale,
                                                          floor=jitter[0].floor, shrink=jitter[0].shrink)
        else:
            self.last_regularisation = None
        self.last_history = None
        if self.record_history and T > 0:
            st, ll, lw, anc = zip(*hist)
            # a resampling step that changes the particle count (num_particles differs from the belief's): every array is
            # padded to the largest count with particles of log-likelihood -inf -- dead paths, which carry no weight and
            # are not counted -- whose ancestor is particle 0
            Mh = max(x.shape[1] for x in st)
            pad = lambda x, fill: x if x.shape[1] == Mh else torch.cat(
                [x, x.new_full((x.shape[0], Mh - x.shape[1]) + tuple(x.shape[2:]), fill)], dim=1)
            self.last_history = base.history_record(
                states=torch.stack([pad(x, 0.0) for x in st]), log_likelihoods=torch.stack([pad(x, -math.inf) for x in ll]),
                log_weights_in=torch.stack([pad(x, -math.inf) for x in lw]),
                ancestors=None if anc[0] is None else torch.stack([pad(x, 0) for x in anc]), resampled=self.last_resampled)
        self._step_history = None
        return torch.stack(out, dim=0)

    @engine.checked_step
    def forward(self, *, observations, controls) -> torch.Tensor:
        if use_autograd(self):
            return self._step_autograd(observations, controls)
        return self._step(observations, controls)

    @engine.checked_loop
    def forward_loop(self, *, observations, controls) -> torch.Tensor:
        """Sequential in ``t``.  Everything that does not depend on the belief (control and
        observation encoders, image CNNs, modality weights) is evaluated ahead of the
        recursion for all ``T*N`` rows at once: rows are independent, so the per-trajectory
        work costs one launch sequence per ``forward_loop`` instead of one per step."""
        T, N = tree_leading_shape(controls)[:2]
        assert tree_leading_shape(observations)[:2] == (T, N)
        flat = lambda x: x.reshape((T * N,) + tuple(x.shape[2:]))
        if use_autograd(self):
            if self.record_history:
                raise RuntimeError("record_history: the training (autograd) paths keep no history; call .eval() first")
            if self._regularisation is not None:
                raise RuntimeError("regularisation: the training (autograd) paths do not jitter; call .eval() first")
            self.last_training_sets = None
            if not engine.use_hip_backward():
                return self._loop_of_steps(T, lambda t, sl: self(
                    observations=tree_index(observations, t), controls=tree_index(controls, t)), N)
            # training, K6 backend: the per-trajectory networks (image CNNs, encoders, weight
            # model) are differentiable torch ops evaluated ONCE on the T*N flattened rows
            dyn_all = meas_all = None
            if hasattr(self.dynamics_model, "encode_controls_autograd"):
                dyn_all = self.dynamics_model.encode_controls_autograd(tree_map(controls, flat))
            if hasattr(self.measurement_model, "encode_observations_autograd"):
                meas_all = self.measurement_model.encode_observations_autograd(tree_map(observations, flat))
            native = self._native_train_loop(dyn_all, meas_all, T, N)
            if native is not None:  # (it only runs without resampling: nobody resampled)
                self.last_resampled = (None if self.resample_ess_threshold is None else
                                       torch.zeros((T, N), dtype=torch.bool, device=native.device))
                return native
            return self._loop_of_steps(T, lambda t, sl: self._step_autograd(
                tree_index(observations, t), tree_index(controls, t),
                None if dyn_all is None else dyn_all[sl],
                None if meas_all is None else {k: v[sl] for k, v in meas_all.items()}), N)
        obs_all = ctrl_all = None
        with torch.no_grad():
            if hasattr(self.measurement_model, "forward_encoded"):
                obs_all = self.measurement_model.encode_observations(tree_map(observations, flat))
            if hasattr(self.dynamics_model, "propagate_encoded"):
                ctrl_all = self.dynamics_model.encode_controls(tree_map(controls, flat))
            native = self._native_loop(obs_all, ctrl_all, T, N)
        est = native if native is not None else self._loop_of_steps(T, lambda t, sl: self._step(
            tree_index(observations, t), tree_index(controls, t),
            None if obs_all is None else {k: v[sl] for k, v in obs_all.items()},
            None if ctrl_all is None else {k: v[sl] for k, v in ctrl_all.items()}), N)
        if self.last_history is not None:
            self.last_history.controls = controls  # (a reference, not a copy) what smooth(method="marginal") predicts with
            from .base_models import CrossmodalParticleFilterMeasurementModel  # (base_models imports this module)

            if isinstance(self.measurement_model, CrossmodalParticleFilterMeasurementModel):  # what belief_modalities()
                self.last_history.observations = observations  # encodes again (a reference, not a copy), and the fusion it
                self.last_history.enabled_models = tuple(self.measurement_model.enabled_models)  # belongs to
        return est


class InnovationSwitches:
    """The two innovation switches of every Kalman filter (evaluation mode only, both off by default; with both off every
    launch and every bit is as without them).  Per step ``t``, sub-filter ``k`` and trajectory ``n`` (``include/mmf.h``,
    "innovation statistics"): ``nu = z - mu-``, ``S = Sigma- + R``, ``nis = nu^T S^-1 nu`` (chi-squared with ``d`` degrees of
    freedom under a consistent filter), ``log_likelihood = -1/2 (nis + log det S + d log 2 pi)``.

    ``record_innovations = True``: ``forward`` / ``forward_loop`` leave ``last_innovations``, a ``base.belief_record`` of
    ``nis``, ``log_likelihood`` (float32) and ``accepted`` (bool) -- ``(N,)`` for a single filter and ``(K, N)`` for a fused
    one (``K`` enabled sub-filters, ``sub_filters = K`` in the record; ``None`` for a single filter), with a leading ``T``
    after ``forward_loop``.
    ``innovation_gate``: ``None`` or a float > 0, the NIS threshold (the caller picks the chi-squared quantile): a
    measurement with ``nis > gate`` (or a NaN ``nis``) is rejected and that (sub-)filter keeps its predicted belief
    ``(mu-, Sigma-)``; fusion and feedback then run on whatever every sub-filter holds.  With the gate alone
    ``last_innovations`` is still left: ``accepted`` is what the caller needs.  A fused filter applies its one gate to
    every sub-filter and ignores the sub-filters' own switches (evaluation mode).
    The native loop then runs as a loop of launches: the persistent launch keeps no innovation and is not taken."""

    def _init_innovation_switches(self):
        self.record_innovations = False
        self._innovation_gate = None
        self.last_innovations = None

    @property
    def innovation_gate(self) -> Optional[float]:
        return self._innovation_gate

    @innovation_gate.setter
    def innovation_gate(self, value) -> None:
        if value is not None:
            ok = isinstance(value, (int, float)) and not isinstance(value, bool) and math.isfinite(value) and value > 0
            if not ok:
                raise ValueError(f"innovation_gate must be None or a finite float > 0 (the NIS threshold), got {value!r}")
            value = float(value)
        self._innovation_gate = value

    def _innovations_on(self) -> bool:
        return bool(self.record_innovations) or self._innovation_gate is not None

    def _refuse_innovations_in_training(self):
        if self.record_innovations:
            raise RuntimeError("record_innovations: the training (autograd) paths record no innovations; call .eval() first")
        if self._innovation_gate is not None:
            raise RuntimeError("innovation_gate: the training (autograd) paths gate no measurement; call .eval() first")

    @staticmethod
    def _innovation_buffers(lead, device):
        """``(nis, log_likelihood, accepted)`` to hand to the step / loop entry: float32, float32, int32 of shape ``lead``."""
        return (torch.empty(lead, dtype=torch.float32, device=device), torch.empty(lead, dtype=torch.float32, device=device),
                torch.empty(lead, dtype=torch.int32, device=device))

    @staticmethod
    def _innovation_record(buffers, fused: bool):
        """The filled buffers ``(..., K, N)`` as the record: a single filter's drop the ``K = 1`` axis."""
        nis, ll, acc = buffers
        if not fused:
            nis, ll, acc = (t.squeeze(-2) for t in (nis, ll, acc))
        return base.belief_record(nis=nis, log_likelihood=ll, accepted=acc != 0, sub_filters=nis.shape[-2] if fused else None)

    @staticmethod
    def _stack_innovation_records(steps):
        if not steps:
            return None
        return base.belief_record(sub_filters=steps[0].sub_filters,
                                  **{k: torch.stack([getattr(s, k) for s in steps]) for k in ("nis", "log_likelihood", "accepted")})


class VirtualSensorExtendedKalmanFilter(base.Filter, InnovationSwitches):
    """EKF whose measurement is a learned virtual sensor ``(z, R^1/2)`` observed through
    ``C = I`` (T2).  predict: ``S- = A S A^T + L L^T`` with ``A`` the dynamics Jacobian;
    correct: ``K = S-(S- + R)^-1``, ``mu = mu- + K(z - mu-)``, ``S = (I - K) S-``.
    ``record_belief = True``: ``last_belief.covariance`` is the posterior covariance as every step leaves it --
    ``(N, d, d)`` after ``forward``, ``(T, N, d, d)`` after ``forward_loop`` (written by the native loop itself).
    ``record_history = True`` (evaluation mode): ``forward_loop`` leaves ``last_history`` -- ``means (T, N, d)``,
    ``covariances (T, N, d, d)`` and ``controls``, a reference to the controls it was given -- which ``smooth()`` turns into
    the Rauch-Tung-Striebel smoothed belief; no other output of the loop changes by a bit.
    ``record_innovations`` / ``innovation_gate`` (evaluation mode): ``InnovationSwitches`` -- ``last_innovations`` with
    ``nis``, ``log_likelihood`` and ``accepted``, ``(N,)`` after ``forward`` and ``(T, N)`` after ``forward_loop``."""

    default_smooth_method = "rts"  # what evaluation.run_filter smooths this filter with when no method is named

    def __init__(self, *, dynamics_model: base.DynamicsModel,
                 virtual_sensor_model: base.VirtualSensorModel):
        super().__init__(state_dim=dynamics_model.state_dim)
        assert isinstance(dynamics_model, base.DynamicsModel)
        assert isinstance(virtual_sensor_model, base.VirtualSensorModel)
        self.dynamics_model = dynamics_model
        self.virtual_sensor_model = virtual_sensor_model
        self._belief_mean = None
        self._belief_covariance = None
        self._initialized = False
        self.record_belief = False
        self.last_belief = None
        self.record_history = False             # forward_loop keeps the filtered beliefs -> last_history
        self.record_transition_moments = False  # smooth() also leaves the two-slice residual moments
        self.last_history = None
        self.last_smoothed = None
        self.last_forecast = None               # belief_forecast(): the k-step-ahead Gaussian forecasts of the recorded beliefs
        self._init_innovation_switches()

    def _record_step_belief(self):
        self.last_belief = base.belief_record(covariance=self._belief_covariance.detach()) if self.record_belief else None

    @property
    def belief_mean(self):
        return self._belief_mean

    @belief_mean.setter
    def belief_mean(self, v):
        self._belief_mean = v

    @property
    def belief_covariance(self):
        return self._belief_covariance

    @belief_covariance.setter
    def belief_covariance(self, v):
        self._belief_covariance = v

    def initialize_beliefs(self, *, mean, covariance):
        N, d = mean.shape
        assert d == self.state_dim
        assert covariance.shape == (N, d, d)
        require_device(mean, "VirtualSensorExtendedKalmanFilter.initialize_beliefs")
        self._belief_mean = mean.to(torch.float32).contiguous().clone()
        self._belief_covariance = covariance.to(torch.float32).contiguous().clone()
        self._initialized = True

    def _predict_pieces(self, controls, ctrl_ctx=None):
        """``(mu-, A, L)`` for the current belief mean; ``L`` is ``(d, d)`` (constant noise)."""
        dyn = self.dynamics_model
        mu = self._belief_mean
        if hasattr(dyn, "predict_with_jacobian"):
            if ctrl_ctx is None:
                ctrl_ctx = dyn.encode_controls(controls)
            return dyn.predict_with_jacobian(mu, ctrl_ctx)
        mu_pred, tril = dyn(initial_states=mu, controls=controls)
        A = dyn.jacobian(initial_states=mu, controls=controls)
        # the C ABI takes one scale_tril per sub-filter: user models must keep it constant
        return mu_pred.detach().contiguous(), A.detach().contiguous(), tril[0].detach().contiguous()

    def _step(self, observations, controls, sensor_out=None, ctrl_ctx=None):
        assert self._initialized, "Kalman filter not initialized!"
        with torch.no_grad():
            z, r_tril = sensor_out if sensor_out is not None else self.virtual_sensor_model(observations=observations)
            mu_pred, A, L = self._predict_pieces(controls, ctrl_ctx)
            N, d = mu_pred.shape
            mu = torch.empty((1, N, d), dtype=torch.float32, device=mu_pred.device)
            Sigma = self._belief_covariance.reshape(1, N, d, d).clone()
            self._k3(A.reshape(1, N, d, d), mu_pred.reshape(1, N, d), L.reshape(1, d, d).contiguous(),
                     z.to(torch.float32).reshape(1, N, d).contiguous(),
                     r_tril.to(torch.float32).reshape(1, N, d, d).contiguous(), mu, Sigma)
            self._belief_mean, self._belief_covariance = mu[0], Sigma[0]
        self._record_step_belief()
        return self._belief_mean

    def _k3(self, A, mu_pred, L, z, r_tril, mu, Sigma):
        """K3 for this filter alone (K = 1, no fusion): ``mmf_ekf_step``, or with an innovation switch set
        ``mmf_ekf_step_innov``, which also leaves ``last_innovations`` ``(N,)``."""
        if not self._innovations_on():
            self.last_innovations = None
            _abi.ekf_step(A, mu_pred, L, z, r_tril, None, mu, Sigma, None, None, fusion=0, feedback=0)
            return
        buf = self._innovation_buffers(tuple(mu_pred.shape[:2]), mu_pred.device)
        _abi.ekf_step_innov(A, mu_pred, L, z, r_tril, None, mu, Sigma, None, None, fusion=0, feedback=0,
                            nis_gate=self._innovation_gate, nis=buf[0], loglik=buf[1], accepted=buf[2])
        self.last_innovations = self._innovation_record(buf, fused=False)

    def _step_autograd(self, observations, controls):
        """Differentiable torch formulation (training backend "autograd")."""
        assert self._initialized, "Kalman filter not initialized!"
        mu, Sigma = self._belief_mean, self._belief_covariance
        z, r_tril = self.virtual_sensor_model(observations=observations)
        dyn = self.dynamics_model
        if engine.use_hip_backward() and hasattr(dyn, "predict_with_jacobian_autograd"):
            # K6: dynamics network + forward-mode Jacobian forward and backward in HIP
            mu_pred, A = dyn.predict_with_jacobian_autograd(mu, controls)
            L = dyn.scale_tril()[None]
        else:
            mu_pred, L = dyn(initial_states=mu, controls=controls)
            A = dyn.jacobian(initial_states=mu, controls=controls)
        # K6's Kalman step takes ONE (d, d) process-noise factor and returns no gradient for it: right for
        # the reference's models (constant Q, requires_grad=False), wrong for a user model whose
        # scale_tril depends on the state / control or is trainable -- those keep the torch algebra below
        q_const = (not L.requires_grad) and (L.shape[0] == 1 or bool((L == L[:1]).all()))
        if engine.use_hip_backward() and q_const:
            # K6: the Kalman algebra forward (K3) and backward (closed-form adjoints) in HIP; the
            # networks around it (sensor, dynamics, Jacobian) keep their autograd form
            self._belief_mean, self._belief_covariance = engine.EkfStepFunction.apply(A, mu_pred, L[0], z, r_tril, Sigma)
            self._record_step_belief()
            return self._belief_mean
        Sp = A @ Sigma @ A.transpose(-1, -2) + L @ L.transpose(-1, -2)
        K = Sp @ torch.inverse(Sp + r_tril @ r_tril.transpose(-1, -2))
        self._belief_mean = mu_pred + (K @ (z - mu_pred)[:, :, None]).squeeze(-1)
        self._belief_covariance = (torch.eye(K.shape[-1], device=K.device) - K) @ Sp
        self._record_step_belief()
        return self._belief_mean

    @engine.checked_step
    def forward(self, *, observations, controls):
        if use_autograd(self):
            self._refuse_innovations_in_training()
            return self._step_autograd(observations, controls)
        return self._step(observations, controls)

    def _native_loop(self, observations, ctrl_all, T, N, flat):
        """All ``T`` steps through ``mmf_ekf_forward_loop`` (K = 1, no fusion) when the virtual
        sensor is row-wise (so it can be evaluated on the ``T*N`` flattened rows at once) and
        the dynamics model is a fused network; ``None`` -> Python loop."""
        dyn, vs = self.dynamics_model, self.virtual_sensor_model
        if ctrl_all is None or T == 0 or not hasattr(dyn, "_net") or not getattr(vs, "row_wise", False):
            return None
        assert self._initialized, "Kalman filter not initialized!"
        d = self.state_dim
        z, r = vs(observations=tree_map(observations, flat))
        z = z.to(torch.float32).reshape(T, 1, N, d).contiguous()
        r = r.to(torch.float32).reshape(T, 1, N, d, d).contiguous()
        mu = self._belief_mean.reshape(1, N, d).contiguous().clone()
        Sigma = self._belief_covariance.reshape(1, N, d, d).contiguous().clone()
        q = dyn.scale_tril().to(torch.float32).reshape(1, d, d).contiguous()
        keep = self.record_belief or self.record_history  # (the same Sigma_steps path for either)
        steps = torch.empty((T, N, d, d), dtype=torch.float32, device=mu.device) if keep else None
        buf = self._innovation_buffers((T, 1, N), mu.device) if self._innovations_on() else None
        est, _ = engine.run_ekf_loop([dyn._net], [ctrl_all["bias"]], q, z, r, mu, Sigma, Sigma_steps=steps,
                                     innovations=buf, nis_gate=self._innovation_gate)
        self.last_innovations = None if buf is None else self._innovation_record(buf, fused=False)
        self._belief_mean, self._belief_covariance = mu[0], Sigma[0]
        self.last_belief = base.belief_record(covariance=steps) if self.record_belief else None
        if self.record_history:
            self.last_history = base.history_record(means=est, covariances=steps)
        return est

    @engine.checked_loop
    def forward_loop(self, *, observations, controls):
        self.last_history = None
        self.last_innovations = None
        if use_autograd(self):
            if self.record_history:
                raise RuntimeError("record_history: the training (autograd) paths keep no history; call .eval() first")
            self._refuse_innovations_in_training()
            return base.Filter.forward_loop(self, observations=observations, controls=controls)
        T, N = tree_leading_shape(controls)[:2]
        flat = lambda t: t.reshape((T * N,) + tuple(t.shape[2:]))
        with torch.no_grad():
            ctrl_all = None
            if hasattr(self.dynamics_model, "predict_with_jacobian"):
                ctrl_all = self.dynamics_model.encode_controls(tree_map(controls, flat))
            native = self._native_loop(observations, ctrl_all, T, N, flat)
            if native is not None:
                if self.last_history is not None:
                    self.last_history.controls = controls  # (a reference, not a copy) what smooth() predicts with
                return native
            sensors = [self.virtual_sensor_model(observations=tree_index(observations, t)) for t in range(T)]
        out, beliefs, covs, innovations = [], [], [], []
        for t in range(T):
            sl = slice(t * N, (t + 1) * N)
            out.append(self._step(tree_index(observations, t), tree_index(controls, t), sensors[t],
                                  None if ctrl_all is None else {k: v[sl] for k, v in ctrl_all.items()}))
            beliefs.append(self.last_belief)
            covs.append(self._belief_covariance)
            innovations.append(self.last_innovations)
        if self.record_belief:
            self.last_belief = base.stack_belief_records(beliefs)
        if self._innovations_on():
            self.last_innovations = self._stack_innovation_records(innovations)
        est = torch.stack(out, dim=0)
        if self.record_history and T > 0:
            self.last_history = base.history_record(means=est, covariances=torch.stack(covs, dim=0), controls=controls)
        return est

    def smooth(self, lag: Optional[int] = None, *, method: str = "rts") -> torch.Tensor:
        """Rauch-Tung-Striebel smoothing of the last ``forward_loop`` run with ``record_history`` set
        (``mmf_ekf_smooth``, ``include/mmf.h``): ``(T, N, d)`` means of ``E[x_t | y_1..s(t)]``, ``s(t) = min(t + lag, T - 1)``
        -- the meaning of ``ParticleFilter.smooth(lag)``.  ``lag = None``: the full smoother; ``lag = 0``: the filter's own
        belief.  The forward recursion is not touched: the Jacobians ``A_t`` and predictions ``f(m_t, u_{t+1})`` of the
        ``T - 1`` transitions are evaluated again here, in one batched call over the ``(T - 1) N`` recorded means (means
        ``[0 : T - 1]`` with controls ``[1 : T]``).  Leaves ``last_smoothed``: ``covariance (T, N, d, d)``, ``gain
        (T - 1, N, d, d)``, ``lag``, ``method = "rts"`` and, with ``self.record_transition_moments`` set (``lag = None``
        only), ``residual_mean (T - 1, N, d)`` / ``residual_second_moment (T - 1, N, d, d)``: mean and RAW second moment of
        the linearised transition residual under the two-slice smoothing distribution, what
        ``evaluation.process_noise_m_step`` refits the process noise from.  The process noise must be one ``scale_tril``
        for the whole batch."""
        if method != "rts":
            raise ValueError(f"smooth: the Kalman filters have one smoother, method='rts'; got {method!r} "
                             "('ancestry', 'marginal' and 'simulation' are the particle filter's)")
        if lag is not None and (isinstance(lag, bool) or not isinstance(lag, int) or lag < 0):
            raise ValueError(f"smooth: lag must be an int >= 0 (None: the full smoother), got {lag!r}")
        moments = bool(self.record_transition_moments)
        if moments and lag is not None:
            raise ValueError("smooth: record_transition_moments is set, and the two-slice moments are the full smoother's; "
                             f"lag={lag!r} has none (unset the switch, or smooth with lag=None)")
        h = self.last_history
        if h is None:
            raise ValueError("smooth() needs a history: set record_history and run forward_loop (evaluation mode) first")
        T, N, d = h.means.shape
        dev = h.means.device
        E = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        with torch.no_grad():
            mu_pred, A, tril = self._smoothing_transition(h)
            mean, cov, gain = E(T, N, d), E(T, N, d, d), E(max(T - 1, 0), N, d, d)
            extra = {}
            if moments:
                extra["residual_mean"], extra["residual_second_moment"] = E(max(T - 1, 0), N, d), E(max(T - 1, 0), N, d, d)
            _abi.ekf_smooth(h.means.to(torch.float32).contiguous(), h.covariances.to(torch.float32).contiguous(), A, mu_pred,
                            tril, lag, mean, cov, gain, None, extra.get("residual_mean"), extra.get("residual_second_moment"))
        self.last_smoothed = base.belief_record(covariance=cov, gain=gain, lag=lag, method="rts", **extra)
        return mean

    def _smoothing_transition(self, h):
        """``(x^ (T - 1, N, d), A (T - 1, N, d, d), L (d, d))`` of the ``T - 1`` recorded transitions, float32 on the
        history's device: the dynamics prediction and Jacobian at ``(means[t], controls[t + 1])`` in one batched call over
        the ``(T - 1) N`` rows (chunks of ``engine.JACOBIAN_MAX_ROWS`` where the Jacobian entry limits its rows) -- K5
        (``predict_with_jacobian``) for the built-in models, ``dyn(...)`` and ``dyn.jacobian(...)`` for a user model.
        A process noise that differs over the batch is refused."""
        T = h.means.shape[0]
        return self._transition_jacobians(h.means[:max(T - 1, 0)], tree_map(h.controls, lambda c: c[1:T]), "smooth(method='rts')")

    def _transition_jacobians(self, means, ctrl, who: str):
        """``(f(m, u) (n, N, d), A (n, N, d, d), L (d, d))`` at the ``n N`` points ``means (n, N, d)`` under the controls ``ctrl
        (n, N, ...)``, float32 on the means' device; a noise that differs over the batch is the ``ValueError`` of ``who``."""
        n, N, d = means.shape
        dev = means.device
        dyn = self.dynamics_model
        R = n * N
        if R == 0:  # (no transition: the noise is never read)
            tril = dyn.scale_tril() if hasattr(dyn, "scale_tril") else torch.eye(d)
            return (torch.empty((n, N, d), dtype=torch.float32, device=dev),
                    torch.empty((n, N, d, d), dtype=torch.float32, device=dev),
                    tril.detach().to(device=dev, dtype=torch.float32).contiguous())
        past = means.reshape(R, d).to(torch.float32).contiguous()
        rows = tree_map(ctrl, lambda c: c.reshape((R,) + tuple(c.shape[2:])))
        preds, jacs, tril = [], [], None
        for r0 in range(0, R, engine.JACOBIAN_MAX_ROWS):
            sl = slice(r0, min(r0 + engine.JACOBIAN_MAX_ROWS, R))
            ctrl_rows = tree_map(rows, lambda c: c[sl])
            if hasattr(dyn, "predict_with_jacobian"):
                x, J, tril = dyn.predict_with_jacobian(past[sl], dyn.encode_controls(ctrl_rows))
            else:
                x, trils = dyn(initial_states=past[sl], controls=ctrl_rows)
                J = dyn.jacobian(initial_states=past[sl], controls=ctrl_rows)
                if (tril is not None and not bool((trils == tril).all())) or not bool((trils == trils[:1]).all()):
                    raise ValueError(f"{who} needs one process-noise scale_tril for all trajectories and steps; "
                                     "this dynamics model returns noise that differs over the batch")
                tril = trils[0]
            preds.append(x.detach())
            jacs.append(J.detach())
        x, J = (preds[0], jacs[0]) if len(preds) == 1 else (torch.cat(preds), torch.cat(jacs))
        return (x.to(torch.float32).reshape(n, N, d).contiguous(), J.to(torch.float32).reshape(n, N, d, d).contiguous(),
                tril.detach().to(device=dev, dtype=torch.float32).contiguous())

    def belief_forecast(self, horizon: int, truth: Optional[torch.Tensor] = None) -> torch.Tensor:
        """k-step-ahead forecasts from every recorded step, the record of ``ParticleFilter.belief_forecast`` for a Gaussian
        belief: with ``T`` recorded steps, origin ``t`` and lead ``h`` in ``1 .. horizon``, the filtered belief ``(means[t],
        covariances[t])`` of ``last_history`` goes through the extended prediction ``h`` times under the recorded controls --
        ``m <- f(m, u_{t+k})``, ``P <- A P A^T + L L^T`` with ``A`` the Jacobian at ``m`` -- one batched call of the dynamics per
        ``k`` over the ``(T - k) N`` beliefs (``predict_with_jacobian`` in chunks of ``engine.JACOBIAN_MAX_ROWS``, or ``dyn()``
        and ``dyn.jacobian()`` for a user model, as the smoother evaluates them), the covariances in torch ops.  Returns ``mean
        (H, T, N, d)`` with the forecast of ``x_{t+h}`` made at ``t`` at ``[h - 1, t]`` and NaN where ``t + h > T - 1``; leaves
        ``last_forecast``: ``mean``, ``covariance (H, T, N, d, d)``, ``horizon`` and, with ``truth (T, N, d)``, ``error`` =
        ``mean - truth[t + h]`` (``evaluation.forecast_filter`` adds the Gaussian closed forms of the scores).  No noise is
        drawn; evaluation mode only; ``last_history`` and ``last_smoothed`` are left as they are.  The unscented filter keeps
        no history and answers so; the fused filters and the LSTM baselines have no such method."""
        who = "belief_forecast"
        if isinstance(horizon, bool) or not isinstance(horizon, numbers.Integral) or horizon < 1:
            raise ValueError(f"{who}: horizon must be an int >= 1, got {horizon!r}")
        if self.training:
            raise RuntimeError(f"{who}: the training (autograd) paths keep no history; call .eval() first")
        h = self.last_history
        if h is None:
            raise ValueError(f"{who} needs a history: set record_history and run forward_loop (evaluation mode) first")
        T, N, d = h.means.shape
        if truth is not None and (not isinstance(truth, torch.Tensor) or tuple(truth.shape) != (T, N, d)):
            raise ValueError(f"{who}: truth must be None or a (T, N, d) = ({T}, {N}, {d}) tensor, got "
                             f"{tuple(truth.shape) if isinstance(truth, torch.Tensor) else type(truth).__name__}")
        H, dev = int(horizon), h.means.device
        blank = lambda *tail: torch.full((H, T, N) + tail, math.nan, dtype=torch.float32, device=dev)
        with torch.no_grad():
            out = {"mean": blank(d), "covariance": blank(d, d)}
            m, P = h.means.to(torch.float32), h.covariances.to(torch.float32)
            for k in range(1, min(H, T - 1) + 1):
                n = T - k
                m, A, tril = self._transition_jacobians(m[:n], tree_map(h.controls, lambda c: c[k:T]), who)
                P = A @ P[:n] @ A.transpose(-1, -2) + tril @ tril.t()
                out["mean"][k - 1, :n], out["covariance"][k - 1, :n] = m, P
            if truth is not None:
                y = truth.detach().to(device=dev, dtype=torch.float32)
                out["error"] = blank(d)
                for k in range(1, min(H, T - 1) + 1):
                    out["error"][k - 1, :T - k] = out["mean"][k - 1, :T - k] - y[k:]
        self.last_forecast = base.belief_record(horizon=H, **out)
        return out["mean"]


# ------------------------------------------------------------------------------ unscented filter
class JulierSigmaPointStrategy:
    """``lambda = 3 - d`` unless given; mean and covariance weights coincide (upstream
    ``torchfilter.utils.JulierSigmaPointStrategy``, its UKFs' default)."""

    def __init__(self, lambd: Optional[float] = None):
        self.lambd = lambd

    def compute_lambda(self, dim: int) -> float:
        return 3.0 - dim if self.lambd is None else float(self.lambd)

    def compute_sigma_weights(self, dim: int):
        """``(wc0, wm0, wi)``: covariance / mean weight of the central point, weight of the rest."""
        lambd = self.compute_lambda(dim)
        w0 = lambd / (dim + lambd)
        return w0, w0, 1.0 / (2.0 * (dim + lambd))


class MerweSigmaPointStrategy:
    """Van der Merwe's scaled points: ``lambda = alpha^2 (d + kappa) - d``, ``kappa = 3 - d`` unless
    given; ``wc0 = wm0 + 1 - alpha^2 + beta`` (upstream ``torchfilter.utils.MerweSigmaPointStrategy``).

    Small ``alpha`` means large weights of opposite sign: the default ``alpha = 1e-2`` has ``wm0 ~ -1e4`` and ``wi ~
    1.7e3``.  ``mmf_ukf_moments`` takes its sums about point 0 (``wm0 + 2 d wi = 1``), which keeps the default within the
    fp32 bar (``tests/test_gpu_kalman_kernels.py``, group F: 1e-4 on the mean, three times the fp32 yardstick's ~1e-4 on the
    covariance).  ``alpha = 1e-3`` (``wi ~ 1.7e5``) is beyond float32 in any summation order -- the covariance is off by
    ~1e-2 -- and is neither tested nor supported at that accuracy; use ``alpha >= 1e-2``."""

    def __init__(self, alpha: float = 1e-2, beta: float = 2.0, kappa: Optional[float] = None):
        self.alpha, self.beta, self.kappa = alpha, beta, kappa

    def compute_lambda(self, dim: int) -> float:
        kappa = 3.0 - dim if self.kappa is None else float(self.kappa)
        return self.alpha ** 2 * (dim + kappa) - dim

    def compute_sigma_weights(self, dim: int):
        lambd = self.compute_lambda(dim)
        wm0 = lambd / (dim + lambd)
        return wm0 + 1.0 - self.alpha ** 2 + self.beta, wm0, 1.0 / (2.0 * (dim + lambd))


class VirtualSensorUnscentedKalmanFilter(VirtualSensorExtendedKalmanFilter):
    """UKF whose measurement is a learned virtual sensor observed through ``C = I`` (SURVEY.md 8f
    rank 2; upstream ``torchfilter.filters.VirtualSensorUnscentedKalmanFilter``, absent and
    un-pinned: published algorithm, restated in ``oracle/tf/filters.py``).

    predict: ``2d + 1`` sigma points of the belief (``mmf_ukf_sigma_points``) go through the
    dynamics model -- for the built-in networks they are rows of K2, ``N x (2d+1)`` "particles"
    without noise -- and ``mmf_ukf_moments`` forms ``mu-`` and ``Sigma- = sum wc (X - mu-)(X - mu-)^T +
    Q``; no Jacobian is evaluated.  correct: with an identity measurement the unscented update is
    the Kalman update on ``(mu-, Sigma-)``, i.e. K3 with ``A = I`` and no added noise.
    Same belief attributes and ``forward`` / ``forward_loop`` contract as the EKF."""

    def __init__(self, *, dynamics_model, virtual_sensor_model, sigma_point_strategy=None):
        super().__init__(dynamics_model=dynamics_model, virtual_sensor_model=virtual_sensor_model)
        self.sigma_point_strategy = sigma_point_strategy if sigma_point_strategy is not None else JulierSigmaPointStrategy()

    _NO_SMOOTHER = ("VirtualSensorUnscentedKalmanFilter has no smoother: the RTS sweep of an unscented filter needs the "
                    "cross-covariance of the sigma points before and after the dynamics, which its forward pass does not "
                    "keep (the extended filter's smoother linearises through the Jacobian instead)")

    @property
    def record_history(self) -> bool:
        return False

    @record_history.setter
    def record_history(self, value: bool) -> None:
        if value:
            raise NotImplementedError(self._NO_SMOOTHER)

    def smooth(self, lag: Optional[int] = None, *, method: str = "rts") -> torch.Tensor:
        raise NotImplementedError(self._NO_SMOOTHER)

    def _unscented_predict(self, controls, ctrl_ctx=None, not_pd=None):
        """``not_pd``: a loop-wide device flag (checked by the caller after the loop) -- ``None`` checks
        this step's own flag right away (one blocking 4-byte read)."""
        dyn = self.dynamics_model
        mu, Sigma = self._belief_mean.contiguous(), self._belief_covariance.contiguous()
        N, d = mu.shape
        P = 2 * d + 1
        lambd = self.sigma_point_strategy.compute_lambda(d)
        wc0, wm0, wi = self.sigma_point_strategy.compute_sigma_weights(d)
        points = torch.empty((N, P, d), dtype=torch.float32, device=mu.device)
        own = not_pd is None
        if own:
            not_pd = torch.zeros(1, dtype=torch.int32, device=mu.device)
        _abi.ukf_sigma_points(mu, Sigma, math.sqrt(d + lambd), points, not_pd)
        # a non-PD belief collapses its points onto the mean inside the kernel (finite rows for the
        # networks); a single step raises here, a forward_loop once after its last step
        if own and int(not_pd.item()):
            raise ValueError("unscented predict: belief covariance is not positive definite")
        if hasattr(dyn, "propagate_encoded"):
            if ctrl_ctx is None:
                ctrl_ctx = dyn.encode_controls(controls)
            moved = dyn.propagate_encoded(points, ctrl_ctx, None)
            L = dyn.scale_tril().to(torch.float32).contiguous()
        else:  # forward-only user model: one call on the N * (2d+1) flattened rows
            rep = tree_map(controls, lambda t: torch.repeat_interleave(t, repeats=P, dim=0))
            pred, _ = dyn(initial_states=points.reshape(N * P, d), controls=rep)
            moved = pred.reshape(N, P, d).to(torch.float32).contiguous()
            # noise evaluated at the belief mean (upstream); must be constant over the batch for the C ABI
            L = dyn(initial_states=mu, controls=controls)[1][0].detach().to(torch.float32).contiguous()
        mu_pred = torch.empty((N, d), dtype=torch.float32, device=mu.device)
        Sigma_pred = torch.empty((N, d, d), dtype=torch.float32, device=mu.device)
        _abi.ukf_moments(moved, wm0, wc0, wi, L, mu_pred, Sigma_pred)
        return mu_pred, Sigma_pred

    def _step(self, observations, controls, sensor_out=None, ctrl_ctx=None, not_pd=None):
        assert self._initialized, "Kalman filter not initialized!"
        with torch.no_grad():
            z, r_tril = sensor_out if sensor_out is not None else self.virtual_sensor_model(observations=observations)
            mu_pred, Sigma_pred = self._unscented_predict(controls, ctrl_ctx, not_pd)
            N, d = mu_pred.shape
            eye = torch.eye(d, dtype=torch.float32, device=mu_pred.device)[None].expand(N, d, d).contiguous()
            mu = torch.empty((1, N, d), dtype=torch.float32, device=mu_pred.device)
            Sigma = Sigma_pred.reshape(1, N, d, d)
            self._k3(eye.reshape(1, N, d, d), mu_pred.reshape(1, N, d),
                     torch.zeros((1, d, d), dtype=torch.float32, device=mu_pred.device),
                     z.to(torch.float32).reshape(1, N, d).contiguous(),
                     r_tril.to(torch.float32).reshape(1, N, d, d).contiguous(), mu, Sigma)
            self._belief_mean, self._belief_covariance = mu[0], Sigma[0]
        self._record_step_belief()
        return self._belief_mean

    def _step_autograd(self, observations, controls):
        raise NotImplementedError("the unscented filter is evaluation-only here; train the models with the EKF / PF")

    def _native_loop(self, observations, ctrl_all, T, N, flat):
        return None  # the step is sigma points -> K2 -> moments -> K3: driven from Python, sensors batched over T*N

    @engine.checked_loop
    def forward_loop(self, *, observations, controls):
        if use_autograd(self):
            self._refuse_innovations_in_training()
        T, N = tree_leading_shape(controls)[:2]
        flat = lambda t: t.reshape((T * N,) + tuple(t.shape[2:]))
        with torch.no_grad():
            ctrl_all = None
            if hasattr(self.dynamics_model, "propagate_encoded"):
                ctrl_all = self.dynamics_model.encode_controls(tree_map(controls, flat))
            if getattr(self.virtual_sensor_model, "row_wise", False):
                z, r = self.virtual_sensor_model(observations=tree_map(observations, flat))
                sensors = [(z[t * N:(t + 1) * N], r[t * N:(t + 1) * N]) for t in range(T)]
            else:
                sensors = [self.virtual_sensor_model(observations=tree_index(observations, t)) for t in range(T)]
        out, beliefs, innovations = [], [], []
        not_pd = torch.zeros(1, dtype=torch.int32, device=self._belief_mean.device)  # one flag, one read per loop
        self.last_innovations = None
        for t in range(T):
            sl = slice(t * N, (t + 1) * N)
            out.append(self._step(tree_index(observations, t), tree_index(controls, t), sensors[t],
                                  None if ctrl_all is None else {k: v[sl] for k, v in ctrl_all.items()}, not_pd))
            beliefs.append(self.last_belief)
            innovations.append(self.last_innovations)
        if self.record_belief:  # the per-step posterior covariances, stacked on the device
            self.last_belief = base.stack_belief_records(beliefs)
        if self._innovations_on():
            self.last_innovations = self._stack_innovation_records(innovations)
        if T > 0 and int(not_pd.item()):
            raise ValueError("unscented predict: belief covariance is not positive definite")
        return torch.stack(out, dim=0)

"""The particle smoothers of ``filters.ParticleFilter``: what ``smooth()`` makes of the history a ``forward_loop`` recorded.
They read ``last_history`` and the dynamics model, write ``last_smoothed`` and touch nothing of the recursion."""
from typing import Optional

import torch

from . import _abi, base
from .utils import CounterNoise, tree_map


class _DefaultDraws(int):
    """The default of ``ParticleFilter.smooth(num_draws=)``: 64, told apart by identity from a 64 the caller passed, since
    ``num_draws`` with a method that draws no paths is an error."""


_DEFAULT_DRAWS = _DefaultDraws(64)


class ParticleSmoothing:
    """``smooth()`` of the particle filter, a mixin like ``filters.InnovationSwitches``; the host class supplies
    ``last_history``, ``dynamics_model`` and ``noise``.
    ``smooth(lag)`` returns the ancestry-smoothed means ``E[x_t | y_1..min(t + lag, T)]`` (``mmf_pf_smooth``).
    ``record_transition_moments = True``: ``smooth(method="marginal")`` also leaves the two-slice moments of the transition
    residual in ``last_smoothed`` (``residual_mean``, ``residual_second_moment``; ``mmf_pf_smooth_pair_moments``), what
    ``evaluation.process_noise_m_step`` refits the process noise from.  A switch like the other ``record_*`` ones and not
    an argument of ``smooth``, whose parameter list stays ``(lag, *, method, num_draws)``; another method with it set raises.
    """

    def _init_smoothing(self):
        self.last_smoothed = None
        self.record_transition_moments = False  # smooth(method="marginal") adds the two-slice residual moments to last_smoothed

    def smooth(self, lag: Optional[int] = None, *, method: str = "ancestry", num_draws: int = _DEFAULT_DRAWS) -> torch.Tensor:
        """Ancestry (genealogy) smoothing of the last ``forward_loop`` run with ``record_history`` set: ``(T, N, d)`` means
        of ``E[x_t | y_1..s(t)]``, ``s(t) = min(t + lag, T - 1)`` -- every particle of the endpoint ``s`` is traced back
        through the ancestors to the particle of step ``t`` it descends from, and the moments of those are taken under the
        endpoint's weights (``mmf_pf_smooth``, ``include/mmf.h``).  ``lag = None`` (or ``>= T - 1``): the full smoother;
        ``lag = 0``: the filter's own weighted set.  Leaves ``last_smoothed``: ``covariance (T, N, d, d)``, ``unique (T, N)``
        int32 -- the distinct particles of step ``t`` still alive on the endpoint's paths; where it drops to a handful the
        genealogy has collapsed and a shorter lag trades bias for variance -- and ``lag``.  The smoothed estimate is the
        weighted MEAN also where ``estimation_method == "argmax"`` makes the filter report another point.
        ``method = "marginal"``: the forward-filter backward-smoothing recursion instead (``_smooth_marginal``); ``lag`` must
        be ``None`` there.
        ``method = "simulation"``: ``num_draws`` (default 64) whole trajectories drawn from the joint smoothing distribution
        by backward simulation (``_smooth_simulation``); returns their mean, ``lag`` must be ``None``.  It draws
        ``(T, N, num_draws)`` uniforms from ``self.noise`` and so ADVANCES the filter's noise stream.  ``num_draws`` belongs
        to this method alone.
        ``method = "map"``: the single most probable index path through the particle history instead (``_smooth_map``): a
        ``(T, N, d)`` PATH of particles, not a mean; ``lag`` must be ``None``.  Its record has no ``covariance`` -- a path is
        not a distribution, so ``evaluation.gaussian_nll`` / ``nees`` / ``coverage`` do not apply to it.
        With ``self.record_transition_moments`` set (``method = "marginal"`` alone; any other method is a ``ValueError``):
        also the two-slice moments of the transition residual ``X_{t+1} - f(X_t, u_{t+1})`` -- ``last_smoothed`` gains
        ``residual_mean (T - 1, N, d)`` and ``residual_second_moment (T - 1, N, d, d)``, what
        ``evaluation.process_noise_m_step`` refits the process noise from."""
        if method not in ("ancestry", "marginal", "simulation", "map"):
            raise ValueError(f"smooth: method must be 'ancestry', 'marginal', 'simulation' or 'map', got {method!r}")
        if method != "ancestry" and lag is not None:
            raise ValueError(f"smooth(method={method!r}) is the full smoother: a fixed-lag {method} smoother is not implemented")
        if method != "simulation" and num_draws is not _DEFAULT_DRAWS:
            raise ValueError(f"smooth: num_draws is the number of paths method='simulation' draws; method={method!r} takes none")
        if isinstance(num_draws, bool) or not isinstance(num_draws, int) or num_draws < 1:
            raise ValueError(f"smooth(method='simulation'): num_draws must be an int >= 1, got {num_draws!r}")
        transition_moments = bool(getattr(self, "record_transition_moments", False))
        if transition_moments and method != "marginal":
            raise ValueError(f"smooth: record_transition_moments is set, and the two-slice moments are method='marginal''s; "
                             f"method={method!r} has none (unset the switch, or smooth with method='marginal')")
        h = self.last_history
        assert h is not None, "smooth() needs a history: set record_history and run forward_loop (evaluation mode) first"
        if method == "marginal":
            return self._smooth_marginal(h, transition_moments)
        if method == "simulation":
            return self._smooth_simulation(h, num_draws)
        if method == "map":
            return self._smooth_map(h)
        assert lag is None or int(lag) >= 0, "lag must be >= 0 (None: the full smoother)"
        T, N, M, d = h.states.shape
        dev = h.states.device
        mean = torch.empty((T, N, d), dtype=torch.float32, device=dev)
        cov = torch.empty((T, N, d, d), dtype=torch.float32, device=dev)
        unique = torch.empty((T, N), dtype=torch.int32, device=dev)
        _abi.pf_smooth(h.states, h.log_likelihoods, h.log_weights_in, None, h.ancestors,
                       max(T - 1, 0) if lag is None else min(int(lag), max(T - 1, 0)), mean, cov, unique)
        self.last_smoothed = base.belief_record(covariance=cov, unique=unique, lag=lag)
        return mean

    def _smooth_marginal(self, h, transition_moments: bool = False) -> torch.Tensor:
        """Marginal smoothing (forward filter, backward smoother; ``mmf_pf_smooth_marginal``, ``include/mmf.h``): every
        particle of step ``t`` is kept and re-weighted through the transition density ``N(X_{t+1}[j]; f(X_t[i], u_{t+1}),
        L L^T)``, so no ancestors are read and every resampling mode is covered; ``O(M^2)`` pairs per trajectory and step.
        The dynamics means of all ``(T - 1) N`` trajectories are evaluated in one go with the controls the history kept.
        Leaves ``last_smoothed``: ``covariance (T, N, d, d)``, ``ess (T, N)`` = ``1 / sum W^2`` of the smoothed weights,
        ``weights (T, N, M)``, ``lag = None``, ``method = "marginal"``.
        ``transition_moments``: the same predictions, noise factor and ``logD`` go on to ``mmf_pf_smooth_pair_moments`` -- one
        more pass over the pairs, all steps in one launch -- and the record gains ``residual_mean (T - 1, N, d)`` and
        ``residual_second_moment (T - 1, N, d, d)``: mean and RAW second moment of ``X_{t+1}[j] - F_t[i]`` under the
        two-slice smoothing distribution over the particle pairs ``(i, j)`` (leading size 0 for ``T == 1``)."""
        T, N, M, d = h.states.shape
        dev = h.states.device
        extra = {}
        with torch.no_grad():
            pred, tril = self._smoothing_transition(h, "marginal")
            weights = torch.empty((T, N, M), dtype=torch.float32, device=dev)
            mean = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            cov = torch.empty((T, N, d, d), dtype=torch.float32, device=dev)
            ess = torch.empty((T, N), dtype=torch.float32, device=dev)
            logd = torch.empty((T - 1, N, M), dtype=torch.float32, device=dev) if transition_moments and T > 1 else None
            _abi.pf_smooth_marginal(h.states, pred, h.log_likelihoods, h.log_weights_in, tril, weights, mean, cov, ess, logd)
            if transition_moments:
                extra["residual_mean"] = torch.empty((max(T - 1, 0), N, d), dtype=torch.float32, device=dev)
                extra["residual_second_moment"] = torch.empty((max(T - 1, 0), N, d, d), dtype=torch.float32, device=dev)
                _abi.pf_smooth_pair_moments(h.states, pred, h.log_likelihoods, h.log_weights_in, tril, weights, logd,
                                            extra["residual_mean"], extra["residual_second_moment"])
        self.last_smoothed = base.belief_record(covariance=cov, ess=ess, weights=weights, lag=None, method="marginal", **extra)
        return mean

    def _smoothing_transition(self, h, method: str):
        """What the smoothers that evaluate the transition density read beside the history: the dynamics means
        ``F_t = f(X_t, u_{t+1})`` of all ``(T - 1) N`` trajectories, evaluated in one go with the controls the history kept
        (``(T - 1, N, M, d)`` float32, ``None`` for ``T < 2``), and the one process-noise ``scale_tril (d, d)`` on the
        history's device.  State-dependent noise is refused."""
        T, N, M, d = h.states.shape
        dev = h.states.device
        dyn = self.dynamics_model
        pred = None
        if T > 1:
            ctrl = tree_map(h.controls, lambda c: c[1:])
            pred, tril = self._transition_means(h.states[:-1], ctrl, f"smooth(method={method!r})")
        elif hasattr(dyn, "scale_tril"):
            tril = dyn.scale_tril()
        else:  # (one step: the transition density is never evaluated)
            tril = torch.eye(d, dtype=torch.float32, device=dev)
        return pred, tril.detach().to(device=dev, dtype=torch.float32).contiguous()

    def _transition_means(self, past, ctrl, who: str):
        """``(f(X, u) (n, N, M, d) float32 contiguous, scale_tril)`` of ``n N`` particle sets ``past (n, N, M, d)`` under the
        controls ``ctrl (n, N, ...)``, noise-free, in one call of the dynamics: K2 (``propagate_encoded``) for the built-in
        models, ``dyn(...)`` on the ``n N M`` rows for a user model, whose state-dependent noise is the ``ValueError`` of
        ``who``."""
        n, N, M, d = past.shape
        dyn = self.dynamics_model
        if hasattr(dyn, "propagate_encoded"):
            ctx = dyn.encode_controls(tree_map(ctrl, lambda c: c.reshape((n * N,) + tuple(c.shape[2:]))))
            pred = dyn.propagate_encoded(past.reshape(n * N, M, d), ctx, None).reshape(n, N, M, d)
            tril = dyn.scale_tril()
        else:
            R = n * N * M
            rows = tree_map(ctrl, lambda c: c[:, :, None].expand((n, N, M) + tuple(c.shape[2:])).reshape(
                (R,) + tuple(c.shape[2:])))
            pred, trils = dyn(initial_states=past.reshape(R, d), controls=rows)
            if not bool((trils == trils[:1]).all()):
                raise ValueError(f"{who} needs one process-noise scale_tril for all particles and "
                                 "steps; this dynamics model returns state-dependent noise")
            pred, tril = pred.reshape(n, N, M, d), trils[0]
        return pred.to(torch.float32).contiguous(), tril

    def _smooth_simulation(self, h, num_draws: int) -> torch.Tensor:
        """Backward-simulation smoothing (forward filtering, backward simulation; ``mmf_pf_smooth_simulate``,
        ``include/mmf.h``): ``num_draws`` whole trajectories per filter trajectory from the joint smoothing distribution --
        the last particle from the filter's weights, then backwards every particle of step ``t`` re-weighted by the
        transition density into the particle the path chose at ``t + 1``.  ``(T - 1) N S M`` densities.  The ``(T, N, S)``
        uniforms are ONE ``self.noise.uniform`` draw (a ``ReplayNoise`` can supply them); the filter's noise stream advances.
        Returns the ``(T, N, d)`` mean of the draws and leaves ``last_smoothed``: ``covariance (T, N, d, d)`` of the draws,
        ``trajectories (T, N, S, d)``, ``indices (T, N, S)`` int32 (``-1`` / NaN where a draw is dead), ``num_draws``,
        ``lag = None``, ``method = "simulation"``."""
        T, N, M, d = h.states.shape
        dev = h.states.device
        S = int(num_draws)
        if isinstance(self.noise, CounterNoise):
            raise ValueError("smooth(method='simulation') draws (T, N, num_draws) uniforms from the filter's noise source; "
                             "CounterNoise draws one uniform per trajectory only: set filter.noise to a NoiseSource (or a "
                             "ReplayNoise holding the uniforms) before smoothing")
        with torch.no_grad():
            pred, tril = self._smoothing_transition(h, "simulation")
            u = self.noise.uniform((T, N, S), like=h.states)
            indices = torch.empty((T, N, S), dtype=torch.int32, device=dev)
            trajectories = torch.empty((T, N, S, d), dtype=torch.float32, device=dev)
            mean = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            cov = torch.empty((T, N, d, d), dtype=torch.float32, device=dev)
            _abi.pf_smooth_simulate(h.states, pred, h.log_likelihoods, h.log_weights_in, tril, u, indices, trajectories, mean, cov)
        self.last_smoothed = base.belief_record(covariance=cov, trajectories=trajectories, indices=indices, num_draws=S,
                                                lag=None, method="simulation")
        return mean

    def _smooth_map(self, h) -> torch.Tensor:
        """MAP path smoothing (``mmf_pf_smooth_map``, ``include/mmf.h``; Godsill, Doucet & West 2001): the most probable
        sequence of particles ``X_0[i_0], .., X_{T-1}[i_{T-1}]`` under ``p(x_0) prod_t p(y_t | x_t) N(x_t; f(x_{t-1}, u_t),
        L L^T)`` restricted to the particle grid, by a max-plus (Viterbi) recursion over the ``(T - 1) N M^2`` particle pairs;
        the incoming log-weights of step 0 stand in for ``log p(x_0)``.  No ancestors are read, so every resampling mode is
        covered, and no noise is drawn: the filter's noise stream does not move.  Returns the ``(T, N, d)`` path -- a state
        the filter did hold at every step, where a smoothed mean may lie between two modes -- and leaves ``last_smoothed``:
        ``indices (T, N)`` int32 (``-1``, with a NaN path, where a step left no particle alive), ``log_posterior (N,)`` the
        joint log-density of the path (``evaluation.path_log_density`` of ``indices``), ``lag = None``, ``method = "map"``.
        There is NO ``covariance``: a path is not a distribution, and ``evaluation.gaussian_nll`` / ``nees`` / ``coverage``
        do not apply."""
        T, N, M, d = h.states.shape
        dev = h.states.device
        with torch.no_grad():
            pred, tril = self._smoothing_transition(h, "map")
            indices = torch.empty((T, N), dtype=torch.int32, device=dev)
            path = torch.empty((T, N, d), dtype=torch.float32, device=dev)
            log_posterior = torch.empty((N,), dtype=torch.float32, device=dev)
            _abi.pf_smooth_map(h.states, pred, h.log_likelihoods, h.log_weights_in, tril, indices, path, log_posterior)
        self.last_smoothed = base.belief_record(indices=indices, log_posterior=log_posterior, lag=None, method="map")
        return path

"""The ``torchfilter.base`` API surface, MI355X-side.

Same class names, keyword-only signatures, shapes and ``assert`` behaviour as the
interfaces the reference's models subclass (``/root/reference/crossmodal/door_models/
dynamics.py:11,37-42``, ``door_models/pf.py:30,63-65``, ``door_models/kf.py:31,81-83``,
``base_models/crossmodal_kf.py:39``), so door-/push-style model classes drop
in unchanged.  On top of that contract, models may implement the *encoded* protocol, which
is what lets a filter hoist per-trajectory work out of the per-particle kernels and batch
observation encoders over a whole ``forward_loop``:

    DynamicsModel.encode_controls(controls)            -> ctx   (tensors with leading N)
    DynamicsModel.propagate_encoded(states, ctx, noise) -> states'
    ParticleFilterMeasurementModel.encode_observations(observations) -> ctx
    ParticleFilterMeasurementModel.forward_encoded(states, ctx)       -> (N, M) log-lik
    VirtualSensorModel.forward(observations)  (already per trajectory)

Models that only implement ``forward`` still work: the filters fall back to calling it
(on the GPU) and use the HIP kernels for the recursion itself.
"""
import abc
from types import SimpleNamespace
from typing import Tuple

import torch
import torch.nn as nn

from .utils import tree_index, tree_leading_shape, tree_map


def belief_record(**fields) -> SimpleNamespace:
    """What a filter with ``record_belief`` set leaves in ``last_belief``: ``covariance (..., N, d, d)`` for every filter;
    ``ess`` / ``log_evidence (..., N)`` for the particle filter (``include/mmf.h``, K1, has the definitions)."""
    return SimpleNamespace(**fields)


def history_record(**fields) -> SimpleNamespace:
    """What a particle filter with ``record_history`` set leaves in ``last_history`` after ``forward_loop`` -- everything a
    smoother needs, each with a leading ``T`` axis: ``states (T, N, M, d)`` the set every step propagated (before
    resampling), ``log_likelihoods (T, N, M)``, ``log_weights_in (T, N, M)`` the log-weights every step started from,
    ``ancestors (T, N, M)`` int32 (``None``: no step resampled -- the identity), ``resampled`` (the filter's
    ``last_resampled``) and ``controls``, a reference to (not a copy of) the controls the loop was given, which
    ``smooth(method="marginal")`` evaluates the dynamics means with; under a crossmodal measurement model also ``observations``,
    a reference to the observations the loop was given, and ``enabled_models``, a tuple: what ``belief_modalities()`` evaluates
    the unimodal log-likelihoods again with.  Where a step changed the particle count, ``M`` is the largest count and the shorter steps are
    padded with dead particles (log-likelihood ``-inf``).  ``include/mmf.h`` ("particle smoothing") has the definitions.
    An extended Kalman filter with ``record_history`` set leaves another record under the same name: ``means (T, N, d)`` and
    ``covariances (T, N, d, d)``, the filtered belief as every step left it, and ``controls`` as above -- what its RTS
    smoother reads (``include/mmf.h``, "RTS smoothing")."""
    return SimpleNamespace(**fields)


def stack_belief_records(steps) -> SimpleNamespace:
    """Per-step records -> one record with a leading ``T`` axis (the step-by-step loops; no host read)."""
    if not steps:
        return None
    return SimpleNamespace(**{k: torch.stack([getattr(s, k) for s in steps]) for k in vars(steps[0])})


class DynamicsModel(nn.Module, abc.ABC):
    """Optional, beside the encoded protocol above: a model with ONE process-noise factor may offer ``scale_tril() -> (d, d)``
    and ``set_scale_tril(L)``, which replaces it in place (and ``diagonal_noise``, true where it holds a diagonal only);
    ``evaluation.fit_process_noise`` refits the noise through them and refuses a model without."""

    def __init__(self, *, state_dim: int):
        super().__init__()
        self.state_dim = state_dim

    @abc.abstractmethod
    def forward(self, *, initial_states, controls) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(R, d), controls (R, ...) -> (states (R, d), scale_trils (R, d, d))``."""

    def forward_loop(self, *, initial_states, controls):
        """Open-loop rollout (``eval_helpers.py:135-137``): ``(T,N,...)`` -> ``(T,N,d)``, ``(T,N,d,d)``."""
        T = tree_leading_shape(controls)[0]
        x, xs, trils = initial_states, [], []
        for t in range(T):
            x, L = self(initial_states=x, controls=tree_index(controls, t))
            xs.append(x)
            trils.append(L)
        return torch.stack(xs, dim=0), torch.stack(trils, dim=0)

    def jacobian(self, *, initial_states, controls) -> torch.Tensor:
        """``J[n,i,j] = d f_i / d x_j``.  Generic autograd default (batch replicated ``d`` times,
        as upstream) for user models written in torch ops; the built-in
        dynamics models override it with the forward-mode HIP kernel (K5)."""
        with torch.enable_grad():
            N, d = initial_states.shape
            x = initial_states.detach().clone()[:, None, :].expand(N, d, d).contiguous()
            rep = tree_map(controls, lambda t: torch.repeat_interleave(t, repeats=d, dim=0))
            x.requires_grad_(True)
            y = self(initial_states=x.reshape(-1, d), controls=rep)[0].reshape(N, d, d)
            mask = torch.eye(d, dtype=x.dtype, device=x.device)[None].expand(N, d, d)
            (jac,) = torch.autograd.grad(y, x, mask, create_graph=True)
        return jac


class ParticleFilterMeasurementModel(nn.Module, abc.ABC):
    def __init__(self, *, state_dim: int):
        super().__init__()
        self.state_dim = state_dim

    @abc.abstractmethod
    def forward(self, *, states, observations) -> torch.Tensor:
        """``states (N, M, d)``, observations with leading ``N`` -> log-likelihoods ``(N, M)``."""


class KalmanFilterMeasurementModel(nn.Module, abc.ABC):
    def __init__(self, *, state_dim: int, observation_dim: int):
        super().__init__()
        self.state_dim = state_dim
        self.observation_dim = observation_dim

    @abc.abstractmethod
    def forward(self, *, states):
        """``(N, d) -> (expected observations (N, o), scale_tril (N, o, o))``."""


class VirtualSensorModel(nn.Module, abc.ABC):
    def __init__(self, *, state_dim: int):
        super().__init__()
        self.state_dim = state_dim

    @abc.abstractmethod
    def forward(self, *, observations):
        """observations -> ``(virtual observation (N, d), scale_tril (N, d, d))``."""


class Filter(nn.Module, abc.ABC):
    """Stateful recursive estimator; the belief lives on the module between calls and is
    reset by ``initialize_beliefs`` (``eval_helpers.py:128-131``)."""

    def __init__(self, *, state_dim: int):
        super().__init__()
        self.state_dim = state_dim

    @abc.abstractmethod
    def initialize_beliefs(self, *, mean: torch.Tensor, covariance: torch.Tensor) -> None:
        ...

    def forward(self, *, observations, controls) -> torch.Tensor:
        out = self.forward_loop(observations=tree_map(observations, lambda t: t[None]),
                                controls=tree_map(controls, lambda t: t[None]))
        return out[0]

    def forward_loop(self, *, observations, controls) -> torch.Tensor:
        """``(T, N, ...)`` in, ``(T, N, d)`` out (``eval_helpers.py:139-146``)."""
        from . import engine  # (engine imports this module's siblings)

        return engine.checked_loop(Filter._forward_loop_steps)(self, observations=observations, controls=controls)

    def _forward_loop_steps(self, *, observations, controls) -> torch.Tensor:
        T = tree_leading_shape(controls)[0]
        assert tree_leading_shape(observations)[0] == T
        out, beliefs = [], []
        for t in range(T):
            out.append(self(observations=tree_index(observations, t), controls=tree_index(controls, t)))
            if getattr(self, "record_belief", False):
                beliefs.append(self.last_belief)
        if beliefs:
            self.last_belief = stack_belief_records(beliefs)
        return torch.stack(out, dim=0)

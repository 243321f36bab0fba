"""Shared by the particle-smoother tests (``include/mmf.h``: ``mmf_pf_smooth``, ``mmf_pf_smooth_marginal``,
``mmf_pf_smooth_simulate``, ``mmf_pf_smooth_pair_moments``): the fp64 definitions the kernels are held to, the histories the
kernel cases run on, the exact linear-Gaussian answers, and the device- and host-side plumbing of the test files.  ``torch``
and the package are imported inside the functions that need them, so the CPU files import this module without a device."""
import ctypes
import math

import numpy as np
import pytest


# ------------------------------------------------------------------------------------------ the fp64 definitions
def softmax_rows(a):
    """``softmax`` over the last axis in fp64; ``-inf`` gives exactly 0."""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def moments(X, W):
    """Mean, covariance and ``1 / sum W^2`` of ``X (..., M, d)`` under ``W (..., M)`` in fp64; rows of zero weight are not read."""
    X = np.where((W > 0)[..., None], np.asarray(X, dtype=np.float64), 0.0)
    mean = np.einsum("...m,...md->...d", W, X)
    dx = np.where((W > 0)[..., None], X - mean[..., None, :], 0.0)
    return mean, np.einsum("...m,...mi,...mj->...ij", W, dx, dx), 1.0 / (W * W).sum(-1)


def reference(X, F, ll, lw, L):
    """The marginal smoother AND the two-slice moments by their definitions in fp64: ``X (T, N, M, d)``, ``F (T - 1, N, M, d)``,
    ``ll (T, N, M)``, ``lw (T, N, M)`` or None, ``L (d, d)`` -> ``dict`` of ``weights (T, N, M)`` = ``W_{t|T}``, their
    ``mean (T, N, d)``, ``cov (T, N, d, d)`` and ``ess (T, N)``, ``residual_mean (T - 1, N, d)``,
    ``residual_second_moment (T - 1, N, d, d)`` (raw), ``row_marginal (T - 1, N, M)`` = ``sum_j xi[i, j]`` and
    ``total (T - 1, N)`` = ``sum_ij xi`` BEFORE the final normalisation (1 by construction).
    The residual ``e = X_{t+1}[j] - F_t[i]`` is formed in the precision ``X`` and ``F`` come in (fp32 histories: in fp32, as
    the pair kernels form it; a caller that wants the fp64 difference passes fp64 arrays) and everything after it in fp64;
    particles of zero weight are left out of every sum, whatever their rows hold."""
    X, F = np.asarray(X), np.asarray(F)
    T, N, M, d = X.shape
    a = np.asarray(ll, dtype=np.float64) + (0.0 if lw is None else np.asarray(lw, dtype=np.float64))
    W = softmax_rows(a)
    Linv = np.linalg.inv(np.tril(np.asarray(L, dtype=np.float64)))
    S = np.zeros((T, N, M))
    S[T - 1] = W[T - 1]
    Tm = max(T - 1, 0)
    mean, second = np.zeros((Tm, N, d)), np.zeros((Tm, N, d, d))
    rowm, total = np.zeros((Tm, N, M)), np.zeros((Tm, N))
    for n in range(N):
        for t in range(T - 2, -1, -1):
            rows, cols = np.flatnonzero(W[t, n] > 0), np.flatnonzero(S[t + 1, n] > 0)
            e = (X[t + 1, n][cols][None, :, :] - F[t, n][rows][:, None, :]).astype(np.float64)  # the difference first, in the inputs' precision
            z = e @ Linv.T
            term = np.log(W[t, n][rows])[:, None] - 0.5 * (z * z).sum(-1)
            top = term.max(0)
            logD = top + np.log(np.exp(term - top).sum(0))
            xi = np.exp(term - logD[None, :]) * S[t + 1, n][cols][None, :]
            total[t, n] = xi.sum()
            rowm[t, n][rows] = xi.sum(1)
            S[t, n][rows] = rowm[t, n][rows] / total[t, n]
            xi = xi / total[t, n]
            mean[t, n] = np.einsum("ij,ijc->c", xi, e)
            second[t, n] = np.einsum("ij,ijc,ijk->ck", xi, e, e)
    smean, scov, ess = moments(X, S)
    return dict(weights=S, mean=smean, cov=scov, ess=ess, residual_mean=mean, residual_second_moment=second, row_marginal=rowm,
                total=total)


def ancestry_reference(X, ll, lw, lw0, A, lag):
    """Definition of ``mmf_pf_smooth`` in fp64 numpy: ``X (T, N, M, d)``, ``ll (T, N, M)``, ``lw (T, N, M)`` or None,
    ``lw0 (N, M)`` or None, ``A (T, N, M)`` or None (identity) -> mean, cov, unique."""
    T, N, M, d = X.shape
    L = min(int(lag), max(T - 1, 0))
    mean, cov, uniq = np.zeros((T, N, d)), np.zeros((T, N, d, d)), np.zeros((T, N), dtype=np.int64)
    for n in range(N):
        for t in range(T):
            s = min(t + L, T - 1)
            a = ll[s, n].astype(np.float64)
            if lw is not None:
                a = a + lw[s, n]
            elif s == 0 and lw0 is not None:
                a = a + lw0[n]
            b = np.arange(M)
            for r in range(s, t, -1):  # from step r to r - 1
                if A is not None:
                    b = A[r - 1, n][b]
            w = np.exp(a - a.max())
            w = w / w.sum()
            alive = a > -np.inf
            x = X[t, n].astype(np.float64)[b[alive]]
            mu = w[alive] @ x
            dx = x - mu
            mean[t, n], cov[t, n], uniq[t, n] = mu, (w[alive][:, None] * dx).T @ dx, len(np.unique(b[alive]))
    return mean, cov, uniq


def ancestry_reference_of_history(h, lag):
    T = h.states.shape[0]
    N = lambda x: None if x is None else x.cpu().numpy()
    return ancestry_reference(N(h.states), N(h.log_likelihoods), N(h.log_weights_in), None, N(h.ancestors), T if lag is None else lag)


# ------------------------------------------------------------------------------------------ the histories of the kernel cases
def systematic(w, u):
    """Ancestors of systematic resampling (numpy, fp64): positions ``(u + k) / M`` in the CDF of ``w``."""
    M = len(w)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    return np.minimum(np.searchsorted(cdf, (u + np.arange(M)) / M, side="right"), M - 1)


def tril(d, full, scale=0.02, seed=5, factor=1.0):
    """The process noise of the kernel cases: ``factor`` times a factor that is 0.01 .. 0.04 wide, diagonal or a full lower
    triangle."""
    L = np.diag(scale * np.array([1.0, 0.5, 2.0, 1.5])[:d])
    if full:
        L = L + np.tril(0.4 * scale * np.random.default_rng(seed).normal(size=(d, d)), -1)
    return (factor * L).astype(np.float32)


def make_case(T, N, M, d, widths, ll_scale, L, seed, use_lw=True, dead=False):
    """A run a filter could have left: step 0 is a cloud of the trajectory's width around an O(1) centre; every later set is
    drawn around the predictions ``F_t = X_t + drift_t`` of ancestors resampled systematically from the step's own weights
    (so the transition densities are not all negligible), with noise ``L``.  ``seed``: a seed, or the generator to go on
    drawing from.  ``use_lw`` off: the ancestors follow the likelihoods alone and the incoming log-weights returned are None.
    ``dead``: every 7th particle (from particle 3) has log-likelihood ``-inf`` and NaN rows in ``X`` and ``F``."""
    rng = np.random.default_rng(seed)
    widths = np.resize(np.asarray(widths, dtype=np.float64), N)
    X = np.zeros((T, N, M, d), dtype=np.float32)
    F = np.zeros((max(T - 1, 0), N, M, d), dtype=np.float32)
    ll = (ll_scale * rng.normal(size=(T, N, M))).astype(np.float32)
    lw = 0.3 * rng.normal(size=(T, N, M))
    lw = (lw - np.log(np.exp(lw).sum(-1, keepdims=True))).astype(np.float32)
    if dead:
        ll[:, :, 3::7] = -np.inf
    X[0] = rng.normal(size=(N, 1, d)) + widths[:, None, None] * rng.normal(size=(N, M, d))
    for t in range(T - 1):
        F[t] = X[t] + 0.05 * rng.normal(size=(N, 1, d))
        for n in range(N):
            a = ll[t, n].astype(np.float64) + (lw[t, n] if use_lw else 0.0)
            A = systematic(np.exp(a - a.max()), rng.uniform())
            X[t + 1, n] = F[t, n][A] + rng.normal(size=(M, d)) @ L.astype(np.float64).T
    if dead:
        X[:, :, 3::7] = np.nan
        F[:, :, 3::7] = np.nan
    return X, F, ll, (lw if use_lw else None)


def make_ancestry_case(T, N, M, d, widths, ll_scale, seed, same_ancestor=None):
    """Clouds of the given widths around an O(1) mean that drifts with the step; ancestors from systematic resampling of
    the step's own weights (so that high-likelihood particles have many descendants)."""
    rng = np.random.default_rng(seed)
    widths = np.resize(np.asarray(widths, dtype=np.float64), N)
    centre = rng.normal(size=(1, N, 1, d)) + 0.1 * rng.normal(size=(T, N, 1, d)).cumsum(0)
    X = (centre + widths[None, :, None, None] * rng.normal(size=(T, N, M, d))).astype(np.float32)
    ll = (ll_scale * rng.normal(size=(T, N, M))).astype(np.float32)
    lw = 0.3 * rng.normal(size=(T, N, M))
    lw = (lw - np.log(np.exp(lw).sum(-1, keepdims=True))).astype(np.float32)
    A = np.zeros((T, N, M), dtype=np.int32)
    for t in range(T):
        for n in range(N):
            a = ll[t, n].astype(np.float64) + lw[t, n]
            A[t, n] = systematic(np.exp(a - a.max()), rng.uniform()) if same_ancestor is None else same_ancestor
    return X, ll, lw, A


# ------------------------------------------------------------------------------------------ the linear-Gaussian known answers
def rts(z, m0, p0, q, r):
    """Exact Kalman filter and Rauch-Tung-Striebel smoother of ``x' = x + q eps``, ``z = x + r eps`` in fp64: every state
    dimension is a scalar problem with the same variances.  ``z (T, ...)``, prior ``N(m0, p0)`` before the first step."""
    T = z.shape[0]
    mf, pf, mp, pp = np.zeros_like(z), np.zeros(T), np.zeros_like(z), np.zeros(T)
    m, p = m0, p0
    for t in range(T):
        mp[t], pp[t] = m, p + q * q
        k = pp[t] / (pp[t] + r * r)
        m, p = mp[t] + k * (z[t] - mp[t]), (1.0 - k) * pp[t]
        mf[t], pf[t] = m, p
    ms = mf.copy()
    for t in range(T - 2, -1, -1):
        ms[t] = mf[t] + pf[t] / pp[t + 1] * (ms[t + 1] - mp[t + 1])
    return ms


def rts_em_step(z, m0, p0, q, r):
    """The exact EM step for the noise of ``x' = x + q eps`` observed through ``z = x + r eps``, in fp64: Kalman filter and
    Rauch-Tung-Striebel smoother under ``q`` (every state dimension is a scalar problem with the same variances), then
    ``q_new^2 = mean over t = 0 .. T - 2, trajectories and dimensions of E[(x_{t+1} - x_t)^2 | z_{0:T-1}]`` with the lag-one
    smoothed covariance ``Cov(x_{t+1}, x_t | z) = Ps_{t+1} G_t``, ``G_t = Pf_t / Pp_{t+1}``.  ``z (T, ...)``, prior
    ``N(m0, p0)`` before the first step.  Returns ``q_new``."""
    z = np.asarray(z, dtype=np.float64)
    T = z.shape[0]
    mf, pf, mp, pp = np.zeros_like(z), np.zeros(T), np.zeros_like(z), np.zeros(T)
    m, p = np.asarray(m0, dtype=np.float64), float(p0)
    for t in range(T):
        mp[t], pp[t] = m, p + q * q
        k = pp[t] / (pp[t] + r * r)
        m, p = mp[t] + k * (z[t] - mp[t]), (1.0 - k) * pp[t]
        mf[t], pf[t] = m, p
    ms, ps = mf.copy(), pf.copy()
    acc = 0.0
    for t in range(T - 2, -1, -1):
        g = pf[t] / pp[t + 1]
        ms[t] = mf[t] + g * (ms[t + 1] - mp[t + 1])
        ps[t] = pf[t] + g * g * (ps[t + 1] - pp[t + 1])
        acc += np.mean((ms[t + 1] - ms[t]) ** 2) + ps[t + 1] + ps[t] - 2.0 * ps[t + 1] * g
    return float(np.sqrt(acc / (T - 1)))


def bootstrap_filter_history(z, m0, p0, q, r, M, seed):
    """A bootstrap particle filter of the same model in fp64 numpy, systematic resampling at every step: ``z (T, N, d)``,
    ``m0 (N, d)`` -> the history ``X (T, N, M, d)``, ``F = X[:-1]`` (a random walk predicts its own state), ``ll (T, N, M)``;
    the incoming weights are uniform."""
    rng = np.random.default_rng(seed)
    T, N, d = z.shape
    X, ll = np.zeros((T, N, M, d)), np.zeros((T, N, M))
    x = np.asarray(m0, dtype=np.float64)[:, None, :] + np.sqrt(p0) * rng.normal(size=(N, M, d))
    for t in range(T):
        X[t] = x + q * rng.normal(size=(N, M, d))
        e = z[t][:, None, :] - X[t]
        ll[t] = -0.5 * (e * e).sum(-1) / (r * r)
        x = np.stack([X[t, n][systematic(np.exp(ll[t, n] - ll[t, n].max()), rng.uniform())] for n in range(N)])
    return X, X[:-1].copy(), ll


def linear_gaussian_models(d, q, r, dev, state_dependent=False):
    """User models of ``x' = x + q eps`` observed through ``z = x + r eps`` (``observations["z"]``)."""
    import torch

    from multimodalfilter_amd import base

    class RandomWalk(base.DynamicsModel):
        def __init__(self):
            super().__init__(state_dim=d)
            self.L = (q * torch.eye(d)).to(dev)

        def forward(self, *, initial_states, controls):
            L = self.L[None].expand(initial_states.shape[0], d, d)
            if state_dependent:
                L = L * (1.0 + initial_states[:, :1, None].abs())
            return initial_states, L

    class GaussianLik(base.ParticleFilterMeasurementModel):
        def __init__(self):
            super().__init__(state_dim=d)

        def forward(self, *, states, observations):
            e = observations["z"][:, None, :] - states
            return -0.5 * (e * e).sum(-1) / (r * r)

    return RandomWalk(), GaussianLik()


def cpu_filter_with_history(T=4, N=2, M=6, d=3, seed=77, state_dependent=False):
    """A random-walk filter on the CPU (``F_t = X_t``, ``L = 0.05 I``) holding a hand-made history, for the API tests that
    need no device: a record of the filter ``f``, ``dims = (T, N, M, d)``, the numpy arrays ``X``, ``ll``, ``lw`` the history
    was made from and the noise factor ``L``."""
    from types import SimpleNamespace

    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import base

    q = 0.05
    L = (q * np.eye(d)).astype(np.float32)
    X, _, ll, lw = make_case(T, N, M, d, (1e-2, 0.3), 0.5, L, seed=seed)
    dyn, meas = linear_gaussian_models(d, q, 0.3, torch.device("cpu"), state_dependent=state_dependent)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.last_history = base.history_record(states=torch.from_numpy(X), log_likelihoods=torch.from_numpy(ll),
                                         log_weights_in=torch.from_numpy(lw), ancestors=None, resampled=None,
                                         controls=torch.zeros((T, N, 7)))
    return SimpleNamespace(f=f, dims=(T, N, M, d), X=X, ll=ll, lw=lw, L=L)


# ------------------------------------------------------------------------------------------ on the device
def dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


def to_device(x, dtype=None):
    """A numpy array (or None) as a contiguous device tensor, float32 unless told otherwise."""
    import torch

    return None if x is None else torch.as_tensor(np.ascontiguousarray(x), dtype=dtype or torch.float32).to(dev())


def small_filter(cls, N, M, T, dev):
    """A task filter of ``M`` particles with calibrated measurement heads and ``N`` synthetic trajectories of ``T`` steps:
    filter, state dimension, trajectories, observations, controls, initial covariance."""
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic
    from oracle import models as om

    tname = "door" if cls.startswith("Door") else "push"
    d = om.TASKS[tname].state_dim
    torch.manual_seed(3)
    f = mmf.model_types(tname)[cls]().to(dev).eval()
    f.num_particles = M
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=17).items()}
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cal = traj["states"][0][:, None, :] + 0.3 * torch.randn((N, 256, d), device=dev)
    synthetic.calibrate_measurement_heads(f, {k: v[0] for k, v in obs.items()}, cal, target_std=1.2)
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
    return f, d, traj, obs, traj["controls"][1:], cov


def gpu_marginal(X, F, ll, lw, L, *, want_cov, want_ess, want_logd):
    """``_abi.pf_smooth_marginal`` on numpy inputs: ``dict`` of the device inputs ``X, F, ll, lw, L`` and of its outputs
    ``weights, mean, cov, ess, logd`` (NaN-filled before the call; the ones not wanted are None)."""
    import torch

    from multimodalfilter_amd import _abi

    d_ = dev()
    T, N, M, d = X.shape
    g = dict(X=to_device(X), F=to_device(F) if T > 1 else None, ll=to_device(ll), lw=to_device(lw), L=to_device(L))
    g["weights"] = torch.full((T, N, M), math.nan, device=d_)
    g["mean"] = torch.full((T, N, d), math.nan, device=d_)
    g["cov"] = torch.full((T, N, d, d), math.nan, device=d_) if want_cov else None
    g["ess"] = torch.full((T, N), math.nan, device=d_) if want_ess else None
    g["logd"] = torch.full((T - 1, N, M), math.nan, device=d_) if want_logd and T > 1 else None
    _abi.pf_smooth_marginal(g["X"], g["F"], g["ll"], g["lw"], g["L"], g["weights"], g["mean"], g["cov"], g["ess"], g["logd"])
    torch.cuda.synchronize()
    return g


def assert_symmetric_psd(c, what):
    """``c (..., d, d)`` on the device: symmetric bit for bit and PSD to ``-1e-4 x trace``."""
    import torch

    assert torch.equal(c, c.transpose(-1, -2)), what
    c = c.double().cpu()
    floor = -1e-4 * torch.diagonal(c, dim1=-2, dim2=-1).sum(-1)
    assert bool((torch.linalg.eigvalsh(c).min(-1).values >= floor - 1e-30).all()), what


# ------------------------------------------------------------------------------------------ on the host
def lib():
    from multimodalfilter_amd import _abi, build

    build.build()
    return _abi.load()


def host_args(struct_cls, pointer_fields, **over):
    """A ``struct_cls`` whose ``pointer_fields`` each point at a 16-float host buffer of their own (kept alive by the struct
    returned), with ``over`` set on top: what the entry points are handed to refuse on the host, before any HIP call."""
    a = struct_cls()
    a._buffers = [(ctypes.c_float * 16)() for _ in pointer_fields]
    for name, b in zip(pointer_fields, a._buffers):
        setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def alias_host_args(a, pointer_fields, alias):
    """Points fields of a ``host_args`` struct into the buffers of other fields: ``alias`` maps a field to ``(the field whose
    buffer it is pointed at, byte offset)``, or is ``None``.  Returns ``a``."""
    for field, (target, offset) in (alias or {}).items():
        setattr(a, field, ctypes.c_void_p(ctypes.addressof(a._buffers[pointer_fields.index(target)]) + offset))
    return a

"""Inputs, references and an independent truth for the innovation statistics and the NIS gate of the Kalman filters
(``mmf_ekf_step_innov`` / ``mmf_ekf_forward_loop_innov``, ``filters.InnovationSwitches``): pure numpy / torch-CPU, shared by
``test_innovation_cases_cpu.py`` (which certifies the inputs and the references without a GPU) and
``test_gpu_innovations.py`` (which runs the kernels on them).

Every case is built once (``functools.lru_cache``) and handed out read-only.  Nothing here replays the kernel's statements: the
step references are torch in fp64 (the truth) and fp32 (``torch.linalg.solve`` / ``slogdet``: the yardstick of the error rule),
the loop's truth is an fp64 Kalman filter in numpy, and ``dense_log_density`` never runs a recursion at all -- it writes the
joint Gaussian of all observations of a linear-Gaussian model down densely and evaluates its log-density.
"""
import functools
import math

import numpy as np
import torch

import _kalman_cases as kc
import _rts_cases as rc

NS = (1, 255, 257)                    # one lane; one short of a 256-block; one past it
DIMS = kc.DIMS
STEP_COMBOS = kc.STEP_COMBOS
GATE = 12.0                           # the NIS threshold of every gated case
NIS_MARGIN = (6.0, 24.0)              # no fp64 NIS of any case lies here: no fp32 evaluation can flip a decision
INLIER_C2, OUTLIER_C2 = (0.1, 2.0), (60.0, 200.0)

# caps on the fp32 torch yardstick's own error against fp64 (``_tol.rel_err``): conditions on the INPUTS, measured by
# test_innovation_cases_cpu.py over all cases (worst: nis 1.6e-6, log_likelihood 8.4e-6, gated mu 3.6e-5, gated Sigma
# 6.1e-5, fused mean 1.41e-3 and fused covariance 5.6e-4, both in the information form); a draw that breaks one is replaced
# through RESEED
CAP_INNOV = kc.CAP_STEP               # 1e-4: nis, log_likelihood, the gated mu and Sigma
CAP_INNOV_FUSED = kc.CAP_FUSED        # 1.7e-3: the fusion outputs of the gated beliefs

# (N, d, K) -> how many times the seed of the case's observations was replaced because a draw broke a cap: the ungated
# information-form mean of (255, 3, 3) came out at 2.0e-3 .. 3.7e-3 for reseeds 0 .. 5 and 1.41e-3 for 6
RESEED = {(255, 3, 3): 6}


def _t(a, dt):
    return torch.from_numpy(np.array(a)).to(dt)  # a copy: the cases are read-only


def _frozen(**arrays):
    for a in arrays.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


def _predicted(A, S0, L):
    """``Sigma- = A Sigma A^T + L L^T`` on torch tensors ``(K, N, d, d)`` with ``L (K, d, d)``: the expression of
    ``_kalman_cases.predict_correct``."""
    return A @ S0 @ A.transpose(-1, -2) + (L @ L.transpose(-1, -2))[:, None]


# ------------------------------------------------------------------------------ one step: a bimodal NIS by construction
@functools.lru_cache(maxsize=None)
def step_case(N, d, K):
    """``_kalman_cases.step_case(N, d, K)`` with other observations: ``z = mu- + c chol(S_fp64) u`` for a random unit vector
    ``u``, so that the NIS is ``c^2`` up to the rounding of ``z`` to float32 -- uniform in [0.1, 2] where ``(n + k) % 3 != 0``
    and uniform in [60, 200] elsewhere.  ``outlier (K, N)`` says which."""
    c = dict(kc.step_case(N, d, K))
    rng = np.random.RandomState(52000 + 1000 * d + 10 * K + (N % 7) + 10007 * RESEED.get((N, d, K), 0))
    A, S0, T, L, mp = (_t(c[k], torch.float64) for k in ("A", "S0", "T", "L", "mu_pred"))
    Sinn = (_predicted(A, S0, L) + T @ T.transpose(-1, -2)).numpy()
    chol = np.linalg.cholesky(0.5 * (Sinn + Sinn.transpose(0, 1, 3, 2)))
    u = rng.standard_normal((K, N, d))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    k_idx, n_idx = np.meshgrid(np.arange(K), np.arange(N), indexing="ij")
    outlier = (n_idx + k_idx) % 3 == 0
    c2 = np.where(outlier, rng.uniform(*OUTLIER_C2, (K, N)), rng.uniform(*INLIER_C2, (K, N)))
    z = mp.numpy() + np.sqrt(c2)[..., None] * np.einsum("knij,knj->kni", chol, u)
    c["z"] = z.astype(np.float32)
    c["outlier"] = outlier
    return _frozen(**c)


def _innovation(Sinn, nu, dtype):
    """``(nis, log_likelihood)`` of innovations ``nu (..., d)`` under ``N(0, Sinn)``: a solve and ``slogdet`` in ``dtype``."""
    d = nu.shape[-1]
    nis = (nu * torch.linalg.solve(Sinn, nu[..., None]).squeeze(-1)).sum(-1)
    logdet = torch.linalg.slogdet(Sinn)[1]
    return nis, -0.5 * (nis + logdet + d * math.log(2.0 * math.pi))


@functools.lru_cache(maxsize=None)
def step_reference(N, d, K, fusion, dtype, gate=None):
    """One ``mmf_ekf_step_innov`` (feedback 0) on ``step_case(N, d, K)`` in ``dtype``: ``nis``, ``log_likelihood``,
    ``accepted (K, N)`` and the gated ``mu``, ``Sigma``, ``mu_f``, ``Sigma_f`` (the fused ones ``None`` for fusion 0).  The
    decisions are those of the fp64 NIS in either ``dtype`` (the CPU test shows that no fp32 evaluation can differ)."""
    c = step_case(N, d, K)
    A, S0, T, L, mp, z, w = (_t(c[k], dtype) for k in ("A", "S0", "T", "L", "mu_pred", "z", "w"))
    mu, S, Sinn = kc.predict_correct(A, S0, T, L, mp, z)
    nis, ll = _innovation(Sinn, z - mp, dtype)
    if gate is None:
        accepted = torch.ones((K, N), dtype=torch.bool)
    elif dtype == torch.float64:
        accepted = nis <= gate
    else:
        accepted = step_reference(N, d, K, fusion, torch.float64, gate)["accepted"]
    mu = torch.where(accepted[..., None], mu, mp)
    S = torch.where(accepted[..., None, None], S, _predicted(A, S0, L))
    out = {"nis": nis, "log_likelihood": ll, "accepted": accepted, "mu": mu, "Sigma": S, "mu_f": None, "Sigma_f": None}
    if fusion:
        out["mu_f"], out["Sigma_f"] = kc.fuse_beliefs(fusion, w, mu, S)[:2]
    return out


# ------------------------------------------------------------------------------ the whole loop: a linear-Gaussian model
LG_T, LG_N, LG_D = rc.LG_T, rc.LG_N, 2
assert (LG_T, LG_N) == (6, 5)
DISPLACED = ((1, 0), (3, 1), (2, 3), (5, 3))   # (t, n) of the four observations moved by 10 sigma in the gated copy


def _lg(d):
    c = rc.lg_model(d)
    return tuple(np.array(c[k], dtype=np.float64) for k in ("A0", "A1", "b", "L", "F", "u", "m_init", "P_init"))


def kalman_filter(d, y, gate=None, dtype=np.float64, decisions=None):
    """The Kalman filter of ``_rts_cases.lg_model(d)`` on observations ``y (T, N, d)`` in numpy -- fp64, the truth, or
    ``dtype=np.float32``, the yardstick -- with the NIS gate when ``gate`` is given (``decisions (T, N)``: impose these
    instead of deciding; the yardstick takes the truth's): ``mean (T, N, d)``, ``cov``, ``nis``, ``log_likelihood`` and
    ``accepted (T, N)``, and the innovation covariances ``S (T, N, d, d)``."""
    A0, A1, b, L, F, u, m, P0 = (a.astype(dtype) for a in _lg(d))
    y = np.asarray(y, dtype=dtype)
    T, N = y.shape[:2]
    Q, R, eye = L @ L.T, F @ F.T, np.eye(d, dtype=dtype)
    P = np.broadcast_to(P0, (N, d, d)).copy()
    const = dtype(d * math.log(2.0 * math.pi))
    out = {k: [] for k in ("mean", "cov", "nis", "log_likelihood", "accepted", "S")}
    for t in range(T):
        At = A0 + u[t][:, :, None] * A1
        mp = np.einsum("nij,nj->ni", At, m) + u[t] * b
        Pp = At @ P @ At.transpose(0, 2, 1) + Q
        S = Pp + R
        nu = y[t] - mp
        nis = np.einsum("ni,ni->n", nu, np.linalg.solve(S, nu[..., None])[..., 0])
        ll = dtype(-0.5) * (nis + np.linalg.slogdet(S)[1].astype(dtype) + const)
        ok = decisions[t] if decisions is not None else (np.ones(N, dtype=bool) if gate is None else nis <= gate)
        G = Pp @ np.linalg.inv(S)
        m = np.where(ok[:, None], mp + np.einsum("nij,nj->ni", G, nu), mp)
        P = np.where(ok[:, None, None], (eye - G) @ Pp, Pp)
        for k, v in zip(out, (m, P, nis, ll, ok, S)):
            out[k].append(v)
    return {k: np.stack(v) for k, v in out.items()}


def dense_log_density(d, y):
    """``log N(y_{0:T-1}; m, C)`` per trajectory, ``(N,)``, for ``lg_model(d)`` with NO recursion over beliefs: the mean and
    the covariance of all ``T d`` observations of a trajectory are written down densely (the construction of
    ``_rts_cases.dense_smoother``) and the log-density is one Cholesky factorisation."""
    A0, A1, b, L, F, u, m_init, P0 = _lg(d)
    T, N = y.shape[:2]
    Q, R = L @ L.T, F @ F.T
    out = np.zeros(N)
    for n in range(N):
        At = [A0 + u[t, n, 0] * A1 for t in range(T)]
        m = np.zeros((T, d))
        C = np.zeros((T, d, T, d))  # Cov(x_s, x_t)
        pm, pC = m_init[n], P0
        for t in range(T):
            m[t] = At[t] @ pm + u[t, n, 0] * b
            C[t, :, t] = At[t] @ pC @ At[t].T + Q
            for s in range(t):
                C[s, :, t] = C[s, :, t - 1] @ At[t].T
                C[t, :, s] = C[s, :, t].T
            pm, pC = m[t], C[t, :, t]
        Cyy = C.reshape(T * d, T * d) + np.kron(np.eye(T), R)
        r = y[:, n].reshape(-1) - m.reshape(-1)
        chol = np.linalg.cholesky(Cyy)
        white = np.linalg.solve(chol, r)
        out[n] = -0.5 * (white @ white) - np.log(np.diag(chol)).sum() - 0.5 * T * d * math.log(2.0 * math.pi)
    return out


@functools.lru_cache(maxsize=None)
def lg_case(displaced=False):
    """``lg_model(2)``: observations ``y``, controls ``u``, the prior, and the fp64 filter's results -- ungated on the model's
    own observations, or (``displaced``) with gate ``GATE`` on a copy whose four observations ``DISPLACED`` are moved by
    ``10 chol(S) e`` (``S`` the innovation covariance of the ungated filter there, ``e`` the unit vector along
    ``(1, ..., 1)``), float32 values in float64 arrays as the model's own."""
    d = LG_D
    c = rc.lg_model(d)
    y = np.array(c["y"], dtype=np.float64)
    gate = None
    if displaced:
        clean = kalman_filter(d, y)
        e = np.ones(d) / math.sqrt(d)
        for t, n in DISPLACED:
            y[t, n] += 10.0 * np.linalg.cholesky(clean["S"][t, n]) @ e
        y = y.astype(np.float32).astype(np.float64)
        gate = GATE
    truth = kalman_filter(d, y, gate)
    return _frozen(y=y, u=np.array(c["u"]), m_init=np.array(c["m_init"]), P_init=np.array(c["P_init"]), gate=gate, **truth)

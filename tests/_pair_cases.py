"""Shared by the two-slice smoothing-moment tests (``include/mmf.h``: ``mmf_pf_smooth_pair_moments``): the definition in fp64
numpy, the histories the kernel cases run on, and the exact linear-Gaussian EM step the estimator is held to.  Test files
are not imported from each other, so the case generator of ``test_gpu_marginal_smoothing.py`` is restated here."""
import numpy as np


def softmax_rows(a):
    """``softmax`` over the last axis in fp64; ``-inf`` gives exactly 0."""
    a = np.asarray(a, dtype=np.float64)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def reference(X, F, ll, lw, L):
    """The marginal smoother AND the two-slice moments by their definitions in fp64: ``X (T, N, M, d)``, ``F (T - 1, N, M, d)``,
    ``ll (T, N, M)``, ``lw (T, N, M)`` or None, ``L (d, d)`` -> ``dict`` of ``weights (T, N, M)`` = ``W_{t|T}``,
    ``residual_mean (T - 1, N, d)``, ``residual_second_moment (T - 1, N, d, d)`` (raw), ``row_marginal (T - 1, N, M)`` =
    ``sum_j xi[i, j]`` and ``total (T - 1, N)`` = ``sum_ij xi`` BEFORE the final normalisation (1 by construction).
    The residual ``e = X_{t+1}[j] - F_t[i]`` is formed in the precision ``X`` and ``F`` come in (fp32 histories: in fp32, as
    the kernels form it) and everything after it in fp64; particles of zero weight are left out of every sum, whatever
    their rows hold."""
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
    return dict(weights=S, residual_mean=mean, residual_second_moment=second, row_marginal=rowm, total=total)


def systematic(w, u):
    """Ancestors of systematic resampling (numpy, fp64): positions ``(u + k) / M`` in the CDF of ``w``."""
    M = len(w)
    cdf = np.cumsum(w / w.sum())
    cdf[-1] = 1.0
    return np.minimum(np.searchsorted(cdf, (u + np.arange(M)) / M, side="right"), M - 1)


def tril(d, full, scale=0.02, seed=5):
    """The process noise of the kernel cases: 0.01 .. 0.04 wide, diagonal or a full lower triangle."""
    L = np.diag(scale * np.array([1.0, 0.5, 2.0, 1.5])[:d])
    if full:
        L = L + np.tril(0.4 * scale * np.random.default_rng(seed).normal(size=(d, d)), -1)
    return L.astype(np.float32)


def make_case(T, N, M, d, widths, ll_scale, L, seed):
    """A run a filter could have left: step 0 is a cloud of the trajectory's width around an O(1) centre; every later set is
    drawn around the predictions ``F_t = X_t + drift_t`` of ancestors resampled systematically from the step's own weights
    (so the transition densities are not all negligible), with noise ``L``."""
    rng = np.random.default_rng(seed)
    widths = np.resize(np.asarray(widths, dtype=np.float64), N)
    X = np.zeros((T, N, M, d), dtype=np.float32)
    F = np.zeros((max(T - 1, 0), N, M, d), dtype=np.float32)
    ll = (ll_scale * rng.normal(size=(T, N, M))).astype(np.float32)
    lw = 0.3 * rng.normal(size=(T, N, M))
    lw = (lw - np.log(np.exp(lw).sum(-1, keepdims=True))).astype(np.float32)
    X[0] = rng.normal(size=(N, 1, d)) + widths[:, None, None] * rng.normal(size=(N, M, d))
    for t in range(T - 1):
        F[t] = X[t] + 0.05 * rng.normal(size=(N, 1, d))
        for n in range(N):
            a = ll[t, n].astype(np.float64) + lw[t, n]
            A = systematic(np.exp(a - a.max()), rng.uniform())
            X[t + 1, n] = F[t, n][A] + rng.normal(size=(M, d)) @ L.astype(np.float64).T
    return X, F, ll, lw


# ------------------------------------------------------------------------------------------ the linear-Gaussian known answer
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

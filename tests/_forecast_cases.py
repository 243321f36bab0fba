"""Inputs and fp64 reference of the predictive-mixture kernel (``include/mmf.h``: ``MmfPfPredictiveArgs`` /
``mmf_pf_predictive``), in numpy / torch on the CPU; shared by ``test_forecast_cases_cpu.py`` and ``test_gpu_forecast.py``.

The reference is the header's definition in fp64: ``a = log_a + log_b`` and ``t = a - max a`` with the kernel's own two fp32
operations (``_summary_cases.log_weight32``), then ``w = exp(float64(t))``, ``W = w / sum w`` over the particles with ``w > 0``
only (a dead particle's NaN row is selected away), ``Q = L L^T``, ``sigma_k = sqrt(Q_kk)`` and

    mean = sum W F                                   covariance = sum W (F - mean)(F - mean)^T + Q
    log_score = logsumexp_i(log W_i - 1/2 |L^-1 (y - F_i)|^2) - sum log L_kk - d/2 log 2 pi
    pit[k] = sum W Phi((y_k - F_ik) / sigma_k)
    spread[k] = sum_i sum_j W_i W_j A(F_ik - F_jk; sqrt(2) sigma_k)        crps[k] = sum W A(y_k - F_ik; sigma_k) - 1/2 spread[k]
    A(m; s) = m erf(m / (s sqrt 2)) + s sqrt(2 / pi) exp(-m^2 / (2 s^2))

the pairs in chunks of ``CHUNK`` rows so that no ``(M, M, d)`` array is formed.  The kernel is held to ``_tol.REL_TOL``: the
scalar scores under ``rel_err_elementwise(floor=1e-3)``, ``mean`` and ``covariance`` under ``rel_err``; ``CAP`` is the
condition on the INPUTS that makes that bar fair: the same formulation in fp32 torch ops must stay within ``REL_TOL / 3`` of
the reference."""
import functools
import math

import numpy as np
import torch

import _smooth_cases as sc
import _summary_cases as sm
from _summary_cases import CHUNK, GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as fk.* by the tests)

# the kernel's own sizes (csrc/pf_summary.h): a row is one workgroup with one i-particle per thread up to I_BLOCK particles and
# ceil(M / I_BLOCK) workgroups with two beyond; j-tiles of J_TILE particles; fp32 runs of RUN pairs
I_BLOCK, J_TILE, RUN = 512, 1024, 64
MS = (1, 2, 63, 64, 65, 257, I_BLOCK - 1, I_BLOCK, I_BLOCK + 1, J_TILE - 1, J_TILE, J_TILE + 1)
BIG_M = 4096                     # one case
SMALL = 257                      # up to here the whole cross; beyond, every variant once
DIMS = (1, 2, 3, 4)
RS = (1, 3)
SCALES = (0.02, 0.3, 3.0)        # of the full lower-triangular L: far below, about and far above the spacing of the centres
VARIANTS = ("plain", "uniform", "only_a", "dead_row", "dead_particles", "nan_truth", "no_truth")
SPECIALS = ("equal_centres", "far_truth")
OUTPUTS = ("mean", "covariance", "log_score", "pit", "spread", "crps")
NEED_TRUTH = ("log_score", "pit", "crps")
NORMWISE = ("mean", "covariance")  # held under rel_err; the others under rel_err_elementwise(floor=1e-3)
CAP = 3e-5                       # REL_TOL / 3, the margin CAP_RTS uses
FAR = 50.0                       # sigmas between the truth and every centre in "far_truth"


def scale_tril(d, scale):
    """The full lower-triangular factor at ``scale`` (``_smooth_cases.tril``): diagonal ``scale (1, 0.5, 2, 1.5)``."""
    return sc.tril(d, True, scale=scale)


def make_case(M, d, R, variant="plain", scale=0.3, seed=0):
    """``dict(states (R, M, d) -- the centres --, log_a, log_b (R, M) or None, scale_tril (d, d), truth (R, d) or None)``: the
    weighted set of ``_summary_cases.weighted_set`` with truths that cycle per row through a draw from the mixture itself (a
    live centre plus ``L eps``), the live mean + 5 and N(0, 1).  ``dead_particles``: every third particle from particle 1 is
    dead too, with a NaN row, at every ``M > 1``.  ``equal_centres``: every centre of a row is the row's first.
    ``far_truth``: the truth lies ``FAR`` sigmas beyond the largest centre in every dimension."""
    names = VARIANTS + SPECIALS
    assert variant in names and scale in SCALES
    rng = np.random.default_rng(3000017 * M + 1013 * d + 103 * R + 11 * names.index(variant) + 7 * SCALES.index(scale) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, variant)
    L = scale_tril(d, scale)
    if variant == "dead_particles" and M > 1:
        dead = np.arange(1, M, 3)
        lb[:, dead] = -np.inf
        X[:, dead] = np.nan
        live[:, dead] = False
    if variant == "equal_centres":
        for r in range(R):
            X[r, live[r]] = X[r, live[r]][0] if live[r].any() else np.float32(0.25)
    sigma = np.sqrt(np.diag(L.astype(np.float64) @ L.astype(np.float64).T))
    truth = np.empty((R, d), np.float32)
    for r in range(R):
        xs = X[r][live[r]] if live[r].any() else np.zeros((1, d), np.float32)
        kind = (r + M + seed) % 3
        drawn = xs[rng.integers(0, len(xs))] + L @ rng.standard_normal(d)
        truth[r] = (drawn, xs.mean(0) + 5.0, rng.standard_normal(d))[kind]
        if variant == "far_truth":
            truth[r] = xs.max(0) + FAR * sigma
    if variant == "nan_truth":
        truth[R // 2, (M + R) % d] = np.nan
    if variant == "no_truth":
        truth = None
    return dict(states=X, log_a=la, log_b=lb, scale_tril=L, truth=truth)


def family():
    """``(M, d, R, variant, scale)``: up to ``SMALL`` particles the whole cross of dimensions, rows, variants and scales, and
    the two special cases at every dimension and scale; beyond it every variant once with the dimension and the scale
    cycling (three rows for ``plain`` and ``dead_row``, one otherwise), ``plain`` at every dimension and the specials once;
    and one case of ``BIG_M`` particles."""
    for M in MS:
        if M <= SMALL:
            for d in DIMS:
                for scale in SCALES:
                    for R in RS:
                        for variant in VARIANTS:
                            yield M, d, R, variant, scale
                    for variant in SPECIALS:
                        yield M, d, 3, variant, scale
            continue
        for i, variant in enumerate(VARIANTS + SPECIALS):
            yield M, DIMS[(i + M) % len(DIMS)], 3 if variant in ("plain", "dead_row") else 1, variant, SCALES[(i + M) % len(SCALES)]
        for i, d in enumerate(DIMS):
            yield M, d, 1, "plain", SCALES[(i + M + 1) % len(SCALES)]
    yield BIG_M, 3, 1, "plain", 0.3


ALL_MS = MS + (BIG_M,)


def _erf(x):
    return torch.erf(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def expected_abs(m, s):
    """``A(m; s) = E|Z|`` for ``Z ~ N(m, s^2)``, fp64."""
    m = np.asarray(m, np.float64)
    return m * _erf(m / (s * math.sqrt(2.0))) + s * math.sqrt(2.0 / math.pi) * np.exp(-m * m / (2.0 * s * s))


def normal_cdf(z):
    return 0.5 * (1.0 + _erf(np.asarray(z, np.float64) / math.sqrt(2.0)))


def reference_rows(F, W, L, truth):
    """The definition on centres ``F (R, M, d)`` under unnormalised fp64 weights ``W (R, M)``: a dict of float64 arrays,
    ``log_score``, ``pit`` and ``crps`` ``None`` without a truth."""
    R, M, d = F.shape
    L = np.asarray(L, np.float64)
    Q = L @ L.T
    sigma = np.sqrt(np.diag(Q))
    out = dict(mean=np.full((R, d), np.nan), covariance=np.full((R, d, d), np.nan), spread=np.full((R, d), np.nan),
               log_score=None, pit=None, crps=None)
    if truth is not None:
        out.update(log_score=np.full((R,), np.nan), pit=np.full((R, d), np.nan), crps=np.full((R, d), np.nan))
    for r in range(R):
        live = W[r] > 0
        if not live.any():
            continue
        x = F[r][live].astype(np.float64)
        w = W[r][live] / W[r][live].sum()
        mean = w @ x
        e = x - mean
        out["mean"][r] = mean
        out["covariance"][r] = (w[:, None] * e).T @ e + Q
        acc = np.zeros(d)
        for c in range(0, len(x), CHUNK):
            wc = w[c:c + CHUNK]
            for k in range(d):
                m = x[c:c + CHUNK, k, None] - x[None, :, k]  # (chunk, n): one dimension at a time
                acc[k] += wc @ expected_abs(m, math.sqrt(2.0) * sigma[k]) @ w
        out["spread"][r] = acc
        if truth is not None:
            with np.errstate(invalid="ignore"):
                y = truth[r].astype(np.float64)
                z = np.linalg.solve(L, (y - x).T)  # (d, n)
                expo = np.log(w) - 0.5 * (z * z).sum(0)
                top = expo.max()
                out["log_score"][r] = (top + np.log(np.exp(expo - top).sum()) - np.log(np.diag(L)).sum()
                                       - 0.5 * d * math.log(2.0 * math.pi))
                for k in range(d):
                    out["pit"][r, k] = w @ normal_cdf((y[k] - x[:, k]) / sigma[k])
                    out["crps"][r, k] = w @ expected_abs(y[k] - x[:, k], sigma[k]) - 0.5 * acc[k]
    return out


def reference(case):
    """The six outputs of a case by the fp64 definition; NaN where the definition puts it."""
    return reference_rows(case["states"], sm.weights64(case), case["scale_tril"], case["truth"])


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, variant, scale):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    case = make_case(M, d, R, variant, scale)
    return case, reference(case)


def torch_formulation(case, dtype=None, chunk=CHUNK):
    """The same definition in torch ops on the CPU, fp32 unless told otherwise: weights ``exp(t) / sum``, dead particles
    (weight 0) with their rows zeroed, chunked broadcast differences.  What a caller without the kernel would write."""
    dtype = dtype or torch.float32
    X = torch.from_numpy(np.ascontiguousarray(case["states"])).to(dtype)
    R, M, d = X.shape
    with np.errstate(invalid="ignore"):
        t = torch.from_numpy(sm.log_weight32(case)).to(dtype)
    w = torch.where(t <= 0, torch.exp(t), torch.zeros_like(t))
    S = w.sum(-1, keepdim=True)
    W = w / S
    X = torch.where((w > 0)[..., None], X, torch.zeros_like(X))
    L = torch.from_numpy(case["scale_tril"]).to(dtype)
    Q = L @ L.t()
    sigma = torch.sqrt(torch.diagonal(Q))
    A = lambda m, s: m * torch.erf(m / (s * math.sqrt(2.0))) + s * math.sqrt(2.0 / math.pi) * torch.exp(-m * m / (2.0 * s * s))
    mean = (W[..., None] * X).sum(1)
    e = X - mean[:, None, :]
    out = dict(mean=mean, covariance=torch.einsum("rm,rmi,rmj->rij", W, e, e) + Q, log_score=None, pit=None, crps=None)
    spread = torch.zeros((R, d), dtype=dtype)
    for c in range(0, M, chunk):
        m = X[:, c:c + chunk, None, :] - X[:, None, :, :]
        ww = W[:, c:c + chunk, None] * W[:, None, :]
        spread += (ww[..., None] * A(m, math.sqrt(2.0) * sigma)).sum((1, 2))
    dead = ~(S[:, 0] > 0)
    spread[dead] = math.nan
    out["spread"] = spread
    if case["truth"] is None:
        return out
    y = torch.from_numpy(case["truth"]).to(dtype)
    m = y[:, None, :] - X
    z = torch.linalg.solve_triangular(L, m.transpose(-1, -2), upper=False)  # (R, d, M)
    expo = torch.log(W) - 0.5 * (z * z).sum(1)
    out["log_score"] = torch.logsumexp(expo, dim=1) - torch.log(torch.diagonal(L)).sum() - 0.5 * d * math.log(2.0 * math.pi)
    out["pit"] = (W[..., None] * (0.5 * torch.erfc(-m / (sigma * math.sqrt(2.0))))).sum(1)
    out["crps"] = (W[..., None] * A(m, sigma)).sum(1) - 0.5 * spread
    return out


def compare(got, want, name, what=""):
    """Holds one output to its reference: NaN exactly where the reference has it, and returns the error over the rest
    (0.0 when nothing is finite): ``rel_err`` for ``mean`` and ``covariance``, ``rel_err_elementwise(floor=1e-3)`` otherwise."""
    from _tol import rel_err, rel_err_elementwise

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, name, "NaN placement", got, want)
    if nan.all():
        return 0.0
    got, want = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    if name in NORMWISE:
        return rel_err(torch.from_numpy(got), torch.from_numpy(want), dims=1 if name == "mean" else 2)
    return rel_err_elementwise(got, want, floor=1e-3)

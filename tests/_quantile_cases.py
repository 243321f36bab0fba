"""Inputs, fp64 reference and acceptance rule of the particle-quantile kernel (``include/mmf.h``: ``MmfPfQuantilesArgs`` /
``mmf_pf_quantiles``), in numpy; shared by ``test_quantile_cases_cpu.py`` and ``test_gpu_quantiles.py``.

The weights: ``a = log_a + log_b`` and ``t = a - max a`` with the kernel's own two fp32 operations, then ``w = exp(float64(t))``
and every sum in fp64.  With ``F(v) = sum_{x <= v} w / S`` and ``F-(v) = sum_{x < v} w / S``:

* a quantile ``v`` returned for ``p`` must be, bit for bit, the coordinate of a live particle of its row, with
  ``F(v) >= p - eps`` and ``F-(v) < p + eps``;
* a cdf must be within ``eps`` of ``F(query)``;
* ``eps = (M + 16) 2^-24``, derived and not measured: the kernel truncates each of the ``M`` weights by at most ``2^-24``
  against a total of at least 1 (the heaviest particle has ``e = 1``), plus a few ulps of ``expf`` on numerator and
  denominator.  Equality with the fp64 pick is NOT the bar: particles below ``2^-24`` of the heaviest are weightless to the
  kernel (K1's fixed point), so at ``p = 0`` / ``p = 1`` and at crossings inside the band the two may differ.

``p`` is the float32 the kernel is handed: ``float32(0.025) > 0.025``, so with 1000 equal weights the exact index is
``ceil(float32(0.025) * 1000) = 26``."""
import math

import numpy as np

import _summary_cases as sm
from _summary_cases import GUARD_ROWS, MAX_M, SENTINEL, log_weight32, weights64  # noqa: F401 (read as qc.* by the tests)

MS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)  # around a wave, a 256-block, a non-power-of-two, the workload's own size
DIMS = (1, 2, 3, 4)
RS = (1, 5)
PROBS = (0.0, 0.025, 0.05, 0.25, 0.5, 0.75, 0.95, 0.975, 1.0)
VARIANTS = ("plain", "dead_row", "uniform", "only_a", "only_b", "cdf_only", "query_particle", "query_below", "query_above")
EXACT = tuple((M, dead) for M in (1, 2, 63, 64, 65, 257, 1000) for dead in (False, True) if M > 8 or not dead)  # (M, an eighth dead)
REF_EPS = 1e-12


def eps(M):
    return (M + 16) * 2.0 ** -24


def probs32(probs=PROBS):
    """The probabilities as the kernel sees them: float32 values, as Python floats."""
    return tuple(float(np.float32(p)) for p in probs)


def make_case(M, d, R, variant="plain", seed=0):
    """``dict(states (R, M, d), log_a, log_b (R, M) or None, query (R, d), probs)`` of the family: the weighted set of
    ``_summary_cases.weighted_set`` with queries that cycle through a particle's own value, below all, above all, N(0, 1) and
    NaN unless the variant fixes the kind."""
    assert variant in VARIANTS
    rng = np.random.default_rng(1000003 * M + 1009 * d + 101 * R + 7 * VARIANTS.index(variant) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, variant)
    query = np.empty((R, d), np.float32)
    kinds = {"query_particle": 0, "query_below": 1, "query_above": 2}
    for r in range(R):
        xs = X[r][live[r]] if live[r].any() else np.zeros((1, d), np.float32)
        for k in range(d):
            kind = kinds.get(variant, (r * d + k + M + seed) % 5)
            col = xs[:, k]
            query[r, k] = (col[rng.integers(0, len(col))], col.min() - 1.0, col.max() + 1.0, rng.standard_normal(), np.nan)[kind]
    return dict(states=X, log_a=la, log_b=lb, query=query, probs=() if variant == "cdf_only" else PROBS)


def exact_case(M, d, R, dead, seed=0):
    """Equal weights (``log_a`` one constant, ``log_b`` 0 or ``-inf``): the result is a rank of the live particles."""
    rng = np.random.default_rng(77 * M + 5 * d + R + 1000 * int(dead) + seed)
    X = sm.duplicated_states(rng, M, d, R)
    la = np.full((R, M), -math.log(M), np.float32)
    lb = None
    if dead:
        lb = np.zeros((R, M), np.float32)
        sm.kill_an_eighth(rng, X, lb)
    query = np.empty((R, d), np.float32)
    for r in range(R):
        for k in range(d):
            col = X[r, :, k][~np.isnan(X[r, :, k])]
            query[r, k] = (col[rng.integers(0, len(col))], rng.standard_normal(), col.max(), col.min() - 1.0)[(r + k) % 4]
    return dict(states=X, log_a=la, log_b=lb, query=query, probs=PROBS)


def exact_expected(case):
    """``np.sort(x)[max(1, ceil(p n)) - 1]`` and ``float32(count / n)`` over the ``n`` live particles of each row."""
    X, lb, query = case["states"], case["log_b"], case["query"]
    R, M, d = X.shape
    ps = probs32(case["probs"])
    quant = np.empty((R, len(ps), d), np.float32)
    cdf = np.empty((R, d), np.float32)
    for r in range(R):
        live = np.ones(M, bool) if lb is None else np.isfinite(lb[r])
        for k in range(d):
            xs = np.sort(X[r, live, k])
            n = len(xs)
            for i, p in enumerate(ps):
                quant[r, i, k] = xs[max(1, math.ceil(p * n)) - 1]
            cdf[r, k] = np.float32(np.count_nonzero(xs <= query[r, k]) / n)
    return quant, cdf


def _sorted_cdf(x, w):
    """The live particles of one row and dimension ascending by ``x``, with the inclusive sums of their weights."""
    live = w > 0
    order = np.argsort(x[live], kind="stable")
    xs, ws = x[live][order], w[live][order]
    return xs, np.cumsum(ws)


def _F(xs, cs, v, side):
    j = np.searchsorted(xs, v, side=side)
    return 0.0 if j == 0 else cs[j - 1] / cs[-1]


def reference(case):
    """The fp64 pick: the first particle, ascending by ``x``, whose inclusive weight sum reaches ``p S``; and ``F(query)``."""
    X, query = case["states"], case["query"]
    R, M, d = X.shape
    ps = probs32(case["probs"])
    W = weights64(case)
    quant = np.full((R, len(ps), d), np.nan, np.float32)
    cdf = np.full((R, d), np.nan, np.float64)  # (not rounded to fp32: it is held to REF_EPS)
    for r in range(R):
        if not W[r].sum() > 0:
            continue
        for k in range(d):
            xs, cs = _sorted_cdf(X[r, :, k], W[r])
            for i, p in enumerate(ps):
                quant[r, i, k] = xs[min(np.searchsorted(cs, p * cs[-1], side="left"), len(xs) - 1)]
            if not np.isnan(query[r, k]):
                cdf[r, k] = _F(xs, cs, query[r, k], "right")
    return quant, cdf


def fixed_point(case):
    """The kernel's definition restated on the host: numpy's fp32 ``exp`` for ``expf``, ``q = floor(e 2^24)``, integer sums."""
    X, query = case["states"], case["query"]
    R, M, d = X.shape
    ps = probs32(case["probs"])
    q = sm.fixed_point_weights(case)
    quant = np.full((R, len(ps), d), np.nan, np.float32)
    cdf = np.full((R, d), np.nan, np.float32)
    for r in range(R):
        Qtot = int(q[r].sum())
        if Qtot == 0:
            continue
        for k in range(d):
            x = X[r, :, k]
            keys = x.view(np.uint32).astype(np.uint64)
            keys = np.where(keys & 0x80000000, ~keys & 0xFFFFFFFF, keys | 0x80000000)
            order = np.argsort((keys << np.uint64(32)) | q[r].astype(np.uint64), kind="stable")
            c = np.cumsum(q[r][order])
            for i, p in enumerate(ps):
                thr = max(1, int(math.ceil(p * float(Qtot))))
                quant[r, i, k] = x[order[np.searchsorted(c, thr, side="left")]]
            if not np.isnan(query[r, k]):
                with np.errstate(invalid="ignore"):
                    cdf[r, k] = np.float32(float(q[r][x <= query[r, k]].sum()) / float(Qtot))
    return quant, cdf


def check(case, quant, cdf, tol=None):
    """Holds ``quant (R, Q, d)`` (or None for no probabilities) and ``cdf (R, d)`` to the rule; returns the worst distance of
    a quantile from its band's centre side (``max(p - F, F- - p, 0)``) and the worst cdf error."""
    X, query = case["states"], case["query"]
    R, M, d = X.shape
    ps = probs32(case["probs"])
    tol = eps(M) if tol is None else tol
    W = weights64(case)
    worst_q = worst_c = 0.0
    for r in range(R):
        if not W[r].sum() > 0:
            assert quant is None or bool(np.isnan(quant[r]).all()), ("a row without a live particle", r)
            assert bool(np.isnan(cdf[r]).all()), ("a row without a live particle", r)
            continue
        for k in range(d):
            xs, cs = _sorted_cdf(X[r, :, k], W[r])
            bits = set(xs.view(np.uint32).tolist())
            for i, p in enumerate(ps):
                v = quant[r, i, k]
                assert int(np.float32(v).view(np.uint32)) in bits, ("not a live particle's value", r, k, p, v)
                F, Fm = _F(xs, cs, v, "right"), _F(xs, cs, v, "left")
                assert F >= p - tol and Fm < p + tol, (r, k, p, float(v), F, Fm, tol)
                worst_q = max(worst_q, p - F, Fm - p)
            if np.isnan(query[r, k]):
                assert np.isnan(cdf[r, k]), ("a NaN query", r, k)
            else:
                err = abs(float(cdf[r, k]) - _F(xs, cs, query[r, k], "right"))
                assert err <= tol, (r, k, float(query[r, k]), float(cdf[r, k]), err, tol)
                worst_c = max(worst_c, err)
    return worst_q, worst_c


def family():
    for M in MS:
        for d in DIMS:
            for R in RS:
                for variant in VARIANTS:
                    yield M, d, R, variant

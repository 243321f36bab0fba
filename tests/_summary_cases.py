"""What the case modules of the particle-posterior summaries share (``_quantile_cases``, ``_score_cases``, ``_density_cases``,
``_mode_cases``, ``_distance_cases``, ``_forecast_cases``): the sizes and sentinels of their tests, the generator of a weighted
particle set, and the weights as the kernels form them (``csrc/pf_summary.h``) -- ``t = (log_a + log_b) - max`` in the kernels'
own two fp32 operations, then fp64, or K1's integer fixed point (``csrc/pf_sort.h``).

The generator draws from the caller's ``rng``, and in one fixed order: each case module keeps its own seed formula and its own
tail (queries, truths, scale, rule), so a case depends on nothing but its module's arguments."""
import math

import numpy as np

MAX_M = 16384       # particles per row that the entry points serve (csrc/pf_summary.h: kMaxM)
SENTINEL = -77.25   # what a guard row and an output that was not asked for hold
GUARD_ROWS = 2
CHUNK = 256         # rows of a chunk of the fp64 pair references


def duplicated_states(rng, M, d, R):
    """``(R, M, d)`` N(0, 1) states, half of them copies of others (resampled sets are full of duplicates)."""
    X = rng.standard_normal((R, M, d)).astype(np.float32)
    for r in range(R):
        dst = rng.choice(M, M // 2, replace=False)
        X[r, dst] = X[r, rng.integers(0, M, M // 2)]
    return X


def kill_an_eighth(rng, X, lb):
    """An eighth of the particles of every row dead, in place: ``log_b = -inf`` and a NaN state row."""
    R, M, _ = X.shape
    for r in range(R):
        dead = rng.choice(M, M // 8, replace=False)
        lb[r, dead] = -np.inf
        X[r, dead] = np.nan


def weighted_set(rng, M, d, R, variant):
    """``(states (R, M, d), log_a, log_b (R, M) or None, live (R, M) bool)``: ``duplicated_states``, ``log_a = -log M + 0.3
    N(0, 1)``, ``log_b = -40 + 6 N(0, 1)``; for ``M > 8`` an eighth of the particles dead.  ``variant``: ``"dead_row"`` (row
    ``R // 2`` without a live particle), ``"uniform"`` (no log-weights, no NaN), ``"only_a"`` (``log_b``'s values as
    ``log_a``), ``"only_b"``; every other name is the plain set."""
    X = duplicated_states(rng, M, d, R)
    la = (-math.log(M) + 0.3 * rng.standard_normal((R, M))).astype(np.float32)
    lb = (-40.0 + 6.0 * rng.standard_normal((R, M))).astype(np.float32)
    if M > 8:
        kill_an_eighth(rng, X, lb)
    if variant == "dead_row":
        lb[R // 2] = -np.inf
    if variant == "uniform":
        la, lb = None, None
        X = np.where(np.isnan(X), np.float32(0.5), X)  # (every particle carries weight: no NaN among them)
    elif variant == "only_a":
        la, lb = lb, None
    elif variant == "only_b":
        la = None
    live = np.ones((R, M), bool) if lb is None and la is None else np.isfinite((lb if lb is not None else la))
    return X, la, lb, live


def log_weight32(case):
    """``t = (log_a + log_b) - max`` with the kernel's fp32 operations: ``(R, M)`` float32; a row without a live particle is NaN."""
    R, M, _ = case["states"].shape
    zero = np.zeros((R, M), np.float32)
    la = zero if case["log_a"] is None else case["log_a"]
    lb = zero if case["log_b"] is None else case["log_b"]
    with np.errstate(invalid="ignore"):
        a = (la + lb).astype(np.float32)
        top = np.fmax.reduce(a, axis=1, initial=-np.inf).astype(np.float32)  # (fmax skips NaN)
        return (a - top[:, None]).astype(np.float32)


def fixed_point_weights(case_or_side):
    """K1's fixed-point weights ``q = floor(exp(t) 2^24)`` where ``t <= 0``, else 0 (a NaN ``t``: 0), formed with the kernels'
    own fp32 operations (numpy's fp32 ``exp`` for ``expf``): ``(R, M)`` int64."""
    t = log_weight32(case_or_side)
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(t).astype(np.float32)
        return np.where(t <= 0, np.floor(e * np.float32(16777216.0)), 0.0).astype(np.int64)


def weights64(case):
    """The live-weight rule in fp64: ``exp(t)`` where ``t <= 0``, else 0."""
    t = log_weight32(case)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, np.exp(t.astype(np.float64)), 0.0)  # (NaN: no weight)

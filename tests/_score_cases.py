"""Inputs and fp64 reference of the particle-score kernel (``include/mmf.h``: ``MmfPfScoresArgs`` / ``mmf_pf_scores``), in
numpy / torch on the CPU; shared by ``test_score_cases_cpu.py`` and ``test_gpu_scores.py``.

The reference is the header's definition in fp64: ``a = log_a + log_b`` and ``t = a - max a`` with the kernel's own two fp32
operations (``_summary_cases.log_weight32``), then ``w = exp(float64(t))``, ``W = w / sum w`` and

    crps[k]   = sum_m W_m |x_mk - y_k| - 1/2 spread[k]          spread[k] = sum_m sum_l W_m W_l |x_mk - x_lk|
    energy    = sum_m W_m |(x_m - y) / s| - 1/2 spread[d]       spread[d] = sum_m sum_l W_m W_l |(x_m - x_l) / s|

over the particles with ``w > 0`` only (a dead particle's NaN row is selected away), the pairs in chunks of ``CHUNK`` rows so
that no ``(M, M, d)`` array is formed.  It differs from the kernel by the ulps of ``expf`` and of the fp32 pair terms, so the
kernel is held to ``_tol.REL_TOL`` under ``rel_err_elementwise(floor=1e-3)``; ``CAP`` is the condition on the INPUTS that
makes that bar fair: the same formulation in fp32 torch ops must stay within ``REL_TOL / 3`` of the reference."""
import functools
import math

import numpy as np

import _summary_cases as sm
from _summary_cases import CHUNK, GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as sk.* by the tests)

# the kernel's own sizes (csrc/pf_scores.hip): a row is one workgroup with one i-particle per thread up to I_BLOCK particles and
# ceil(M / I_BLOCK) workgroups with two beyond; j-tiles of J_TILE particles; fp32 runs of RUN pairs
I_BLOCK, J_TILE, RUN = 512, 1024, 64
MS = (1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096)
EDGE_MS = (I_BLOCK - 1, I_BLOCK, I_BLOCK + 1, J_TILE - 1, J_TILE, J_TILE + 1)  # (2 I_BLOCK = J_TILE: two | three workgroups)
ALL_MS = tuple(sorted(set(MS + EDGE_MS)))
SMALL = 257                      # up to here the whole cross of dimensions, rows and variants; beyond, every variant once
DIMS = (1, 2, 3, 4)
RS = (1, 3)
VARIANTS = ("plain", "uniform", "only_a", "only_b", "dead_row", "nan_truth", "no_truth", "scaled")
SCALE = (0.5, 2.0, 1.0, 4.0)
CAP = 3e-5                       # REL_TOL / 3, the margin CAP_RTS uses


def make_case(M, d, R, variant="plain", seed=0):
    """``dict(states (R, M, d), log_a, log_b (R, M) or None, truth (R, d) or None, scale (d floats) or None)``: the weighted
    set of ``_summary_cases.weighted_set`` with truths that cycle per row through a live particle's own value, the live mean
    + 5 and N(0, 1)."""
    assert variant in VARIANTS
    rng = np.random.default_rng(2000003 * M + 1013 * d + 103 * R + 11 * VARIANTS.index(variant) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, variant)
    truth = np.empty((R, d), np.float32)
    for r in range(R):
        xs = X[r][live[r]] if live[r].any() else np.zeros((1, d), np.float32)
        kind = (r + M + seed) % 3
        truth[r] = (xs[rng.integers(0, len(xs))], xs.mean(0) + 5.0, rng.standard_normal(d))[kind]
    if variant == "nan_truth":
        truth[R // 2, (M + R) % d] = np.nan
    if variant == "no_truth":
        truth = None
    return dict(states=X, log_a=la, log_b=lb, truth=truth, scale=SCALE[:d] if variant == "scaled" else None)


def family():
    """``(M, d, R, variant)``: up to ``SMALL`` particles the whole cross; beyond it every variant once with the dimension
    cycling (three rows for ``plain`` and ``dead_row``, one otherwise) and ``plain`` at every dimension."""
    for M in ALL_MS:
        if M <= SMALL:
            for d in DIMS:
                for R in RS:
                    for variant in VARIANTS:
                        yield M, d, R, variant
            continue
        for i, variant in enumerate(VARIANTS):
            yield M, DIMS[(i + M) % len(DIMS)], 3 if variant in ("plain", "dead_row") else 1, variant
        for d in DIMS:
            yield M, d, 1, "plain"


def _scale64(case):
    d = case["states"].shape[-1]
    return np.ones(d) if case["scale"] is None else np.asarray(case["scale"], np.float64)


def reference_rows(X, W, truth, scale):
    """The definition on ``X (R, M, d)`` under unnormalised fp64 weights ``W (R, M)``: ``crps (R, d)`` and ``energy (R,)``
    (``None`` without a truth), ``spread (R, d + 1)``, all float64."""
    R, M, d = X.shape
    s = np.asarray(scale, np.float64)
    crps = None if truth is None else np.full((R, d), np.nan)
    energy = None if truth is None else np.full((R,), np.nan)
    spread = np.full((R, d + 1), np.nan)
    for r in range(R):
        live = W[r] > 0
        if not live.any():
            continue
        x = X[r][live].astype(np.float64)
        w = W[r][live] / W[r][live].sum()
        acc = np.zeros(d + 1)
        for c in range(0, len(x), CHUNK):
            wc = w[c:c + CHUNK]
            n2 = np.zeros((len(wc), len(x)))
            for k in range(d):
                e = x[c:c + CHUNK, k, None] - x[None, :, k]         # (chunk, n): one dimension at a time
                acc[k] += wc @ np.abs(e) @ w
                e /= s[k]
                e *= e
                n2 += e
            acc[d] += wc @ np.sqrt(n2) @ w
        spread[r] = acc
        if truth is not None:
            with np.errstate(invalid="ignore"):
                e = x - truth[r].astype(np.float64)
                crps[r] = w @ np.abs(e) - 0.5 * acc[:d]
                energy[r] = w @ np.sqrt(((e / s) ** 2).sum(-1)) - 0.5 * acc[d]
    return crps, energy, spread


def reference(case):
    """``(crps, energy, spread)`` of a case by the fp64 definition; NaN where the definition puts it."""
    return reference_rows(case["states"], sm.weights64(case), case["truth"], _scale64(case))


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, variant):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    case = make_case(M, d, R, variant)
    return case, reference(case)


def torch_formulation(case, dtype=None, chunk=CHUNK):
    """The same definition in torch ops on the CPU, fp32 unless told otherwise: weights ``exp(t) / sum``, dead particles
    (weight 0) with their rows zeroed, chunked broadcast differences.  What a caller without the kernel would write."""
    import torch

    dtype = dtype or torch.float32
    X = torch.from_numpy(np.ascontiguousarray(case["states"])).to(dtype)
    R, M, d = X.shape
    with np.errstate(invalid="ignore"):
        t = torch.from_numpy(sm.log_weight32(case)).to(dtype)
    w = torch.where(t <= 0, torch.exp(t), torch.zeros_like(t))
    S = w.sum(-1, keepdim=True)
    W = w / S
    X = torch.where((w > 0)[..., None], X, torch.zeros_like(X))
    s = torch.tensor(_scale64(case), dtype=dtype)
    spread = torch.zeros((R, d + 1), dtype=dtype)
    for c in range(0, M, chunk):
        e = X[:, c:c + chunk, None, :] - X[:, None, :, :]
        ww = W[:, c:c + chunk, None] * W[:, None, :]
        spread[:, :d] += (ww[..., None] * e.abs()).sum((1, 2))
        spread[:, d] += (ww * torch.linalg.vector_norm(e / s, dim=-1)).sum((1, 2))
    dead = ~(S[:, 0] > 0)
    spread[dead] = math.nan
    if case["truth"] is None:
        return None, None, spread
    y = torch.from_numpy(case["truth"]).to(dtype)
    e = X - y[:, None, :]
    crps = (W[..., None] * e.abs()).sum(1) - 0.5 * spread[:, :d]
    energy = (W * torch.linalg.vector_norm(e / s, dim=-1)).sum(1) - 0.5 * spread[:, d]
    return crps, energy, spread


def compare(got, want, what=""):
    """Holds one output to its reference: NaN exactly where the reference has it, and returns
    ``rel_err_elementwise(floor=1e-3)`` over the rest (0.0 when nothing is finite)."""
    from _tol import rel_err_elementwise

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, "NaN placement", got, want)
    if nan.all():
        return 0.0
    return rel_err_elementwise(np.where(nan, 0.0, got), np.where(nan, 0.0, want), floor=1e-3)

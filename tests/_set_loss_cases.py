"""Inputs and fp64 reference of the particle-set log score (``include/mmf.h``: ``MmfPfSetNllArgs`` / ``mmf_pf_set_nll``), in
numpy / torch on the CPU; shared by ``test_set_loss_cases_cpu.py``, ``test_gpu_set_loss.py`` and ``test_gpu_set_loss_training.py``.

The reference is the header's definition in fp64 on the fp32 inputs: per row, over the live particles (``a_m > -inf``),

    z_mj = (y_j - x_mj) / sigma_j              e_m = a_m - 1/2 sum_j z_mj^2
    nll  = logsumexp_m a_m - logsumexp_m e_m + sum_j log sigma_j + (d / 2) log 2 pi
    r = softmax(e)      p = softmax(a)
    g_states = -r_m z_mj / sigma_j      g_logw = p_m - r_m      g_log_scale = 1 - sum_m r_m z_mj^2    (per row)

with zeros at dead particles, and ``nll = NaN`` with zero gradients for a row without a live particle or with a NaN in ``y``.
The kernel is held to ``_tol.REL_TOL``: ``nll`` and ``g_log_scale`` under ``rel_err_elementwise(floor=1e-3)``, ``g_states``
(every particle's vector) and ``g_logw`` (every row's vector) under ``rel_err``; ``CAP`` is the condition on the INPUTS that
makes that bar fair: the same formulation in fp32 torch ops must stay within ``REL_TOL / 3`` of the reference.

What the condition decides about the cases.  The exponent ``e_m`` carries ``q_m = 1/2 |z_m|^2`` in fp32, so ``r`` is known to
``ulp(q)``: with ``q`` in the thousands (``far_truth``) or at ``10^6`` (``collapsed``) a softmax over several near-tied
exponents is not determined to ``REL_TOL`` by ANY fp32 evaluation of this formulation.  Those two variants therefore move one
live particle of every row -- the ``lead`` -- beyond all the others, towards the truth, so that it alone carries the
responsibility (the next exponent lies more than 30 below): what they test is the log-sum-exp about its own maximum, where a
naive ``exp(e)`` is 0 and the result ``inf - inf``.  The soft competition of many particles is what the other variants test,
with truths inside or near the cloud (``q`` of the particles that matter of order 10) and log-weights within a few nats of
each other, as a set that was never resampled has them.
Three outputs are differences of O(1) quantities -- ``nll`` (two log-sum-exps), ``g_logw = p - r`` and ``g_log_scale = 1 - sum
r z^2``, which is 0 exactly where the mixture is calibrated -- and no fp32 evaluation holds a difference to ``REL_TOL`` of
itself once it is a small fraction of its terms.  ``well_conditioned`` states that on the fp64 reference alone: every value
the metric measures against itself (beyond the metric's own floor of 1e-3 of the tensor's largest) is at least ``MIN_SHARE`` of
the sum of the magnitudes of its terms.  ``make_case`` redraws (the next seed) until its case satisfies it."""
import functools
import math

import numpy as np
import torch

import _summary_cases as sm
from _summary_cases import GUARD_ROWS, SENTINEL  # noqa: F401 (read as lc.* by the tests)

WAVE_M = 256                     # csrc/pf_set_loss.hip: a wave owns a row up to WAVE_M particles, a workgroup of 512 threads beyond
ROWS_PER_BLOCK = 4               # rows (waves) of a workgroup of the wave form
MS = (1, 2, 30, 63, 64, 65, WAVE_M - 1, WAVE_M, WAVE_M + 1)
BIG_M = 4096                     # every variant once
SMALL = 257                      # up to here the whole cross
DIMS = (1, 2, 3, 4)
RS = (1, 3)
BIG_R = (1031, 30, 3)            # (R, M, d): more rows than a grid of 256 workgroups of ROWS_PER_BLOCK rows holds at once
SCALES = (0.3, 1.0)              # of the component scales sigma = scale * AXES[:d]
AXES = (1.0, 0.5, 2.0, 1.5)
VARIANTS = ("plain", "uniform", "dead_particles", "dead_row", "nan_truth", "far_truth", "collapsed")
OUTPUTS = ("nll", "g_states", "g_logw", "g_log_scale")
NORMWISE = ("g_states", "g_logw")  # held under rel_err (vectors of the last axis); the others under rel_err_elementwise(floor=1e-3)
CAP = 1e-4 / 3                   # REL_TOL / 3
FAR = 50.0                       # sigmas between the truth and the nearest particle in "far_truth", in every dimension
MIN_SHARE = 0.05                 # well_conditioned: a measured difference is at least this share of its terms' magnitudes
COLLAPSED = 1e-3                 # every component scale of "collapsed"; its truth lies 1.0 from the nearest particle


def sigma_of(d, scale):
    return (np.float32(scale) * np.asarray(AXES[:d], np.float32)).astype(np.float32)


def make_case(M, d, R, variant="plain", scale=0.3, seed=0):
    """``draw_case`` at the first of the seeds ``seed, seed + 1, ..`` whose case is ``well_conditioned``."""
    for attempt in range(200):
        case = draw_case(M, d, R, variant, scale, seed + attempt)
        if well_conditioned(case, reference(case)):
            return case
    raise AssertionError(("no well-conditioned draw", M, d, R, variant, scale))


def draw_case(M, d, R, variant="plain", scale=0.3, seed=0):
    """``dict(states (R, M, d), logw (R, M), truth (R, d), scale (d))``, float32: the weighted set of
    ``_summary_cases.weighted_set`` with ``logw = log_a - 3 + (log_b + 40) / 6`` (not normalised, a spread of about one nat;
    ``uniform``: all 0) and truths that cycle per
    row through a draw from the mixture itself, the live mean + 1.7 and N(0, 1).  ``dead_particles``: every third particle from
    particle 1 is dead too, with a NaN row, at every ``M > 1``.  ``dead_row``: row ``R // 2`` has no live particle.
    ``nan_truth``: one coordinate of the truth of row ``R // 2`` is NaN.  ``far_truth``: the row's lead particle lies 4.0 beyond
    every other in every dimension and the truth ``FAR`` sigma beyond the lead.  ``collapsed``: every sigma is ``COLLAPSED``
    (``scale`` is not read), the lead lies 1.0 beyond every other particle and the truth 1.0 (Euclidean) beyond the lead."""
    assert variant in VARIANTS and scale in SCALES
    rng = np.random.default_rng(5000011 * M + 1009 * d + 101 * R + 13 * VARIANTS.index(variant) + 7 * SCALES.index(scale) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, "uniform" if variant == "uniform" else "dead_row" if variant == "dead_row" else "plain")
    logw = np.zeros((R, M), np.float32) if la is None else (la - np.float32(3.0) + (lb + np.float32(40.0)) / np.float32(6.0)).astype(np.float32)
    if variant == "dead_particles" and M > 1:
        dead = np.arange(1, M, 3)
        logw[:, dead] = -np.inf
        X[:, dead] = np.nan
        live[:, dead] = False
    sigma = np.full(d, COLLAPSED, np.float32) if variant == "collapsed" else sigma_of(d, scale)
    truth = np.empty((R, d), np.float32)
    for r in range(R):
        ids = np.flatnonzero(live[r])
        xs = X[r][ids] if len(ids) else np.zeros((1, d), np.float32)
        kind = (r + M + seed) % 3
        drawn = xs[rng.integers(0, len(xs))] + sigma * rng.standard_normal(d)
        truth[r] = (drawn, xs.mean(0) + 1.7, rng.standard_normal(d))[kind]
        if variant in ("far_truth", "collapsed") and len(ids):
            lead, gap = ids[0], (4.0 if variant == "far_truth" else 1.0)
            others = np.delete(xs, 0, axis=0)
            X[r, lead] = (others.max(0) if len(others) else xs[0]) + np.float32(gap)
            truth[r] = X[r, lead] + (FAR * sigma if variant == "far_truth" else np.float32(1.0 / math.sqrt(d)))
    if variant == "nan_truth":
        truth[R // 2, (M + R) % d] = np.nan
    return dict(states=X, logw=logw, truth=truth, scale=sigma)


def family():
    """``(M, d, R, variant, scale)``: up to ``SMALL`` particles the whole cross of dimensions, rows, variants and scales
    (``collapsed`` reads no scale: once); ``BIG_M`` particles with every variant once, the dimension and the scale cycling;
    and ``BIG_R`` rows once."""
    for M in MS:
        for d in DIMS:
            for R in RS:
                for variant in VARIANTS:
                    for scale in (SCALES[:1] if variant == "collapsed" else SCALES):
                        yield M, d, R, variant, scale
    for i, variant in enumerate(VARIANTS):
        yield BIG_M, DIMS[(i + 2) % len(DIMS)], 3 if variant in ("plain", "dead_row", "nan_truth") else 1, variant, SCALES[i % len(SCALES)]
    yield BIG_R[1], BIG_R[2], BIG_R[0], "plain", SCALES[0]


def _lse(v):
    return v.max() + math.log(np.exp(v - v.max()).sum())


def well_conditioned(case, ref):
    """Is every difference that ``compare`` measures against itself at least ``MIN_SHARE`` of its terms?  Per live row, on the
    fp64 reference: ``nll`` against ``|lse a| + |lse e| + |sum log sigma| + d/2 log 2 pi``, ``g_log_scale[j]`` against ``1 + sum
    r z_j^2``, the row vector ``g_logw`` against ``|p| + |r|`` (an exact 0 -- one live particle -- is no difference); a value
    below the metric's floor, 1e-3 of the output's largest, is measured against that floor and counts with it."""
    X, A, Y = (case[k].astype(np.float64) for k in ("states", "logw", "truth"))
    s = case["scale"].astype(np.float64)
    d = X.shape[-1]
    rows = np.flatnonzero(~np.isnan(ref["nll"]))
    if not len(rows):
        return True
    floor = {k: 1e-3 * float(np.abs(ref[k][rows]).max()) for k in ("nll", "g_log_scale")}
    floor["g_logw"] = 1e-3 * float(np.linalg.norm(ref["g_logw"][rows], axis=1).max())
    for r in rows:
        live = A[r] > -np.inf
        x, a = X[r][live], A[r][live]
        z = (Y[r] - x) / s
        e = a - 0.5 * (z * z).sum(1)
        p, q = np.exp(a - _lse(a)), np.exp(e - _lse(e))
        terms = abs(_lse(a)) + abs(_lse(e)) + abs(np.log(s).sum()) + 0.5 * d * math.log(2.0 * math.pi)
        if max(abs(ref["nll"][r]), floor["nll"]) < MIN_SHARE * terms:
            return False
        moments = 1.0 + (q[:, None] * z * z).sum(0)
        if (np.maximum(np.abs(ref["g_log_scale"][r]), floor["g_log_scale"]) < MIN_SHARE * moments).any():
            return False
        norm = float(np.linalg.norm(p - q))
        if live.sum() > 1 and max(norm, floor["g_logw"]) < MIN_SHARE * (np.linalg.norm(p) + np.linalg.norm(q)):
            return False
    return True


ALL_MS = MS + (BIG_M,)
assert max(MS) <= SMALL


def reference(case):
    """The four outputs of a case by the fp64 definition (``g_nll`` = 1); NaN / zeros where the definition puts them."""
    X, A, Y = (case[k].astype(np.float64) for k in ("states", "logw", "truth"))
    s = case["scale"].astype(np.float64)
    R, M, d = X.shape
    out = dict(nll=np.full((R,), np.nan), g_states=np.zeros((R, M, d)), g_logw=np.zeros((R, M)), g_log_scale=np.zeros((R, d)))
    for r in range(R):
        live = A[r] > -np.inf
        if not live.any() or np.isnan(Y[r]).any():
            continue
        x, a = X[r][live], A[r][live]
        z = (Y[r] - x) / s
        e = a - 0.5 * (z * z).sum(1)
        lse = _lse
        out["nll"][r] = lse(a) - lse(e) + np.log(s).sum() + 0.5 * d * math.log(2.0 * math.pi)
        p, q = np.exp(a - lse(a)), np.exp(e - lse(e))
        out["g_states"][r][live] = -q[:, None] * z / s
        out["g_logw"][r][live] = p - q
        out["g_log_scale"][r] = 1.0 - (q[:, None] * z * z).sum(0)
    return out


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, variant, scale):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    case = make_case(M, d, R, variant, scale)
    return case, reference(case)


def autograd64(case):
    """The definition by plain fp64 torch autograd, NOTHING masked: a dead particle enters as ``-inf`` with its NaN row, so the
    gradients are NaN wherever autograd makes them so (a row with a dead particle).  ``(nll, g_states, g_logw, g_log_scale)``
    with ``g_log_scale`` per row."""
    X, A, Y = (torch.from_numpy(case[k]).double() for k in ("states", "logw", "truth"))
    R, M, d = X.shape
    X.requires_grad_(True)
    A.requires_grad_(True)
    theta = torch.from_numpy(case["scale"]).double().log()[None].repeat(R, 1).requires_grad_(True)
    z = (Y[:, None, :] - X) / theta.exp()[:, None, :]
    nll = torch.logsumexp(A, 1) - torch.logsumexp(A - 0.5 * (z * z).sum(-1), 1) + theta.sum(1) + 0.5 * d * math.log(2.0 * math.pi)
    grads = torch.autograd.grad(nll.sum(), (X, A, theta))
    return tuple(t.detach().numpy() for t in (nll,) + grads)


def torch_formulation(case, dtype=torch.float32):
    """The library's own torch formulation (``engine.particle_set_nll_torch``) on CPU tensors, fp32 unless told otherwise, its
    gradients by autograd with one scale row per set row, so that ``g_log_scale`` comes per row."""
    from multimodalfilter_amd import engine

    X, A, Y = (torch.from_numpy(case[k]).to(dtype) for k in ("states", "logw", "truth"))
    R = X.shape[0]
    X.requires_grad_(True)
    A.requires_grad_(True)
    theta = torch.from_numpy(case["scale"]).to(dtype).log()[None].repeat(R, 1).requires_grad_(True)
    nll = engine.particle_set_nll_torch(X, A, Y, theta.exp())
    fin = torch.where(torch.isnan(nll), torch.zeros_like(nll), nll)
    grads = torch.autograd.grad(fin.sum(), (X, A, theta))
    return dict(zip(OUTPUTS, (t.detach().numpy() for t in (nll,) + grads)))


def compare(got, want, name, what=""):
    """Holds one output to its reference: NaN exactly where the reference has it, and returns the error over the rest (0.0
    when nothing is finite): ``rel_err`` over the vectors of the last axis for ``g_states`` and ``g_logw``,
    ``rel_err_elementwise(floor=1e-3)`` otherwise."""
    from _tol import rel_err, rel_err_elementwise

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, name, "NaN placement", got, want)
    if nan.all():
        return 0.0
    got, want = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    if name in NORMWISE:
        return rel_err(torch.from_numpy(got), torch.from_numpy(want), dims=1)
    return rel_err_elementwise(got, want, floor=1e-3)

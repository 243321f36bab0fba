"""Inputs and fp64 reference of the gradients of CRPS and the energy score of a weighted particle set (``include/mmf.h``:
``MmfPfScoresBackwardArgs`` / ``mmf_pf_scores_backward``), in numpy / torch on the CPU; shared by
``test_set_score_cases_cpu.py``, ``test_gpu_set_scores.py`` and ``test_gpu_set_score_training.py``.

The reference is the header's closed form in fp64 on the fp32 inputs, with the weights as the kernels form them
(``_summary_cases.weights64``: ``t = a - max a`` in fp32, then fp64): per row, over the live particles, ``W = w / sum w``,

    t_mk = |x_mk - y_k|          s_mk = sum_l W_l |x_mk - x_lk|
    t_mE = |(x_m - y)/s|_2       s_mE = sum_l W_l |(x_m - x_l)/s|_2
    c_m  = sum_k g_k (t_mk - s_mk) + g_E (t_mE - s_mE)
    g_logw[m]      = W_m (c_m - sum_l W_l c_l)
    g_states[m, k] = W_m [g_k (sgn(x_mk - y_k) - sum_l W_l sgn(x_mk - x_lk)) + g_E (u_k(x_m - y) - sum_l W_l u_k(x_m - x_l))]

with zeros at dead particles and on rows without a live particle, and a term whose forward value is NaN (``crps[k]`` where
``y_k`` is NaN, ``energy`` where any is) taken out.  The kernel is held to ``_tol.REL_TOL``: ``g_states`` under ``rel_err`` over
every particle's vector, ``g_logw`` under ``rel_err`` over every row's vector.  ``CAP`` is the condition on the INPUTS that makes
that bar fair: the same closed form in fp32 torch ops, the weights unnormalised and divided by their sum last
(``closed_form(case, torch.float32)``), must stay within ``REL_TOL / 3`` of the reference.  (With normalised weights, or
through autograd of the forward -- two separately rounded quotients per gradient --, uniform weights at ``M >= 255`` reach
2e-4 on ``g_states`` through the fp32 rounding of ``1 / sum w`` alone: the bracket of a particle at the edge of the cloud in
``d = 1`` is ``1 / M`` of its two terms.)

What the condition decides about the cases.  ``g_logw[m] = W_m (c_m - sum W c)`` is a difference, and ``c_m`` itself a sum of
differences ``t - s``; no fp32 evaluation holds a difference to ``REL_TOL`` of itself once it is a small fraction of its terms.
Three kinds of input make it one: weights peaked on one particle (``_score_cases``' ``log_b = -40 + 6 N``: the dominant
particle's ``c_m`` IS the row's mean), which the log-weights here, within about a nat as in a set that was never resampled,
avoid; ``M = 2`` with one particle a copy of the other, where ``g_logw`` is 0 in exact arithmetic and rounding noise
otherwise; and a row whose every term is taken out.  ``well_conditioned`` states the condition on the fp64 reference alone: a
row's ``g_logw`` vector (or, below it, the metric's floor of 1e-3 of the case's largest row) is at least ``MIN_SHARE`` of the
vector of the magnitudes of its terms, ``W_m (|c|_m + sum W |c|)`` with ``|c|_m = sum_k |g_k| (t_mk + s_mk) + |g_E| (t_mE +
s_mE)``; a row whose ``g_logw`` is exactly 0 (one live particle, no term left) is no difference.  ``make_case`` redraws (the
next seed) until its case satisfies it.  ``g_states`` needs no condition of its own: the bracket of a particle at the edge of
the cloud is small, but then so is its vector against the largest of the case, and the metric measures it against the floor."""
import functools

import numpy as np
import torch

import _summary_cases as sm
from _summary_cases import GUARD_ROWS, SENTINEL  # noqa: F401 (read as sc.* by the tests)

I_BLOCK = 512                    # csrc/pf_summary.h: a row is one workgroup up to I_BLOCK particles, ceil(M / I_BLOCK) beyond
J_TILE = 1024                    # particles of an LDS tile
RUN = 64                         # pairs of an fp32 sum
SMALL_MS = (1, 2, 30, 63, 64, 65)                      # the whole cross of dimensions, rows and variants
LARGE_MS = (511, 512, 513, 1023, 1024, 1025)           # one -> two -> three workgroups, the j-tile: every variant and dimension
MS = SMALL_MS + LARGE_MS
BIG_M = 4096                     # every variant once
ALL_MS = MS + (BIG_M,)
DIMS = (1, 2, 3, 4)
RS = (1, 3)
BIG_R = (1031, 30, 3)            # (R, M, d)
AXES = (1.0, 0.5, 2.0, 1.5)      # the scale of "scaled" is 0.75 * AXES[:d]: exact in fp32, as the argument struct holds it
VARIANTS = ("plain", "uniform", "dead_particles", "dead_row", "nan_truth", "scaled", "crps_only", "energy_only")
OUTPUTS = ("g_states", "g_logw")
CAP = 1e-4 / 3                   # REL_TOL / 3
MIN_SHARE = 0.01                 # well_conditioned: a row's g_logw is at least this share of its terms' magnitudes: an fp32 evaluation
                                 # holds every term to a few ulps, say 4 x 2^-24 = 2.4e-7 of it, which is CAP of a difference of 0.7 %
CHUNK = 256                      # i-particles of a chunk of the fp64 pair sums


def make_case_and_reference(M, d, R, variant="plain", seed=0):
    """``draw_case`` at the first of the seeds ``seed, seed + 1, ..`` whose case is ``well_conditioned``, with its reference."""
    for attempt in range(200):
        case = draw_case(M, d, R, variant, seed + attempt)
        ref = reference(case)
        if well_conditioned(case, ref):
            return case, ref
    raise AssertionError(("no well-conditioned draw", M, d, R, variant))


def make_case(M, d, R, variant="plain", seed=0):
    return make_case_and_reference(M, d, R, variant, seed)[0]


def draw_case(M, d, R, variant="plain", seed=0):
    """``dict(states (R, M, d), logw (R, M) or None, truth (R, d), scale (d floats or None), g_crps (R, d) or None, g_energy (R)
    or None)``, float32: the weighted set of ``_summary_cases.weighted_set`` with ``logw = log_a - 3 + (log_b + 40) / 6`` (not
    normalised, a spread of about one nat; ``uniform``: no log-weights) and truths that cycle per row through a draw near a
    live particle, the live mean + 1.7 and N(0, 1); upstream gradients uniform in ``[0.5, 1.5]``.  ``dead_particles``: every
    third particle from particle 1 is dead too, with a NaN row, at every ``M > 1``.  ``dead_row``: row ``R // 2`` has no live
    particle.  ``nan_truth``: one coordinate of the truth of row ``R // 2`` is NaN.  ``scaled``: ``scale = 0.75 AXES[:d]``.
    ``crps_only`` / ``energy_only``: the other upstream gradient is ``None``."""
    assert variant in VARIANTS
    rng = np.random.default_rng(7000003 * M + 1013 * d + 103 * R + 17 * VARIANTS.index(variant) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, "uniform" if variant == "uniform" else "dead_row" if variant == "dead_row" else "plain")
    logw = None if la is None else (la - np.float32(3.0) + (lb + np.float32(40.0)) / np.float32(6.0)).astype(np.float32)
    if variant == "dead_particles" and M > 1:
        dead = np.arange(1, M, 3)
        logw[:, dead] = -np.inf
        X[:, dead] = np.nan
        live[:, dead] = False
    truth = np.empty((R, d), np.float32)
    for r in range(R):
        ids = np.flatnonzero(live[r])
        xs = X[r][ids] if len(ids) else np.zeros((1, d), np.float32)
        kind = (r + M + seed) % 3
        near = xs[rng.integers(0, len(xs))] + 0.3 * rng.standard_normal(d)
        truth[r] = (near, xs.mean(0) + 1.7, rng.standard_normal(d))[kind]
    if variant == "nan_truth":
        truth[R // 2, (M + R) % d] = np.nan
    g_crps = rng.uniform(0.5, 1.5, (R, d)).astype(np.float32)
    g_energy = rng.uniform(0.5, 1.5, (R,)).astype(np.float32)
    return dict(states=X, logw=logw, truth=truth, scale=tuple(0.75 * a for a in AXES[:d]) if variant == "scaled" else None,
                g_crps=None if variant == "energy_only" else g_crps, g_energy=None if variant == "crps_only" else g_energy)


def family():
    """``(M, d, R, variant)``: at ``SMALL_MS`` the whole cross of dimensions, rows and variants; at ``LARGE_MS`` every variant
    in every dimension, the rows alternating; ``BIG_M`` particles with every variant once, the dimension cycling; and ``BIG_R``
    rows once."""
    for M in SMALL_MS:
        for d in DIMS:
            for R in RS:
                for variant in VARIANTS:
                    yield M, d, R, variant
    for M in LARGE_MS:
        for i, variant in enumerate(VARIANTS):
            for d in DIMS:
                yield M, d, RS[(i + d) % 2] if variant not in ("dead_row", "nan_truth") else 3, variant
    for i, variant in enumerate(VARIANTS):
        yield BIG_M, DIMS[(i + 2) % len(DIMS)], 2 if variant in ("dead_row", "nan_truth") else 1, variant
    yield BIG_R[1], BIG_R[2], BIG_R[0], "plain"


def _weights(case):
    R, M, _ = case["states"].shape
    return sm.weights64(dict(states=case["states"], log_a=case["logw"], log_b=None))


def _scale64(case):
    d = case["states"].shape[-1]
    return torch.ones(d, dtype=torch.float64) if case["scale"] is None else torch.tensor([np.float32(s) for s in case["scale"]], dtype=torch.float64)


def closed_form(case, dtype=torch.float64):
    """The header's closed form in torch ops of ``dtype`` on the CPU, the weights unnormalised in every sum and the division by
    ``S = sum w`` taken last -- ``S sgn(x_mk - y_k) - sum_l w_l sgn(x_mk - x_lk)`` is then the difference of the sums themselves,
    not of two rounded quotients: ``g_states (R, M, d)``, ``g_logw (R, M)`` (zeros where the definition puts them), the
    forward's ``crps (R, d)`` and ``energy (R)`` (NaN where it puts it) and ``terms_logw (R, M)``, the magnitudes of
    ``g_logw``'s terms that ``well_conditioned`` reads.  fp64: the reference (``weights64``); fp32: the yardstick of ``CAP``
    (``exp`` in fp32 too)."""
    X = torch.from_numpy(case["states"]).to(dtype)
    R, M, d = X.shape
    if dtype == torch.float64:
        w = torch.from_numpy(_weights(case))
    else:
        t = torch.from_numpy(sm.log_weight32(dict(states=case["states"], log_a=case["logw"], log_b=None)))
        w = torch.where(t <= 0, torch.exp(t), torch.zeros_like(t)).to(dtype)
    Y = torch.from_numpy(case["truth"]).to(dtype)
    s = _scale64(case).to(dtype)
    zeros = lambda *shape: torch.zeros(shape, dtype=dtype)
    out = dict(g_states=zeros(R, M, d), g_logw=zeros(R, M), crps=torch.full((R, d), np.nan, dtype=dtype),
               energy=torch.full((R,), np.nan, dtype=dtype), terms_logw=zeros(R, M))
    tiny = torch.finfo(dtype).tiny
    for r in range(R):
        live = w[r] > 0
        if not bool(live.any()):
            continue
        x, wl = X[r][live], w[r][live]
        S = wl.sum()
        m = x.shape[0]
        y_ok = ~torch.isnan(Y[r])
        y = torch.where(y_ok, Y[r], torch.zeros_like(Y[r]))
        gk = zeros(d) if case["g_crps"] is None else torch.from_numpy(case["g_crps"][r]).to(dtype)
        gk = torch.where(y_ok, gk, torch.zeros_like(gk))
        gE = float(case["g_energy"][r]) if case["g_energy"] is not None and bool(y_ok.all()) else 0.0
        e = x - y
        t_abs, t_sgn, z = e.abs(), torch.sign(e), e / s
        t_n = z.pow(2).sum(-1).sqrt()
        t_u = torch.where(t_n[:, None] > 0, z / s / t_n.clamp_min(tiny)[:, None], torch.zeros_like(z))
        s_abs, s_sgn, s_u, s_n = zeros(m, d), zeros(m, d), zeros(m, d), zeros(m)   # sums over l with w_l, not W_l
        for i0 in range(0, m, CHUNK):
            E = x[i0:i0 + CHUNK, None, :] - x[None, :, :]
            s_abs[i0:i0 + CHUNK] = (wl[None, :, None] * E.abs()).sum(1)
            s_sgn[i0:i0 + CHUNK] = (wl[None, :, None] * torch.sign(E)).sum(1)
            Z = E / s
            n = Z.pow(2).sum(-1).sqrt()
            s_n[i0:i0 + CHUNK] = (wl[None, :] * n).sum(1)
            U = torch.where(n[..., None] > 0, Z / s / n.clamp_min(tiny)[..., None], torch.zeros_like(Z))
            s_u[i0:i0 + CHUNK] = (wl[None, :, None] * U).sum(1)
        c = (((S * t_abs - s_abs) * gk).sum(1) + gE * (S * t_n - s_n)) / S
        mag = (((S * t_abs + s_abs) * gk.abs()).sum(1) + abs(gE) * (S * t_n + s_n)) / S
        out["g_logw"][r][live] = wl * (S * c - (wl * c).sum()) / (S * S)
        out["terms_logw"][r][live] = wl * (S * mag + (wl * mag).sum()) / (S * S)
        out["g_states"][r][live] = wl[:, None] * (gk * (S * t_sgn - s_sgn) + gE * (S * t_u - s_u)) / (S * S)
        crps = ((wl[:, None] * t_abs).sum(0) - 0.5 * (wl[:, None] * s_abs).sum(0) / S) / S
        out["crps"][r] = torch.where(y_ok, crps, torch.full_like(crps, np.nan))
        if bool(y_ok.all()):
            out["energy"][r] = ((wl * t_n).sum() - 0.5 * (wl * s_n).sum() / S) / S
    return {k: v.numpy() for k, v in out.items()}


def reference(case):
    """``closed_form`` in fp64."""
    return closed_form(case, torch.float64)


def well_conditioned(case, ref):
    """Is every row's ``g_logw`` -- or, below it, the metric's floor, 1e-3 of the largest row of the case -- at least
    ``MIN_SHARE`` of its terms' magnitudes?  On the fp64 reference alone; a row that is exactly 0 is no difference."""
    norm = np.linalg.norm(ref["g_logw"], axis=1)
    terms = np.linalg.norm(ref["terms_logw"], axis=1)
    floor = 1e-3 * float(norm.max()) if len(norm) else 0.0
    for r in range(len(norm)):
        if norm[r] == 0.0 and (terms[r] == 0.0 or (_weights(case)[r] > 0).sum() <= 1):
            continue
        if max(norm[r], floor) < MIN_SHARE * terms[r]:
            return False
    return True


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, variant):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    return make_case_and_reference(M, d, R, variant)


def _loss(crps, energy, case, dtype):
    total = 0.0
    if case["g_crps"] is not None:
        total = total + (torch.where(torch.isnan(crps), torch.zeros_like(crps), crps) * torch.from_numpy(case["g_crps"]).to(dtype)).sum()
    if case["g_energy"] is not None:
        total = total + (torch.where(torch.isnan(energy), torch.zeros_like(energy), energy) * torch.from_numpy(case["g_energy"]).to(dtype)).sum()
    return total


def autograd64(case):
    """The forward definition (``E|X - y| - 1/2 E|X - X'|`` with ``W = softmax`` of the live log-weights) by plain fp64 torch
    autograd on the LIVE particles of every row -- nothing is dead in what autograd sees, and a row without a live particle or
    with a NaN in its truth is left out (zeros) -> ``(g_states, g_logw)`` scattered back, zeros elsewhere."""
    R, M, d = case["states"].shape
    w = _weights(case)
    s = _scale64(case)
    gx, ga = np.zeros((R, M, d)), np.zeros((R, M))
    for r in range(R):
        live = w[r] > 0
        if not live.any() or np.isnan(case["truth"][r]).any():
            continue
        x = torch.from_numpy(case["states"][r][live]).double().requires_grad_(True)
        a = torch.from_numpy(np.log(w[r][live])).requires_grad_(True)   # (the kernels' a - max a, rounded to fp32 as they round it)
        y = torch.from_numpy(case["truth"][r]).double()
        W = torch.softmax(a, 0)
        E = x[:, None, :] - x[None, :, :]
        WW = W[:, None] * W[None, :]
        crps = (W[:, None] * (x - y).abs()).sum(0) - 0.5 * (WW[..., None] * E.abs()).sum((0, 1))
        energy = (W * torch.linalg.vector_norm((x - y) / s, dim=-1)).sum() - 0.5 * (WW * torch.linalg.vector_norm(E / s, dim=-1)).sum()
        loss = 0.0
        if case["g_crps"] is not None:
            loss = loss + (crps * torch.from_numpy(case["g_crps"][r]).double()).sum()
        if case["g_energy"] is not None:
            loss = loss + energy * float(case["g_energy"][r])
        g = torch.autograd.grad(loss, (x, a))
        gx[r][live], ga[r][live] = g[0].numpy(), g[1].numpy()
    return gx, ga


def torch_formulation(case):
    """The yardstick of ``CAP``: the same closed form in fp32 torch ops, weights unnormalised (``closed_form``)."""
    return closed_form(case, torch.float32)


def library_autograd(case, dtype=torch.float64):
    """The library's own torch formulation (``engine.particle_set_scores_torch``) on CPU tensors with its gradients by autograd
    -> ``dict`` of ``crps``, ``energy``, ``g_states``, ``g_logw`` (uniform weights enter as zeros)."""
    from multimodalfilter_amd import engine

    X = torch.from_numpy(case["states"]).to(dtype).requires_grad_(True)
    A = (torch.zeros(case["states"].shape[:2]) if case["logw"] is None else torch.from_numpy(case["logw"])).to(dtype).requires_grad_(True)
    Y = torch.from_numpy(case["truth"]).to(dtype)
    crps, energy = engine.particle_set_scores_torch(X, A, Y, case["scale"])
    gx, ga = torch.autograd.grad(_loss(crps, energy, case, dtype), (X, A))
    return dict(crps=crps.detach().numpy(), energy=energy.detach().numpy(), g_states=gx.numpy(), g_logw=ga.numpy())


def compare(got, want, name, what=""):
    """Holds one gradient to its reference: no NaN, and the ``rel_err`` over the vectors of the last axis -- every particle's
    for ``g_states``, every row's for ``g_logw``."""
    from _tol import rel_err

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, name, got.shape, want.shape)
    assert not np.isnan(got).any(), (what, name, "NaN")
    return rel_err(torch.from_numpy(got), torch.from_numpy(want), dims=1)

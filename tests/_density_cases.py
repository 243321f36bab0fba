"""Inputs and fp64 reference of the particle-density kernel (``include/mmf.h``: ``MmfPfDensityArgs`` / ``mmf_pf_density``), in
numpy / torch on the CPU; shared by ``test_density_cases_cpu.py`` and ``test_gpu_density.py``.

The cases are those of ``_score_cases.make_case`` (its ``family()`` without ``"scaled"``, which means nothing here), a variant
``"moderate"`` whose log-weights ``log_b = 0.5 N(0, 1)`` give ``n_eff ~ M`` -- the family's ``-40 + 6 N(0, 1)`` gives 1 to 3,
so the bandwidth rules would otherwise only be exercised there -- and three bandwidth variants: Silverman, Scott and the
fixed bandwidths ``FIXED[:d]``.

The reference is the header's definition in fp64, weights as in ``_score_cases`` (``_summary_cases.weights64``: the kernel's
own two fp32 operations on the log-weights, then fp64), the ``M + 1`` log-sum-exps in chunks of ``CHUNK`` queries so that no
``(M, M, d)`` array is formed.

The bar of every log-valued output is ``log_err(got, want) = max |got - want| / max(1, |want|) <= REL_TOL``: an absolute
error in a log is a relative error in the density, and the relative branch is what fp32 can hold of a log score of -1e4.
``-inf``, NaN and ``-1`` sit exactly where the definition puts them.  ``CAP`` is the condition on the INPUTS that makes the bar
fair: the same formulation in fp32 torch ops must stay within ``REL_TOL / 3`` of the reference under the same metric."""
import functools
import math

import numpy as np

import _score_cases as sk
import _summary_cases as sm
from _summary_cases import CHUNK, GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as dc.* by the tests)

RULES = ("silverman", "scott", "fixed")
FIXED = (0.3, 0.5, 1.0, 2.0)
MIN_BANDWIDTH = 1e-6
VARIANTS = tuple(v for v in sk.VARIANTS if v != "scaled") + ("moderate",)
CAP = sk.CAP                      # REL_TOL / 3
FLOAT_OUTPUTS = ("log_density", "log_score", "entropy", "mode", "bandwidth")
OUTPUTS = FLOAT_OUTPUTS + ("mode_index",)


def make_case(M, d, R, variant="plain", rule="silverman", seed=0):
    """A case of ``_score_cases.make_case`` with ``rule``, ``bandwidth`` (``FIXED[:d]`` under ``"fixed"``, else ``None``) and
    ``min_bandwidth`` (``d`` floats).  ``"moderate"``: the plain case with ``log_b = 0.5 N(0, 1)`` on its live particles."""
    assert variant in VARIANTS and rule in RULES
    if variant == "moderate":
        case = dict(sk.make_case(M, d, R, "plain", seed))
        rng = np.random.default_rng(77003 * M + 31 * d + R + seed)
        lb = (0.5 * rng.standard_normal((R, M))).astype(np.float32)
        case["log_b"] = np.where(np.isfinite(case["log_b"]), lb, case["log_b"]).astype(np.float32)
    else:
        case = dict(sk.make_case(M, d, R, variant, seed))
    del case["scale"]
    case.update(rule=rule, bandwidth=FIXED[:d] if rule == "fixed" else None, min_bandwidth=(MIN_BANDWIDTH,) * d)
    return case


def family():
    """``(M, d, R, variant, rule)``: ``_score_cases.family()`` without ``"scaled"`` and with ``"moderate"`` beside every
    ``"plain"`` (beyond ``_score_cases.SMALL`` particles: beside the three-row one); up to ``SMALL`` under every rule, beyond
    it the rule cycling and ``"plain"`` at ``d = 3`` under all three."""
    n = 0
    for M, d, R, variant in sk.family():
        if variant == "scaled":
            continue
        for v in ((variant, "moderate") if variant == "plain" and (M <= sk.SMALL or R == 3) else (variant,)):
            if M <= sk.SMALL:
                for rule in RULES:
                    yield M, d, R, v, rule
            else:
                n += 1
                yield M, d, R, v, RULES[n % 3]
    for M in sk.ALL_MS:
        if M > sk.SMALL:
            for rule in RULES:
                yield M, 3, 1, "plain", rule


def bandwidth_factor(rule, d, n_eff):
    if rule == "silverman":
        return (4.0 / ((d + 2.0) * n_eff)) ** (1.0 / (d + 4.0))
    assert rule == "scott"
    return n_eff ** (-1.0 / (d + 4.0))


def _log_p(q, x, logw, h):
    """``log sum_m exp(logw_m - 1/2 |(q - x_m) / h|^2) - sum log h - d/2 log 2 pi`` for the queries ``q (n, d)``, fp64."""
    d = x.shape[1]
    out = np.empty(len(q))
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(0, len(q), CHUNK):
            z = np.zeros((len(q[c:c + CHUNK]), len(x)))
            for k in range(d):
                e = (q[c:c + CHUNK, k, None] - x[None, :, k]) / h[k]       # (chunk, n): one dimension at a time
                e *= e
                z += e
            e = logw[None, :] - 0.5 * z
            top = np.max(e, axis=1)
            safe = np.where(np.isfinite(top), top, 0.0)
            out[c:c + CHUNK] = safe + np.log(np.exp(e - safe[:, None]).sum(axis=1))
            out[c:c + CHUNK] = np.where(np.isnan(top), np.nan, out[c:c + CHUNK])
    return out - np.log(h).sum() - 0.5 * d * math.log(2.0 * math.pi)


def reference_rows(X, W, truth, rule, bandwidth=None, min_bandwidth=None):
    """The definition on ``X (R, M, d)`` under unnormalised fp64 weights ``W (R, M)`` -> ``dict`` of float64 arrays
    ``log_density (R, M)``, ``log_score (R,)`` (``None`` without a truth), ``entropy (R,)``, ``bandwidth (R, d)``.  No mode:
    particles tie (``check_mode``)."""
    R, M, d = X.shape
    out = dict(log_density=np.full((R, M), np.nan), log_score=None if truth is None else np.full((R,), np.nan),
               entropy=np.full((R,), np.nan), bandwidth=np.full((R, d), np.nan))
    for r in range(R):
        live = W[r] > 0
        if not live.any():
            continue
        x = X[r][live].astype(np.float64)
        w = W[r][live] / W[r][live].sum()
        if rule == "fixed":
            h = np.asarray(bandwidth, np.float32).astype(np.float64)
        else:
            mu = w @ x
            sigma = np.sqrt(w @ (x - mu) ** 2)
            floor = np.asarray(min_bandwidth, np.float32).astype(np.float64)
            h = np.maximum(sigma * bandwidth_factor(rule, d, 1.0 / (w ** 2).sum()), floor)
        logw = np.log(w)
        ld = _log_p(x, x, logw, h)
        out["log_density"][r] = -np.inf
        out["log_density"][r, live] = ld
        out["entropy"][r] = -(w * ld).sum()
        out["bandwidth"][r] = h
        if truth is not None:
            out["log_score"][r] = _log_p(truth[r].astype(np.float64)[None], x, logw, h)[0]
    return out


def reference(case):
    """The outputs of a case by the fp64 definition; NaN and ``-inf`` where the definition puts them."""
    return reference_rows(case["states"], sm.weights64(case), case["truth"], case["rule"], case["bandwidth"], case["min_bandwidth"])


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, variant, rule):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    case = make_case(M, d, R, variant, rule)
    return case, reference(case)


def torch_formulation(case, dtype=None, chunk=CHUNK, device=None):
    """The same definition in torch ops, fp32 on the CPU unless told otherwise: weights ``exp(t) / sum``, dead particles
    (weight 0) with their rows zeroed and ``log W = -inf``, chunked broadcast differences and ``torch.logsumexp``.  What a
    caller without the kernel would write -> ``dict`` of tensors, with ``mode_index`` and ``mode`` by ``argmax``."""
    import torch

    dtype = dtype or torch.float32
    X = torch.from_numpy(np.ascontiguousarray(case["states"])).to(device=device, dtype=dtype)
    with np.errstate(invalid="ignore"):
        t = torch.from_numpy(sm.log_weight32(case)).to(device=device, dtype=dtype)
    y = None if case["truth"] is None else torch.from_numpy(case["truth"]).to(device=device, dtype=dtype)
    return torch_rows(X, t, y, case["rule"], case["bandwidth"], case["min_bandwidth"], chunk)


def torch_rows(X, t, y, rule, bandwidth, min_bandwidth, chunk=CHUNK):
    """``torch_formulation`` on tensors: ``X (R, M, d)``, ``t (R, M)`` the log-weights minus their row maximum, ``y (R, d)``
    or ``None``."""
    import torch

    R, M, d = X.shape
    dtype = X.dtype
    w = torch.where(t <= 0, torch.exp(t), torch.zeros_like(t))
    live = w > 0
    S = w.sum(-1, keepdim=True)
    W = w / S
    X0 = torch.where(live[..., None], X, torch.zeros_like(X))
    if rule == "fixed":
        h = torch.tensor(bandwidth, dtype=dtype, device=X.device).expand(R, d)
    else:
        mu = (W[..., None] * X0).sum(1)
        var = (W[..., None] * (X0 - mu[:, None, :]) ** 2).sum(1)
        n_eff = 1.0 / (W * W).sum(-1)
        c = (4.0 / ((d + 2.0) * n_eff)) ** (1.0 / (d + 4.0)) if rule == "silverman" else n_eff ** (-1.0 / (d + 4.0))
        h = torch.maximum(var.sqrt() * c[:, None], torch.tensor(min_bandwidth, dtype=dtype, device=X.device))
    logw = torch.where(live, torch.log(W), torch.full_like(W, -math.inf))
    const = h.log().sum(-1) + 0.5 * d * math.log(2.0 * math.pi)

    def log_p(Q):  # (R, n, d) -> (R, n)
        out = []
        for c0 in range(0, Q.shape[1], chunk):
            e = (Q[:, c0:c0 + chunk, None, :] - X0[:, None, :, :]) / h[:, None, None, :]
            out.append(torch.logsumexp(logw[:, None, :] - 0.5 * (e * e).sum(-1), dim=-1))
        return torch.cat(out, 1) - const[:, None]

    dead = ~(S[:, 0] > 0)
    nan = torch.full((), math.nan, dtype=dtype, device=X.device)
    ld = log_p(X0)
    entropy = -torch.where(live, W * ld, torch.zeros_like(ld)).sum(-1)
    ld = torch.where(live, ld, torch.full_like(ld, -math.inf))
    index = torch.argmax(ld, dim=-1)
    mode = torch.gather(X, 1, index[:, None, None].expand(R, 1, d))[:, 0]
    out = dict(log_density=torch.where(dead[:, None], nan, ld), entropy=torch.where(dead, nan, entropy),
               bandwidth=torch.where(dead[:, None], nan, h), mode=torch.where(dead[:, None], nan, mode),
               mode_index=torch.where(dead, torch.full_like(index, -1), index), log_score=None)
    if y is not None:
        out["log_score"] = torch.where(dead, nan, log_p(y[:, None, :])[:, 0])
    return out


def log_err(got, want, what=""):
    """Holds a log-valued output to its reference: NaN, ``-inf`` and ``+inf`` exactly where the reference has them, and
    returns ``max |got - want| / max(1, |want|)`` over the rest (0.0 when nothing is finite)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, "NaN placement", got, want)
    inf = np.isinf(want)
    assert bool((got[inf] == want[inf]).all()) and not bool(np.isinf(got[~inf & ~nan]).any()), (what, "inf placement", got, want)
    ok = ~nan & ~inf
    if not ok.any():
        return 0.0
    return float((np.abs(got[ok] - want[ok]) / np.maximum(1.0, np.abs(want[ok]))).max())


def bandwidth_err(got, want, what=""):
    """``rel_err_elementwise`` of the bandwidths, NaN exactly where the reference has it."""
    return sk.compare(got, want, what)


def check_mode(states, weights, log_density, mode_index, mode, ref_log_density, what=""):
    """The mode is not compared by index -- particles tie: ``mode_index`` is the first maximum of the caller's OWN
    ``log_density`` (float32, bit-wise) among the live particles, ``-1`` in a row without one; ``mode`` is the bit copy of
    ``states[mode_index]`` (NaN in such a row).  Returns the worst distance, under the metric of ``log_err``, of the
    reference log density at ``mode_index`` from the reference maximum.  Any of ``mode_index`` / ``mode`` may be ``None``."""
    states = np.ascontiguousarray(states, np.float32)
    ld = np.asarray(log_density, np.float32)
    worst = 0.0
    for r in range(len(states)):
        live = np.asarray(weights[r]) > 0
        if not live.any():
            assert mode_index is None or mode_index[r] == -1, (what, r, mode_index[r])
            assert mode is None or bool(np.isnan(np.asarray(mode[r])).all()), (what, r, mode[r])
            continue
        first = int(np.flatnonzero(live & (ld[r] == ld[r][live].max()))[0])
        if mode_index is not None:
            assert int(mode_index[r]) == first, (what, r, int(mode_index[r]), first)
        if mode is not None:
            got = np.ascontiguousarray(mode[r], np.float32).view(np.uint32)
            assert bool((got == states[r, first].view(np.uint32)).all()), (what, r, mode[r], states[r, first])
        top = float(ref_log_density[r][live].max())
        worst = max(worst, abs(float(ref_log_density[r, first]) - top) / max(1.0, abs(top)))
    return worst

"""Inputs and fp64 reference of the modality-attribution kernel (``include/mmf.h``: ``MmfPfModalitiesArgs`` /
``mmf_pf_modalities``), in numpy / torch on the CPU; shared by ``test_modality_cases_cpu.py``, ``test_gpu_modalities.py`` and
``scripts/bench_modalities.py``.

A case is the plain weighted set of ``_summary_cases.weighted_set`` -- duplicated N(0, 1) states, ``log_w = -log M + 0.3
N(0, 1)``, an eighth of the particles dead (``log_w = -inf`` and a NaN state row) -- with ``K`` log-likelihood columns ``l_k =
-40 + 6 N(0, 1) + 3 k``, a deliberate mismatch of scale between the modalities, and ``beta = log_softmax(N(0, 1))``.

The reference is the header's definition in fp64 from the fp32 inputs, row by row, nothing of it in fp32.  The bars
(``REL_TOL`` of ``_tol.py``): ``log_evidence`` and ``divergence`` under ``log_err`` (an absolute error in a log is a relative
error in what it is the log of); ``responsibility``, ``ess`` and ``overlap`` under ``rel_err_elementwise(floor=1e-3)``;
``mean`` as ``max |got - want|`` over the largest live ``|coordinate|`` of its row -- a mean of N(0, 1) particles cancels, and
the element-wise relative error of a number near 0 measures the cancellation, not the kernel.  ``-inf``, NaN and exact zeros
sit exactly where the definition puts them.  ``CAP = REL_TOL / 3`` is the condition on the INPUTS that makes the bars fair:
the same definition in fp32 torch ops (``torch_formulation``) must stay within it on every family case."""
import functools
import math

import numpy as np

import _summary_cases as sm
from _density_cases import log_err
from _score_cases import compare as rel_compare
from _summary_cases import GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as mc.* by the tests)

# the kernel's own sizes (csrc/pf_modalities.hip): a row is one workgroup with a thread to every RUN_PT particles, rounded up to a
# wave (another wave every 64 RUN_PT = 256 particles), THREADS at most; a thread loads RUN_PT of its particles together and its fp32
# sums take as many, so a second batch begins beyond THREADS * RUN_PT particles and a third beyond twice that
THREADS, RUN_PT, MAX_K = 512, 4, 4
MS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, THREADS * RUN_PT, THREADS * RUN_PT + 1, 4096, 2 * THREADS * RUN_PT + 1)
SMALL = 257                      # up to here the whole cross of modalities, dimensions, rows and variants; beyond, every variant once
KS = (1, 2, 3, 4)
DIMS = (1, 2, 3, 4)
RS = (1, 3)
VARIANTS = ("plain", "moderate", "no_beta", "uniform", "identical", "disjoint", "blackout", "dead_row", "nan_loglik")
CAP = 1e-4 / 3                   # REL_TOL / 3
OUTPUTS = ("log_evidence", "responsibility", "ess", "mean", "divergence", "overlap")


def shapes(R, K, d):
    """The trailing shape of every output."""
    return {"log_evidence": (K + 1,), "responsibility": (K,), "ess": (K + 1,), "mean": (K + 1, d), "divergence": (K,), "overlap": (K, K)}


def make_case(M, d, R, K, variant="plain", seed=0):
    """``dict(states (R, M, d), log_w (R, M) or None, loglik (K, R, M), beta (R, K) or None)``, all float32."""
    assert variant in VARIANTS and 1 <= K <= MAX_K
    rng = np.random.default_rng(3000017 * M + 7919 * d + 389 * R + 53 * K + 11 * VARIANTS.index(variant) + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, "uniform" if variant == "uniform" else "plain")
    log_w = None if la is None else np.where(live, la, -np.inf).astype(np.float32)
    scale, shift = (0.5, 0.0) if variant == "moderate" else (6.0, -40.0)
    l = np.stack([shift + scale * rng.standard_normal((R, M)) + (0.0 if variant == "moderate" else 3.0 * k) for k in range(K)])
    l = l.astype(np.float32)
    beta = rng.standard_normal((R, K))
    beta = (beta - np.log(np.exp(beta).sum(-1, keepdims=True))).astype(np.float32)
    if variant == "no_beta":
        beta = None
    elif variant == "identical":
        l[:] = l[0]
    elif variant == "disjoint":
        l[0][:, 1::2] = -np.inf
        if K > 1:
            l[1][:, 0::2] = -np.inf
    elif variant == "blackout":
        l[K - 1][R // 2] = -np.inf
    elif variant == "dead_row":
        log_w[R // 2] = -np.inf
        X[R // 2] = np.nan
    elif variant == "nan_loglik":
        for k in range(K):
            at = rng.integers(0, M, max(1, M // 16))
            l[k][rng.integers(0, R, len(at)), at] = np.nan
    return dict(states=X, log_w=log_w, loglik=l, beta=beta)


def family():
    """``(M, d, R, K, variant)``: up to ``SMALL`` particles the whole cross; beyond it every variant once with the modalities
    and the dimension cycling (three rows for the variants that single out row ``R // 2``, one otherwise) and ``plain`` at
    the widest shape."""
    n = 0
    for M in MS:
        if M <= SMALL:
            for K in KS:
                for d in DIMS:
                    for R in RS:
                        for variant in VARIANTS:
                            yield M, d, R, K, variant
            continue
        for variant in VARIANTS:
            n += 1
            yield M, DIMS[n % 4], 3 if variant in ("plain", "blackout", "dead_row") else 1, KS[(n // 2 + M) % 4], variant
        yield M, 4, 1, 4, "plain"


def _lse(x, axis):
    """``logsumexp`` in fp64; ``-inf`` where every term is."""
    with np.errstate(invalid="ignore", divide="ignore"):
        top = np.max(x, axis=axis, keepdims=True)
        safe = np.where(np.isfinite(top), top, 0.0)
        return (safe + np.log(np.exp(x - safe).sum(axis=axis, keepdims=True))).squeeze(axis)


def reference_rows(X, log_w, loglik, beta):
    """The definition on ``X (R, M, d)``, ``log_w (R, M)`` or ``None``, ``loglik (K, R, M)``, ``beta (R, K)`` or ``None`` ->
    ``dict`` of float64 arrays; NaN, ``-inf`` and 0 where the definition puts them."""
    R, M, d = X.shape
    K = len(loglik)
    out = {k: np.full((R,) + tail, np.nan) for k, tail in shapes(R, K, d).items()}
    for r in range(R):
        a = np.zeros(M) if log_w is None else log_w[r].astype(np.float64)
        with np.errstate(invalid="ignore"):
            alive = a > -np.inf                                       # (a NaN is dead)
        if not alive.any():
            continue
        x, a = X[r][alive].astype(np.float64), a[alive]
        l = loglik[:, r, alive].astype(np.float64)
        l = np.where(np.isnan(l), -np.inf, l)                         # a NaN carries no weight
        b = np.zeros(K) if beta is None else beta[r].astype(np.float64)
        A = _lse(a, 0)
        cols = np.concatenate([a + l, (a + _lse(b[:, None] + l, 0))[None]])   # u_k, then v: (K + 1, m)
        z = _lse(cols, 1)
        has = z > -np.inf
        with np.errstate(invalid="ignore"):
            logW = cols - z[:, None]
        W = np.where(has[:, None], np.exp(logW), np.nan)
        le = np.where(has, z - A, -np.inf)
        out["log_evidence"][r] = le
        out["responsibility"][r] = [math.exp(b[k] + le[k] - le[K]) if has[k] and b[k] > -np.inf else 0.0 for k in range(K)]
        for q in range(K + 1):
            if has[q]:
                out["ess"][r, q] = 1.0 / (W[q] ** 2).sum()
                out["mean"][r, q] = W[q] @ x
        for k in range(K):
            if has[k]:
                on = W[k] > 0
                out["divergence"][r, k] = (W[k][on] * (logW[k][on] - logW[K][on])).sum()
            for j in range(K):
                if has[k] and has[j]:
                    out["overlap"][r, j, k] = np.sqrt(W[j] * W[k]).sum()
    return out


def reference(case):
    return reference_rows(case["states"], case["log_w"], case["loglik"], case["beta"])


@functools.lru_cache(maxsize=None)
def family_case(M, d, R, K, variant):
    """A family case with its reference, computed once and shared (treat both as read-only)."""
    case = make_case(M, d, R, K, variant)
    return case, reference(case)


def torch_formulation(case, dtype=None, device=None):
    """The same definition in torch ops, fp32 on the CPU unless told otherwise: what a caller without the kernel would
    write -> ``dict`` of tensors."""
    import torch

    dtype = dtype or torch.float32
    to = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(device=device, dtype=dtype)
    return torch_rows(to(case["states"]), to(case["log_w"]), to(case["loglik"]), to(case["beta"]))


def torch_rows(X, log_w, loglik, beta):
    """``torch_formulation`` on tensors: ``X (R, M, d)``, ``log_w (R, M)`` or ``None``, ``loglik (K, R, M)``, ``beta (R, K)``
    or ``None``."""
    import torch

    R, M, d = X.shape
    K = loglik.shape[0]
    ninf = torch.full((), -math.inf, dtype=X.dtype, device=X.device)
    nan = torch.full((), math.nan, dtype=X.dtype, device=X.device)
    a = torch.zeros((R, M), dtype=X.dtype, device=X.device) if log_w is None else log_w
    b = torch.zeros((R, K), dtype=X.dtype, device=X.device) if beta is None else beta
    alive = a > -math.inf                                             # (a NaN is dead)
    l = torch.where(torch.isnan(loglik), ninf, loglik)
    L = torch.logsumexp(b.t()[:, :, None] + l, dim=0)
    cols = torch.where(alive, torch.cat([a + l, (a + L)[None]]), ninf)   # (K + 1, R, M)
    z = torch.logsumexp(cols, dim=-1)                                 # (K + 1, R)
    A = torch.logsumexp(torch.where(alive, a, ninf), dim=-1)
    dead = ~(A > -math.inf)
    has = z > -math.inf
    le = torch.where(dead, nan, z - A)
    logW = cols - z[..., None]
    W = torch.where(has[..., None], torch.exp(logW), nan)
    X0 = torch.where(alive[..., None], X, torch.zeros_like(X))
    rho = torch.where(has[:K] & (b.t() > -math.inf), torch.exp(b.t() + le[:K] - le[K]), torch.zeros_like(le[:K]))
    on = W[:K] > 0
    div = torch.where(on, W[:K] * (logW[:K] - logW[K]), torch.zeros_like(W[:K])).sum(-1)
    root = torch.sqrt(W[:K])
    out = dict(log_evidence=le.t(), responsibility=torch.where(dead, nan, rho).t(), ess=(1.0 / (W * W).sum(-1)).t(),
               mean=torch.einsum("qrm,rmd->rqd", W, X0), divergence=torch.where(has[:K], div, nan).t(),
               overlap=torch.einsum("jrm,krm->rjk", root, root))
    return {k: v.contiguous() for k, v in out.items()}


def mean_err(got, want, states, log_w, what=""):
    """``max |got - want|`` over the largest live ``|coordinate|`` of the row, the worst row; NaN exactly where the reference has it."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, "NaN placement", got, want)
    worst = 0.0
    for r in range(len(want)):
        if nan[r].all():
            continue
        with np.errstate(invalid="ignore"):
            alive = np.ones(states.shape[1], bool) if log_w is None else log_w[r] > -np.inf
        top = float(np.abs(states[r][alive]).max())
        worst = max(worst, float(np.abs(np.where(nan[r], 0.0, got[r] - want[r])).max()) / top)
    return worst


def compare(case, got, ref, what=""):
    """Holds the outputs of ``got`` (a ``dict``; ``None`` entries are skipped) to ``ref`` under the bars of the module
    docstring -> ``dict`` of errors.  Placement of NaN, ``-inf`` and exact zeros is asserted here."""
    N = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
    errs = {}
    for k in OUTPUTS:
        if got.get(k) is None:
            continue
        g, w = N(got[k]), ref[k]
        if k in ("responsibility", "overlap"):  # a modality without weight, two modalities without a common particle
            assert bool((g[w == 0] == 0).all()), (what, k, "an exact zero of the definition", g, w)
        if k in ("log_evidence", "divergence"):
            errs[k] = log_err(g, w, f"{what} {k}")
        elif k == "mean":
            errs[k] = mean_err(g, w, case["states"], case["log_w"], f"{what} {k}")
        else:
            errs[k] = rel_compare(g, w, f"{what} {k}")
    return errs

"""Inputs, fp64 reference and acceptance rule of the particle-distance kernels (``include/mmf.h``: ``MmfPfDistanceArgs`` /
``mmf_pf_distance``), in numpy; shared by ``test_distance_cases_cpu.py`` and ``test_gpu_distance.py``.

The reference restates the header's definitions, not the kernel:

    per dimension   ``q = floor(exp(t) 2^24)`` with ``t = (log_a + log_b) - max`` and the ``exp`` in fp32
                    (``_summary_cases.log_weight32``), per set; the coordinates of the particles with ``q > 0`` of both sets
                    in one STABLE sort; the two CDFs as int64 prefix sums divided once by the set's total; then
                    ``wasserstein = sum gap |D|``, ``cramer = sum gap D^2``, ``ks = max |D|`` over the ends of the tie groups
    multivariate    ``w = exp(t)`` where ``t <= 0`` (``_summary_cases.weights64``), normalised; the three expectations
                    ``E|(X - Y) / s|``, ``E|(X - X') / s|``, ``E|(Y - Y') / s|`` over dense pairs in chunks of ``CHUNK`` rows;
                    ``energy = sqrt(max(2 terms[0] - terms[1] - terms[2], 0))``

``dtype=np.float64`` is the reference.  The SAME functions with ``dtype=np.float32`` -- the divisions, gaps, pair terms and
sums in fp32 -- are the yardstick of the error rule: the kernel is held to ``err < max(REL_TOL, 3 x the yardstick's own error
against fp64)`` under ``_tol.rel_err``, and ``CAP`` is the condition on the INPUTS that keeps that bar at ``REL_TOL``."""
import functools

import numpy as np

import _summary_cases as sm
from _summary_cases import CHUNK, GUARD_ROWS, SENTINEL  # noqa: F401 (read as dc.* by the tests)

MAX_UNION = sm.MAX_M             # particles of both sets of a row pair together (the union sort's limit)
OUTPUTS = ("wasserstein", "cramer", "ks", "energy", "terms")
CDF_OUTPUTS = OUTPUTS[:3]
# (Ma, Mb): one particle; the roles swapped; exactly one wave of slots; the union 512 and one past it; both pair plans beyond
# one workgroup (workspace and finish); one past a j-tile on either side
PAIRS = ((1, 1), (1, 37), (37, 300), (300, 37), (64, 64), (255, 257), (257, 256), (513, 600), (1025, 64), (300, 1025))
SMALL_UNION = 128                # up to here the whole cross of dimensions, rows and variants; beyond, every variant once
DIMS = (1, 2, 3, 4)
RS = (1, 5)
# (variant of set A, variant of set B, scaled): the siblings' variants on either side
VARIANTS = (("plain", "plain", False), ("uniform", "plain", False), ("plain", "uniform", False), ("uniform", "uniform", False),
            ("only_a", "only_b", False), ("only_b", "only_a", False), ("dead_row", "plain", False), ("plain", "dead_row", False),
            ("plain", "plain", True))
SCALE = (0.5, 2.0, 1.0, 4.0)
CAP = 3e-5                       # REL_TOL / 3 on the yardstick's own error: with it the GPU bar is REL_TOL on every output
ENERGY_MARGIN = 0.1              # 2 terms[0] - terms[1] - terms[2] >= this share of (terms[1] + terms[2]) / 2

# (Ma, Mb, d, R, variant index) -> how many times the case's seed was replaced because a draw broke CAP or ENERGY_MARGIN;
# test_distance_cases_cpu.py holds every case to both.  All five are the uniform pair, whose two clouds overlap most: the
# first draws had margins of 0.03 .. 0.08 in their worst row
RESEED = {(64, 64, 1, 5, 3): 15, (64, 64, 2, 1, 3): 1, (64, 64, 2, 5, 3): 1, (64, 64, 3, 5, 3): 1, (1025, 64, 1, 1, 3): 1}


def make_case(Ma, Mb, d, R, variant=0, seed=0):
    """``dict(a=dict(states (R, Ma, d), log_a, log_b (R, Ma) or None), b=the same with Mb, scale=d floats or None)``: set A
    is ``_summary_cases.weighted_set``, set B an independent draw of it scaled by 1.2 and shifted by 0.5."""
    va, vb, scaled = VARIANTS[variant]
    reseed = RESEED.get((Ma, Mb, d, R, variant), 0)
    rng = np.random.default_rng(3000017 * Ma + 7013 * Mb + 1013 * d + 103 * R + 11 * variant + seed + 10007 * reseed)
    Xa, la_a, lb_a, _ = sm.weighted_set(rng, Ma, d, R, va)
    Xb, la_b, lb_b, _ = sm.weighted_set(rng, Mb, d, R, vb)
    Xb = (Xb * np.float32(1.2) + np.float32(0.5)).astype(np.float32)
    return dict(a=dict(states=Xa, log_a=la_a, log_b=lb_a), b=dict(states=Xb, log_a=la_b, log_b=lb_b),
                scale=SCALE[:d] if scaled else None)


def family():
    """``(Ma, Mb, d, R, variant)``: up to ``SMALL_UNION`` particles in the union the whole cross; beyond it every variant once
    with the dimension cycling (five rows for the variants with ``plain`` or ``dead_row`` alone, one otherwise) and the plain
    pair at every dimension."""
    for Ma, Mb in PAIRS:
        if Ma + Mb <= SMALL_UNION:
            for d in DIMS:
                for R in RS:
                    for v in range(len(VARIANTS)):
                        yield Ma, Mb, d, R, v
            continue
        for v, (va, vb, _) in enumerate(VARIANTS):
            yield Ma, Mb, DIMS[(v + Ma + Mb) % len(DIMS)], 5 if {va, vb} <= {"plain", "dead_row"} else 1, v
        for d in DIMS:
            yield Ma, Mb, d, 1, 0


def swapped(case):
    """The case with the roles of A and B exchanged."""
    return dict(case, a=case["b"], b=case["a"])


def scale64(case):
    d = case["a"]["states"].shape[-1]
    return np.ones(d) if case["scale"] is None else np.asarray(case["scale"], np.float64)


fixed_point = sm.fixed_point_weights  # K1's fixed-point weights of one set: ``(R, M)`` int64


def cdf_rows(Xa, qa, Xb, qb, dtype=np.float64):
    """The per-dimension definition on ``Xa (R, Ma, d)`` / ``Xb (R, Mb, d)`` under integer weights ``qa``, ``qb``:
    ``wasserstein, cramer, ks (R, d)`` in ``dtype``; NaN where a set has no particle with ``q > 0``."""
    R, _, d = Xa.shape
    out = [np.full((R, d), np.nan, dtype) for _ in range(3)]
    for r in range(R):
        live_a, live_b = qa[r] > 0, qb[r] > 0
        if not live_a.any() or not live_b.any():
            continue
        wa = np.concatenate([qa[r][live_a], np.zeros(int(live_b.sum()), np.int64)])
        wb = np.concatenate([np.zeros(int(live_a.sum()), np.int64), qb[r][live_b]])
        Qa, Qb = int(wa.sum()), int(wb.sum())
        for k in range(d):
            z = np.concatenate([Xa[r][live_a, k], Xb[r][live_b, k]])
            order = np.argsort(z, kind="stable")
            z = z[order].astype(dtype)
            Fa = np.cumsum(wa[order]).astype(dtype) / dtype(Qa)
            Fb = np.cumsum(wb[order]).astype(dtype) / dtype(Qb)
            D = (Fa - Fb)[:-1]
            gap = np.diff(z)
            out[0][r, k] = (gap * np.abs(D)).sum(dtype=dtype)
            out[1][r, k] = (gap * (D * D)).sum(dtype=dtype)
            ends = gap > 0
            out[2][r, k] = np.abs(D[ends]).max() if ends.any() else 0.0
    return tuple(out)


def _mean_norm(x, wx, y, wy, s, dtype):
    """``sum_i sum_j wx_i wy_j |(x_i - y_j) / s|_2`` over dense pairs in chunks of ``CHUNK`` rows of ``x``, in ``dtype``."""
    acc = dtype(0.0)
    for c in range(0, len(x), CHUNK):
        n2 = np.zeros((len(x[c:c + CHUNK]), len(y)), dtype)
        for k in range(x.shape[1]):
            e = (x[c:c + CHUNK, k, None] - y[None, :, k]) / s[k]
            e *= e
            n2 += e
        acc += dtype(wx[c:c + CHUNK] @ np.sqrt(n2) @ wy)
    return acc


def pair_rows(Xa, Wa, Xb, Wb, scale, dtype=np.float64):
    """The multivariate definition under unnormalised weights ``Wa (R, Ma)``, ``Wb (R, Mb)``: ``energy (R,)``, ``terms
    (R, 3)`` in ``dtype``; NaN where a set has no live particle."""
    R = Xa.shape[0]
    s = np.asarray(scale, dtype)
    energy, terms = np.full((R,), np.nan, dtype), np.full((R, 3), np.nan, dtype)
    for r in range(R):
        live_a, live_b = Wa[r] > 0, Wb[r] > 0
        if not live_a.any() or not live_b.any():
            continue
        x, y = Xa[r][live_a].astype(dtype), Xb[r][live_b].astype(dtype)
        wx, wy = Wa[r][live_a].astype(dtype), Wb[r][live_b].astype(dtype)
        wx, wy = wx / wx.sum(dtype=dtype), wy / wy.sum(dtype=dtype)
        t = np.array([_mean_norm(x, wx, y, wy, s, dtype), _mean_norm(x, wx, x, wx, s, dtype), _mean_norm(y, wy, y, wy, s, dtype)], dtype)
        terms[r] = t
        energy[r] = np.sqrt(max(dtype(2.0) * t[0] - t[1] - t[2], dtype(0.0)))
    return energy, terms


def _weights(side, dtype):
    """The live-weight rule of ``csrc/pf_summary.h`` with the ``exp`` in ``dtype``."""
    if dtype == np.float64:
        return sm.weights64(side)
    t = sm.log_weight32(side)
    with np.errstate(invalid="ignore"):
        return np.where(t <= 0, np.exp(t).astype(np.float32), np.float32(0.0))


def reference(case, dtype=np.float64, outputs=OUTPUTS):
    """``dict`` of the ``outputs`` of a case by the definition in ``dtype``; NaN where the definition puts it."""
    a, b = case["a"], case["b"]
    out = {}
    if set(outputs) & set(CDF_OUTPUTS):
        w, c, k = cdf_rows(a["states"], fixed_point(a), b["states"], fixed_point(b), dtype)
        out.update(wasserstein=w, cramer=c, ks=k)
    if set(outputs) & {"energy", "terms"}:
        e, t = pair_rows(a["states"], _weights(a, dtype), b["states"], _weights(b, dtype), scale64(case), dtype)
        out.update(energy=e, terms=t)
    return {k: out[k] for k in outputs}


def compare(got, want, what=""):
    """Holds one output to its reference: NaN exactly where the reference has it, and returns ``_tol.rel_err`` over the rest
    -- a row's ``d`` (or three) values as one vector, ``energy`` row by row -- or 0.0 when nothing is finite."""
    from _tol import rel_err

    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert bool((np.isnan(got) == nan).all()), (what, "NaN placement", got, want)
    if nan.all():
        return 0.0
    got, want = np.where(nan, 0.0, got), np.where(nan, 0.0, want)
    if got.ndim == 1:
        got, want = got[:, None], want[:, None]
    return rel_err(got, want, dims=1)


def bar(yardstick_error):
    """The house rule: ``max(REL_TOL, 3 x the yardstick's own error)``."""
    from _tol import REL_TOL

    return max(REL_TOL, 3.0 * yardstick_error)


@functools.lru_cache(maxsize=None)
def family_case(Ma, Mb, d, R, variant):
    """A family case with its fp64 reference and the yardstick's own error per output, computed once and shared (treat all
    three as read-only)."""
    case = make_case(Ma, Mb, d, R, variant)
    ref = reference(case)
    yard = reference(case, np.float32)
    return case, ref, {k: compare(yard[k], ref[k], k) for k in OUTPUTS}

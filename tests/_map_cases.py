"""Shared by the MAP-path-smoothing tests (``include/mmf.h``: ``mmf_pf_smooth_map``): the fp64 definition the kernel is held to
(``viterbi_reference``), a brute-force enumerator of all ``M^T`` index paths, the one-step restatement that recomputes step
``t`` in fp64 from a GIVEN previous row (so per-step checks carry no accumulated error), an fp32 yardstick -- the recursion
in numpy float32 in the kernel's operation order -- and the cases the GPU tests run and the bars they hold the kernel to.
Inputs come from ``_smooth_cases.make_case`` / ``tril``.  ``torch`` is imported inside the functions that need it.

The bars (``test_map_smoothing_cpu.py::test_the_bars_are_three_times_the_yardstick`` measures them over ``GPU_CASES`` and
checks the constants below against the rule): the yardstick's worst one-step error of ``v`` against fp64 is
``YARDSTICK_V``, its worst ``log_posterior`` error ``YARDSTICK_LP``, its worst argmax regret ``YARDSTICK_REGRET``; ``V_BAR`` and
``LP_BAR`` are each the smallest of 1e-6, 3e-6, 1e-5, 3e-5, 1e-4 that is at least three times the measured error, and
``REGRET`` is three times the measured regret -- three times is the project's allowance for summation details, which is all
the kernel differs from the yardstick in."""
import math

import numpy as np

import _smooth_cases as sc

LADDER = (1e-6, 3e-6, 1e-5, 3e-5, 1e-4)
# measured over GPU_CASES: see the module docstring.  The worst v is the "sharp" case's, where log-likelihoods of +-150 leave
# half an ulp of 8e-6 on values that the rescaling by the row's maximum brings down to O(1); the other cases stay below 5e-7.
YARDSTICK_V = 1.94e-6
YARDSTICK_LP = 1.25e-7
YARDSTICK_REGRET = 0.0   # the yardstick takes the fp64-best pair at every one of the cases' decisions
V_BAR = 1e-5
LP_BAR = 1e-6
REGRET = 3.0 * YARDSTICK_REGRET
# what two fp64 evaluations of one path's density differ by (sum_t top_t against the sum over the path's pairs: 1e-14
# measured); the allowance the brute-force comparison is given, and the end-to-end comparison on top of T * REGRET
REF_EPS = 1e-10


def ladder(err):
    """The smallest bar of ``LADDER`` that is at least three times ``err``."""
    return next(b for b in LADDER if b >= 3.0 * err)


# ------------------------------------------------------------------------------------------ the fp64 definition
def log_norm_const(L):
    """``c = sum_k log L_kk + (d / 2) log 2 pi`` in fp64."""
    L = np.asarray(L, dtype=np.float64)
    return float(np.log(np.diagonal(L)).sum() + 0.5 * L.shape[0] * math.log(2.0 * math.pi))


def pair_logp(x_next, f_prev, L):
    """``lp[i, j] = -1/2 |L^-1 (x_next[j] - f_prev[i])|^2`` in fp64 (the difference in fp64 too): ``(M, d)`` x2 -> ``(M, M)``.
    Rows or columns that hold NaN give NaN entries: the callers mask them with the dead particles they belong to."""
    Linv = np.linalg.inv(np.tril(np.asarray(L, dtype=np.float64)))
    with np.errstate(invalid="ignore"):
        e = np.asarray(x_next, dtype=np.float64)[None, :, :] - np.asarray(f_prev, dtype=np.float64)[:, None, :]
        z = e @ Linv.T
        return -0.5 * (z * z).sum(-1)


def one_step_reference(v_prev, top_prev, x_t, f_prev, ll_t, L):
    """Step ``t`` of the definition in fp64 from a given previous row: ``v_prev (M,)``, ``top_prev`` its maximum,
    ``x_t (M, d)``, ``f_prev (M, d)``, ``ll_t (M,)`` -> ``v (M,)``, ``psi (M,)`` (the first maximiser, -1 where the column is
    dead or no candidate is above ``-inf``) and the table ``cand (M, M)`` of ``(v_prev[i] - top_prev) + lp[i, j]`` with
    ``-inf`` in the rows of dead particles, which the regret checks read."""
    v_prev, ll_t = np.asarray(v_prev, dtype=np.float64), np.asarray(ll_t, dtype=np.float64)
    M = v_prev.shape[0]
    lp = pair_logp(x_t, f_prev, L)
    alive = v_prev > -np.inf
    with np.errstate(invalid="ignore"):
        cand = np.where(alive[:, None], (v_prev - top_prev)[:, None] + lp, -np.inf)
    cand[:, ll_t == -np.inf] = -np.inf
    best = cand.max(0)
    psi = np.where(best > -np.inf, cand.argmax(0), -1)
    with np.errstate(invalid="ignore"):
        v = np.where(best > -np.inf, ll_t + best, -np.inf)
    return v, psi, cand


def backtrack(v_last, psi, X):
    """``indices (T,)`` and ``path (T, d)`` of one trajectory from its last row ``v_last (M,)``, ``psi (T, M)`` and
    ``X (T, M, d)``: -1 and NaN throughout where no particle of the last step is alive."""
    T, M, d = X.shape
    idx, path = np.full(T, -1, dtype=np.int64), np.full((T, d), np.nan, dtype=X.dtype)
    if not (v_last.max() > -np.inf):
        return idx, path
    i = int(np.argmax(v_last))
    for t in range(T - 1, -1, -1):
        idx[t], path[t] = i, X[t, i]
        if t > 0:
            i = int(psi[t, i])
    return idx, path


def viterbi_reference(X, F, ll, lw0, L):
    """The definition of ``mmf_pf_smooth_map`` in fp64: ``X (T, N, M, d)``, ``F (T - 1, N, M, d)``, ``ll (T, N, M)``,
    ``lw0 (N, M)`` or None, ``L (d, d)`` -> ``dict`` of ``v (T, N, M)``, ``step_max (T, N)``, ``psi (T, N, M)``,
    ``indices (T, N)``, ``path (T, N, d)`` (the rows of ``X``, in its dtype) and ``log_posterior (N,)``."""
    X = np.asarray(X)
    T, N, M, d = X.shape
    c = log_norm_const(L)
    v, psi = np.zeros((T, N, M)), np.full((T, N, M), -1, dtype=np.int64)
    top = np.zeros((T, N))
    indices, path = np.zeros((T, N), dtype=np.int64), np.zeros((T, N, d), dtype=X.dtype)
    logpost = np.zeros(N)
    for n in range(N):
        v[0, n] = np.asarray(ll[0, n], dtype=np.float64) + (0.0 if lw0 is None else np.asarray(lw0[n], dtype=np.float64))
        top[0, n] = v[0, n].max()
        for t in range(1, T):
            v[t, n], psi[t, n], _ = one_step_reference(v[t - 1, n], top[t - 1, n], X[t, n], F[t - 1, n], ll[t, n], L)
            top[t, n] = v[t, n].max()
        indices[:, n], path[:, n] = backtrack(v[T - 1, n], psi[:, n], X[:, n])
        logpost[n] = top[:, n].sum() - (T - 1) * c if indices[0, n] >= 0 else -np.inf
    return dict(v=v, step_max=top, psi=psi, indices=indices, path=path, log_posterior=logpost)


def path_density(X, F, ll, lw0, L, idx):
    """The joint log-density of the index paths ``idx (T, N)`` in fp64, by the second form of the definition; a ``-1``
    anywhere on a path gives ``-inf``."""
    T, N = idx.shape
    c = log_norm_const(L)
    out = np.zeros(N)
    for n in range(N):
        i = idx[:, n]
        if (i < 0).any():
            out[n] = -np.inf
            continue
        s = float(ll[0, n, i[0]]) + (0.0 if lw0 is None else float(lw0[n, i[0]]))
        for t in range(1, T):
            s += float(ll[t, n, i[t]]) + pair_logp(X[t, n, i[t]][None], F[t - 1, n, i[t - 1]][None], L)[0, 0] - c
        out[n] = s
    return out


def brute_force(X, F, ll, lw0, L):
    """All ``M^T`` index paths of every trajectory scored in fp64: ``indices (T, N)`` of the best (the first in
    lexicographic order among equals; -1 where no path is above ``-inf``) and ``log_posterior (N,)``."""
    T, N, M, d = np.asarray(X).shape
    c = log_norm_const(L)
    indices, logpost = np.full((T, N), -1, dtype=np.int64), np.full(N, -np.inf)
    for n in range(N):
        score = np.asarray(ll[0, n], dtype=np.float64) + (0.0 if lw0 is None else np.asarray(lw0[n], dtype=np.float64))
        alive = [np.asarray(ll[t, n]) > -np.inf for t in range(T)]
        for t in range(1, T):
            lp = pair_logp(X[t, n], F[t - 1, n], L)
            step = np.where(alive[t - 1][:, None] & alive[t][None, :], lp + np.asarray(ll[t, n], dtype=np.float64)[None, :] - c, -np.inf)
            score = score[..., :, None] + step.reshape((1,) * (t - 1) + (M, M))
        if score.max() > -np.inf:
            indices[:, n] = np.unravel_index(int(np.argmax(score)), score.shape)
            logpost[n] = score.max()
    return indices, logpost


# ------------------------------------------------------------------------------------------ the fp32 yardstick
_F = np.float32


def _fma(a, b, c):
    """``fmaf`` on float32 arrays: the product is exact in fp64, the sum rounded once more to fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(_F)


def _whitener32(L):
    """``sqrt(log2(e) / 2) L^-1`` by forward substitution in float32, column by column (csrc/pf_smooth_math.h)."""
    L = np.asarray(L, dtype=_F)
    d = L.shape[0]
    s = np.sqrt(_F(0.5) * _F(1.4426950408889634))
    W = np.zeros((d, d), dtype=_F)
    for c in range(d):
        for r in range(c, d):
            acc = s if r == c else _F(0.0)
            for k in range(c, r):
                acc = _F(acc - _F(L[r, k] * W[k, c]))
            W[r, c] = _F(acc / L[r, r])
    return W


def yardstick32(X, F, ll, lw0, L):
    """The recursion in numpy float32 in the kernel's operation order (csrc/pf_smooth_map.hip): the difference ``x - f`` in
    fp32, the whitening as one product and fused multiply-adds, the staged ``(v - top) log2(e)``, the base-2 maximum with the
    first index, ``v = loglik + best ln 2``, the tops summed in ascending ``t``.  Same outputs as ``viterbi_reference``, float32."""
    X, F, ll = np.asarray(X, dtype=_F), np.asarray(F, dtype=_F), np.asarray(ll, dtype=_F)
    T, N, M, d = X.shape
    W = _whitener32(L)
    log2e, ln2 = _F(1.4426950408889634), _F(0.6931471805599453)
    c = _F(_F(0.5) * _F(d)) * np.log(_F(6.283185307179586))
    for r in range(d):
        c = _F(c + np.log(_F(L[r, r])))
    v, psi = np.zeros((T, N, M), dtype=_F), np.full((T, N, M), -1, dtype=np.int64)
    top = np.zeros((T, N), dtype=_F)
    indices, path = np.zeros((T, N), dtype=np.int64), np.zeros((T, N, d), dtype=_F)
    logpost = np.zeros(N, dtype=_F)
    with np.errstate(invalid="ignore", over="ignore"):
        for n in range(N):
            v[0, n] = ll[0, n] if lw0 is None else ll[0, n] + np.asarray(lw0[n], dtype=_F)
            top[0, n] = v[0, n].max()
            for t in range(1, T):
                prev = v[t - 1, n]
                dead_row, dead_col = prev == -np.inf, ll[t, n] == -np.inf
                w = np.where(dead_row, _F(-np.inf), (prev - top[t - 1, n]) * log2e).astype(_F)
                f = np.where(dead_row[:, None], _F(0.0), F[t - 1, n])
                x = np.where(dead_col[:, None], _F(0.0), X[t, n])
                dx = (x[None, :, :] - f[:, None, :]).astype(_F)                       # (i, j, d)
                g = np.broadcast_to(w[:, None], (M, M)).astype(_F)
                for r in range(d):
                    z = (W[r, 0] * dx[..., 0]).astype(_F)
                    for k in range(1, r + 1):
                        z = _fma(np.broadcast_to(W[r, k], z.shape), dx[..., k], z)
                    g = _fma(-z, z, g)
                best = g.max(0)
                none = dead_col | ~(best > -np.inf)
                psi[t, n] = np.where(none, -1, g.argmax(0))
                v[t, n] = np.where(none, _F(-np.inf), ll[t, n] + (best * ln2).astype(_F)).astype(_F)
                top[t, n] = v[t, n].max()
            indices[:, n], path[:, n] = backtrack(v[T - 1, n], psi[:, n], X[:, n])
            s = _F(0.0)
            for t in range(T):
                s = _F(s + top[t, n])
            logpost[n] = _F(s - _F(_F(T - 1) * c)) if indices[0, n] >= 0 else _F(-np.inf)
    return dict(v=v, step_max=top, psi=psi, indices=indices, path=path, log_posterior=logpost)


# ------------------------------------------------------------------------------------------ the measures
def row_error(v, ref):
    """Worst ``|v - ref| / max(1, |ref|)`` of one row against its fp64 restatement, both rescaled by their own maximum;
    entries that are ``-inf`` in both count nothing, in one alone ``inf``.  A row whose reference is all ``-inf``: 0 or ``inf``."""
    v, ref = np.asarray(v, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    dead_v, dead_r = ~(v > -np.inf) & ~np.isnan(v), ref == -np.inf
    if (dead_v != dead_r).any() or np.isnan(v).any():
        return math.inf
    if dead_r.all():
        return 0.0
    a, b = v[~dead_r] - v[~dead_r].max(), ref[~dead_r] - ref[~dead_r].max()
    return float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())


def scalar_error(a, ref):
    """``|a - ref| / max(1, |ref|)`` elementwise-worst; equal infinities count nothing."""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    same = (a == ref)
    with np.errstate(invalid="ignore"):
        e = np.where(same, 0.0, np.abs(a - ref) / np.maximum(1.0, np.abs(ref)))
    return float(np.nan_to_num(e, nan=math.inf).max()) if e.size else 0.0


def step_regret(psi_t, cand):
    """Per column ``j``: how far the fp64 value of the chosen pair ``(psi_t[j], j)`` lies below the fp64 maximum over ``i``,
    and the gap between that maximum and the fp64 runner-up (``inf`` with one candidate).  Dead columns (every candidate
    ``-inf``) must have ``psi = -1`` and count 0; a live column with ``psi = -1`` counts ``inf``."""
    M = cand.shape[1]
    best = cand.max(0)
    live = best > -np.inf
    regret = np.zeros(M)
    chosen = np.where(psi_t >= 0, cand[np.clip(psi_t, 0, M - 1), np.arange(M)], -np.inf)
    with np.errstate(invalid="ignore"):
        regret[live] = (best - chosen)[live]
    regret[~live & (psi_t >= 0)] = math.inf
    gap = np.full(M, math.inf)
    if cand.shape[0] > 1:
        two = np.sort(cand, axis=0)[-2:]
        with np.errstate(invalid="ignore"):
            gap = np.where(two[0] > -np.inf, two[1] - two[0], math.inf)
    return regret, gap


def check_run(got, X, F, ll, lw0, L):
    """The figures every comparison of a run ``got`` (the outputs of the kernel or of the yardstick, numpy) with fp64 rests on,
    each step restated from ``got``'s own previous row: ``v`` the worst ``row_error``, ``regret`` the worst ``step_regret``,
    ``psi_ok`` whether ``psi`` equals the fp64 first maximiser wherever the fp64 runner-up is farther than ``REGRET`` away,
    ``lp`` the worst error of ``log_posterior`` against ``path_density`` of ``got``'s own indices, ``end`` how far the fp64
    density of ``got``'s path lies below the fp64 optimum (worst trajectory; 0 where both are ``-inf``)."""
    T, N, M = got["v"].shape
    e_v, e_regret, psi_ok = 0.0, 0.0, True
    for n in range(N):
        v0 = np.asarray(ll[0, n], dtype=np.float64) + (0.0 if lw0 is None else np.asarray(lw0[n], dtype=np.float64))
        e_v = max(e_v, row_error(got["v"][0, n], v0))
        psi_ok = psi_ok and bool((got["psi"][0, n] == -1).all())
        for t in range(1, T):
            want, wpsi, cand = one_step_reference(got["v"][t - 1, n], got["step_max"][t - 1, n], X[t, n], F[t - 1, n], ll[t, n], L)
            e_v = max(e_v, row_error(got["v"][t, n], want))
            regret, gap = step_regret(np.asarray(got["psi"][t, n], dtype=np.int64), cand)
            e_regret = max(e_regret, float(regret.max()))
            clear = gap > REGRET
            psi_ok = psi_ok and bool((got["psi"][t, n][clear] == wpsi[clear]).all())
    idx = np.asarray(got["indices"], dtype=np.int64)
    own = path_density(X, F, ll, lw0, L, idx)
    best = viterbi_reference(X, F, ll, lw0, L)["log_posterior"]
    with np.errstate(invalid="ignore"):
        end = np.where(best == own, 0.0, best - own)
    return dict(v=e_v, regret=e_regret, psi_ok=psi_ok, lp=scalar_error(got["log_posterior"], own), end=float(end.max()))


# ------------------------------------------------------------------------------------------ the cases of the GPU tests
_WIDTHS = (1e-3, 1e-2, 0.3)
TILE, GROUP, CHUNK = 64, 8, 256  # csrc/pf_smooth_math.h: kPairThreads, kPairGroup, kPairChunk

# name -> T, N, M, d, full lower triangle, incoming log-weights given, log-likelihood scale, dead particles
GPU_CASES = {
    **{f"M{M}": (7, 3, M, 3, True, True, 0.5, None) for M in (1, 63, 64, 65, 250, 257)},   # tile, group and chunk edges
    **{f"d{d}": (7, 3, 65, d, d > 1, True, 0.5, None) for d in (1, 2, 4)},
    "T1": (1, 3, 65, 3, True, True, 0.5, None),
    "T2_N1_no_lw": (2, 1, 65, 3, False, False, 0.5, None),
    "N1_no_lw": (7, 1, 250, 2, True, False, 0.5, None),
    "sharp": (7, 3, 250, 3, True, True, 50.0, None),      # a particle or two hold the weight of every step
    "dead_some": (7, 3, 257, 3, True, True, 0.5, "some"),  # every 7th particle, NaN in its rows
    "dead_tile": (7, 3, 250, 3, True, False, 0.5, "tile"),  # particles 64 .. 127: a whole tile of columns, a quarter chunk of rows
    "dead_step": (7, 3, 65, 3, True, True, 0.5, "step"),   # step 3 of trajectory 1 has no particle alive
}


def build_case(name):
    """``X, F, ll, lw, L`` of a case of ``GPU_CASES``; ``lw`` is ``(T, N, M)`` (step 0 is what the smoother reads) or None."""
    T, N, M, d, full, use_lw, scale, dead = GPU_CASES[name]
    L = sc.tril(d, full)
    seed = 7000 + sorted(GPU_CASES).index(name)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, scale, L, seed=seed, use_lw=use_lw, dead=dead == "some")
    if dead == "tile":
        ll[:, :, TILE:2 * TILE] = -np.inf
        X[:, :, TILE:2 * TILE] = np.nan
        F[:, :, TILE:2 * TILE] = np.nan
    if dead == "step":
        ll[3, 1, :] = -np.inf
    return X, F, ll, lw, L


def planted_case(T=7, N=3, M=257, d=3, seed=41):
    """A case with one chain of particles per trajectory whose likelihood is boosted until its fp64 margin over every other
    path exceeds 10: the chain's particle at step ``t + 1`` sits exactly on the prediction of its particle at step ``t``, and
    each of its log-likelihoods is raised by 40 (any path that leaves the chain at ``k`` steps loses ``40 k`` and can win back
    at most the transition terms of its ``<= 2`` junctions with the chain, which are ``<= 0`` on the chain itself).  Returns
    ``X, F, ll, lw, L, chain (T, N)``; the CPU test checks the margin."""
    L = sc.tril(d, True)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=seed)
    rng = np.random.default_rng(seed + 1)
    chain = rng.integers(0, M, size=(T, N))
    for n in range(N):
        for t in range(T):
            ll[t, n, chain[t, n]] = ll[t, n].max() + 40.0
        for t in range(T - 1):
            F[t, n, chain[t, n]] = X[t, n, chain[t, n]]
            X[t + 1, n, chain[t + 1, n]] = F[t, n, chain[t, n]]
    return X, F, ll, lw, L, chain


def tie_case(M, T=4, N=2, d=3, seed=43):
    """Duplicated rows: particle ``a`` of every step is copied bit for bit (state, prediction, likelihood, incoming weight)
    onto particles ``b`` and ``e`` with ``a < b < e`` in different groups, chunks (``M = 257``: ``e = 256``) and column tiles,
    and boosted so that the optimum runs through it; every decision between the copies is an exact tie, which the lower
    index wins.  Returns ``X, F, ll, lw, L, a``."""
    L = sc.tril(d, True)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, 0.5, L, seed=seed)
    a, b, e = 5, min(70, M - 2), M - 1
    assert a < b < e
    for t in range(T):
        if t > 0:
            X[t, :, a] = F[t - 1, :, a]
        if t < T - 1:
            F[t, :, a] = X[t, :, a]
        ll[t, :, a] = ll[t].max(-1) + 40.0
        for k in (b, e):
            X[t, :, k], ll[t, :, k], lw[t, :, k] = X[t, :, a], ll[t, :, a], lw[t, :, a]
            if t < T - 1:
                F[t, :, k] = F[t, :, a]
    return X, F, ll, lw, L, a

"""Inputs, fp64 reference and comparison rules of the particle-mode kernel (``include/mmf.h``: ``MmfPfModesArgs`` /
``mmf_pf_modes``), in numpy on the CPU; shared by ``test_mode_cases_cpu.py`` and ``test_gpu_modes.py``.

Three families of cases:

random           ``_density_cases.family()`` without the truth variants; ``log_density`` and ``bandwidth`` are the fp64 density
                 reference's values rounded to fp32, so the kernel under test gets exact inputs and is tested alone;
                 ``link_radius`` cycles through ``TAUS`` and ``max_modes`` through ``KS``
lattice          coordinates integers / 8 in ``[-8, 8]``, levels integers / 4 in ``[0, 4)`` (many exact ties), bandwidths
                 ``LATTICE_H[:d]``, an eighth of the particles dead with NaN rows, the live ones equally weighted: every ``D2`` is
                 exact in fp32 in any evaluation order and every ``q_m`` is ``2^40``, so ``parent``, ``labels``, ``count`` and
                 ``index`` are held to exact equality; shifted by ``LATTICE_SHIFT`` (still exact) the links must not move
by construction  chains, a duplicated point and separated clusters, whose answer is known in ``O(M)``

The reference is the header's definition in fp64, the pairs in chunks of ``CHUNK`` rows so that no ``(M, M, d)`` array is
formed.  A particle takes part where its fp32 live weight is positive (``exp`` in float32: what the kernel's ``expf`` decides, far
from every weight these cases hold) and its level is not NaN.

The comparison rules are ``check_parents`` and ``check_forest``; their bars are in their docstrings."""
import functools

import numpy as np

import _density_cases as dc
import _score_cases as sk
import _summary_cases as sm
from _summary_cases import CHUNK, GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as mc.* by the tests)

MAX_MODES = 8
LDS_MASS_M = 8192        # csrc/pf_modes.hip: kLdsMassM = MMF_PF_MODES_LDS_MASS_M, beyond it the masses sit in the workspace
MASS_SCALE = 2.0 ** 40
TAUS = (1.0, 3.0)
KS = (1, 4, 8)
EPS = 1e-5               # a differing link is certified within this of the radius and of the reference's distance
MAX_CERTIFIED = 1e-3     # of a case's participating particles
CAP_FP32 = 1e-4          # of a case's particles: where numpy fp32 may differ from fp64 (the condition on the inputs)
TRUTH_VARIANTS = ("nan_truth", "no_truth")
LATTICE_H = (0.5, 1.0, 2.0, 0.25)
LATTICE_SHIFT = 1024.0
LATTICE_MS = (2, 65, 257, 513, 1025)
BY_MS = tuple(sorted({1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4096, LDS_MASS_M - 1, LDS_MASS_M, LDS_MASS_M + 1, MAX_M}))
INT_OUTPUTS = ("parent", "labels", "count", "index")
FLOAT_OUTPUTS = ("modes", "mass", "mean")
OUTPUTS = INT_OUTPUTS + FLOAT_OUTPUTS


# ------------------------------------------------------------------------------------------ the cases
def random_family():
    """``(M, d, R, variant, rule)`` of ``_density_cases.family()`` without the truth variants."""
    for case_id in dc.family():
        if case_id[3] not in TRUTH_VARIANTS:
            yield case_id


@functools.lru_cache(maxsize=None)
def random_case(M, d, R, variant, rule):
    """The density case with the fp64 reference's ``log_density`` and ``bandwidth`` rounded to fp32 as inputs (read-only)."""
    case, ref = dc.family_case(M, d, R, variant, rule)
    n = (1009 * M + 101 * d + 11 * R + dc.VARIANTS.index(variant) + dc.RULES.index(rule))
    with np.errstate(over="ignore"):
        return dict(states=case["states"], log_a=case["log_a"], log_b=case["log_b"],
                    log_density=ref["log_density"].astype(np.float32), bandwidth=ref["bandwidth"].astype(np.float32),
                    link_radius=TAUS[n % len(TAUS)], max_modes=KS[(n // len(TAUS)) % len(KS)])


def lattice_case(M, d, R, seed=0, shift=0.0, link_radius=None, max_modes=None):
    rng = np.random.default_rng(500009 * M + 71 * d + 7 * R + seed)
    X = (rng.integers(-64, 65, (R, M, d)) / 8.0).astype(np.float32)
    ell = (rng.integers(0, 16, (R, M)) / 4.0).astype(np.float32)
    lb = np.zeros((R, M), np.float32)
    sm.kill_an_eighth(rng, X, lb)
    n = M + d + R + seed
    return dict(states=(X + np.float32(shift)).astype(np.float32), log_a=None, log_b=lb, log_density=ell,
                bandwidth=np.tile(np.asarray(LATTICE_H[:d], np.float32), (R, 1)),
                link_radius=TAUS[n % 2] if link_radius is None else link_radius,
                max_modes=KS[n % 3] if max_modes is None else max_modes)


def lattice_family():
    for M in LATTICE_MS:
        for d in sk.DIMS:
            yield M, d, 3 if d == 3 else 1


def _uniform(X, ell, h, tau, K, log_b=None):
    R, M, d = X.shape
    return dict(states=X.astype(np.float32), log_a=None, log_b=log_b, log_density=ell.astype(np.float32),
                bandwidth=np.tile(np.asarray(h, np.float32), (R, 1)), link_radius=tau, max_modes=K)


CONSTRUCTIONS = ("chain", "reversed_chain", "chain_all_roots", "duplicated_point", "clusters")
CLUSTERS = 3
CLUSTER_LOG_B = (0.0, -1.0, -2.5)
CLUSTER_CENTRES = ((100.0, -3.0), (0.0, 50.0), (-80.0, 7.0))


def constructed_case(kind, M):
    """``(case, expected)`` of one row (``R = 1``): ``expected`` holds what is known without an ``M^2`` reference -- some of
    ``parent``, ``labels (M,)``, ``count``, ``index``, ``mass`` and ``mean`` (the latter three over the reported ranks, float64)."""
    m = np.arange(M)
    if kind in ("chain", "reversed_chain", "chain_all_roots"):
        # x_m = m h in the first of two dimensions, the level rising (falling) with m by 2^-10: depth M - 1
        h = (0.5, 2.0)
        X = np.zeros((1, M, 2))
        X[0, :, 0] = m * h[0]
        up = kind != "reversed_chain"
        ell = (m if up else M - 1 - m) / 1024.0
        tau = 0.5 if kind == "chain_all_roots" else 1.0
        K = 4
        case = _uniform(X, ell[None], h, tau, K)
        if kind == "chain_all_roots":
            n = min(K, M)
            exp = dict(parent=np.full(M, -1), labels=m.copy(), count=M, index=np.arange(n), mass=np.full(n, 1.0 / M),
                       mean=np.stack([X[0, :n, 0], np.zeros(n)], -1))
        else:
            root = M - 1 if up else 0
            parent = np.where(m == root, -1, m + (1 if up else -1))
            exp = dict(parent=parent, labels=np.full(M, root), count=1, index=np.asarray([root]), mass=np.ones(1),
                       mean=np.asarray([[0.5 * (M - 1) * h[0], 0.0]]))
        return case, exp
    if kind == "duplicated_point":
        X = np.tile(np.asarray([0.75, -1.5, 3.0]), (1, M, 1))
        case = _uniform(X, np.full((1, M), -2.25), (0.3, 0.5, 1.0), 3.0, 8)
        exp = dict(parent=np.where(m == 0, -1, 0), labels=np.zeros(M, int), count=1, index=np.zeros(1, int), mass=np.ones(1),
                   mean=X[0, :1].astype(np.float32).astype(np.float64))
        return case, exp
    assert kind == "clusters"
    # cluster g = m % 3 around its centre: offsets -1/4, 0, +1/4 bandwidths in the first dimension cycling with m // 3, the level
    # -|offset|: the root is the cluster's first particle at the centre (g + 3), or its only particle (g) where there is none
    g, o = m % CLUSTERS, ((m // CLUSTERS) % 3 - 1) * 0.25
    X = np.asarray(CLUSTER_CENTRES)[g][None].copy()
    X[0, :, 0] += o
    lb = np.asarray(CLUSTER_LOG_B, np.float32)[g][None]
    case = _uniform(X, -np.abs(o)[None], (1.0, 1.0), 3.0, 4, log_b=lb)
    roots = np.asarray([c + CLUSTERS if c + CLUSTERS < M else c for c in range(min(CLUSTERS, M))])
    w = np.exp((lb[0] - lb[0].max()).astype(np.float64))
    mass = np.asarray([w[g == c].sum() for c in range(len(roots))]) / w.sum()
    x64 = case["states"][0].astype(np.float64)
    mean = np.stack([(w[g == c, None] * x64[g == c]).sum(0) / w[g == c].sum() for c in range(len(roots))])
    order = np.lexsort((roots, -mass))  # (the masses differ by far more than expf's ulps)
    exp = dict(labels=roots[g], count=len(roots), index=roots[order], mass=mass[order], mean=mean[order])
    return case, exp


# ------------------------------------------------------------------------------------------ the fp64 reference
def takes_part(case):
    """``(R, M)`` bool: the fp32 live weight is positive and the level is not NaN."""
    t = sm.log_weight32(case)
    with np.errstate(invalid="ignore", under="ignore"):
        w32 = np.where(t <= 0, np.exp(t.astype(np.float32)), np.float32(0))
    return (w32 > 0) & ~np.isnan(case["log_density"])


def _above(lj, j, li, i):
    """``j > i`` in the order of the definition (broadcasting)."""
    return (lj > li) | ((lj == li) & (j < i))


def _d2(xi, xj, h):
    """``sum_k ((xi_k - xj_k) / h_k)^2`` of ``xi (n, d)`` against ``xj (m, d)`` -> ``(n, m)``, in the arrays' own precision."""
    out = np.zeros((len(xi), len(xj)), xi.dtype)
    for k in range(xi.shape[1]):
        e = (xi[:, k, None] - xj[None, :, k]) / h[k]
        e *= e
        out += e
    return out


def parents_of_row(x, ell, part, h, tau, dtype=np.float64):
    """The links of one row: ``dtype = float64`` is the reference; ``float32`` is the kernel's own arithmetic in numpy -- the
    difference, times the fp32 reciprocal, the squares summed in order."""
    M = len(x)
    parent = np.full(M, -1, np.int64)
    idx = np.flatnonzero(part)
    if not len(idx):
        return parent
    lv = ell[idx]
    if dtype == np.float64:
        xs, hs, tau2 = x[idx].astype(np.float64), h.astype(np.float64), float(np.float32(tau)) ** 2
    else:
        xs, hs, tau2 = x[idx].astype(np.float32), None, np.float32(tau) * np.float32(tau)
        ih = (np.float32(1) / h.astype(np.float32)).astype(np.float32)
    for c in range(0, len(idx), CHUNK):
        rows = slice(c, c + CHUNK)
        if dtype == np.float64:
            D2 = _d2(xs[rows], xs, hs)
        else:
            D2 = np.zeros((len(xs[rows]), len(xs)), np.float32)
            for k in range(xs.shape[1]):
                e = ((xs[rows, k, None] - xs[None, :, k]) * ih[k]).astype(np.float32)
                D2 = (D2 + e * e).astype(np.float32)
        ok = _above(lv[None, :], idx[None, :], lv[rows, None], idx[rows, None]) & (D2 <= tau2)
        j = np.argmin(np.where(ok, D2, np.inf), axis=1)  # (the first minimum: the lowest j)
        parent[idx[rows]] = np.where(ok.any(1), idx[j], -1)
    return parent


def parents(case, dtype=np.float64):
    part = takes_part(case)
    R = len(part)
    return np.stack([parents_of_row(case["states"][r], case["log_density"][r], part[r], case["bandwidth"][r], case["link_radius"],
                                    dtype) for r in range(R)])


def forest(case, parent):
    """Everything the definition derives from the links ``parent (R, M)``: ``labels (R, M)``, ``count (R,)``, and per row the
    ``roots`` (ascending), their ``Q`` (uint64), ``mass`` and ``mean`` (float64, NaN where ``Q = 0``), and the reported
    ``index (R, K)`` with ``modes``, ``mass``, ``mean`` padded as the header says."""
    X, K = case["states"], case["max_modes"]
    R, M, d = X.shape
    part = takes_part(case)
    q = np.where(part, np.floor(sm.weights64(case) * MASS_SCALE), 0.0).astype(np.uint64)
    out = dict(labels=np.full((R, M), -1, np.int64), count=np.zeros(R, np.int64), index=np.full((R, K), -1, np.int64),
               modes=np.full((R, K, d), np.nan, np.float32), mass=np.zeros((R, K)), mean=np.full((R, K, d), np.nan), rows=[])
    for r in range(R):
        idx = np.flatnonzero(part[r])
        lab = np.arange(M)
        lab[idx] = np.where(parent[r, idx] < 0, idx, parent[r, idx])
        for _ in range(max(1, int(np.ceil(np.log2(max(M, 2)))))):
            lab = lab[lab]
        assert bool((lab[lab] == lab).all()), "the links hold a cycle"
        out["labels"][r, idx] = lab[idx]
        roots = idx[parent[r, idx] < 0]
        out["count"][r] = len(roots)
        Q = np.zeros(M, np.uint64)
        np.add.at(Q, lab[idx], q[r, idx])
        total = int(q[r].sum())
        sums = np.zeros((M, d))
        np.add.at(sums, lab[idx], q[r, idx, None].astype(np.float64) * X[r, idx].astype(np.float64))
        with np.errstate(invalid="ignore", divide="ignore"):
            mass = np.where(Q[roots] > 0, Q[roots].astype(np.float64) / max(total, 1), 0.0)
            mean = sums[roots] / Q[roots].astype(np.float64)[:, None]
        out["rows"].append(dict(roots=roots, Q=Q[roots], mass=mass, mean=mean))
        order = np.lexsort((roots, -Q[roots].astype(np.float64)))[:K]  # (Q < 2^54 is exact in a double)
        n = len(order)
        out["index"][r, :n] = roots[order]
        out["modes"][r, :n] = X[r, roots[order]]
        out["mass"][r, :n] = mass[order]
        out["mean"][r, :n] = mean[order]
    return out


def reference(case):
    """The outputs of a case by the fp64 definition -> ``dict`` with ``parent`` and the keys of ``forest``."""
    parent = parents(case)
    return dict(forest(case, parent), parent=parent)


@functools.lru_cache(maxsize=None)
def random_reference(*case_id):
    return reference(random_case(*case_id))


@functools.lru_cache(maxsize=None)
def lattice_reference(M, d, R):
    return reference(lattice_case(M, d, R))


# ------------------------------------------------------------------------------------------ the comparison rules
def check_parents(case, ref_parent, got_parent, what="", cap=MAX_CERTIFIED):
    """Where ``parent`` differs from the reference the kernel's choice must be certified in fp64, all of: the chosen ``j``
    takes part and is above ``i`` (exact on the inputs), ``D2(i, j) <= tau^2 (1 + EPS)`` and ``D2(i, j) <= D2(i, ref) (1 + EPS)``
    (where the reference has a root: only the first two); a root where the reference links needs ``D2(i, ref) >= tau^2
    (1 - EPS)``.  The fp32 error of a difference-first ``D2`` is at most ``(7 + d)`` ulp, about ``7e-7``: ``EPS`` leaves a
    factor of 15.  Dead particles hold ``-1`` exactly.  No uncertified difference, and certified ones on at most ``cap`` of the
    case's participating particles.  Returns ``(certified, participating)``."""
    got_parent = np.asarray(got_parent).astype(np.int64)
    assert got_parent.shape == ref_parent.shape, (what, got_parent.shape, ref_parent.shape)
    part = takes_part(case)
    assert bool((got_parent[~part] == -1).all()), (what, "a dead particle has a parent")
    tau2 = float(np.float32(case["link_radius"])) ** 2
    certified = 0
    for r, i in zip(*np.nonzero((got_parent != ref_parent) & part)):
        j, jr = int(got_parent[r, i]), int(ref_parent[r, i])
        x, ell, h = case["states"][r].astype(np.float64), case["log_density"][r], case["bandwidth"][r].astype(np.float64)
        d2 = lambda k: float((((x[i] - x[k]) / h) ** 2).sum())
        if j < 0:
            assert j == -1 and d2(jr) >= tau2 * (1 - EPS), (what, r, i, j, jr, d2(jr), tau2)
        else:
            assert 0 <= j < len(x) and part[r, j] and bool(_above(ell[j], j, ell[i], i)), (what, r, i, j, "not above i")
            assert d2(j) <= tau2 * (1 + EPS), (what, r, i, j, d2(j), tau2)
            assert jr < 0 or d2(j) <= d2(jr) * (1 + EPS), (what, r, i, j, jr, d2(j), d2(jr))
        certified += 1
    n = int(part.sum())
    assert certified <= cap * n, (what, f"{certified} certified differences among {n} particles")
    return certified, n


def check_forest(case, got, what="", exact_index=False):
    """``labels``, ``count``, ``index``, ``modes``, ``mass`` and ``mean`` of ``got`` (numpy arrays; any may be ``None`` except
    ``parent``) against the reference evaluated on ``got["parent"]``: labels and count exactly, modes the bit copies of the
    states at ``index``, ranks beyond the count padded ``-1 / NaN / 0 / NaN``; every reported root's mass and mean against the
    reference's for THAT root under ``_score_cases.compare`` (returned: the worst of them, to be held to ``REL_TOL``); the
    ranking as a property -- the reported masses do not increase, the roots are distinct roots of the forest, and no
    unreported root's reference mass exceeds the smallest reported one by more than ``REL_TOL``.  ``exact_index``: the index
    equals the reference's (cases whose ``q_m`` are exact)."""
    from _tol import REL_TOL

    ref = forest(case, np.asarray(got["parent"]).astype(np.int64))
    R, K = ref["index"].shape
    if got.get("labels") is not None:
        assert np.array_equal(np.asarray(got["labels"]), ref["labels"]), (what, "labels")
    if got.get("count") is not None:
        assert np.array_equal(np.asarray(got["count"]), ref["count"]), (what, "count", got["count"], ref["count"])
    index = got.get("index")
    if index is None:  # (the float outputs cannot be placed without it)
        return 0.0
    index = np.asarray(index).astype(np.int64)
    if exact_index:
        assert np.array_equal(index, ref["index"]), (what, "index", index, ref["index"])
    states = np.ascontiguousarray(case["states"], np.float32)
    worst = 0.0
    for r in range(R):
        row, n = ref["rows"][r], min(int(ref["count"][r]), K)
        assert bool((index[r, n:] == -1).all()) and bool((index[r, :n] >= 0).all()), (what, r, index[r], n)
        assert len(set(index[r, :n].tolist())) == n and set(index[r, :n].tolist()) <= set(row["roots"].tolist()), (what, r, index[r])
        at = np.searchsorted(row["roots"], index[r, :n])
        if got.get("modes") is not None:
            m = np.ascontiguousarray(got["modes"][r], np.float32)
            assert bool((m[:n].view(np.uint32) == states[r, index[r, :n]].view(np.uint32)).all()), (what, r, "modes")
            assert bool(np.isnan(m[n:]).all()), (what, r, "modes beyond the count")
        if got.get("mass") is not None:
            mass = np.asarray(got["mass"][r], np.float64)
            assert bool((mass[n:] == 0).all()), (what, r, "mass beyond the count")
            if n:
                worst = max(worst, sk.compare(mass[:n], row["mass"][at], f"{what} mass"))
                assert bool((np.diff(mass[:n]) <= 0).all()), (what, r, "the reported masses increase", mass)
                rest = np.delete(row["mass"], at)
                bar = REL_TOL * max(rest.max(), 1e-3 * row["mass"].max()) if len(rest) else 0.0  # (the metric of compare)
                assert not len(rest) or rest.max() <= mass[:n].min() + bar, (what, r, "an unreported root is heavier")
        if got.get("mean") is not None:
            mean = np.asarray(got["mean"][r], np.float64)
            assert bool(np.isnan(mean[n:]).all()), (what, r, "mean beyond the count")
            if n:
                worst = max(worst, sk.compare(mean[:n], row["mean"][at], f"{what} mean"))
    return worst

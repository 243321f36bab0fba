"""Backward-simulation particle smoothing on the GPU (``include/mmf.h``: ``mmf_pf_smooth_simulate``;
``ParticleFilter.smooth(method="simulation")`` / ``evaluation.run_filter(smooth_method="simulation")``).

A sampler has no single right answer to compare with, so the kernel's draws are held to an fp64 restatement of the definition
one step at a time: for every step of every path the drawn index must sit where the uniform falls in the fp64 CDF
CONDITIONED ON THE KERNEL'S OWN ``j_{t+1}`` (``_violations``), within ``2 REL_TOL`` -- the project's bar of 1e-4 on the
exponent, once in the numerator and once in the normaliser.  One boundary crossing then cannot make later steps incomparable.
The copies, ranges and reproducibility are exact checks; the distribution is held to the marginal smoother's moments."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _smooth_cases as sc
from _tol import REL_TOL, rel_err

B = 2            # draws of a workgroup (csrc/pf_smooth_simulate.hip: kSimDraws)
THREADS = 256    # threads of a workgroup (kSimThreads): a thread owns ceil(M / THREADS) rows, staged 1, 2 or 4 at a time
CDF_TOL = 2 * REL_TOL
MIN_PROB, MIN_SHARE = 2e-3, 0.8  # the share of drawn particles whose fp64 probability makes a misplaced index visible


# ------------------------------------------------------------------------------------------ the fp64 restatement
def _step_cdf(X, F, a, Linv, t, n, jnext):
    """``c_t`` of the definition for trajectory ``n``, normalised, one row per draw: ``a (T, N, M)`` the fp64 log-weights,
    ``jnext (S,)`` the particles chosen at ``t + 1`` (``None`` at the last step: one row).  Rows of dead particles are not read."""
    alive = a[t, n] > -np.inf
    v = np.where(alive, a[t, n], -np.inf)[None, :]
    if jnext is not None:
        x = X[t + 1, n][jnext].astype(np.float64)
        f = np.where(alive[:, None], F[t, n].astype(np.float64), 0.0)
        z = (x[:, None, :] - f[None, :, :]) @ Linv.T
        v = v - 0.5 * (z * z).sum(-1)
    with np.errstate(invalid="ignore"):
        p = np.exp(v - v.max(-1, keepdims=True))
    c = np.cumsum(p, -1)
    return c / c[:, -1:]


def _log_weights(ll, lw):
    return ll.astype(np.float64) + (0.0 if lw is None else lw.astype(np.float64))


def _violations(X, F, ll, lw, L, u, idx, steps=None, trajs=None):
    """Every drawn index against the fp64 CDF conditioned on the drawn ``j_{t+1}``: ``c[j - 1] - u`` and ``u - c[j]`` (<= 0
    and < 0 where the uniform falls inside the particle's interval) and the fp64 probability of every drawn particle,
    ``(T, N, S)`` each.  ``steps`` / ``trajs``: the ones to look at (default all)."""
    T, N, M, d = X.shape
    S = idx.shape[2]
    a = _log_weights(ll, lw)
    Linv = np.linalg.inv(np.tril(np.asarray(L, dtype=np.float64)))
    below, above, prob = np.full((T, N, S), -np.inf), np.full((T, N, S), -np.inf), np.ones((T, N, S))
    rows = np.arange(S)
    for n in (range(N) if trajs is None else trajs):
        for t in (range(T) if steps is None else steps):
            c = _step_cdf(X, F, a, Linv, t, n, idx[t + 1, n] if t < T - 1 else None)
            c = np.broadcast_to(c, (S, M))
            j = idx[t, n]
            hi = c[rows, j]
            lo = np.where(j > 0, c[rows, np.maximum(j - 1, 0)], 0.0)
            uu = u[t, n].astype(np.float64)
            below[t, n], above[t, n], prob[t, n] = lo - uu, uu - hi, hi - lo
    return below, above, prob


def _simulate64(X, F, ll, lw, L, u):
    """The definition in fp64 numpy: ``indices (T, N, S)``."""
    T, N, M, d = X.shape
    S = u.shape[2]
    a = _log_weights(ll, lw)
    Linv = np.linalg.inv(np.tril(np.asarray(L, dtype=np.float64)))
    idx = np.zeros((T, N, S), dtype=np.int64)
    for n in range(N):
        for t in range(T - 1, -1, -1):
            c = np.broadcast_to(_step_cdf(X, F, a, Linv, t, n, idx[t + 1, n] if t < T - 1 else None), (S, M))
            hit = c > u[t, n].astype(np.float64)[:, None]
            last = M - 1 - np.argmax((np.diff(c, prepend=0.0, axis=1) > 0)[:, ::-1], axis=1)  # the last particle with weight
            idx[t, n] = np.where(hit.any(1), hit.argmax(1), last)
    return idx


def _tril(d, full, factor=0.3):
    """The process noise of the kernel cases: ``factor`` times the factor of the marginal smoother's cases."""
    return sc.tril(d, full, factor=factor)


_WIDTHS = (1e-2, 0.1, 0.3)


def _make_case(T, N, M, d, L, seed, S, use_lw=True, ll_scale=0.5, dead=True):
    """A run a filter could have left (``_smooth_cases.make_case``; ``dead``: every 7th particle, from particle 3, has
    log-likelihood ``-inf`` and NaN rows in ``X`` and ``F``), and after it, from the same generator, the uniforms
    ``(T, N, S)`` float32 in [0, 1)."""
    rng = np.random.default_rng(seed)
    X, F, ll, lw = sc.make_case(T, N, M, d, _WIDTHS, ll_scale, L, rng, use_lw=use_lw, dead=dead)
    return X, F, ll, lw, rng.random(size=(T, N, S), dtype=np.float32)


def _run(X, F, ll, lw, L, u, want_cov=True):
    """``_abi.pf_smooth_simulate`` on numpy inputs -> ``indices, trajectories, mean, cov`` on the device (pre-filled with
    values a forgotten write would leave visible)."""
    from multimodalfilter_amd import _abi

    dev = sc.dev()
    T, N, M, d = X.shape
    S = u.shape[2]
    G = sc.to_device
    idx = torch.full((T, N, S), -7, dtype=torch.int32, device=dev)
    traj = torch.full((T, N, S, d), 12345.0, device=dev)
    mean = torch.full((T, N, d), 12345.0, device=dev)
    cov = torch.full((T, N, d, d), 12345.0, device=dev) if want_cov else None
    _abi.pf_smooth_simulate(G(X), G(F) if T > 1 else None, G(ll), G(lw), G(L), G(u), idx, traj, mean, cov)
    torch.cuda.synchronize()
    return idx, traj, mean, cov


def _gather(X, idx):
    """``X[t, n, idx[t, n, s]]``: ``(T, N, S, d)``."""
    X = torch.as_tensor(X)
    return torch.gather(X, 2, idx.long().cpu()[..., None].expand(idx.shape + (X.shape[-1],)))


def _check_draws(X, F, ll, lw, L, u, idx, what, steps=None, trajs=None, share=True):
    """Check 1 on a run; prints the figures before asserting and returns the worst violation."""
    below, above, prob = _violations(X, F, ll, lw, L, u, idx.cpu().numpy().astype(np.int64), steps, trajs)
    worst = float(max(below.max(), above.max()))
    big = float((prob >= MIN_PROB).mean())
    print(f"{what}: worst CDF violation {worst:.3e} (bound {CDF_TOL:.0e}), share of drawn particles with fp64 probability >= "
          f"{MIN_PROB:.0e}: {big:.3f}")
    assert not share or big >= MIN_SHARE, (what, big)
    assert bool((below <= CDF_TOL).all()) and bool((above < CDF_TOL).all()), (what, worst)  # c[j - 1] - tol <= u < c[j] + tol
    return worst


# ------------------------------------------------------------------------------------------ 1 + 2. kernel cases
# (M, d, T, S, N, incoming log-weights, full L, noise factor): every M of {1, 63, 65, 300, 1100}, d of 1 .. 4, T of {1, 2, 6},
# S of {1, B - 1, B + 1, 70} and N of {1, 3}, with and without logw_in, full and diagonal L; and the particle counts on either
# side of the two changes of staging depth (one / two / four rows of a segment per chunk: M = 256 | 257, 512 | 513).
_CASES = [
    (65, 1, 6, 70, 3, True, False, 0.3),
    (300, 3, 6, 70, 3, True, True, 0.3),
    (300, 3, 6, B + 1, 1, False, True, 0.05),
    (1100, 2, 6, 70, 3, True, True, 0.3),
    (63, 4, 6, B - 1, 3, False, False, 0.3),
    (1, 2, 6, 1, 1, True, True, 0.3),
    (65, 2, 2, 70, 3, False, True, 0.3),
    (63, 1, 1, B + 1, 1, True, False, 0.3),
    (65, 3, 1, 70, 3, False, True, 0.3),
    (300, 4, 2, 70, 1, True, False, 0.3),
    (65, 4, 6, B - 1, 1, True, False, 0.3),
    (1100, 3, 6, 1, 3, False, False, 0.05),
    (300, 1, 6, B + 1, 3, True, False, 0.3),
    (1, 4, 1, 70, 3, False, False, 0.3),
    (256, 3, 6, 70, 1, True, True, 0.3),
    (257, 3, 6, 70, 1, True, True, 0.3),
    (512, 2, 6, 70, 1, True, True, 0.3),
    (513, 2, 6, 70, 1, True, True, 0.3),
    (1100, 1, 6, 70, 3, True, False, 0.05),
]
_IDS = ["M{}-d{}-T{}-S{}-N{}-{}-{}-x{}".format(M, d, T, S, N, "lw" if lw else "nolw", "full" if full else "diag", k)
        for M, d, T, S, N, lw, full, k in _CASES]


@functools.lru_cache(maxsize=None)
def _case_run(case):
    M, d, T, S, N, use_lw, full, factor = case
    L = _tril(d, full, factor)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed=1000 * M + 100 * d + 10 * T + S + N, S=S, use_lw=use_lw)
    return (X, F, ll, lw, L, u), _run(X, F, ll, lw, L, u)


@pytest.mark.parametrize("case", _CASES, ids=_IDS)
def test_every_drawn_index_is_consistent_with_the_fp64_cdf(case):
    """Check 1: ``c[j - 1] - tol <= u < c[j] + tol`` for every ``(t, n, s)``, in fp64, conditioned on the kernel's own
    ``j_{t+1}``; and the inputs have teeth: at least 80 % of the drawn particles have fp64 probability >= 2e-3, so that an
    index off by one is a violation of 1e-3 or more."""
    inputs, (idx, traj, mean, cov) = _case_run(case)
    M = case[0]
    assert bool(((idx >= 0) & (idx < M)).all())
    _check_draws(*inputs, idx, "case " + _IDS[_CASES.index(case)])


@pytest.mark.parametrize("case", _CASES, ids=_IDS)
def test_trajectories_are_copies_and_no_dead_particle_is_drawn(case):
    """Check 2: ``trajectories`` is the gather of ``X`` by ``indices``, bit for bit; every index is in ``[0, M)``; no chosen
    particle has weight zero (every 7th particle has ``loglik = -inf`` and NaN rows in ``X`` and ``F``); the moments are
    finite and are those of the trajectories."""
    (X, F, ll, lw, L, u), (idx, traj, mean, cov) = _case_run(case)
    M, d, T, S, N = case[:5]
    assert idx.dtype == torch.int32 and idx.shape == (T, N, S) and traj.shape == (T, N, S, d)
    assert bool(((idx >= 0) & (idx < M)).all())
    assert torch.equal(traj.cpu(), _gather(X, idx))
    chosen_ll = torch.gather(torch.as_tensor(ll), 2, idx.long().cpu())
    assert bool(torch.isfinite(chosen_ll).all()) and bool(torch.isfinite(traj).all())
    if M > 3:
        assert not bool((idx % 7 == 3).any())
    t64 = traj.double().cpu()
    m64 = t64.mean(2)
    c64 = torch.einsum("tnsi,tnsj->tnij", t64 - m64[:, :, None], t64 - m64[:, :, None]) / S
    e_mean = max(rel_err(mean[:, n], m64[:, n], dims=1) for n in range(N))
    scale = float(c64.flatten(2).norm(dim=-1).max())
    e_cov = 0.0 if scale == 0.0 else max(rel_err(cov[:, n], c64[:, n], dims=2) for n in range(N))
    print(f"moments of the draws against fp64: mean {e_mean:.2e} cov {e_cov:.2e}")
    assert e_mean <= REL_TOL and e_cov <= REL_TOL
    assert torch.equal(cov, cov.transpose(-1, -2))
    if scale == 0.0:
        assert float(cov.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------ 3. edge draws
def _flat_case(T, N, M, d, seed, S, tail=2):
    """Weights and transition densities all within a few e-folds of each other (noise as wide as the cloud): no particle's
    probability underflows in fp32, so the first and the last particle of positive weight are what ``u = 0`` and the largest
    float below 1 must give.  The first two and the last ``tail`` particles are dead beside every 7th."""
    L = (0.5 * np.eye(d)).astype(np.float32)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed, S)
    for x, fill in ((ll, -np.inf), (X, np.nan), (F, np.nan)):
        x[:, :, :2] = fill
        x[:, :, M - tail:] = fill
    return X, F, ll, lw, L, u


@pytest.mark.parametrize("M", [300, 1100, 65 * THREADS])
def test_the_ends_of_the_unit_interval_give_the_first_and_the_last_live_particle(M):
    """``u = 0``: the first particle of positive weight at every step; the largest float below 1: the last one.  M = 16640:
    a thread's segment is 65 rows, longer than a wave, and the last live particle sits in the second lap of the walk over it."""
    T, N, d, S = 3, 2, 3, B + 1
    X, F, ll, lw, L, u = _flat_case(T, N, M, d, seed=7 + M, S=S, tail=0 if M == 65 * THREADS else 2)
    alive = np.flatnonzero(np.isfinite(ll[0, 0]))
    first, last = int(alive[0]), int(alive[-1])
    assert first == 2 and np.isfinite(ll[:, :, [first, last]]).all()
    assert last == M - 1 if M == 65 * THREADS else last in (M - 3, M - 4)  # (M - 1: row 64 of the last thread's segment)
    idx, traj, mean, cov = _run(X, F, ll, lw, L, np.zeros_like(u))
    assert bool((idx == first).all()), idx.unique()
    assert torch.equal(traj.cpu(), _gather(X, idx))
    below_one = np.full_like(u, np.nextafter(np.float32(1.0), np.float32(0.0)))
    idx, traj, mean, cov = _run(X, F, ll, lw, L, below_one)
    assert bool((idx == last).all()), idx.unique()
    assert torch.equal(traj.cpu(), _gather(X, idx))
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)  # (and ordinary uniforms at this size: check 1, without the share)
    assert bool(((idx >= 0) & (idx < M)).all())
    _check_draws(X, F, ll, lw, L, u, idx, f"flat M={M}", share=False)


@pytest.mark.parametrize("M", [300, 1100])
def test_a_uniform_of_one_takes_the_rounding_fallback_to_the_last_live_particle(M):
    """``u = 1`` is outside the contract's ``[0, 1)``, and it is the one input that is CERTAIN to leave no particle with
    ``c[i] > u c[M - 1]``: the path the definition reserves for rounding (no thread's inclusive sum exceeds the goal; the last
    thread with weight, and in its segment the last row with weight).  Draws of ordinary uniforms in the same workgroups are
    the ones they are without it."""
    T, N, d, S = 3, 2, 3, B + 1
    X, F, ll, lw, L, u = _flat_case(T, N, M, d, seed=70 + M, S=S)
    last = int(np.flatnonzero(np.isfinite(ll[0, 0]))[-1])
    idx, traj, mean, cov = _run(X, F, ll, lw, L, np.ones_like(u))
    assert bool((idx == last).all()), idx.unique()
    assert torch.equal(traj.cpu(), _gather(X, idx))
    ref = _run(X, F, ll, lw, L, u)
    mixed = u.copy()
    mixed[:, :, 2] = 1.0  # one draw of every workgroup's first block takes the fallback, its neighbours do not
    idx, traj, mean, cov = _run(X, F, ll, lw, L, mixed)
    assert bool((idx[:, :, 2] == last).all())
    keep = [s for s in range(S) if s != 2]
    assert torch.equal(idx[:, :, keep], ref[0][:, :, keep]) and torch.equal(traj[:, :, keep], ref[1][:, :, keep])


def test_single_step_and_single_particle():
    """``T = 1``: the draws follow the filter's own weights (check 1 against their CDF) and read neither ``pred_steps`` nor
    ``L``'s off-diagonal; ``M = 1``: the one particle at every step, ``mean`` its state, ``cov`` zero."""
    L = _tril(3, True)
    X, F, ll, lw, u = _make_case(1, 3, 65, 3, L, seed=1, S=70)
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    _check_draws(X, F, ll, lw, L, u, idx, "T=1")
    assert torch.equal(traj.cpu(), _gather(X, idx))
    L = _tril(2, False)
    X, F, ll, lw, u = _make_case(5, 2, 1, 2, L, seed=2, S=B + 1, dead=False)
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    assert bool((idx == 0).all())
    assert torch.equal(traj.cpu(), torch.from_numpy(X[:, :, :1]).expand(5, 2, B + 1, 2))
    assert torch.equal(mean.cpu(), torch.from_numpy(X[:, :, 0])) and float(cov.abs().max()) == 0.0


def test_one_heavy_particle_beside_weights_that_underflow():
    """Particle 18 has ``exp(200)`` times the weight of the others: their probabilities underflow in fp32.  At the last step
    alone: every path ends in particle 18 and goes back from there as check 1 says.  At every step, with a transition as wide
    as the cloud (whitened distances of a few units, nothing beside 200): every draw takes particle 18 at every step."""
    T, N, M, d, S = 5, 3, 300, 3, 70
    L = _tril(d, True)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed=12, S=S)
    ll[-1, :, 18] = 200.0
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    assert bool((idx[-1] == 18).all()) and bool(((idx >= 0) & (idx < M)).all())
    assert torch.equal(mean[-1].cpu(), torch.from_numpy(X[-1, :, 18])) and float(cov[-1].abs().max()) == 0.0
    _check_draws(X, F, ll, lw, L, u, idx, "one heavy particle at the last step", share=False)
    X, F, ll, lw, L, u = _flat_case(T, N, M, d, seed=13, S=S)
    ll[:, :, 18] = 200.0
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    assert bool((idx == 18).all())
    assert torch.equal(mean.cpu(), torch.from_numpy(X[:, :, 18])) and float(cov.abs().max()) == 0.0
    _check_draws(X, F, ll, lw, L, u, idx, "one heavy particle at every step")


# ------------------------------------------------------------------------------------------ 4. reproducibility
@pytest.mark.parametrize("M", [300, 1100])
def test_two_calls_fewer_draws_and_fewer_trajectories_give_the_same_paths(M):
    """Two calls are bit-equal; ``S = 70`` against ``S = 8`` on ``u[..., :8]`` gives the same first 8 paths, trajectories
    included (another grid, another place in the workgroup's block of draws for none of them, other neighbours for all);
    ``N = 3`` against trajectory 1 alone gives the same paths for that trajectory.  A null ``cov`` changes nothing else and
    null incoming log-weights are uniform ones."""
    T, N, d, S = 6, 3, 3, 70
    L = _tril(d, True)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed=3 + M, S=S)
    a, b = _run(X, F, ll, lw, L, u), _run(X, F, ll, lw, L, u)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    few = _run(X, F, ll, lw, L, u[..., :8])
    assert torch.equal(few[0], a[0][..., :8]) and torch.equal(few[1], a[1][:, :, :8])
    shifted = _run(X, F, ll, lw, L, u[..., 3:])  # (every draw in another slot of another workgroup)
    assert torch.equal(shifted[0], a[0][..., 3:]) and torch.equal(shifted[1], a[1][:, :, 3:])
    one = _run(X[:, 1:2], F[:, 1:2], ll[:, 1:2], lw[:, 1:2], L, u[:, 1:2])
    for x, y in zip(a, one):
        assert torch.equal(x[:, 1:2], y)
    bare = _run(X, F, ll, lw, L, u, want_cov=False)
    assert bare[3] is None and all(torch.equal(x, y) for x, y in zip(bare[:3], a[:3]))
    uniform, zeros = _run(X, F, ll, None, L, u), _run(X, F, ll, np.zeros_like(lw), L, u)
    for x, y in zip(uniform, zeros):
        assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------ 5. dead draws, no faults
def test_a_step_without_weight_kills_the_draws_from_there_back():
    """Trajectory 1's step ``t = 2`` has every ``loglik = -inf``: its indices are -1 and its states NaN for ``t <= 2``, valid
    for ``t > 2``; ``mean`` / ``cov`` NaN exactly there.  The other trajectories have the bits of the run without it."""
    T, N, M, d, S = 6, 3, 300, 3, B + 1
    L = _tril(d, True)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed=41, S=S)
    ref = _run(X, F, ll, lw, L, u)
    ll = ll.copy()
    ll[2, 1] = -np.inf
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    assert bool((idx[:3, 1] == -1).all()) and bool(torch.isnan(traj[:3, 1]).all())
    assert bool(torch.isnan(mean[:3, 1]).all()) and bool(torch.isnan(cov[:3, 1]).all())
    assert bool(((idx[3:, 1] >= 0) & (idx[3:, 1] < M)).all())
    for x, y in zip((idx, traj, mean, cov), ref):
        assert torch.equal(x[3:, 1], y[3:, 1])
        assert torch.equal(x[:, 0], y[:, 0]) and torch.equal(x[:, 2], y[:, 2])
    assert bool(torch.isfinite(mean[:, 0]).all()) and bool(torch.isfinite(cov[:, 2]).all())
    # a NaN log-weight at one step of trajectory 0: a v is NaN, the draws die there
    ll[4, 0, 5] = np.nan
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    assert bool((idx[:5, 0] == -1).all()) and bool((idx[5, 0] >= 0).all()) and bool(torch.isnan(traj[:5, 0]).all())
    assert torch.equal(idx[:, 2], ref[0][:, 2])


def test_a_bad_noise_factor_kills_every_draw_and_does_not_fault():
    """A zero and a NaN on the diagonal of ``L`` (and a negative and an infinite one): every index is -1, everything else is
    NaN, and the call returns 0 -- ``T = 1``, where ``L`` is not used, included."""
    L = _tril(3, True)
    X, F, ll, lw, u = _make_case(3, 2, 70, 3, L, seed=21, S=B + 1)
    for T in (3, 1):
        for bad in (0.0, math.nan, -0.02, math.inf):
            Lb = L.copy()
            Lb[1, 1] = bad
            idx, traj, mean, cov = _run(X[:T], F[:T - 1], ll[:T], lw[:T], Lb, u[:T])  # (raises unless the call returns 0)
            assert bool((idx == -1).all()), (T, bad)
            for x in (traj, mean, cov):
                assert bool(torch.isnan(x).all()), (T, bad)


# ------------------------------------------------------------------------------------------ 6. the smoothing distribution
@pytest.mark.parametrize("M,d,T,N,S", [(64, 2, 5, 2, 4096), (300, 3, 5, 2, 2048)])
def test_the_draws_follow_the_smoothing_distribution(M, d, T, N, S):
    """The mean over the draws lies within ``5 sqrt(var_marg / S) + REL_TOL`` per coordinate of the mean that
    ``mmf_pf_smooth_marginal`` gives on the same inputs (``var_marg``: the diagonal of its covariance): given the particles,
    the expectation of a backward-simulation draw's state at step ``t`` IS the marginal smoother's mean and its variance the
    marginal smoother's.  Statistical, but seeded: deterministic.  The fp64 restatement is held to the bound first, so that a
    failure points at the kernel.  ``cov`` is the sample covariance of ``trajectories``."""
    from multimodalfilter_amd import _abi

    dev = sc.dev()
    L = _tril(d, True)
    X, F, ll, lw, u = _make_case(T, N, M, d, L, seed=600 + M, S=S, dead=False)
    G = sc.to_device
    mw, mmean, mcov = torch.empty((T, N, M), device=dev), torch.empty((T, N, d), device=dev), torch.empty((T, N, d, d), device=dev)
    _abi.pf_smooth_marginal(G(X), G(F), G(ll), G(lw), G(L), mw, mmean, mcov, None)
    mmean = mmean.double().cpu()
    bound = 5.0 * (torch.diagonal(mcov.double().cpu(), dim1=-2, dim2=-1) / S).sqrt() + REL_TOL
    idx64 = torch.from_numpy(_simulate64(X, F, ll, lw, L, u))
    mean64 = _gather(X, idx64).double().mean(2)
    idx, traj, mean, cov = _run(X, F, ll, lw, L, u)
    r64, r = ((mean64 - mmean).abs() / bound).max(), ((mean.double().cpu() - mmean).abs() / bound).max()
    same = float((idx.cpu() == idx64).all(0).float().mean())
    print(f"M={M} S={S}: |mean - marginal mean| / bound: fp64 restatement {float(r64):.3f}, kernel {float(r):.3f}; "
          f"whole paths equal to the restatement's: {same:.4f}")
    assert bool(((mean64 - mmean).abs() <= bound).all()), "the fp64 restatement itself misses the bound"
    assert bool(((mean.double().cpu() - mmean).abs() <= bound).all())
    t64 = traj.double().cpu()
    m64 = t64.mean(2)
    c64 = torch.einsum("tnsi,tnsj->tnij", t64 - m64[:, :, None], t64 - m64[:, :, None]) / S
    e_cov = max(rel_err(cov[:, n], c64[:, n], dims=2) for n in range(N))
    e_mean = max(rel_err(mean[:, n], m64[:, n], dims=1) for n in range(N))
    print(f"cov against the fp64 sample covariance of the trajectories: {e_cov:.2e}; mean {e_mean:.2e}")
    assert e_cov <= REL_TOL and e_mean <= REL_TOL
    assert torch.equal(cov, cov.transpose(-1, -2))
    _check_draws(X, F, ll, lw, L, u, idx, f"distribution M={M}", share=False)


# ------------------------------------------------------------------------------------------ 7. whole filters
_CONFIGS = {"plain": {}, "ess": {"resample_ess_threshold": 0.5}}


@pytest.mark.parametrize("config", list(_CONFIGS))
@pytest.mark.parametrize("cls", ["DoorParticleFilter", "DoorCrossmodalParticleFilter"])
def test_filter_simulation_smoothing(cls, config):
    """``forward_loop`` with ``record_history``, then ``smooth(method="simulation", num_draws=16)``: the estimates and the
    belief on return have the bits of a run without smoothing; ``last_smoothed`` has the stated fields and shapes; check 1
    holds on the recorded history with the predictions ``F_t`` the test obtains itself; ``ReplayNoise`` uniforms reproduce
    the paths; the other two methods leave the records they left before."""
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    N, M, T, S = 4, 300, 8, 16
    f, d, traj, obs, ctrl, cov = sc.small_filter(cls, N, M, T, dev)
    for k, v in _CONFIGS[config].items():
        setattr(f, k, v)

    def run(history):
        f.record_history = history
        f.noise = mmf.NoiseSource(99)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        return est.clone(), f.particle_states.clone(), f.particle_log_weights.clone()

    plain = run(False)
    kept = run(True)
    h = f.last_history
    mean = f.smooth(method="simulation", num_draws=S)
    torch.cuda.synchronize()
    for x, y in zip(plain, kept):
        assert torch.equal(x, y)
    assert torch.equal(f.particle_states, kept[1]) and torch.equal(f.particle_log_weights, kept[2])  # smoothing touches no belief
    rec = f.last_smoothed
    assert set(vars(rec)) == {"covariance", "trajectories", "indices", "num_draws", "lag", "method"}
    assert rec.method == "simulation" and rec.lag is None and rec.num_draws == S
    assert mean.shape == (T, N, d) and rec.covariance.shape == (T, N, d, d)
    assert rec.trajectories.shape == (T, N, S, d) and rec.indices.shape == (T, N, S) and rec.indices.dtype == torch.int32
    assert bool(((rec.indices >= 0) & (rec.indices < M)).all())
    assert torch.equal(rec.trajectories, torch.gather(h.states, 2, rec.indices.long()[..., None].expand(T, N, S, d)))
    assert torch.equal(rec.covariance, rec.covariance.transpose(-1, -2))
    assert rel_err(mean, rec.trajectories.double().mean(2), dims=1) <= REL_TOL
    # the uniforms it drew: the same stream position, drawn again
    f.noise = mmf.NoiseSource(99)
    f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
    f.record_history = True
    f.forward_loop(observations=obs, controls=ctrl)
    u = f.noise.uniform((T, N, S), like=h.states)
    dyn = f.dynamics_model
    with torch.no_grad():
        ctx = dyn.encode_controls(h.controls[1:].reshape((T - 1) * N, -1))
        F = dyn.propagate_encoded(h.states[:-1].reshape((T - 1) * N, M, d), ctx, None).reshape(T - 1, N, M, d)
    C = lambda x: x.detach().cpu().numpy()
    _check_draws(C(h.states), C(F), C(h.log_likelihoods), C(h.log_weights_in), C(dyn.scale_tril()), C(u), rec.indices,
                 f"{cls} {config}", share=False)
    f.last_history = h
    f.noise = mmf.ReplayNoise(uniforms=[u.cpu()])
    again = f.smooth(method="simulation", num_draws=S)
    assert torch.equal(again, mean) and torch.equal(f.last_smoothed.indices, rec.indices)
    assert torch.equal(f.last_smoothed.trajectories, rec.trajectories) and torch.equal(f.last_smoothed.covariance, rec.covariance)
    f.smooth()  # the other methods' records are what they were
    assert set(vars(f.last_smoothed)) == {"covariance", "unique", "lag"}
    f.smooth(method="marginal")
    assert set(vars(f.last_smoothed)) == {"covariance", "ess", "weights", "lag", "method"}
    f.record_history = False


def test_run_filter_returns_the_simulation_record():
    """``evaluation.run_filter(smooth_method="simulation", smooth_draws=16, return_belief=True)`` returns what the direct call
    does on the same noise stream."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N, M, T, S = 4, 300, 8, 16
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorParticleFilter", N, M, T, dev)
    f.noise = mmf.NoiseSource(7)
    est, rec = evaluation.run_filter(f, traj, smooth_method="simulation", smooth_draws=S, return_belief=True)
    assert f.record_history is False and f.record_belief is False  # switched back
    assert est.shape == (T, N, d) and rec.method == "simulation" and rec.num_draws == S and rec.trajectories.shape == (T, N, S, d)
    f.noise = mmf.NoiseSource(7)
    f.record_history = True
    f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
    f.forward_loop(observations=obs, controls=ctrl)
    direct = f.smooth(method="simulation", num_draws=S)
    f.record_history = False
    assert torch.equal(est, direct) and torch.equal(rec.indices, f.last_smoothed.indices)
    assert torch.equal(rec.trajectories, f.last_smoothed.trajectories) and torch.equal(rec.covariance, f.last_smoothed.covariance)
    f.noise = mmf.NoiseSource(7)
    only = evaluation.run_filter(f, traj, smooth_lag=None, smooth_method="simulation", smooth_draws=S)
    assert torch.is_tensor(only) and torch.equal(only, est)
    with pytest.raises(ValueError, match="fixed-lag"):
        evaluation.run_filter(f, traj, smooth_lag=2, smooth_method="simulation")
    assert f.record_history is False
    f.noise = mmf.NoiseSource(7)
    with pytest.raises(ValueError, match="smooth_draws"):  # (as smooth() refuses num_draws with another method)
        evaluation.run_filter(f, traj, smooth_method="marginal", smooth_draws=S)
    f.noise = mmf.CounterNoise(7)
    with pytest.raises(ValueError, match="CounterNoise"):
        evaluation.run_filter(f, traj, smooth_method="simulation", smooth_draws=S)
    assert f.record_history is False


# ------------------------------------------------------------------------------------------ linear-Gaussian known answer
def test_simulation_is_no_worse_than_ancestry_against_the_exact_smoother():
    """The random-walk states of ``synthetic.make_trajectories`` (x' = x + 0.05 eps) observed through ``z = x + 0.3 eps``,
    filtered with the model that generated them (user models: the step-by-step history and the generic prediction path):
    N = 8, M = 512, T = 40, 256 draws.  Over steps 0 .. T - 10 and all trajectories the RMSE of the simulation mean to the
    exact RTS smoother is not larger than the ancestry smoother's on the same run.  A direction, no ratio; the fp64
    restatement of the sampler on the same history is held to it first."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    dev = sc.dev()
    d, N, M, T, S = 3, 8, 512, 40, 256
    q, r = 0.05, 0.3
    truth = synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=23)["states"]
    z = truth[1:] + r * torch.randn((T, N, d), generator=torch.Generator().manual_seed(29))
    dyn, meas = sc.linear_gaussian_models(d, q, r, dev)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.record_history = True
    f.noise = mmf.NoiseSource(31)
    f.initialize_beliefs(mean=truth[0].to(dev), covariance=(0.1 * torch.eye(d))[None].expand(N, d, d).to(dev))
    est = f.forward_loop(observations={"z": z.to(dev)}, controls=torch.zeros((T, N, 7), device=dev))
    h = f.last_history
    ancestry = f.smooth()
    u = torch.rand((T, N, S), generator=torch.Generator().manual_seed(37))
    f.noise = mmf.ReplayNoise(uniforms=[u])
    simulation = f.smooth(method="simulation", num_draws=S)
    rec = f.last_smoothed
    C = lambda x: x.detach().cpu().numpy()
    L = C(q * torch.eye(d))
    idx64 = torch.from_numpy(_simulate64(C(h.states), C(h.states[:-1]), C(h.log_likelihoods), C(h.log_weights_in), L, C(u)))
    sim64 = _gather(h.states.cpu(), idx64).double().mean(2)
    exact = torch.from_numpy(sc.rts(z.double().numpy(), truth[0].double().numpy(), 0.1, q, r))
    rmse = lambda x: float((x.double().cpu()[:T - 9] - exact[:T - 9]).pow(2).sum(-1).mean().sqrt())
    print(f"RMSE to the exact smoother over steps 0 .. T-10: simulation {rmse(simulation):.5f} (fp64 restatement "
          f"{rmse(sim64):.5f}), ancestry {rmse(ancestry):.5f}, filter {rmse(est):.5f}")
    assert bool((rec.indices >= 0).all()) and bool(torch.isfinite(simulation).all()) and bool(torch.isfinite(rec.covariance).all())
    assert rmse(sim64) <= rmse(ancestry), "the fp64 restatement itself is worse than the ancestry smoother"
    assert rmse(simulation) <= rmse(ancestry)


def test_state_dependent_noise_is_refused():
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    d, N, M, T = 2, 2, 64, 3
    dyn, meas = sc.linear_gaussian_models(d, 0.05, 0.3, dev, state_dependent=True)
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=M)
    f.eval()
    f.record_history = True
    f.noise = mmf.NoiseSource(5)
    f.initialize_beliefs(mean=torch.zeros((N, d), device=dev), covariance=(0.1 * torch.eye(d))[None].expand(N, d, d).to(dev))
    f.forward_loop(observations={"z": torch.zeros((T, N, d), device=dev)}, controls=torch.zeros((T, N, 7), device=dev))
    with pytest.raises(ValueError, match="state-dependent"):
        f.smooth(method="simulation", num_draws=4)

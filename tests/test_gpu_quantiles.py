"""Particle-posterior quantiles on the GPU: ``mmf_pf_quantiles`` (``csrc/pf_quantiles.hip``) against the fp64 rule of
``tests/_quantile_cases.py`` on its whole family, its bit-for-bit identities (two calls, a row alone, equal weights against
``np.sort``), properties that need no reference, the limit ``M = 16384``, and ``ParticleFilter.belief_quantiles`` /
``evaluation.run_filter(return_quantiles=)`` end to end on a small real filter.

The rule: a quantile is a live particle's own value ``v`` with ``F(v) >= p - eps`` and ``F-(v) < p + eps``; a cdf is within
``eps`` of ``F(query)``; ``eps = (M + 16) 2^-24`` (derived in ``_quantile_cases``).  Every worst distance is printed before the
next case is asserted."""

import numpy as np
import pytest
import torch

import _quantile_cases as qc
import _smooth_cases as sc
from _summary_gpu import N, _case_of, _filter_run, _Guarded, _same_bits

pytestmark = pytest.mark.gpu


def _run(case, with_query=True, rows=None):
    """``_abi.pf_quantiles`` on a case (or on ``rows`` of it) with both outputs between guard rows -> (quantiles (R, Q, d) or
    None, cdf (R, d) or None) as device tensors.  Without probabilities the quantile buffer is handed over all the same, as
    an ``(R, 0, d)`` view of real memory, and must come back untouched."""
    from multimodalfilter_amd import _abi

    dev = sc.dev()
    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    X, la, lb, qy = (sc.to_device(pick(case[k])) for k in ("states", "log_a", "log_b", "query"))
    R, M, d = X.shape
    Q = len(case["probs"])
    quant = _Guarded(R, (max(Q, 1), d), dev)
    cdf = _Guarded(R, (d,), dev)
    _abi.pf_quantiles(X, la, lb, case["probs"], quant.view[:, :Q], qy if with_query else None, cdf.view if with_query else None)
    torch.cuda.synchronize()
    assert quant.guards_intact() and cdf.guards_intact(), f"a guard row was written (M={M} d={d} R={R} Q={Q})"
    if Q == 0:
        assert quant.untouched(), "Q == 0 wrote quantiles"
    if not with_query:
        assert cdf.untouched()
    return (quant.view.clone() if Q else None), (cdf.view.clone() if with_query else None)


# ------------------------------------------------------------------------------------------ 1. the kernel against the rule
@pytest.mark.parametrize("M", qc.MS)
def test_kernel_holds_the_rule_on_the_family(M):
    for M_, d, R, variant in qc.family():
        if M_ != M:
            continue
        case = qc.make_case(M, d, R, variant)
        quant, cdf = _run(case)
        wq, wc = qc.check(case, N(quant), N(cdf))
        print(f"M={M} d={d} R={R} {variant}: worst F-distance {wq:.3e}, worst cdf error {wc:.3e} (eps {qc.eps(M):.3e})")
        if case["probs"] and variant in ("plain", "dead_row"):  # the query changes no quantile
            alone, none = _run(case, with_query=False)
            assert none is None and _same_bits(alone, quant)


@pytest.mark.parametrize("M", [512, 513, 1024, 1025])
def test_kernel_holds_the_rule_where_the_workgroup_changes(M):
    """512 | 513: the last one-wave sort and the first of 256 threads; 1024 | 1025: the next padded size."""
    for d, variant in ((1, "plain"), (3, "dead_row"), (4, "only_b")):
        case = qc.make_case(M, d, 5, variant)
        quant, cdf = _run(case)
        wq, wc = qc.check(case, N(quant), N(cdf))
        print(f"M={M} d={d} {variant}: worst F-distance {wq:.3e}, worst cdf error {wc:.3e} (eps {qc.eps(M):.3e})")


def test_kernel_at_the_particle_limit():
    case = qc.make_case(qc.MAX_M, 1, 1, "plain")
    quant, cdf = _run(case)
    wq, wc = qc.check(case, N(quant), N(cdf))
    print(f"M={qc.MAX_M}: worst F-distance {wq:.3e}, worst cdf error {wc:.3e} (eps {qc.eps(qc.MAX_M):.3e})")
    case = qc.exact_case(qc.MAX_M, 1, 1, dead=True)
    quant, cdf = _run(case)
    want_q, want_c = qc.exact_expected(case)
    assert bool((N(quant) == want_q).all()) and bool((N(cdf) == want_c).all())


# ------------------------------------------------------------------------------------------ 2. bit-for-bit identities
@pytest.mark.parametrize("M", [1, 65, 257, 512, 513, 1000, 4096, 4097])  # (512 | 513: one wave | 256 threads; 4097: 32 slots)
def test_two_calls_and_a_row_alone_give_the_same_bits(M):
    for d, variant in ((1, "plain"), (3, "dead_row"), (4, "plain")):
        case = qc.make_case(M, d, 5, variant)
        quant, cdf = _run(case)
        again_q, again_c = _run(case)
        assert _same_bits(quant, again_q) and _same_bits(cdf, again_c)
        for r in range(5):
            q1, c1 = _run(case, rows=slice(r, r + 1))
            assert _same_bits(q1, quant[r:r + 1]) and _same_bits(c1, cdf[r:r + 1]), (M, d, variant, r)


@pytest.mark.parametrize("M,dead", qc.EXACT + ((512, True), (513, True), (4096, False), (4096, True), (4097, True)))
def test_equal_weights_are_a_rank_of_np_sort(M, dead):
    for d, R in ((1, 1), (3, 5), (4, 2)):
        case = qc.exact_case(M, d, R, dead)
        quant, cdf = _run(case)
        want_q, want_c = qc.exact_expected(case)
        assert bool((N(quant) == want_q).all()), (M, d, R, dead)
        assert bool((N(cdf) == want_c).all()), (M, d, R, dead)


# ------------------------------------------------------------------------------------------ 3. properties without a reference
@pytest.mark.parametrize("M", [2, 64, 255, 1000, 4096])
def test_properties_that_need_no_reference(M):
    """Non-decreasing in ``p``; ``p = 0`` / ``p = 1`` bracket every particle that surely carries integer weight (``w >= 2^-23``
    of the heaviest: ``q >= 1`` whatever the last bits of ``expf``); the cdf at the ``p`` quantile is at least ``p - eps``."""
    from multimodalfilter_amd import _abi

    d, R = 3, 5
    case = qc.make_case(M, d, R, "plain")
    quant, _ = _run(case)
    q = N(quant)
    assert bool((q[:, 1:] >= q[:, :-1]).all())
    W = qc.weights64(case)
    for r in range(R):
        sure = W[r] >= 2.0 ** -23
        assert sure.any()
        xs = case["states"][r][sure]
        assert bool((q[r, 0] <= xs.min(0)).all()) and bool((q[r, -1] >= xs.max(0)).all())
    X, la, lb = (sc.to_device(case[k]) for k in ("states", "log_a", "log_b"))
    ps = qc.probs32(case["probs"])
    for i, p in enumerate(ps):
        cdf = torch.full((R, d), float("nan"), device=X.device)
        _abi.pf_quantiles(X, la, lb, (), None, quant[:, i].contiguous(), cdf)
        assert bool((cdf >= p - qc.eps(M)).all()) and bool((cdf <= 1.0).all()), (p, cdf)


# ------------------------------------------------------------------------------------------ 4. through the filter
def test_belief_quantiles_on_a_real_filter():
    """``of="filtered"`` and, after the marginal smoother, ``of="smoothed"`` are held to the rule on the CPU from the records'
    own tensors; after backward simulation the draws' quantiles are a rank of ``torch.sort``.  Nothing else moves: the
    estimates, the history, the smoothed record and the noise stream are what they are without the calls."""
    from multimodalfilter_amd.utils import ReplayNoise

    f, forward, traj, (T, N_, M, d) = _filter_run("DoorParticleFilter", 64)
    est = forward().clone()
    h = f.last_history
    truth = traj["states"][1:]
    before = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in", "ancestors") if getattr(h, k) is not None}
    probs = (0.025, 0.5, 0.975)
    assert f.last_quantiles is None
    quant = f.belief_quantiles(probs, of="filtered", truth=truth)
    rec = f.last_quantiles
    assert set(vars(rec)) == {"probs", "quantiles", "of", "pit"} and rec.of == "filtered" and rec.probs == probs
    assert rec.quantiles is quant and quant.shape == (T, N_, 3, d) and rec.pit.shape == (T, N_, d)
    case = _case_of(h.states, h.log_weights_in, h.log_likelihoods, truth, point="query", probs=probs)
    wq, wc = qc.check(case, N(quant).reshape(T * N_, 3, d), N(rec.pit).reshape(T * N_, d))
    print(f"filtered: worst F-distance {wq:.3e}, worst pit error {wc:.3e} (eps {qc.eps(M):.3e})")
    assert bool(((rec.pit >= 0) & (rec.pit <= 1)).all())
    plain = f.belief_quantiles(probs)  # without a truth: the same quantiles, no pit
    assert torch.equal(plain, quant) and not hasattr(f.last_quantiles, "pit")
    after = f.noise.uniform((4, 5), like=h.states).clone()  # where the noise stream stands after the calls ...
    assert torch.equal(forward(), est)
    assert torch.equal(f.noise.uniform((4, 5), like=h.states), after)  # ... is where it stands without them
    f.last_history = h
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k

    # the marginal smoother's weights over the history's states
    mean = f.smooth(method="marginal").clone()
    s = f.last_smoothed
    weights = s.weights.clone()
    quant = f.belief_quantiles(probs, of="smoothed", truth=truth)
    assert f.last_smoothed is s and torch.equal(s.weights, weights) and f.last_quantiles.of == "smoothed"
    case = _case_of(h.states, torch.log(weights), None, truth, point="query", probs=probs)
    wq, wc = qc.check(case, N(quant).reshape(T * N_, 3, d), N(f.last_quantiles.pit).reshape(T * N_, d))
    print(f"marginal: worst F-distance {wq:.3e}, worst pit error {wc:.3e} (eps {qc.eps(M):.3e})")
    assert torch.equal(f.smooth(method="marginal"), mean)

    # backward simulation: 16 equally weighted draws per step
    S = 16
    f.noise = ReplayNoise(uniforms=[torch.rand((T, N_, S), generator=torch.Generator().manual_seed(5))])
    f.smooth(method="simulation", num_draws=S)
    s = f.last_smoothed
    assert bool(torch.isfinite(s.trajectories).all())
    quant = f.belief_quantiles(probs, of="smoothed")
    ordered = torch.sort(s.trajectories, dim=2).values  # (T, N, S, d)
    for i, p in enumerate(qc.probs32(probs)):
        assert bool((quant[:, :, i] == ordered[:, :, max(1, int(np.ceil(p * S))) - 1]).all()), p
    assert f.last_smoothed is s and f.last_history is h
    for k, x in before.items():
        assert torch.equal(getattr(h, k), x), k
    for method in ("ancestry", "map"):
        f.smooth(method=method)
        kept = f.last_quantiles
        with pytest.raises(ValueError, match="of='smoothed'"):
            f.belief_quantiles(probs, of="smoothed")
        assert f.last_quantiles is kept


def test_run_filter_returns_the_quantile_record_last():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    dev = sc.dev()
    N_, M, T = 3, 64, 6
    f, d, traj, obs, ctrl, cov = sc.small_filter("DoorParticleFilter", N_, M, T, dev)
    f.noise = mmf.CounterNoise(7)
    plain = evaluation.run_filter(f, traj)
    f.noise = mmf.CounterNoise(7)
    est, rec = evaluation.run_filter(f, traj, return_quantiles=(0.025, 0.5, 0.975))
    assert f.record_history is False  # put back
    assert torch.equal(est, plain)
    assert rec is f.last_quantiles and rec.of == "filtered" and rec.quantiles.shape == (T, N_, 3, d)
    assert rec.pit.shape == (T, N_, d) and bool(((rec.pit >= 0) & (rec.pit <= 1)).all())
    cover = evaluation.interval_coverage(rec.quantiles[:, :, 0], rec.quantiles[:, :, 2], traj["states"][1:], start=0)
    assert cover.shape == (N_, d) and bool(((cover >= 0) & (cover <= 1)).all())
    hist = evaluation.pit_histogram(rec.pit, bins=5, start=0)
    assert hist.shape == (d, 5) and torch.allclose(hist.sum(1), torch.ones(d, device=hist.device), atol=1e-6)
    f.noise = mmf.CounterNoise(7)
    out = evaluation.run_filter(f, traj, return_belief=True, smooth_method="marginal", return_quantiles=(0.5,))
    assert len(out) == 3 and out[2] is f.last_quantiles and out[2].of == "smoothed" and out[1] is f.last_smoothed
    assert out[2].quantiles.shape == (T, N_, 1, d) and f.record_history is False and f.record_belief is False

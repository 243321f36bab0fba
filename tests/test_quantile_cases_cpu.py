"""CPU-side checks of the particle-posterior quantiles (``include/mmf.h``: ``MmfPfQuantilesArgs`` / ``mmf_pf_quantiles``;
``ParticleFilter.belief_quantiles``; ``evaluation.interval_coverage`` / ``pit_histogram`` / ``run_filter(return_quantiles=)``):
the references of ``_quantile_cases`` against their own rule on the whole family, the exact cases against ``np.sort``, the
entry point's refusals on the host before any HIP call, the LDS size query, the Python refusals before any device work, and
the evaluation helpers against hand-computed arrays."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _quantile_cases as qc
import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2
_POINTERS = ("states", "log_a", "log_b", "query", "quantiles", "cdf")


@pytest.fixture(autouse=True, scope="module")
def _the_entry_these_tests_describe():
    """The family, the references and the rule of this module define ONE entry point: without the binding and the method
    there is nothing they are the reference of."""
    from multimodalfilter_amd import _abi, evaluation, filters

    assert hasattr(_abi, "MmfPfQuantilesArgs") and callable(getattr(_abi, "pf_quantiles", None))
    assert callable(getattr(filters.ParticleFilter, "belief_quantiles", None))
    assert callable(getattr(evaluation, "interval_coverage", None)) and callable(getattr(evaluation, "pit_histogram", None))


# ------------------------------------------------------------------------------------------ 1. the references and the rule
@pytest.mark.parametrize("M", qc.MS)
def test_the_references_satisfy_the_rule_on_the_family(M):
    """The fp64 pick to ``REF_EPS``; the host restatement of the kernel's integer CDF (numpy's fp32 ``exp``) to the derived
    ``eps = (M + 16) 2^-24`` -- every case is held to the band, none is skipped."""
    worst = [0.0, 0.0, 0.0, 0.0]
    differ = total = 0
    for M_, d, R, variant in qc.family():
        if M_ != M:
            continue
        case = qc.make_case(M, d, R, variant)
        quant, cdf = qc.reference(case)
        a = qc.check(case, quant if case["probs"] else None, cdf, tol=qc.REF_EPS)
        fq, fc = qc.fixed_point(case)
        b = qc.check(case, fq if case["probs"] else None, fc)
        worst = [max(x, y) for x, y in zip(worst, a + b)]
        both = ~np.isnan(quant)
        differ += int(np.count_nonzero(quant[both] != fq[both]))
        total += int(both.sum())
    print(f"M={M}: fp64 pick {worst[0]:.3e} / {worst[1]:.3e}; integer CDF {worst[2]:.3e} / {worst[3]:.3e} (eps {qc.eps(M):.3e}); "
          f"{differ} of {total} row-quantiles differ from the fp64 pick")
    assert total > 0


@pytest.mark.parametrize("M,dead", qc.EXACT)
def test_equal_weights_are_a_rank_of_np_sort(M, dead):
    for d, R in ((1, 1), (3, 5)):
        case = qc.exact_case(M, d, R, dead)
        want_q, want_c = qc.exact_expected(case)
        got_q, got_c = qc.fixed_point(case)
        assert bool((got_q == want_q).all()) and bool((got_c == want_c).all())
        qc.check(case, want_q, want_c)


def test_float32_probabilities_set_the_rank():
    """``float32(0.025) * 1000 > 25``: the kernel is handed floats, and the rank follows the float."""
    assert math.ceil(qc.probs32((0.025,))[0] * 1000) == 26 and math.ceil(qc.probs32((0.5,))[0] * 1000) == 500


# ------------------------------------------------------------------------------------------ 2. the entry point's host checks
def _args(alias=None, probs=(0.25, 0.75), **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfQuantilesArgs, _POINTERS, **{**dict(R=2, M=2, d=2, Q=len(probs)), **over})
    for i, p in enumerate(probs):
        a.probs[i] = p
    return sc.alias_host_args(a, _POINTERS, alias)


def test_quantiles_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    lib = sc.lib()
    call = lambda alias=None, probs=(0.25, 0.75), **over: lib.mmf_pf_quantiles(ctypes.byref(_args(alias, probs, **over)), None)
    assert lib.mmf_pf_quantiles(None, None) == EINVAL
    assert call(states=None) == EINVAL
    assert call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(M=0) == EINVAL and call(M=-2) == EINVAL and call(R=-1) == EINVAL
    assert call(Q=17) == EINVAL and call(Q=-1) == EINVAL
    for bad in (-0.001, 1.001, math.nan, math.inf):
        assert call(probs=(0.5, bad)) == EINVAL, bad
    assert call(probs=(), query=None, cdf=None) == EINVAL        # nothing requested
    assert call(quantiles=None) == EINVAL                         # Q > 0 without an output
    assert call(query=None) == EINVAL and call(cdf=None) == EINVAL  # exactly one of the pair
    for out, target in (("quantiles", "states"), ("quantiles", "log_a"), ("quantiles", "log_b"), ("quantiles", "query"),
                        ("cdf", "states"), ("cdf", "log_a"), ("cdf", "log_b"), ("cdf", "query"), ("cdf", "quantiles")):
        assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"cdf": ("states", 28)}) == EINVAL and call({"quantiles": ("cdf", 12)}) == EINVAL  # partly on top
    assert call(M=16385) == ETOOLARGE and call(M=1 << 20) == ETOOLARGE
    assert call(R=1 << 30, d=4) == ETOOLARGE                       # R * d beyond a 32-bit grid
    assert call(M=16385, states=None) == EINVAL                    # an invalid call is invalid whatever its size
    # successful no-ops: no rows
    assert call(R=0) == 0 and call(R=0, M=16384, d=4) == 0 and call(R=0, M=16385) == ETOOLARGE
    assert call(R=0, log_a=None, log_b=None) == 0 and call(R=0, query=None, cdf=None) == 0
    assert call(R=0, probs=(), quantiles=None) == 0 and call(R=0, probs=(0.0, 1.0)) == 0
    assert call({"cdf": ("states", 0)}, R=0) == 0                  # (empty ranges overlap nothing)


def test_lds_bytes_is_monotone_and_fits_a_cu():
    from multimodalfilter_amd import _abi

    sc.lib()
    sizes = [_abi.pf_quantiles_lds_bytes(M) for M in range(1, 16385)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0
    assert all(s >= 8 * M for M, s in zip(range(1, 16385), sizes))  # 8 B per slot
    assert sizes[-1] <= 160 << 10
    assert _abi.QUANTILES_MAX == 16 and _abi.QUANTILES_MAX_M == 16384 == qc.MAX_M


def test_the_binding_refuses_cpu_tensors():
    import torch

    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_quantiles(x, None, None, (0.5,), torch.zeros((2, 1, 3)))
    with pytest.raises(_abi.MmfError):
        _abi.pf_quantiles(x, None, None, tuple([0.5] * 17), None)


# ------------------------------------------------------------------------------------------ 3. the Python refusals
def test_belief_quantiles_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import base

    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_quantiles is None
    with pytest.raises(ValueError, match="history"):
        pf.belief_quantiles((0.5,))
    with pytest.raises(ValueError, match="smoothed record"):
        pf.belief_quantiles((0.5,), of="smoothed")
    with pytest.raises(ValueError, match="of must be"):
        pf.belief_quantiles((0.5,), of="predicted")
    assert pf.last_quantiles is None

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    before = (f.last_history, f.last_smoothed)
    f.last_smoothed = base.belief_record(covariance=torch.zeros((T, N, d, d)), unique=torch.zeros((T, N), dtype=torch.int32), lag=None)
    with pytest.raises(ValueError, match="no per-step weights"):
        f.belief_quantiles((0.5,), of="smoothed")
    f.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_quantiles((0.5,), of="smoothed")
    f.last_smoothed = before[1]
    for bad in ((), [0.5] * 17, (0.5, 1.5), (-0.1,), (math.nan,), ("0.5",), (None,), (True,), 0.5, None):
        with pytest.raises(ValueError, match="probs"):
            f.belief_quantiles(bad)
    for bad in (torch.zeros((T, N)), torch.zeros((T + 1, N, d)), torch.zeros((T, N, d + 1)), np.zeros((T, N, d))):
        with pytest.raises(ValueError, match="truth"):
            f.belief_quantiles((0.5,), truth=bad)
    big = base.history_record(states=torch.zeros((1, 1, qc.MAX_M + 1, 1)), log_likelihoods=torch.zeros((1, 1, qc.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="16384"):
        f.belief_quantiles((0.5,))
    f.last_history = before[0]
    assert f.last_quantiles is None and f.last_history is before[0] and f.last_smoothed is before[1]
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    from multimodalfilter_amd import _abi

    with pytest.raises(_abi.MmfError):
        f.belief_quantiles((0.025, 0.5, 0.975), truth=torch.zeros((T, N, d)))
    assert f.last_quantiles is None


# ------------------------------------------------------------------------------------------ 4. the evaluation helpers
def test_interval_coverage_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import evaluation

    lower = torch.tensor([[[0.0, 0.0]], [[0.0, 0.0]], [[0.0, 0.0]], [[0.0, math.nan]]])     # (T = 4, N = 1, d = 2)
    upper = torch.tensor([[[1.0, 1.0]], [[1.0, 1.0]], [[1.0, 1.0]], [[1.0, 1.0]]])
    true = torch.tensor([[[0.5, 2.0]], [[1.0, 0.5]], [[-0.1, 0.0]], [[0.2, 0.5]]])           # ends are inside
    got = evaluation.interval_coverage(lower, upper, true, start=0)
    assert got.shape == (1, 2) and torch.equal(got, torch.tensor([[0.75, 0.5]]))
    assert torch.equal(evaluation.interval_coverage(lower, upper, true, start=2), torch.tensor([[0.5, 0.5]]))
    assert inspect.signature(evaluation.interval_coverage).parameters["start"].default == evaluation.START_TRUNCATION


def test_pit_histogram_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import evaluation

    pit = torch.tensor([[[0.0, 1.0]], [[0.05, 1.0]], [[0.1, 0.999]], [[0.95, 0.5]], [[1.0, math.nan]]])  # (T = 5, N = 1, d = 2)
    got = evaluation.pit_histogram(pit, bins=10, start=0)
    want = torch.zeros((2, 10))
    want[0, 0], want[0, 1], want[0, 9] = 2 / 5, 1 / 5, 2 / 5      # 0, 0.05 | 0.1 | 0.95, 1.0
    want[1, 9], want[1, 5] = 3 / 4, 1 / 4                         # 1, 1, 0.999 | 0.5; the NaN is left out
    assert got.shape == (2, 10) and torch.allclose(got, want, atol=1e-7, rtol=0)
    assert torch.allclose(got.sum(dim=1), torch.ones(2), atol=1e-6, rtol=0)
    got = evaluation.pit_histogram(pit, bins=2, start=3)
    assert torch.allclose(got, torch.tensor([[0.0, 1.0], [0.0, 1.0]]))  # 0.95, 1.0 | 0.5 sits in the upper half
    sig = inspect.signature(evaluation.pit_histogram).parameters
    assert sig["bins"].default == 10 and sig["start"].default == evaluation.START_TRUNCATION


def test_run_filter_switch_and_refusals():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert sig["return_quantiles"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_quantiles"].default is None
    assert sig["smooth_method"].kind is inspect.Parameter.KEYWORD_ONLY and sig["smooth_method"].default == "ancestry"
    kf = mmf.door_models.DoorKalmanFilter().eval()
    with pytest.raises(ValueError, match="return_quantiles"):
        evaluation.run_filter(kf, {}, return_quantiles=(0.5,))
    pf = mmf.door_models.DoorParticleFilter().eval()
    for kw in (dict(smooth_method="map"), dict(smooth_lag=3), dict(smooth_lag=None), dict(smooth_method="ancestry", smooth_lag=0)):
        with pytest.raises(ValueError, match="return_quantiles"):
            evaluation.run_filter(pf, {}, return_quantiles=(0.5,), **kw)
    assert pf.record_history is False and pf.last_quantiles is None

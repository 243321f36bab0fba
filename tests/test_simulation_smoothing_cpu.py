"""CPU-side checks of backward-simulation particle smoothing's boundary (``include/mmf.h``: ``MmfPfSmoothSimulateArgs`` /
``mmf_pf_smooth_simulate``): the entry point refuses bad arguments on the host, before any HIP call; the Python switches
refuse what they cannot do and keep what they did before.  (The struct's layout: ``test_abi_cpu.py``, for every struct of the
binding.)"""
import ctypes
import inspect
import os

import pytest

import _smooth_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2


def test_the_header_section_says_what_it_stands_in_for():
    with open(os.path.join(ROOT, "include", "mmf.h")) as f:
        header = f.read()
    start = header.index("backward-simulation particle smoothing")
    section = header[header.rindex("/* ----", 0, start):header.index("} MmfPfSmoothSimulateArgs;")]
    assert header.rindex("/* ----", 0, start) > header.index("} MmfPfSmoothMarginalArgs;")  # a section of its own, after the marginal one
    assert "torchfilter" in section and "additive to ABI 42" in section


_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "uniforms", "indices", "trajectories",
             "mean", "cov")


def _args(**over):
    from multimodalfilter_amd import _abi

    return sc.host_args(_abi.MmfPfSmoothSimulateArgs, _POINTERS, **{**dict(T=4, N=2, M=64, d=3, S=8), **over})


def test_simulate_refuses_bad_arguments_on_the_host():
    """Nulls, negative sizes and ``M``, ``S`` or ``d`` below 1 -> ``MMF_EINVAL``; ``d``, ``M``, ``N`` or ``S`` beyond the limits
    -> ``MMF_ETOOLARGE``; no trajectories or no steps -> a successful no-op.  All decided before any HIP call: the pointers
    are host memory and never dereferenced, and the stream is null."""
    lib = sc.lib()
    call = lambda **over: lib.mmf_pf_smooth_simulate(ctypes.byref(_args(**over)), None)
    assert lib.mmf_pf_smooth_simulate(None, None) == EINVAL
    for field in ("states_steps", "loglik_steps", "scale_tril", "uniforms", "indices", "trajectories", "mean", "pred_steps"):
        assert call(**{field: None}) == EINVAL, field
        assert call(N=0, **{field: None}) == EINVAL, field  # (T = 4: invalid also where there is nothing to do)
    assert call(d=0) == EINVAL and call(d=-1) == EINVAL and call(d=5) == ETOOLARGE
    assert call(M=0) == EINVAL and call(M=-3) == EINVAL and call(M=65537) == ETOOLARGE
    assert call(S=0) == EINVAL and call(S=-1) == EINVAL and call(S=65536) == ETOOLARGE
    assert call(T=-1) == EINVAL and call(N=-1) == EINVAL and call(N=65536) == ETOOLARGE
    # an invalid call is invalid whatever its size
    assert call(d=5, states_steps=None) == EINVAL and call(M=65537, S=0) == EINVAL and call(S=65536, uniforms=None) == EINVAL
    assert call(N=0) == 0 and call(T=0) == 0
    assert call(N=0, M=65536, d=4, S=65535) == 0 and call(N=0, M=65537) == ETOOLARGE  # (the limits hold for the no-ops too)
    assert call(T=0, S=65536) == ETOOLARGE
    # the optional ones; without a second step there is no transition, so no predictions are needed
    assert call(N=0, logw_in_steps=None, cov=None) == 0
    assert call(T=0, pred_steps=None) == 0 and call(T=1, N=0, pred_steps=None) == 0
    assert call(T=2, N=0, pred_steps=None) == EINVAL


def test_smooth_checks_method_lag_and_draws_before_anything_else():
    import multimodalfilter_amd as mmf

    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.record_history = True
    params = inspect.signature(pf.smooth).parameters
    assert params["method"].kind is inspect.Parameter.KEYWORD_ONLY and params["method"].default == "ancestry"
    assert params["num_draws"].kind is inspect.Parameter.KEYWORD_ONLY and params["num_draws"].default == 64
    assert list(params) == ["lag", "method", "num_draws"] and params["lag"].default is None
    with pytest.raises(ValueError, match="fixed-lag"):
        pf.smooth(lag=2, method="simulation")
    with pytest.raises(ValueError, match="fixed-lag"):
        pf.smooth(0, method="simulation")
    for bad in (0, -3, 2.0, "8", None, True):
        with pytest.raises(ValueError, match="num_draws"):
            pf.smooth(method="simulation", num_draws=bad)
    with pytest.raises(ValueError, match="num_draws"):
        pf.smooth(method="marginal", num_draws=8)
    with pytest.raises(ValueError, match="num_draws"):
        pf.smooth(num_draws=64)  # (the default's value, passed: still another method's argument)
    with pytest.raises(ValueError, match="bogus"):
        pf.smooth(method="bogus")
    with pytest.raises(ValueError, match="fixed-lag"):  # the two existing methods: as before
        pf.smooth(lag=2, method="marginal")
    for kw in ({}, {"method": "marginal"}, {"method": "simulation"}, {"method": "simulation", "num_draws": 16}):
        with pytest.raises(AssertionError, match="history"):  # the old assertion, for every method
            pf.smooth(**kw)
    assert pf.last_smoothed is None


def test_run_filter_smooth_draws_is_keyword_only_and_defaults_to_64():
    from multimodalfilter_amd import evaluation

    params = inspect.signature(evaluation.run_filter).parameters
    p = params["smooth_draws"]
    assert p.default == 64 and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert params["smooth_method"].default == "ancestry" and params["smooth_lag"].default is False  # (unchanged)


def test_run_filter_refuses_smooth_draws_with_another_method_before_it_runs():
    from multimodalfilter_amd import evaluation

    for kw in ({"smooth_method": "marginal"}, {"smooth_lag": 3}, {}):
        with pytest.raises(ValueError, match="smooth_draws"):
            evaluation.run_filter(None, None, smooth_draws=16, **kw)  # (neither the filter nor the data is touched)


def test_counter_noise_is_refused_by_name_before_any_prediction():
    """``CounterNoise`` draws one uniform per trajectory: the simulation method says so itself, before it reads the history."""
    from types import SimpleNamespace

    import torch

    import multimodalfilter_amd as mmf

    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.noise = mmf.CounterNoise(3)
    pf.last_history = SimpleNamespace(states=torch.zeros((2, 1, 4, 3)))
    with pytest.raises(ValueError, match="CounterNoise"):
        pf.smooth(method="simulation", num_draws=4)
    assert pf.last_smoothed is None

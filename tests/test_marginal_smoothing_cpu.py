"""CPU-side checks of marginal particle smoothing's boundary (``include/mmf.h``: ``MmfPfSmoothMarginalArgs`` /
``mmf_pf_smooth_marginal``): the entry point refuses bad arguments on the host, before any HIP call; the Python switches
refuse what they cannot do and keep what they did before.  (The struct's layout: ``test_abi_cpu.py``, for every struct of the
binding.)"""
import ctypes
import inspect

import pytest

import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2

_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "logd", "weights", "mean", "cov", "ess")


def _args(**over):
    from multimodalfilter_amd import _abi

    return sc.host_args(_abi.MmfPfSmoothMarginalArgs, _POINTERS, **{**dict(T=4, N=2, M=64, d=3), **over})


def test_marginal_refuses_bad_arguments_on_the_host():
    """Nulls and negative sizes -> ``MMF_EINVAL``; ``d``, ``M`` or ``N`` beyond the limits -> ``MMF_ETOOLARGE``; no
    trajectories or no steps -> a successful no-op.  All decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    lib = sc.lib()
    call = lambda **over: lib.mmf_pf_smooth_marginal(ctypes.byref(_args(**over)), None)
    assert lib.mmf_pf_smooth_marginal(None, None) == EINVAL
    for field in ("states_steps", "loglik_steps", "scale_tril", "weights", "mean", "pred_steps", "logd"):
        assert call(**{field: None}) == EINVAL, field
    assert call(d=0) == EINVAL and call(d=-1) == EINVAL and call(d=5) == ETOOLARGE
    assert call(M=0) == EINVAL and call(M=-3) == EINVAL and call(M=65537) == ETOOLARGE
    assert call(T=-1) == EINVAL and call(N=-1) == EINVAL and call(N=65536) == ETOOLARGE
    assert call(d=5, states_steps=None) == EINVAL  # an invalid call is invalid whatever its size
    assert call(N=0) == 0 and call(T=0) == 0
    assert call(N=0, M=65536, d=4) == 0 and call(N=0, M=65537) == ETOOLARGE  # (the limits hold for the no-ops too)
    # the optional ones; without a second step there is no transition, so neither predictions nor the workspace are needed
    assert call(N=0, logw_in_steps=None, cov=None, ess=None) == 0
    assert call(T=0, pred_steps=None, logd=None) == 0 and call(T=1, N=0, pred_steps=None, logd=None) == 0
    assert call(T=2, N=0, pred_steps=None) == EINVAL and call(T=2, N=0, logd=None) == EINVAL


def test_smooth_checks_method_and_lag_before_anything_else():
    import multimodalfilter_amd as mmf

    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.record_history = True
    assert inspect.signature(pf.smooth).parameters["method"].kind is inspect.Parameter.KEYWORD_ONLY
    assert inspect.signature(pf.smooth).parameters["method"].default == "ancestry"
    with pytest.raises(ValueError, match="fixed-lag"):
        pf.smooth(lag=2, method="marginal")
    with pytest.raises(ValueError, match="fixed-lag"):
        pf.smooth(0, method="marginal")
    with pytest.raises(ValueError, match="bogus"):
        pf.smooth(method="bogus")
    with pytest.raises(AssertionError, match="history"):  # the old assertion, for both methods
        pf.smooth()
    with pytest.raises(AssertionError, match="history"):
        pf.smooth(method="marginal")
    assert pf.last_smoothed is None


def test_run_filter_smooth_method_is_keyword_only_and_defaults_to_ancestry():
    from multimodalfilter_amd import evaluation

    params = inspect.signature(evaluation.run_filter).parameters
    p = params["smooth_method"]
    assert p.default == "ancestry" and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert params["smooth_lag"].default is False  # (unchanged)

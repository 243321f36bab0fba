"""CPU-side checks of particle smoothing's boundary (``include/mmf.h``: ``MmfPfHistory`` / ``mmf_pf_forward_loop_history``,
``MmfPfSmoothArgs`` / ``mmf_pf_smooth``): the entry points refuse bad arguments on the host, before any HIP call; the
Python switches refuse what they cannot do.  (The structs' layout: ``test_abi_cpu.py``, for every struct of the binding.)"""
import ctypes

import pytest

import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2

_POINTERS = ("states_steps", "loglik_steps", "logw_in_steps", "logw_in0", "indices_steps", "mean", "cov", "unique")


def _smooth_args(**over):
    from multimodalfilter_amd import _abi

    return sc.host_args(_abi.MmfPfSmoothArgs, _POINTERS, **{**dict(T=4, N=2, M=64, d=3, lag=1), **over})


def test_smooth_refuses_bad_arguments_on_the_host():
    """Nulls, a negative lag, d = 5 -> ``MMF_EINVAL``; an ``M`` beyond the LDS plan -> ``MMF_ETOOLARGE``; no trajectories or
    no steps -> a successful no-op.  All decided before any HIP call: the pointers are host memory, never dereferenced."""
    lib = sc.lib()
    call = lambda **over: lib.mmf_pf_smooth(ctypes.byref(_smooth_args(**over)), None)
    assert lib.mmf_pf_smooth(None, None) == EINVAL
    for field in ("states_steps", "loglik_steps", "mean"):
        assert call(**{field: None}) == EINVAL, field
    assert call(lag=-1) == EINVAL
    assert call(d=5) == EINVAL and call(d=0) == EINVAL
    assert call(M=0) == EINVAL and call(T=-1) == EINVAL and call(N=-1) == EINVAL
    too_many = 40000
    assert lib.mmf_pf_smooth_lds_bytes(too_many) > 160 * 1024
    assert call(M=too_many) == ETOOLARGE and call(M=65537) == ETOOLARGE
    assert call(N=0) == 0 and call(T=0) == 0
    assert call(N=0, logw_in_steps=None, logw_in0=None, indices_steps=None, cov=None, unique=None) == 0  # the optional ones


def test_smooth_lds_bytes_is_monotone_and_covers_what_it_holds():
    lib = sc.lib()
    sizes = [lib.mmf_pf_smooth_lds_bytes(M) for M in (1, 2, 37, 64, 300, 1024, 1100, 4096, 20000, 39000, 40000, 65536)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), sizes
    assert sizes[0] < sizes[-1]
    for M in (1, 300, 4096, 39000):  # a weight per particle and a bit per particle
        assert lib.mmf_pf_smooth_lds_bytes(M) >= 4 * M + (M + 7) // 8
    assert lib.mmf_pf_smooth_lds_bytes(39000) <= 160 * 1024


def test_history_loop_refuses_null_arguments_on_the_host():
    """``mmf_pf_forward_loop_history``: null args / history / arrays, and the certificates it relies on
    (``loglik_steps``; ``indices_steps`` with a resampling mode; ``logw_in_steps`` where weights travel)."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    bufs = [(ctypes.c_float * 16)() for _ in range(4)]
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    a, h = _abi.MmfPfLoopArgs(), _abi.MmfPfHistory()
    call = lambda thr=0.0: lib.mmf_pf_forward_loop_history(ctypes.byref(a), ctypes.byref(h), thr, None, None, None)
    assert lib.mmf_pf_forward_loop_history(None, None, 0.0, None, None, None) == EINVAL
    assert lib.mmf_pf_forward_loop_history(ctypes.byref(a), None, 0.0, None, None, None) == EINVAL
    assert call() == EINVAL                      # empty history
    h.states_steps, h.logw_in0 = P[0], P[1]
    assert call() == EINVAL                      # no loglik_steps
    a.loglik_steps = P[2]
    a.resample_mode = 1
    assert call() == EINVAL                      # resampling without indices_steps
    a.indices_steps = P[3]
    assert call(0.5) == EINVAL                   # an ESS threshold carries weights: logw_in_steps is required
    assert call(1.5) == EINVAL and call(-0.5) == EINVAL
    a.resample_mode = 0
    assert call() == EINVAL                      # no resampling: weights travel
    h.logw_in_steps = P[1]
    assert call() == EINVAL                      # ... and the loop's own checks refuse the empty MmfPfLoopArgs (N = 0)


def test_record_history_is_refused_on_a_training_mode_filter_and_smooth_needs_a_history():
    import multimodalfilter_amd as mmf

    pf = mmf.door_models.DoorParticleFilter()
    assert pf.record_history is False and pf.last_history is None and pf.last_smoothed is None
    pf.train()
    with pytest.raises(RuntimeError, match="record_history"):
        pf.record_history = True
    assert pf.record_history is False
    pf.record_history = False  # switching it off is always allowed
    pf.eval()
    pf.record_history = True
    assert pf.record_history is True
    with pytest.raises(AssertionError, match="history"):
        pf.smooth()
    with pytest.raises(AssertionError, match="history"):
        pf.smooth(lag=3)


def test_reserve_accounts_for_the_history(monkeypatch):
    """``4 (d + 3)`` bytes per particle-step on top of what ``reserve`` plans without it (the allocator calls are stubbed:
    the arithmetic needs no device)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, filters

    asked = []
    monkeypatch.setattr(filters, "reserve_memory", lambda dev, nbytes: asked.append(nbytes))
    monkeypatch.setattr(engine, "_image_workspace", lambda *a, **k: None)
    pf = mmf.door_models.DoorParticleFilter().eval()
    T, N, M, d = 300, 256, 4096, pf.state_dim
    without = pf.reserve(steps=T, batch=N, particles=M)
    pf.record_history = True
    with_history = pf.reserve(steps=T, batch=N, particles=M)
    assert asked == [without, with_history]
    assert with_history - without == 4 * (d + 3) * N * M * T == 7549747200  # the 7.5 GB the documents quote


def test_run_filter_keeps_its_signature_by_default():
    import inspect

    from multimodalfilter_amd import evaluation

    p = inspect.signature(evaluation.run_filter).parameters["smooth_lag"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY

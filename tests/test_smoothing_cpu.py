"""CPU-side checks of particle smoothing's boundary (``include/mmf.h``: ``MmfPfHistory`` / ``mmf_pf_forward_loop_history``,
``MmfPfSmoothArgs`` / ``mmf_pf_smooth``): header, binding and exports agree on the two structs; the entry points refuse
bad arguments on the host, before any HIP call; the Python switches refuse what they cannot do."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2


def _lib():
    from multimodalfilter_amd import _abi, build

    build.build()
    return _abi.load()


def test_history_and_smooth_structs_match_the_header_field_by_field(tmp_path):
    """``offsetof`` / ``sizeof`` as gcc lays ``include/mmf.h`` out against ctypes' (the technique of ``test_abi_cpu.py``),
    and the library exports the three new symbols the binding declares."""
    from multimodalfilter_amd import _abi

    lib = _lib()
    for name in ("mmf_pf_forward_loop_history", "mmf_pf_smooth", "mmf_pf_smooth_lds_bytes"):
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert lib.mmf_version() == 42  # purely additive
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    structs = ["MmfPfHistory", "MmfPfSmoothArgs"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {"]
    for name in structs:
        cls = getattr(_abi, name)
        lines.append(f'  printf("{name} size %zu\\n", sizeof({name}));')
        for field, _t in cls._fields_:
            lines.append(f'  printf("{name} {field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    out = subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = {}
    for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines():
        name, field, value = line.split()
        got[(name, field)] = int(value)
    for name in structs:
        cls = getattr(_abi, name)
        assert got[(name, "size")] == ctypes.sizeof(cls), (name, got[(name, "size")], ctypes.sizeof(cls))
        for field, _t in cls._fields_:
            assert got[(name, field)] == getattr(cls, field).offset, (name, field)
        last, last_t = cls._fields_[-1]
        assert getattr(cls, last).offset + ctypes.sizeof(last_t) + 8 > ctypes.sizeof(cls), name  # no hidden C field at the end


def _smooth_args(keep, **over):
    from multimodalfilter_amd import _abi

    bufs = [(ctypes.c_float * 16)() for _ in range(8)]
    keep.append(bufs)
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    a = _abi.MmfPfSmoothArgs()
    a.T, a.N, a.M, a.d, a.lag = 4, 2, 64, 3, 1
    a.states_steps, a.loglik_steps, a.logw_in_steps, a.logw_in0 = P[0], P[1], P[2], P[3]
    a.indices_steps, a.mean, a.cov, a.unique = P[4], P[5], P[6], P[7]
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_smooth_refuses_bad_arguments_on_the_host():
    """Nulls, a negative lag, d = 5 -> ``MMF_EINVAL``; an ``M`` beyond the LDS plan -> ``MMF_ETOOLARGE``; no trajectories or
    no steps -> a successful no-op.  All decided before any HIP call: the pointers are host memory, never dereferenced."""
    lib = _lib()
    keep = []
    call = lambda **over: lib.mmf_pf_smooth(ctypes.byref(_smooth_args(keep, **over)), None)
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
    lib = _lib()
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

    lib = _lib()
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

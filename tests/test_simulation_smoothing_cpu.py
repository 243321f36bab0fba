"""CPU-side checks of backward-simulation particle smoothing's boundary (``include/mmf.h``: ``MmfPfSmoothSimulateArgs`` /
``mmf_pf_smooth_simulate``): header, binding and exports agree on the struct; the entry point refuses bad arguments on the
host, before any HIP call; the Python switches refuse what they cannot do and keep what they did before."""
import ctypes
import inspect
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2


def _lib():
    from multimodalfilter_amd import _abi, build

    build.build()
    return _abi.load()


def test_simulate_struct_matches_the_header_field_by_field(tmp_path):
    """``offsetof`` / ``sizeof`` as gcc lays ``include/mmf.h`` out against ctypes' (the technique of
    ``test_marginal_smoothing_cpu.py``); the library exports the symbol the binding declares and is still ABI 42."""
    from multimodalfilter_amd import _abi, build

    assert "pf_smooth_simulate.hip" in build.SOURCES
    lib = _lib()
    assert "mmf_pf_smooth_simulate" in _abi.SIGNATURES and hasattr(lib, "mmf_pf_smooth_simulate")
    assert callable(_abi.pf_smooth_simulate)
    assert lib.mmf_version() == 42 == _abi.ABI_VERSION  # purely additive
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    name, cls = "MmfPfSmoothSimulateArgs", _abi.MmfPfSmoothSimulateArgs
    assert [f for f, _t in cls._fields_] == ["T", "N", "M", "d", "S", "states_steps", "pred_steps", "loglik_steps", "logw_in_steps",
                                             "scale_tril", "uniforms", "indices", "trajectories", "mean", "cov"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             f'  printf("size %zu\\n", sizeof({name}));']
    for field, _t in cls._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof({name}, {field}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    out = subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict((k, int(v)) for k, v in (line.split() for line in
                                        subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines()))
    assert got["size"] == ctypes.sizeof(cls), (got["size"], ctypes.sizeof(cls))
    for field, _t in cls._fields_:
        assert got[field] == getattr(cls, field).offset, field
    last, last_t = cls._fields_[-1]
    assert getattr(cls, last).offset + ctypes.sizeof(last_t) + 8 > ctypes.sizeof(cls)  # no hidden C field at the end


def test_the_header_section_says_what_it_stands_in_for():
    with open(os.path.join(ROOT, "include", "mmf.h")) as f:
        header = f.read()
    start = header.index("backward-simulation particle smoothing")
    section = header[header.rindex("/* ----", 0, start):header.index("} MmfPfSmoothSimulateArgs;")]
    assert header.rindex("/* ----", 0, start) > header.index("} MmfPfSmoothMarginalArgs;")  # a section of its own, after the marginal one
    assert "torchfilter" in section and "additive to ABI 42" in section


_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "uniforms", "indices", "trajectories",
             "mean", "cov")


def _args(keep, **over):
    from multimodalfilter_amd import _abi

    bufs = [(ctypes.c_float * 16)() for _ in _POINTERS]
    keep.append(bufs)
    a = _abi.MmfPfSmoothSimulateArgs()
    a.T, a.N, a.M, a.d, a.S = 4, 2, 64, 3, 8
    for name, b in zip(_POINTERS, bufs):
        setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_simulate_refuses_bad_arguments_on_the_host():
    """Nulls, negative sizes and ``M``, ``S`` or ``d`` below 1 -> ``MMF_EINVAL``; ``d``, ``M``, ``N`` or ``S`` beyond the limits
    -> ``MMF_ETOOLARGE``; no trajectories or no steps -> a successful no-op.  All decided before any HIP call: the pointers
    are host memory and never dereferenced, and the stream is null."""
    lib = _lib()
    keep = []
    call = lambda **over: lib.mmf_pf_smooth_simulate(ctypes.byref(_args(keep, **over)), None)
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

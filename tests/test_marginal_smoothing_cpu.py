"""CPU-side checks of marginal particle smoothing's boundary (``include/mmf.h``: ``MmfPfSmoothMarginalArgs`` /
``mmf_pf_smooth_marginal``): header, binding and exports agree on the struct; the entry point refuses bad arguments on the
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


def test_marginal_struct_matches_the_header_field_by_field(tmp_path):
    """``offsetof`` / ``sizeof`` as gcc lays ``include/mmf.h`` out against ctypes' (the technique of
    ``test_smoothing_cpu.py``); the library exports the symbol the binding declares and is still ABI 42."""
    from multimodalfilter_amd import _abi

    lib = _lib()
    assert "mmf_pf_smooth_marginal" in _abi.SIGNATURES and hasattr(lib, "mmf_pf_smooth_marginal")
    assert lib.mmf_version() == 42 == _abi.ABI_VERSION  # purely additive
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    name, cls = "MmfPfSmoothMarginalArgs", _abi.MmfPfSmoothMarginalArgs
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


_POINTERS = ("states_steps", "pred_steps", "loglik_steps", "logw_in_steps", "scale_tril", "logd", "weights", "mean", "cov", "ess")


def _args(keep, **over):
    from multimodalfilter_amd import _abi

    bufs = [(ctypes.c_float * 16)() for _ in _POINTERS]
    keep.append(bufs)
    a = _abi.MmfPfSmoothMarginalArgs()
    a.T, a.N, a.M, a.d = 4, 2, 64, 3
    for name, b in zip(_POINTERS, bufs):
        setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
    for k, v in over.items():
        setattr(a, k, v)
    return a


def test_marginal_refuses_bad_arguments_on_the_host():
    """Nulls and negative sizes -> ``MMF_EINVAL``; ``d``, ``M`` or ``N`` beyond the limits -> ``MMF_ETOOLARGE``; no
    trajectories or no steps -> a successful no-op.  All decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    lib = _lib()
    keep = []
    call = lambda **over: lib.mmf_pf_smooth_marginal(ctypes.byref(_args(keep, **over)), None)
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

"""What the kernel-level GPU tests that call the C ABI on guarded buffers share (``test_gpu_kalman_kernels.py``,
``test_gpu_jacobian.py``): the device, the loaded library, an output buffer with sentinel guard rows behind it, the raw C
call and the project's error rule.  Imported by GPU tests only."""
import numpy as np
import pytest
import torch

import _tol
from _kalman_cases import GUARD_ROWS, SENTINEL


def dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X (run with -m gpu on the GPU box)")
    return torch.device("cuda:0")


def abi():
    from multimodalfilter_amd import _abi

    _abi.load()
    return _abi


def bits(t):
    return t.contiguous().view(torch.int32)


class Out:
    """An output buffer of ``lead`` rows of shape ``tail`` followed by ``GUARD_ROWS`` guard rows, all filled with the
    sentinel (``init``: the in/out operand's input)."""

    def __init__(self, lead, tail, init=None):
        self.rows = int(np.prod(lead))
        self.full = torch.full((self.rows + GUARD_ROWS,) + tuple(tail), SENTINEL, device=dev())
        self.t = self.full[:self.rows].view(tuple(lead) + tuple(tail))
        if init is not None:
            self.t.copy_(init)

    def guard_intact(self):
        g = self.full[self.rows:]
        return torch.equal(bits(g), bits(torch.full_like(g, SENTINEL)))

    def untouched(self):
        return torch.equal(bits(self.full), bits(torch.full_like(self.full, SENTINEL)))


def raw(name, *args):
    """The C entry point itself (tensors -> device pointers, None -> null, current stream appended): for the calls the typed
    wrappers cannot express (N = 0, a null gate on the gated entry)."""
    lib = abi()
    conv = [lib.ptr(a, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in args]
    with torch.cuda.device(dev()):
        return getattr(lib.load(), name)(*conv, torch.cuda.current_stream().cuda_stream)


def hold(prefix, group, tag, name, got, truth, yardstick, ceiling=None, dims=None):
    """Print (lines begin with ``prefix``), then assert, ``rel_err(got, fp64) < max(1e-4, 3 rel_err(yardstick, fp64))`` (at
    most ``ceiling``); ``dims``: as ``_tol.rel_err``."""
    assert bool(torch.isfinite(got).all()), (group, tag, name, "not finite")
    err, ref = _tol.rel_err(got, truth, dims), _tol.rel_err(yardstick, truth, dims)
    bar = max(_tol.REL_TOL, 3.0 * ref)
    if ceiling is not None:
        bar = min(bar, ceiling)
    print(f"{prefix} group={group} {tag} what={name} kernel={err:.3e} fp32={ref:.3e} bar={bar:.3e}")
    assert err < bar, (group, tag, name, err, ref)
    return err

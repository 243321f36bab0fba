"""The run-table path of the particle-filter loop where no GPU is needed: which modes take it, how large its workspace is,
and that the binding and ``include/mmf.h`` agree on the new struct and entry points (purely additive: ABI 42 and
``MmfPfLoopArgs`` keep their version and layout)."""
import ctypes
import os
import shutil
import subprocess

import pytest
import torch

from multimodalfilter_amd import _abi, engine, filters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2


def test_plan_takes_plain_systematic_resampling_only():
    plan = _abi.load().mmf_pf_dedup_plan
    assert plan(4096, 3, 1, 0.0, 0) == 1 and plan(4096, 2, 1, 1.0, 0) == 1 and plan(64, 3, 1, 0.0, 1) == 1
    assert plan(4096, 3, 0, 0.0, 0) == 0          # no resampling
    assert plan(4096, 3, 2, 0.0, 0) == 0          # multinomial
    assert plan(4096, 3, 1, 0.5, 0) == 0          # soft
    assert plan(300, 3, 1, 0.0, 0) == 0           # M % 64
    assert plan(4096, 1, 1, 0.0, 0) == 0 and plan(4096, 4, 1, 0.0, 0) == 0  # the dynamics kernels exist for d = 2, 3
    # K1's run variant keeps 8 B of CDF and 4 B of marks per particle in the 160 KiB of LDS (+ the record's rows)
    assert plan(8192, 3, 1, 0.0, 0) == 1 and plan(13568, 3, 1, 0.0, 0) == 1 and plan(13696, 3, 1, 0.0, 0) == 0
    assert plan(13568, 3, 1, 0.0, 1) == 0 and plan(13440, 3, 1, 0.0, 1) == 1
    assert plan(0, 3, 1, 0.0, 0) == EINVAL and plan(64, 0, 1, 0.0, 0) == EINVAL


def test_filter_side_eligibility_follows_the_switch_the_loop_length_and_the_plan():
    ok = dict(T=5, M=4096, d=3, mode=1, soft_alpha=0.0, adaptive=False)
    saved = engine.PF_DEDUP
    try:
        engine.PF_DEDUP = True
        assert filters.dedup_eligible(**ok) and filters.dedup_eligible(**{**ok, "T": 2, "recording": True})
        assert not filters.dedup_eligible(**{**ok, "T": 1})            # no step consumes a table
        assert not filters.dedup_eligible(**{**ok, "adaptive": True})
        assert not filters.dedup_eligible(**{**ok, "soft_alpha": 0.5})
        assert not filters.dedup_eligible(**{**ok, "mode": 2}) and not filters.dedup_eligible(**{**ok, "mode": 0})
        assert not filters.dedup_eligible(**{**ok, "M": 300})
        engine.PF_DEDUP = False
        assert not filters.dedup_eligible(**ok)
    finally:
        engine.PF_DEDUP = saved


def test_switch_follows_the_environment():
    env = dict(os.environ, PYTHONPATH=ROOT)
    code = "from multimodalfilter_amd import engine; print(int(engine.PF_DEDUP))"
    env.pop("MMF_PF_DEDUP", None)
    assert engine.PF_DEDUP == (os.environ.get("MMF_PF_DEDUP", "1") not in ("", "0"))
    import sys
    for value, want in (("0", "0"), ("1", "1")):
        out = subprocess.run([sys.executable, "-c", code], env=dict(env, MMF_PF_DEDUP=value), capture_output=True, text=True, check=True)
        assert out.stdout.strip() == want


def test_workspace_size_and_carving():
    lib = _abi.load()
    for N, M in ((1, 64), (3, 192), (256, 4096), (32, 4096)):
        words = N * M + 2 * N * (M + 1) + N
        assert lib.mmf_pf_dedup_workspace_words(N, M) == words == filters.dedup_workspace_words(N, M) == _abi.pf_dedup_workspace_words(N, M)
    assert lib.mmf_pf_dedup_workspace_words(-1, 64) == 0 and lib.mmf_pf_dedup_workspace_words(4, 0) == 0
    N, M = 3, 192
    buf = torch.zeros(filters.dedup_workspace_words(N, M), dtype=torch.int32)
    ws = _abi.pf_dedup_workspace(buf, N, M)
    base = buf.data_ptr()
    assert ws.rank == base and ws.run_anc == base + 4 * N * M
    assert ws.run_start == ws.run_anc + 4 * N * (M + 1) and ws.n_runs == ws.run_start + 4 * N * (M + 1)
    assert ws.n_runs + 4 * N == base + 4 * buf.numel()        # the four arrays tile the buffer exactly
    with pytest.raises(AssertionError):
        _abi.pf_dedup_workspace(buf[:-1], N, M)


def test_reserve_counts_the_workspace():
    import multimodalfilter_amd as mmf

    f = mmf.door_models.DoorCrossmodalParticleFilter()
    got = {}
    real = filters.reserve_memory
    filters.reserve_memory = lambda dev, nbytes: got.setdefault("n", nbytes)
    real_ws = engine._image_workspace
    engine._image_workspace = lambda *a, **k: None
    try:
        n = f.reserve(steps=4, batch=8, particles=256)
    finally:
        filters.reserve_memory, engine._image_workspace = real, real_ws
    d = f.state_dim
    assert n == got["n"] == 4 * 8 * 64 * 4 * 12 + 8 * (8 * 256 * 4 * (2 * d + 4) + 4 * filters.dedup_workspace_words(8, 256)) + (64 << 20)


def test_entry_points_are_bound_and_purely_additive():
    lib = _abi.load()
    for name in ("mmf_pf_forward_loop_dedup", "mmf_pf_dedup_plan", "mmf_pf_dedup_workspace_words", "mmf_pf_resample_runs",
                 "mmf_pf_dynamics_runs", "mmf_pf_dynamics_runs_philox"):
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert _abi.ABI_VERSION == 42 == lib.mmf_version()
    assert [n for n, _ in _abi.MmfPfDedupWorkspace._fields_] == ["rank", "run_anc", "run_start", "n_runs"]
    assert "dedup" not in " ".join(n for n, _ in _abi.MmfPfLoopArgs._fields_)


def test_entry_points_refuse_what_the_header_says_they_refuse():
    lib = _abi.load()
    bufs = [(ctypes.c_float * 256)() for _ in range(12)]
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    k1 = lambda **kw: lib.mmf_pf_resample_runs(kw.get("loglik", P[0]), P[1], kw.get("states", P[2]), kw.get("u", P[3]),
                                               kw.get("estimate", P[4]), None, None, kw.get("rank", P[5]), kw.get("anc", P[6]),
                                               kw.get("start", P[7]), kw.get("n_runs", P[8]), kw.get("N", 0), kw.get("M", 64),
                                               kw.get("d", 3), None, None, kw.get("ess", None), None)
    assert k1() == 0                                                   # an empty batch is a no-op
    for required in ("loglik", "states", "u", "estimate", "rank", "anc", "start", "n_runs"):
        assert k1(**{required: None}) == EINVAL, required
    assert k1(M=0) == EINVAL and k1(d=5) == EINVAL and k1(d=0) == EINVAL
    assert k1(M=13568) == 0 and k1(M=13696) == ETOOLARGE and k1(M=13568, ess=P[9]) == ETOOLARGE and k1(M=65537) == ETOOLARGE
    F32 = _abi.PREC_F32
    dyn = lambda **kw: lib.mmf_pf_dynamics_runs(P[0], kw.get("n_res", 3), kw.get("prec", F32), kw.get("prev", P[1]), P[2], P[3], P[4],
                                                kw.get("rank", P[5]), P[6], P[7], kw.get("n_runs", P[8]), kw.get("out", P[9]), None,
                                                kw.get("N", 0), kw.get("M", 64), kw.get("d", 3), None)
    assert dyn() == 0
    assert dyn(M=96) == EINVAL and dyn(M=0) == EINVAL                  # a tile is 64 (32) runs of one trajectory
    assert dyn(out=P[1]) == EINVAL                                     # the ancestors' rows are read while slots are written
    assert dyn(rank=None) == EINVAL and dyn(n_runs=None) == EINVAL and dyn(prev=None) == EINVAL
    assert dyn(n_res=2) == EINVAL
    assert dyn(N=1 << 20, M=1 << 12) == ETOOLARGE
    phil = lib.mmf_pf_dynamics_runs_philox
    assert phil(P[0], 3, F32, P[1], P[2], 1, 0, 0, P[4], P[5], P[6], P[7], P[8], P[9], None, 0, 64, 3, None) == 0
    assert phil(P[0], 3, F32, P[1], P[2], 1, 0, 0, None, P[5], P[6], P[7], P[8], P[9], None, 0, 64, 3, None) == EINVAL
    # the loop: a null workspace or null fields make it mmf_pf_forward_loop, which checks its own arguments
    a, ws = _abi.MmfPfLoopArgs(), _abi.MmfPfDedupWorkspace()
    assert lib.mmf_pf_forward_loop_dedup(None, None, None) == EINVAL
    assert lib.mmf_pf_forward_loop_dedup(ctypes.byref(a), ctypes.byref(ws), None) == EINVAL  # N = 0
    assert lib.mmf_pf_forward_loop_dedup(ctypes.byref(a), None, None) == lib.mmf_pf_forward_loop(ctypes.byref(a), None)


def test_workspace_struct_matches_the_header(tmp_path):
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _abi.MmfPfDedupWorkspace
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(MmfPfDedupWorkspace));']
    lines += [f'  printf("{n} %zu\\n", offsetof(MmfPfDedupWorkspace, {n}));' for n, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "ws.c", tmp_path / "ws"
    src.write_text("\n".join(lines))
    out = subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls) == 32
    for n, _ in cls._fields_:
        assert int(got[n]) == getattr(cls, n).offset, n

"""The run-consuming dynamics launch (``mmf_pf_dynamics_runs``, ``csrc/particle_net.hip``: ``RUNS``) at the sizes where the
benchmark's instantiation runs.  ``launch_runs`` picks the 64-run tile (pipelined in f16x3) from ``N M >= 131072``, and the
workgroups claim their tiles from the LDS counter from ``N M > 262144``; ``tests/test_gpu_dedup_dynamics.py`` stops at 8192.

Kernel level: a real dynamics network's packed weights, random previous states / per-trajectory terms / noise, and a run
table built here with numpy from ancestor rows the test chooses.  Expected: ``mmf_pf_dynamics`` (``_philox``) on the gathered
set ``states_prev[n, anc[n, k]]`` with the same noise -- the path is exact, so the comparison is ``torch.equal``.  The output
buffer starts as NaN: a slot that no tile writes fails the comparison.

Shapes (the smallest that reach each path): 32 x 4096 -- the 64-run tile, one tile per wave, no claims; 66 x 4096 -- claims,
N no multiple of a workgroup's stride; 4160 x 64 -- claims, one tile per trajectory (rotation modulus 1); 1056 x 256 -- four
tiles per trajectory.  Ancestor patterns: see ``_n_runs``.  One more case, 8200 x 4096, is the smallest whose per-workgroup
index list no longer fits the probe list in LDS."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_SHAPES = [(32, 4096), (66, 4096), (4160, 64), (1056, 256)]
_PATTERNS = ["random", "collapsed", "distinct", "alternating", "tile_edges", "first_tile_empty"]
_TILE = 64


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _n_runs(pattern, N, M):
    """Runs per trajectory, ``(N,)``."""
    n = np.arange(N)
    Q = M // _TILE
    if pattern == "random":  # about 0.55 M, spread over trajectories
        return np.random.default_rng(N + M).integers(int(0.45 * M), int(0.65 * M) + 1, size=N)
    if pattern == "collapsed":  # almost every tile is empty, whole workgroups find nothing
        return np.ones(N, dtype=np.int64)
    if pattern == "distinct":  # no empty tile
        return np.full(N, M)
    if pattern == "alternating":
        return np.where(n % 2 == 0, 1, M)
    if pattern == "tile_edges":  # exactly 64 k and 64 k + 1
        edges = [_TILE * k for k in range(1, Q + 1)] + [_TILE * k + 1 for k in range(Q)]
        return np.array(edges)[n % len(edges)]
    if pattern == "first_tile_empty":
        # a wave's first tile is tile `wave id` = (q' = 0, traj = wave id): after the rotation q = traj mod Q, empty as
        # soon as 64 q >= n_runs[traj] -- every trajectory but those with traj mod Q = 0 stops right below its first tile
        return np.where(n % Q == 0, M, _TILE * (n % Q))
    raise ValueError(pattern)


def _choose(rng, N, width, k):
    """Boolean ``(N, width)`` with exactly ``k[n]`` true entries in row n, at random places."""
    order = np.argsort(np.argsort(rng.random((N, width), dtype=np.float32), axis=1), axis=1)
    return order < k[:, None]


@functools.lru_cache(maxsize=None)
def _table(pattern, N, M):
    """numpy: non-decreasing ancestor rows with ``_n_runs`` runs each -> (anc (N, M), rank (N, M), run_anc (N, M + 1),
    run_start (N, M + 1), n_runs (N)), int32; entries of run_anc / run_start past the table's end hold -7."""
    k = _n_runs(pattern, N, M).astype(np.int64)
    assert k.shape == (N,) and k.min() >= 1 and k.max() <= M
    rng = np.random.default_rng(1000 + N + M + len(pattern))
    survivors = _choose(rng, N, M, k)                                   # which particles have offspring
    starts = np.concatenate([np.ones((N, 1), dtype=bool), _choose(rng, N, M - 1, k - 1)], axis=1)  # first slot of every run
    rank = np.cumsum(starts, axis=1) - 1
    run_anc = np.full((N, M + 1), -7, dtype=np.int32)
    run_start = np.full((N, M + 1), -7, dtype=np.int32)
    rows, cols = np.nonzero(survivors)                                  # row-major: ancestors ascending inside a row
    run_anc[rows, np.cumsum(survivors, axis=1)[rows, cols] - 1] = cols
    rows, cols = np.nonzero(starts)
    run_start[rows, rank[rows, cols]] = cols
    run_start[np.arange(N), k] = M
    anc = np.take_along_axis(run_anc, rank.astype(np.int64), axis=1)
    assert (np.diff(anc, axis=1) >= 0).all() and anc.min() >= 0 and anc.max() < M
    assert ((1 + (np.diff(anc, axis=1) != 0).sum(1)) == k).all()
    return anc.astype(np.int32), rank.astype(np.int32), run_anc, run_start, k.astype(np.int32)


@functools.lru_cache(maxsize=None)
def _dynamics(d):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    task, cls = ("push", "PushCrossmodalParticleFilter") if d == 2 else ("door", "DoorCrossmodalParticleFilter")
    torch.manual_seed(3)
    f = mmf.model_types(task)[cls]().to(torch.device("cuda", 0)).eval()
    synthetic.stabilise_dynamics(f)
    assert f.state_dim == d
    return f.dynamics_model


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("pattern", _PATTERNS)
@pytest.mark.parametrize("N,M", _SHAPES)
def test_dynamics_runs_equals_dynamics_on_the_gathered_set(N, M, pattern, d, precision, noise):
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    dyn = _dynamics(d)
    prec = _abi.PRECISIONS[precision]
    blob = dyn._net.blob(prec)  # packed the way engine.run_dynamics packs it
    tril = dyn.scale_tril().contiguous()
    g = torch.Generator(device=dev).manual_seed(N + M + d)
    prev = torch.randn((N, M, d), generator=g, device=dev)
    bias = torch.randn((N, _abi.MMF_UNITS), generator=g, device=dev)
    eps = torch.randn((N, M, d), generator=g, device=dev) if noise == "tensor" else None
    seed, step, traj0 = 99, 7, 5
    anc, rank, run_anc, run_start, n_runs = (torch.from_numpy(x).to(dev) for x in _table(pattern, N, M))
    flag = engine.range_flag(dev)

    gathered = torch.gather(prev, 1, anc.long()[:, :, None].expand(N, M, d)).contiguous()
    want = torch.full((N, M, d), float("nan"), device=dev)
    got = torch.full((N, M, d), float("nan"), device=dev)
    if noise == "tensor":
        _abi.pf_dynamics(blob, dyn._net.n_res, prec, gathered, bias, eps, tril, want, flag, N, M, d)
        _abi.pf_dynamics_runs(blob, dyn._net.n_res, prec, prev, bias, eps, tril, rank, run_anc, run_start, n_runs, got, flag, N, M, d)
    else:
        _abi.pf_dynamics_philox(blob, dyn._net.n_res, prec, gathered, bias, seed, step, traj0, tril, want, flag, N, M, d)
        _abi.pf_dynamics_runs_philox(blob, dyn._net.n_res, prec, prev, bias, seed, step, traj0, tril, rank, run_anc, run_start,
                                     n_runs, got, flag, N, M, d)
    assert bool(torch.isfinite(want).all())
    bad = (got != want) | torch.isnan(got)
    print(f"{N} x {M} {pattern} d={d} {precision} {noise}: runs / slots {float(n_runs.sum()) / (N * M):.3f}, differing values {int(bad.sum())}")
    if bool(bad.any()):
        where = bad.any(-1).nonzero()[:4].tolist()
        raise AssertionError(f"{int(bad.any(-1).sum())} slots differ; first (trajectory, slot): {where}")
    assert torch.equal(got, want)


def test_dynamics_runs_with_an_index_list_longer_than_the_probe_list_in_lds():
    """A workgroup keeps the ``n_runs`` of its index list in LDS while the list has at most 2048 entries; 8200 x 4096 gives
    every workgroup 2056, the smallest N at M = 4096 that takes the scalar load per index instead.  Trajectories alternate
    between one run and M runs; the table is written on the device (no sort is needed for these two patterns)."""
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    N, M, d = 8200, 4096, 2
    assert -(-(N * M // _TILE) // 2048) * 8 > 2048
    dyn = _dynamics(d)
    prec = _abi.PRECISIONS["f16x3"]
    blob = dyn._net.blob(prec)
    tril = dyn.scale_tril().contiguous()
    g = torch.Generator(device=dev).manual_seed(N + M + d)
    prev = torch.randn((N, M, d), generator=g, device=dev)
    bias = torch.randn((N, _abi.MMF_UNITS), generator=g, device=dev)
    i32 = dict(dtype=torch.int32, device=dev)
    one = (torch.arange(N, device=dev) % 2 == 0)[:, None]             # even trajectories: everything descends from one particle
    survivor = torch.randint(0, M, (N, 1), generator=g, device=dev).int()
    slots = torch.arange(M, **i32)[None, :].expand(N, M)
    anc = torch.where(one, survivor.expand(N, M), slots).contiguous()
    rank = torch.where(one, torch.zeros_like(slots), slots).contiguous()
    run_anc = torch.full((N, M + 1), -7, **i32)
    run_start = torch.full((N, M + 1), -7, **i32)
    run_anc[:, :M] = anc
    run_start[:, :M] = slots
    run_start[:, M] = M
    run_start[:, 1] = torch.where(one[:, 0], torch.full((N,), M, **i32), run_start[:, 1])
    n_runs = torch.where(one[:, 0], 1, M).int()
    flag = engine.range_flag(dev)
    gathered = torch.gather(prev, 1, anc.long()[:, :, None].expand(N, M, d)).contiguous()
    want = torch.full((N, M, d), float("nan"), device=dev)
    got = torch.full((N, M, d), float("nan"), device=dev)
    _abi.pf_dynamics_philox(blob, dyn._net.n_res, prec, gathered, bias, 99, 7, 5, tril, want, flag, N, M, d)
    _abi.pf_dynamics_runs_philox(blob, dyn._net.n_res, prec, prev, bias, 99, 7, 5, tril, rank, run_anc, run_start, n_runs, got,
                                 flag, N, M, d)
    assert bool(torch.isfinite(want).all())
    assert torch.equal(got, want)


def test_dedup_on_equals_off_through_forward_loop_with_claims():
    """The whole filter, 66 x 4096 door, f16x3, T = 3: ON against OFF as ``tests/test_gpu_dedup_dynamics.py`` compares them
    (the loop of launches, pinned off the persistent form by its ``_run``)."""
    import test_gpu_dedup_dynamics as small
    from multimodalfilter_amd import engine

    dev = _dev()
    old = engine.DEFAULT_PRECISION
    engine.set_default_precision("f16x3")
    try:
        f, d, traj, obs, ctrl, cov, rnd = small._setup("door", 66, 4096, dev)
        f.record_indices = True
        got = small._compare(f, traj, obs, ctrl, cov, rnd, "tensor", segments=(3,))
        idx = got[-2]
        distinct = (1 + (idx.diff(dim=-1) != 0).sum(-1)).float() / 4096
        print(f"66 x 4096: distinct ancestors / M in [{float(distinct.min()):.3f}, {float(distinct.max()):.3f}]")
    finally:
        engine.set_default_precision(old)

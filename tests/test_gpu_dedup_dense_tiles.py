"""The run-consuming dynamics launch (``mmf_pf_dynamics_runs``, ``csrc/particle_net.hip``: ``RUNS``) where a workgroup builds
the dense list of its real tiles (tiles are claimed, N <= 2048, lists of at most 2048 entries: ``csrc/particle_net_deal.h``)
and where the expansion's passes are requested ahead of their use (a ring of 8 passes: 7 ahead).

Method of ``tests/test_gpu_dedup_dynamics_large.py``: a run table built with numpy (``_run_tables``), expected output from
``mmf_pf_dynamics`` (``_philox``) on the gathered set with the same noise, ``torch.equal``, outputs pre-filled with NaN -- a
slot no tile writes, or one written from the wrong run or with the wrong pass's rank / noise, fails the comparison.

| shape | pattern | what it reaches |
|---|---|---|
| 66 x 4096 | ``one_full``: one trajectory with M runs, the rest 1 | 129 real tiles for 256 workgroups: empty and one-entry lists, waves without a tile at the barriers |
| 66 x 4096 | ``ramp``: n_runs from 1 to M over the trajectories | lists that mix many trajectories, the search at every depth |
| 66 x 4096 | ``spans``: tiles of 64 p - 1, 64 p, 64 p + 1 slots for p = 1 .. 10 (ring length + 2), one tile of 4096 slots | first, last, tail-guarded and fully queued passes of the expansion, the ring wrapping round |
| 1056 x 256 | ``below`` / ``above``: the real tiles number one below / one above a multiple of 256 | the last round of the dealing |
| 2048 x 192, 2049 x 192 | ``random`` | both sides of the dense mode's cap on N (N M > 262,144: tiles are claimed) |

Every pattern runs with f16x3 and f32, tensor and Philox noise; d = 2 and 3 alternate over them."""
import functools

import numpy as np
import pytest
import torch

import _run_tables as rt

pytestmark = pytest.mark.gpu

_TILE = rt.TILE
_AHEAD = 8        # kExpandAhead (csrc/particle_net.hip): the ring's length
_TRAJ_CAP = 2048  # kDenseTrajCap

_CASES = [(66, 4096, "one_full"), (66, 4096, "ramp"), (66, 4096, "spans"), (1056, 256, "below"), (1056, 256, "above"),
          (_TRAJ_CAP, 192, "random"), (_TRAJ_CAP + 1, 192, "random")]
_MODES = [("f16x3", "tensor", 3), ("f32", "philox", 2), ("f16x3", "philox", 2), ("f32", "tensor", 3)]


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _real_tiles(n_runs):
    return int((-(-np.asarray(n_runs, dtype=np.int64) // _TILE)).sum())


def _lengths(pattern, N, M):
    rng = np.random.default_rng(7 * N + M + len(pattern))
    if pattern == "one_full":
        k = np.ones(N, dtype=np.int64)
        k[17] = M
        assert _real_tiles(k) == 129
        return rt.lengths_from_counts(rng, k, M)
    if pattern == "ramp":
        return rt.lengths_from_counts(rng, np.linspace(1, M, N).round().astype(np.int64), M)
    if pattern == "random":
        return rt.lengths_from_counts(rng, rng.integers(1, M + 1, size=N), M)
    if pattern in ("below", "above"):
        k = rng.integers(1, M + 1, size=N)
        want, n = (255 if pattern == "below" else 1), 0
        while _real_tiles(k) % 256 != want:  # whole tiles added to single trajectories
            if k[n] + _TILE <= M:
                k[n] += _TILE
            n = (n + 1) % N
        return rt.lengths_from_counts(rng, k, M)
    if pattern == "spans":
        k = rng.integers(1, M + 1, size=N)
        lengths = rt.lengths_from_counts(rng, k, M)
        for p in range(1, _AHEAD + 3):
            # tiles of 64 p + 1 and 64 p slots, tiles of 64 slots in between, and a last tile of 7 runs in 64 p - 1 slots
            middle = (M - 3 * _TILE * p) // _TILE
            tiles = [(_TILE, _TILE * p + 1), (_TILE, _TILE * p)] + [(_TILE, _TILE)] * middle + [(7, _TILE * p - 1)]
            lengths[5 * p] = rt.lengths_from_tiles(rng, tiles)
        lengths[3] = np.array([M])  # one run: one tile of 4096 slots, 64 passes
        return lengths
    raise ValueError(pattern)


@functools.lru_cache(maxsize=None)
def _table(pattern, N, M):
    tab = rt.table(_lengths(pattern, N, M), M, seed=1000 + N + M + len(pattern))
    anc, rank, run_anc, run_start, n_runs = tab
    assert (np.diff(anc, axis=1) >= 0).all() and anc.min() >= 0 and anc.max() < M
    assert N * M // _TILE > 2 * 2048, "tiles are claimed"
    if pattern == "spans":
        passes = rt.passes_per_tile(run_start, n_runs, M)
        assert set(range(1, _AHEAD + 4)) <= set(passes.tolist()) and passes.max() == M // _TILE
    if pattern in ("below", "above"):
        assert _real_tiles(n_runs) % 256 == (255 if pattern == "below" else 1)
    return tab


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


@pytest.mark.parametrize("precision,noise,d", _MODES)
@pytest.mark.parametrize("N,M,pattern", _CASES)
def test_dynamics_runs_dense_equals_dynamics_on_the_gathered_set(N, M, pattern, precision, noise, d):
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    dyn = _dynamics(d)
    prec = _abi.PRECISIONS[precision]
    blob = dyn._net.blob(prec)
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
    print(f"{N} x {M} {pattern} d={d} {precision} {noise}: real tiles {_real_tiles(n_runs.cpu().numpy())}, differing values {int(bad.sum())}")
    if bool(bad.any()):
        where = bad.any(-1).nonzero()[:4].tolist()
        raise AssertionError(f"{int(bad.any(-1).sum())} slots differ; first (trajectory, slot): {where}")
    assert torch.equal(got, want)

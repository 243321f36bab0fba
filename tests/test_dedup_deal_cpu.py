"""``mmf_pf_dedup_deal`` (include/mmf.h): the dealing of the run-consuming dynamics launch's dense mode, on the host -- the
functions of ``csrc/particle_net_deal.h`` that the kernel calls -- against the numpy restatement in ``_run_tables.deal``.

Properties, over all workgroups of a launch: every real tile exactly once and no empty one; list lengths differ by at
most one; an entry decodes through the rotation to ``(traj, q)`` with ``64 q < n_runs[traj]`` (clamped as the kernel's
``clamp_runs``: 1 .. M)."""
import numpy as np
import pytest

import _run_tables as rt

TILE = rt.TILE


def _deal_native(n_runs, N, M, tile, grid, cap=None):
    from multimodalfilter_amd import _abi

    n_runs = np.ascontiguousarray(n_runs, dtype=np.int32)
    lists = []
    for b in range(grid):
        room = N * (M // tile) if cap is None else cap
        out = np.full(room + 1, -99, dtype=np.int32)
        length = _abi.pf_dedup_deal(n_runs, N, M, tile, grid, b, out, room)
        assert length >= 0
        assert (out[min(length, room):] == -99).all(), "wrote past the list / past cap"
        lists.append((length, out[:min(length, room)].copy()))
    return lists


def _tables():
    """name -> (n_runs, N, M, grid)"""
    M, Q = 4096, 4096 // TILE
    t = {}
    t["all_ones"] = (np.ones(66), 66, M, 256)
    t["all_M"] = (np.full(66, M), 66, M, 256)
    edges = [TILE * k for k in range(1, Q + 1)] + [TILE * k + 1 for k in range(Q)]
    t["tile_edges"] = (np.array(edges)[np.arange(256) % len(edges)], 256, M, 256)
    t["total_below_G"] = (np.ones(66), 66, M, 256)                       # 66 tiles, 256 workgroups: empty lists
    t["one_trajectory"] = (np.array([130]), 1, 256, 4)
    rng = np.random.default_rng(5)
    base = rng.integers(1, 257, size=1056)
    for name, want in (("total_multiple_of_G", 0), ("total_multiple_minus_1", 255), ("total_multiple_plus_1", 1)):
        t[name] = (_with_total(base, 256, TILE, 256, want), 1056, 256, 256)
    t["out_of_range_runs"] = (np.array([0, -5, 5000, 1, 4096, 4097, -2**31, 2**31 - 1, 64, 65] * 7)[:66], 66, M, 256)
    t["small_grid"] = (rng.integers(1, M + 1, size=7), 7, M, 3)
    t["tile_32"] = (rng.integers(1, 129, size=50), 50, 128, 16)
    return t


def _with_total(n_runs, M, tile, grid, residue):
    """``n_runs`` nudged (whole tiles added to / taken from single trajectories) until the real tiles number ``residue`` mod grid."""
    n_runs = np.array(n_runs, dtype=np.int64)
    tiles = lambda: int((-(-np.clip(n_runs, 1, M) // tile)).sum())
    n = 0
    while tiles() % grid != residue:
        if n_runs[n] + tile <= M:
            n_runs[n] += tile
        n = (n + 1) % len(n_runs)
    return n_runs


_TABLES = _tables()


@pytest.mark.parametrize("name", sorted(_TABLES))
def test_deal_equals_the_numpy_restatement_and_covers_every_real_tile_once(name):
    n_runs, N, M, grid = _TABLES[name]
    tile = 32 if name == "tile_32" else TILE
    got = _deal_native(n_runs, N, M, tile, grid)
    want = rt.deal(n_runs, N, M, tile, grid)
    clamped = np.clip(np.asarray(n_runs, dtype=np.int64), 1, M)
    total = int((-(-clamped // tile)).sum())
    lengths = [length for length, _ in got]
    assert sum(lengths) == total
    assert max(lengths) - min(lengths) <= 1
    seen = []
    for b, (length, entries) in enumerate(got):
        assert length == len(want[b]) and np.array_equal(entries, want[b]), f"workgroup {b}"
        assert (entries >= 0).all() and (entries < N * (M // tile)).all()
        traj, q = rt.decode(entries, N, M, tile)
        assert (tile * q < clamped[traj]).all(), f"workgroup {b} holds an empty tile"
        seen.append(traj * (M // tile) + q)
    seen = np.concatenate(seen) if seen else np.zeros(0, dtype=np.int64)
    assert len(np.unique(seen)) == len(seen) == total  # every real tile, once
    if name == "total_below_G":
        assert lengths.count(0) == grid - total and lengths.count(1) == total
    if name == "total_multiple_minus_1":
        assert total % grid == grid - 1 and lengths[-1] == lengths[0] - 1
    if name == "total_multiple_plus_1":
        assert total % grid == 1 and lengths[0] == lengths[1] + 1


def test_deal_writes_at_most_cap_entries_and_still_returns_the_length():
    n_runs, N, M, grid = _TABLES["all_M"]
    full = _deal_native(n_runs, N, M, TILE, grid)
    for cap in (0, 1, 5):
        cut = _deal_native(n_runs, N, M, TILE, grid, cap=cap)
        for (length, entries), (length_c, entries_c) in zip(full, cut):
            assert length_c == length and np.array_equal(entries_c, entries[:cap])


def test_deal_refuses_null_arguments_and_a_tile_that_does_not_divide_M():
    from multimodalfilter_amd import _abi

    n_runs = np.ones(4, dtype=np.int32)
    out = np.zeros(16, dtype=np.int32)
    assert _abi.pf_dedup_deal(n_runs, 4, 256, 64, 2, 0, out, 16) == 2
    assert _abi.pf_dedup_deal(None, 4, 256, 64, 2, 0, out, 16) < 0
    assert _abi.pf_dedup_deal(n_runs, 4, 256, 64, 2, 0, None, 16) < 0
    assert _abi.pf_dedup_deal(n_runs, 4, 250, 64, 2, 0, out, 16) < 0
    for N, M, tile, grid, b in ((0, 256, 64, 2, 0), (4, 256, 0, 2, 0), (4, 256, 64, 0, 0), (4, 256, 64, 2, 2), (4, 256, 64, 2, -1)):
        assert _abi.pf_dedup_deal(n_runs, N, M, tile, grid, b, out, 16) < 0
    assert (out[2:] == 0).all()

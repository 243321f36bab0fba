"""Run tables for tests of the run-consuming dynamics launch, built with numpy from the RUN LENGTHS a test chooses:
trajectory n is a list of positive run lengths that sum to M -- run r covers ``lengths[r]`` consecutive output slots --
and the surviving ancestors are drawn at random, ascending.  The layout is the one K1 writes (include/mmf.h,
``MmfPfDedupWorkspace``); entries of ``run_anc`` / ``run_start`` past a trajectory's table hold -7.

Also the numpy restatement of the dense dealing (``mmf_pf_dedup_deal``)."""
import numpy as np

TILE = 64


def compose(rng, total, parts):
    """``parts`` positive integers that sum to ``total``, at random."""
    assert 1 <= parts <= total
    cuts = np.sort(rng.choice(total - 1, size=parts - 1, replace=False)) + 1 if parts > 1 else np.zeros(0, dtype=np.int64)
    return np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int64)


def lengths_from_counts(rng, n_runs, M):
    """Per trajectory: ``n_runs[n]`` random run lengths that sum to M."""
    return [compose(rng, M, int(k)) for k in n_runs]


def lengths_from_tiles(rng, tiles):
    """One trajectory from its tiles, each ``(runs, slots)``: every tile but the last holds TILE runs."""
    assert all(r == TILE for r, _ in tiles[:-1]) and 1 <= tiles[-1][0] <= TILE
    return np.concatenate([compose(rng, slots, runs) for runs, slots in tiles])


def table(lengths, M, seed):
    """-> (anc (N, M), rank (N, M), run_anc (N, M + 1), run_start (N, M + 1), n_runs (N)), int32."""
    N = len(lengths)
    rng = np.random.default_rng(seed)
    anc = np.empty((N, M), dtype=np.int32)
    rank = np.empty((N, M), dtype=np.int32)
    run_anc = np.full((N, M + 1), -7, dtype=np.int32)
    run_start = np.full((N, M + 1), -7, dtype=np.int32)
    n_runs = np.empty(N, dtype=np.int32)
    for n, ln in enumerate(lengths):
        ln = np.asarray(ln, dtype=np.int64)
        k = len(ln)
        assert k >= 1 and ln.min() >= 1 and int(ln.sum()) == M
        survivors = np.sort(rng.choice(M, size=k, replace=False))
        n_runs[n] = k
        run_anc[n, :k] = survivors
        run_start[n, :k] = np.cumsum(ln) - ln
        run_start[n, k] = M
        rank[n] = np.repeat(np.arange(k), ln)
        anc[n] = survivors[rank[n]]
    return anc, rank, run_anc, run_start, n_runs


def passes_per_tile(run_start, n_runs, M):
    """Expansion passes (64 slots each) of every real tile, flattened."""
    out = []
    for n, k in enumerate(n_runs):
        edges = list(range(0, int(k), TILE)) + [int(k)]
        slots = np.diff(run_start[n, edges])
        out.extend((-(-slots // TILE)).tolist())
    return np.array(out)


# ---- the dense dealing, restated
def deal(n_runs, N, M, tile, grid):
    """Workgroup lists of the dense dealing: real tile k (trajectory-major) goes to workgroup k mod grid, entry
    ``q' N + traj`` with ``q = (q' + traj) mod (M / tile)``.  -> list of int arrays, one per workgroup."""
    T = M // tile
    c = -(-np.clip(np.asarray(n_runs, dtype=np.int64), 1, M) // tile)
    traj = np.repeat(np.arange(N), c)
    q = np.arange(int(c.sum())) - np.repeat(np.cumsum(c) - c, c)
    entry = ((q - traj) % T) * N + traj
    return [entry[b::grid] for b in range(grid)]


def decode(entry, N, M, tile):
    """Tile number -> (traj, q), the kernel's ``run_tile``."""
    entry = np.asarray(entry, dtype=np.int64)
    traj = entry % N
    return traj, (entry // N + traj) % (M // tile)

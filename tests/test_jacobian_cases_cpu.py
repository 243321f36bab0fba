"""Certifies, without a GPU, the inputs ``test_gpu_jacobian.py`` runs the forward-mode Jacobian kernel on
(``_jacobian_cases.py``): that the margin filter keeps every fp32 ReLU mask equal to the fp64 one, that the fp32 reference --
the yardstick of the GPU test's error rule -- is then close to the fp64 one ROW BY ROW, that the written-out recursion is the
oracle's autograd Jacobian, that the tie case is an exact tie which tells ``>`` from ``>=``, and that the row counts are the
edges of the launch code.

The caps are conditions on the INPUTS: a seed that breaks one is replaced, the cap stays."""
import pytest
import torch

import _jacobian_cases as jc
import _tol

POOLS = [(task, seed) for task in jc.TASKS for seed in jc.MULTI_SEEDS]


def test_row_counts_are_the_edges_of_the_launch_code():
    """``launch_ct``: ``big`` begins at ``R = 4 N = 256 * 8 * 64``; ``launch_variant``: 256 workgroups of 8 waves of one
    32-column tile of 8 groups each cover 16384 rows in one pass."""
    assert jc.BIG_N == 32768 and 4 * jc.BIG_N == 256 * 8 * 64
    assert jc.TILE_ROWS == 8 and jc.WORKGROUP_ROWS == 64 and jc.PASS_ROWS == 16384
    assert jc.NS == (1, 2, 7, 8, 9, 63, 64, 65, 257, 16384, 16385, 32767, 32768, 32777)
    assert jc.POOL_ROWS == max(jc.NS)

    def launch(N):  # launch_ct / launch_variant restated: (CT, tiles, grid)
        R = jc.GROUP * N
        ct = 2 if R >= jc.BIG_COLS else 1
        tiles = -(-R // (jc.TILE_COLS * ct))
        return ct, tiles, min(jc.MAX_GRID, max(1, -(-tiles // jc.WAVES)))

    assert launch(257) == (1, 33, 5)                       # several workgroups, the last one wave
    assert launch(16384) == (1, 2048, 256)                 # every wave of the capped grid: exactly one tile
    assert launch(16385) == (1, 2049, 256)                 # ... and wave 0 of workgroup 0 a second one
    assert launch(32767) == (1, 4096, 256)                 # every wave two tiles, the last short of one group
    assert launch(32768) == (2, 2048, 256)                 # 64-column tiles, one pass
    assert launch(32777) == (2, 2049, 256)
    # the last 64-column tile of N = 32777: 9 groups, i.e. a full first half and one live group in the second
    assert 32777 - 2048 * jc.BIG_TILE_ROWS == jc.TILE_ROWS + 1 == 9
    assert all(N <= jc.WORKGROUP_ROWS + 1 or N == jc.POOL_ROWS for _, N in jc.MULTI_CONFIGS)
    assert max(K for K, _ in jc.MULTI_CONFIGS) <= len(jc.MULTI_SEEDS) and jc.MAIN_SEED in jc.MULTI_SEEDS


@pytest.mark.parametrize("task,seed", POOLS)
def test_pools_keep_the_masks_and_the_fp32_reference(task, seed):
    """A pool needs to reject no more than a fifth of its candidates; on the kept rows the fp32 reference takes the fp64
    masks at all nine sites and is within ``FP32_CAP`` of the fp64 one in every row (``x'`` within ``X_BAR`` by that bar's own measure)."""
    p = jc.pool(task, seed)
    d = 3 if task == "door" else 2
    assert p.x.shape == (jc.POOL_ROWS, d) and p.u.shape == (jc.POOL_ROWS, 7) and p.x.dtype == p.u.dtype == torch.float32
    truth, fp32 = jc.reference(task, seed, torch.float64), jc.reference(task, seed, torch.float32)
    assert truth.pre.shape == (jc.POOL_ROWS, jc.N_SITES, 64)
    low = float(jc.margin(truth.pre).min())
    flips = int(((truth.pre > 0) != (fp32.pre > 0)).sum())
    err_J, err_x = _tol.rel_err(fp32.J, truth.J, dims=2), jc.x_err(fp32.x_next, truth.x_next)
    print(f"JACOBIAN pool task={task} seed={seed} kept_share={p.kept_share:.4f} margin_min={low:.3e} flips={flips} "
          f"fp32_J={err_J:.3e} fp32_x={err_x:.3e}")
    assert p.kept_share >= jc.MIN_KEPT_SHARE
    assert low >= jc.MARGIN
    assert flips == 0
    assert err_J < jc.FP32_CAP
    assert err_x < jc.X_BAR
    # the three input scales really occur, and the main pool's Jacobians are no identity in disguise
    assert float(p.x.abs().max()) > 6.0 and float(p.x.abs().flatten().median()) < 1.0
    part = (truth.J - torch.eye(d, dtype=torch.float64)).flatten(1).norm(dim=1)
    q10, q50 = (float(torch.quantile(part, q)) for q in (0.1, 0.5))
    print(f"JACOBIAN pool task={task} seed={seed} ||J - I||_F: 10 % of the rows below {q10:.3e}, median {q50:.3e}")
    if seed == jc.MAIN_SEED:   # (push at seeds 0 and 1: 1e-8 and 4e-6 -- the gate is shut on many rows; they serve group C's bit comparison)
        assert q10 > 0.1
    # every size is a prefix of the pool
    x9, u9 = jc.case(task, seed, 9)
    assert torch.equal(x9, p.x[:9]) and torch.equal(u9, p.u[:9])
    assert jc.outputs(task, seed, torch.float64)[1] is truth.J


@pytest.mark.parametrize("task,seed", POOLS)
def test_written_out_recursion_is_the_oracles_autograd_jacobian(task, seed):
    """Two independent derivations of the same operation, in fp64, on 300 rows: to 1e-12."""
    x, u = jc.case(task, seed, 300)
    m = jc.oracle_model(task, seed, torch.float64)
    want_J = m.jacobian(initial_states=x.double(), controls=u.double()).detach()
    with torch.no_grad():
        want_x = m(initial_states=x.double(), controls=u.double())[0]
    got = jc.forward_mode(jc.state_dict(task, seed), x, u, torch.float64)
    assert _tol.rel_err(got.J, want_J, dims=2) < 1e-12
    assert _tol.rel_err(got.x_next, want_x, dims=1) < 1e-12


@pytest.mark.parametrize("task", jc.TASKS)
def test_tie_case_is_an_exact_tie_that_tells_the_two_mask_rules_apart(task):
    t = jc.tie_case(task)
    assert t.x.shape[0] == jc.TIE_ROWS and not bool(t.x.any())
    truth, fp32 = jc.tie_reference(task, torch.float64), jc.tie_reference(task, torch.float32)
    for r in (truth, fp32):
        assert bool((r.pre[:, 0, :jc.TIE_UNITS] == 0).all())
        assert float(r.pre[:, 0, jc.TIE_UNITS:].abs().min()) > 0.0
    assert float(jc.margin(truth.pre, skip_first=jc.TIE_UNITS).min()) >= jc.MARGIN
    assert not bool(((truth.pre > 0) != (fp32.pre > 0)).any())
    assert _tol.rel_err(fp32.J, truth.J, dims=2) < jc.FP32_CAP
    # relu'(0) = 0 in autograd
    m = jc.oracle_model(task, jc.MAIN_SEED, torch.float64, tie=True)
    want = m.jacobian(initial_states=t.x.double(), controls=t.u.double()).detach()
    assert _tol.rel_err(truth.J, want, dims=2) < 1e-12
    # the >= rule is a hundred times the GPU bar away in every row
    ge = jc.tie_reference(task, torch.float64, True)
    diff = (ge.J - truth.J).flatten(1).norm(dim=1) / truth.J.flatten(1).norm(dim=1)
    print(f"JACOBIAN tie task={task} kept_of_first_64={t.kept} ge_vs_gt min={float(diff.min()):.3e} max={float(diff.max()):.3e}")
    assert torch.equal(diff, t.diff) and float(diff.min()) >= jc.TIE_MIN_DIFF >= 100 * _tol.REL_TOL
    assert torch.equal(ge.x_next, truth.x_next)

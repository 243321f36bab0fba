"""What the GPU tests of the particle-posterior summaries share (``test_gpu_quantiles.py``, ``_scores``, ``_density``,
``_modes``, ``_modalities``, ``_distance``, ``_forecast``): guarded output buffers and the call between them, the bit
comparison and its two loops (two calls and a row alone; every subset of the outputs), a small real filter with a history, and
the records' tensors as a case of the case modules."""
import functools
import itertools

import torch

import _smooth_cases as sc
import _summary_cases as sm

INT_SENTINEL = -77


class _Guarded:
    """A device array of ``rows`` leading slices between ``GUARD_ROWS`` guard slices holding the sentinel."""

    def __init__(self, rows, tail, dev, dtype=torch.float32):
        self.sentinel = sm.SENTINEL if dtype == torch.float32 else INT_SENTINEL
        self.full = torch.full((rows + 2 * sm.GUARD_ROWS,) + tuple(tail), self.sentinel, dtype=dtype, device=dev)
        self.view = self.full[sm.GUARD_ROWS:sm.GUARD_ROWS + rows]

    def guards_intact(self):
        g = sm.GUARD_ROWS
        return bool((self.full[:g] == self.sentinel).all()) and bool((self.full[self.full.shape[0] - g:] == self.sentinel).all())

    def untouched(self):
        return bool((self.full == self.sentinel).all())


N = lambda t: None if t is None else t.cpu().numpy()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def guarded_call(call, R, tails, want, outputs, what, dtypes=None):
    """``call(views)`` with every output of ``outputs`` between guard rows: ``views[k]`` is the ``(R,) + tails[k]`` view of
    output ``k`` (float32, or ``dtypes[k]``) if ``k`` is in ``want`` and ``None`` otherwise.  The guard rows must come back
    intact and the buffers not asked for untouched -> ``dict`` of device tensors (``None`` for those).  ``what``: the sizes,
    for the messages."""
    dev = sc.dev()
    bufs = {k: _Guarded(R, tails[k], dev, (dtypes or {}).get(k, torch.float32)) for k in outputs}
    call({k: (bufs[k].view if k in want else None) for k in outputs})
    torch.cuda.synchronize()
    for k, b in bufs.items():
        assert b.guards_intact(), f"a guard row of {k} was written ({what})"
        if k not in want:
            assert b.untouched(), f"{k} was not asked for and was written ({what})"
    return {k: (bufs[k].view.clone() if k in want else None) for k in outputs}


def assert_repeatable(run, case, outputs, rows, what=()):
    """Two calls of ``run(case)`` give the same bits, and so does each row of ``rows`` alone (``run(case, rows=slice)``)
    -> the outputs of the first call."""
    got, again = run(case), run(case)
    for k in outputs:
        assert _same_bits(got[k], again[k]), what + ("again", k)
    for r in rows:
        one = run(case, rows=slice(r, r + 1))
        for k in outputs:
            assert _same_bits(one[k], got[k][r:r + 1]), what + (r, k)
    return got


def assert_subsets_match_full(run, case, outputs, full=None, what=()):
    """Every proper non-empty subset ``want`` of ``outputs`` writes, in ``run(case, want)``, the bits of the full call (the
    untouched buffers are checked by ``guarded_call``) -> the full call's outputs."""
    full = run(case) if full is None else full
    for n in range(1, len(outputs)):
        for want in itertools.combinations(outputs, n):
            got = run(case, want)
            for k in want:
                assert _same_bits(got[k], full[k]), what + (want, k)
    return full


@functools.lru_cache(maxsize=None)
def _filter_run(kind, M, N_=3, T=6, owner=""):
    """A small ``kind`` filter, ``forward()`` that runs it with ``record_history`` from one fixed noise seed, its trajectories
    and ``(T, N, M, d)``; built once per argument tuple.  ``owner``: test modules that must not share a filter name themselves."""
    import multimodalfilter_amd as mmf

    dev = sc.dev()
    f, d, traj, obs, ctrl, cov = sc.small_filter(kind, N_, M, T, dev)

    def forward():
        f.record_history = True
        f.noise = mmf.NoiseSource(31)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        torch.cuda.synchronize()
        return est

    return f, forward, traj, (T, N_, M, d)


def _case_of(states, log_a, log_b, truth, point="truth", **extra):
    """``(T, N, ...)`` tensors of a record as a case of ``T N`` rows: the four common arrays flattened (the truth under the
    key ``point``), ``extra`` as it is."""
    T, N_, M, d = states.shape
    flat = lambda x, tail: None if x is None else x.detach().cpu().numpy().reshape((T * N_,) + tail)
    return dict(states=flat(states, (M, d)), log_a=flat(log_a, (M,)), log_b=flat(log_b, (M,)), **{point: flat(truth, (d,))}, **extra)

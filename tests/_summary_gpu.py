"""What the GPU tests of the three particle-posterior summaries share (``test_gpu_quantiles.py``, ``test_gpu_scores.py``,
``test_gpu_density.py``): guarded output buffers, the bit comparison, a small real filter with a history, and the records'
tensors as a case of the case modules."""
import functools

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

"""``scripts/_bench_common.py`` on the device: the recorded run of the feature benchmarks is the same run whenever it is asked
for, and the timing loop calls what it is given in the order it says."""
import os

import pytest

SCRIPTS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "scripts")
N, M, T = 2, 64, 3


@pytest.fixture
def bc(monkeypatch):
    monkeypatch.syspath_prepend(SCRIPTS)
    import _bench_common

    return _bench_common


def _dev():
    import torch

    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


@pytest.mark.gpu
def test_the_recorded_run_is_the_same_run_every_time(bc):
    import torch

    dev = _dev()
    first = bc.recorded_door_run(N, M, T, dev)
    torch.randn(7)  # a caller that has drawn from both generators in between gets the same history
    torch.randn(7, device=dev)
    second = bc.recorded_door_run(N, M, T, dev)
    for door in (first, second):
        f = door.f
        assert not f.training and f.record_history is True and f.num_particles == M
        assert door.dims == (T, N, M, 3) and f.last_history.states.shape == (T, N, M, 3)
        assert door.truth.shape == (T, N, 3) and door.truth.is_contiguous() and torch.equal(door.truth, door.traj["states"][1:])
        assert door.ctrl.shape[0] == T and all(v.shape[0] == T for v in door.obs.values())
        assert door.cov0.shape == (N, 3, 3)
    a, b = first.f.last_history, second.f.last_history
    for name in ("states", "log_likelihoods", "log_weights_in"):
        x, y = getattr(a, name), getattr(b, name)
        assert x.dtype == torch.float32 and torch.equal(x.view(torch.int32), y.view(torch.int32)), name


@pytest.mark.gpu
def test_run_false_stops_before_the_loop(bc):
    door = bc.recorded_door_run(N, M, T, _dev(), run=False)
    assert door.f.last_history is None and door.f.num_particles == M and not door.f.training
    assert door.dims == (T, N, M, 3) and door.truth.shape == (T, N, 3)


@pytest.mark.gpu
def test_time_alternating_calls_in_the_order_it_says(bc):
    _dev()
    calls = []
    times = bc.time_alternating({"a": (lambda: calls.append("a"), 3), "b": lambda: calls.append("b")}, 2)
    assert calls == ["a", "b"] + ["a", "a", "a", "b"] * 2
    assert list(times) == ["a", "b"] and all(len(v) == 2 and all(t >= 0.0 for t in v) for v in times.values())

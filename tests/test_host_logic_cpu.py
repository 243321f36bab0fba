"""Host-side logic that needs no GPU: noise sources, struct layouts of the step-loop arguments,
the training entry points' loud failures."""
import ctypes

import pytest
import torch

import multimodalfilter_amd as mmf
from multimodalfilter_amd import _abi, engine, train


def test_stacked_noise_serves_steps_in_replay_order():
    """``StackedNoise`` hands out the same tensors, in the same order, as ``ReplayNoise`` fed
    the same draws one by one -- and ``draw_steps`` returns zero-copy views of its blocks."""
    g = torch.Generator().manual_seed(0)
    N, M, d, T = 3, 5, 2, 4
    eps0 = torch.randn((N, M, d), generator=g)
    eps = torch.randn((T, N, M, d), generator=g)
    u = torch.rand((T, N), generator=g)
    like = torch.zeros(1)
    a = mmf.StackedNoise(eps0, eps, u)
    b = mmf.ReplayNoise([eps0] + list(eps), list(u))
    assert torch.equal(a.gaussian((N, M, d), like=like), b.gaussian((N, M, d), like=like))
    for _ in range(2):
        assert torch.equal(a.gaussian((N, M, d), like=like), b.gaussian((N, M, d), like=like))
        assert torch.equal(a.uniform((N,), like=like), b.uniform((N,), like=like))
    gs, us = a.draw_steps(2, (N, M, d), (N,), like=like)
    assert torch.equal(gs, eps[2:4]) and torch.equal(us, u[2:4])
    assert gs.data_ptr() == eps[2].data_ptr()
    gs2, us2 = b.draw_steps(2, (N, M, d), (N,), like=like)
    assert torch.equal(gs2, gs) and torch.equal(us2, us)


def test_stacked_noise_checks_shapes():
    a = mmf.StackedNoise(torch.zeros(2, 3, 2), torch.zeros(1, 2, 3, 2), torch.zeros(1, 2))
    with pytest.raises(AssertionError):
        a.gaussian((2, 4, 2), like=torch.zeros(1))


def test_loop_argument_structs_match_the_header():
    """Field order / sizes of the host structs handed to the native step loops."""
    P, I = ctypes.sizeof(ctypes.c_void_p), 4
    # + feedback_gate (ABI 33); + persistent, n_sync_words (two int32 = one pointer slot), sync_words (ABI 40)
    assert ctypes.sizeof(_abi.MmfEkfLoopArgs) == 8 * I + (2 * _abi.LOOP_MAX_MEAS + 12) * P + 2 * I + P
    assert _abi.MmfEkfLoopArgs.sync_words.offset == _abi.MmfEkfLoopArgs.persistent.offset + 2 * I
    pf = _abi.MmfPfLoopArgs
    assert pf.T.offset == 0 and pf.dyn_packed.offset == 10 * I
    assert pf.event_stride.offset + I <= ctypes.sizeof(pf)
    assert [n for n, _ in _abi.MmfEkfLoopArgs._fields_][:9] == ["T", "N", "d", "K", "fusion", "feedback", "n_res_dyn",
                                                                "precision", "range_flag"]
    assert _abi.MmfEkfLoopArgs.range_flag.offset == 8 * I  # eight int32 fields, then pointers


def test_training_entry_points_fail_loudly_without_backend_or_gpu():
    f = mmf.door_models.DoorParticleFilter().train()
    batch = {"states": torch.zeros(3, 2, 3), "controls": torch.zeros(3, 2, 7), "image": torch.zeros(3, 2, 32, 32),
             "gripper_pos": torch.zeros(3, 2, 3), "gripper_sensors": torch.zeros(3, 2, 7)}
    engine.set_training_backend(None)
    with pytest.raises(AssertionError):
        train.filter_loss(f, batch, initial_covariance=torch.eye(3) * 0.1)
    engine.set_training_backend("hip")
    try:
        with pytest.raises(_abi.MmfError):  # CPU tensors: the HIP path refuses them, nothing falls back
            train.filter_loss(f, batch, initial_covariance=torch.eye(3) * 0.1)
    finally:
        engine.set_training_backend(None)
    with pytest.raises(AssertionError):
        engine.set_training_backend("cpu")


def test_packed_weight_cache_rebuilds_exactly_when_a_source_changes():
    """``utils.cached``, the staleness rule of every packed-weight blob: the same object while nothing changed; a
    rebuild after an in-place update, a version bump with no write (what a graph replay's writes need), a replaced
    tensor, a move to another device, and under another key."""
    from multimodalfilter_amd.utils import cached

    builds = []

    def build():
        builds.append(1)
        return object()

    w, b = torch.zeros(4, 3), torch.zeros(4)
    cache = {}
    first = cached(cache, "k", [w, b], build)
    assert cached(cache, "k", [w, b], build) is first and len(builds) == 1
    w.add_(1.0)
    v = cached(cache, "k", [w, b], build)
    assert v is not first and len(builds) == 2
    assert cached(cache, "k", [w, b], build) is v and len(builds) == 2
    torch.autograd.graph.increment_version(b)
    v = cached(cache, "k", [w, b], build)
    assert len(builds) == 3 and cached(cache, "k", [w, b], build) is v
    w2 = w.clone()
    v = cached(cache, "k", [w2, b], build)
    assert len(builds) == 4 and cached(cache, "k", [w2, b], build) is v
    other = cached(cache, "other", [w2, b], build)
    assert len(builds) == 5 and other is not v and cached(cache, "k", [w2, b], build) is v
    if torch.cuda.is_available():
        wd = w2.to("cuda:0")
        cached(cache, "k", [wd, b], build)
        assert len(builds) == 6


class _FakeLoopArgs(ctypes.Structure):
    _fields_ = [("persistent", ctypes.c_int32), ("n_sync_words", ctypes.c_int32), ("sync_words", ctypes.c_void_p),
                ("range_flag", ctypes.c_void_p)]


def test_run_persistent_is_the_give_up_protocol_of_every_loop():
    """``engine.run_persistent`` with a fake entry point on host tensors: one plain call when not eligible; one persistent
    call when all goes well; after a give-up the in-place tensors are restored BEFORE the second call, ``FLAG_GAVE_UP`` is
    consumed and every other bit left alone, one warning, all three switches off, and the next invocation does not try
    again; ``restore=None`` never reads the status word.  ``persistent_forms`` puts switches and latch back."""
    import warnings

    cpu = torch.device("cpu")
    flag = engine.range_flag(cpu)
    flag.zero_()
    start = (engine.PF_PERSISTENT, engine.EKF_PERSISTENT, engine.LSTM_PERSISTENT, engine._PERSISTENT_WARNED)
    mu, Sigma = torch.arange(6.0), torch.arange(18.0)
    mu0, Sigma0 = mu.clone(), Sigma.clone()
    seen = []

    def call(a, sabotage=False):
        seen.append((int(a.persistent), int(a.n_sync_words), a.sync_words, a.range_flag, mu.clone(), Sigma.clone()))
        if sabotage and a.persistent:
            mu.fill_(float("nan"))
            Sigma.fill_(float("nan"))
            flag.bitwise_or_(_abi.FLAG_GAVE_UP | _abi.FLAG_RANGE)
        return len(seen)

    with engine.persistent_forms(pf=True, ekf=True, lstm=True):
        # not eligible
        a = _FakeLoopArgs()
        assert engine.run_persistent(a, lambda: call(a), n_sync_words=0, device=cpu, restore=(mu, Sigma)) == 1
        assert [s[:4] for s in seen] == [(0, 0, None, None)]
        # eligible, and the launch ran to its end
        del seen[:]
        a = _FakeLoopArgs()
        assert engine.run_persistent(a, lambda: call(a), n_sync_words=40, device=cpu, restore=(mu, Sigma)) == 1
        assert [s[:2] for s in seen] == [(1, 40)] and seen[0][2] and seen[0][3] == flag.data_ptr()
        assert int(flag.item()) == 0
        # eligible, and the launch gave up
        del seen[:]
        a = _FakeLoopArgs()
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            assert engine.run_persistent(a, lambda: call(a, True), n_sync_words=40, device=cpu, restore=(mu, Sigma)) == 2  # the rerun's result
            assert [s[0] for s in seen] == [1, 0]
            assert torch.equal(seen[1][4], mu0) and torch.equal(seen[1][5], Sigma0)  # restored before the second call
            assert int(flag.item()) == _abi.FLAG_RANGE
            assert (engine.PF_PERSISTENT, engine.EKF_PERSISTENT, engine.LSTM_PERSISTENT) == (False, False, False)
            # what a caller's eligibility expression now yields: no further attempt, and no second warning after another give-up
            a = _FakeLoopArgs()
            engine.run_persistent(a, lambda: call(a, True), n_sync_words=40 if engine.EKF_PERSISTENT else 0, device=cpu, restore=(mu, Sigma))
            assert [s[0] for s in seen] == [1, 0, 0]
            a = _FakeLoopArgs()
            engine.run_persistent(a, lambda: call(a, True), n_sync_words=40, device=cpu, restore=(mu, Sigma))
        assert len(caught) == 1 and "gave up" in str(caught[0].message)
        with pytest.raises(_abi.MmfError, match="f16x3 operand range"):  # FLAG_RANGE is still there for the loop's own check
            engine.check_range(cpu)
        # restore=None: a launch without hand-offs -- no copies, and the status word is not read at all
        del seen[:]
        a = _FakeLoopArgs()
        flag.item = lambda: pytest.fail("the status word was read")
        try:
            engine.run_persistent(a, lambda: call(a, True), n_sync_words=40, device=cpu, restore=None)
        finally:
            del flag.item
        assert [s[0] for s in seen] == [1] and bool(torch.isnan(mu).all())
        flag.zero_()
    # the switches and the warned-once latch are back where they started, although a give-up cleared all three inside
    assert (engine.PF_PERSISTENT, engine.EKF_PERSISTENT, engine.LSTM_PERSISTENT, engine._PERSISTENT_WARNED) == start
    with engine.persistent_forms(ekf=False):
        assert (engine.PF_PERSISTENT, engine.EKF_PERSISTENT, engine.LSTM_PERSISTENT) == (start[0], False, start[2])
    assert (engine.PF_PERSISTENT, engine.EKF_PERSISTENT, engine.LSTM_PERSISTENT, engine._PERSISTENT_WARNED) == start


def test_check_range_names_the_three_reports():
    cpu = torch.device("cpu")
    flag = engine.range_flag(cpu)
    for bits, exc, text in ((_abi.FLAG_NOT_PD | _abi.FLAG_GAVE_UP | _abi.FLAG_RANGE, ValueError, "not positive definite"),
                            (_abi.FLAG_GAVE_UP | _abi.FLAG_RANGE, _abi.MmfError, "MMF_EKF_PERSISTENT=0"),
                            (_abi.FLAG_RANGE, _abi.MmfError, "f16x3 operand range")):
        flag.fill_(bits)
        with pytest.raises(exc, match=text):
            engine.check_range(cpu)
        assert int(flag.item()) == 0
    engine.check_range(cpu)


def test_capturing_is_seen_by_the_capturing_thread_only():
    import threading

    seen = {}
    inside, done = threading.Event(), threading.Event()

    def other():
        inside.wait(10)
        seen["other"] = engine.is_capturing()
        done.set()

    t = threading.Thread(target=other)
    t.start()
    assert not engine.is_capturing()
    with engine.capturing():
        with engine.capturing():  # nests
            pass
        seen["own"] = engine.is_capturing()
        inside.set()
        assert done.wait(10)
    t.join()
    assert seen == {"own": True, "other": False} and not engine.is_capturing()


# What a ParticleFilter step does, as ``_step``, ``_step_autograd``, ``_native_loop`` and ``_native_train_loop`` each spelled it
# before ``_step_policy`` was the one place: (training, ``resample`` switch) -> does the step resample
_STEP_RESAMPLES = {(False, None): True, (True, None): False,   # None: resample iff not training
                   (False, True): True, (True, True): True, (False, False): False, (True, False): False}


@pytest.mark.parametrize("training,switch", list(_STEP_RESAMPLES))
def test_step_policy_is_what_the_four_step_paths_decided(training, switch):
    """``ParticleFilter._step_policy(M)`` over ``training`` x ``resample`` x both modes x ``num_particles`` equal to and
    different from the belief's ``M`` x threshold set / unset x alpha 1 / 0.5, against the record written out by hand."""
    import itertools

    import _smooth_cases as sc

    dyn, meas = sc.linear_gaussian_models(3, 0.05, 0.3, torch.device("cpu"))
    M = 6
    resamples = _STEP_RESAMPLES[(training, switch)]
    for (name, code), count, thr, alpha in itertools.product((("systematic", 1), ("multinomial", 2)), (6, 9), (None, 0.5),
                                                             (1.0, 0.5)):
        f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=count, resample=switch,
                                       resample_mode=name, soft_resample_alpha=alpha, resample_ess_threshold=thr)
        f.train(training)
        got = f._step_policy(M)
        case = (training, switch, name, count, thr, alpha)
        assert isinstance(got, tuple) and got._fields == ("resample", "mode", "M_out", "soft", "threshold"), case
        assert got.resample is resamples, case
        assert got.M_out == count, case
        if not resamples:  # a step that does not resample: mode 0 whatever resample_mode says, nothing soft, no threshold
            assert (got.mode, got.soft, got.threshold) == (0, False, None), case
            continue
        assert got.mode == code, case
        assert got.soft is (alpha == 0.5), case
        # a step that changes the particle count resamples everybody: the threshold is dropped
        assert got.threshold == (0.5 if thr is not None and count == M else None), case
    with pytest.raises(AttributeError):  # the record is immutable
        got.mode = 3


def test_step_policy_drops_the_threshold_with_the_count_and_the_mode_without_resampling():
    """The two facts the code after the policy depends on, one example each."""
    import _smooth_cases as sc

    dyn, meas = sc.linear_gaussian_models(3, 0.05, 0.3, torch.device("cpu"))
    f = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, num_particles=9, resample_mode="multinomial",
                                   resample_ess_threshold=0.5).eval()
    assert f._step_policy(9) == (True, 2, 9, False, 0.5)
    assert f._step_policy(6) == (True, 2, 9, False, None)      # 6 -> 9 particles: K1 resamples every trajectory
    f.train()
    assert f._step_policy(9) == (False, 0, 9, False, None)     # no resampling: mode 0, and no decision to take
    f.resample = True
    assert f._step_policy(9) == (True, 2, 9, False, 0.5)

"""The recurrence kernel of the LSTM baselines (``csrc/lstm.hip``) on the MI355X over its whole input contract -- any in_dim
that is a multiple of 8 in [8, 512], any N >= 1, any T >= 0 -- driven directly through ``engine.packed_lstm`` +
``engine.run_lstm_loop``: against the fp64 recurrence of ``_lstm_cases.py`` (which ``test_lstm_cases_cpu.py`` certifies) in
five input families, both forms bit for bit; the bit-level properties that follow from the fixed K split and partial-sum
order (a trajectory's bits do not depend on its batch position; one call over T steps is two chained calls); the packed
layout against ``include/mmf.h``; and the argument contract with real device pointers.

The error rule is the one of ``test_gpu_lstm.py::test_lstm_eval_against_fp64_with_saturated_gates``: per tensor,
``rel_err(engine, fp64) <= 2 rel_err(torch fp32 CPU, fp64) + 1e-6``.  Measured on one MI355X, worst tensor of each family
(engine / torch fp32 on the CPU): plain 3.4e-7 / 6.0e-7, saturated 8.2e-7 / 1.0e-6, small_signal_1e-3 3.3e-7 / 7.5e-7,
small_signal_1e-4 3.4e-7 / 7.5e-7, zero_state 4.4e-7 / 5.8e-7.  With tanh evaluated as ``2 sigmoid(2x) - 1`` (before
``mmf_det_tanh``) the same machine gave 7.1e-4 (small_signal_1e-3), 7.2e-3 (small_signal_1e-4) and 2.4e-6 (zero_state) against
bars of 1.4e-6 to 2.0e-6, and 7.5e-7 / 8.6e-7 on plain / saturated."""
import ctypes

import numpy as np
import pytest
import torch

import _lstm_cases as lc
from _tol import rel_err

pytestmark = pytest.mark.gpu

NAMES = ("h2", "hT", "cT")
SENTINEL = -1234.5
_MODULE = {}


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _packed(in_dim, variant, seed=0):
    """``engine.PackedLstm`` of the case weights on the device (the most recent set is kept: the cases come ordered)."""
    from multimodalfilter_amd import engine

    key = (in_dim, variant, seed)
    if _MODULE.get("key") != key:
        _MODULE.clear()
        m = lc.module(in_dim, lc.tensors(in_dim, variant, seed)).to(torch.device("cuda:0"))
        _MODULE.update(key=key, module=m, packed=engine.packed_lstm(m))
    return _MODULE["packed"]


def _run(packed, x, h0, c0, persistent):
    """One ``run_lstm_loop`` with the persistent switch as given -> (which form the C call was asked for, outputs)."""
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    taken = []
    real = _abi.lstm_forward

    def spy(a, like):
        taken.append(int(a.persistent))
        return real(a, like)

    _abi.lstm_forward = spy
    try:
        with engine.persistent_forms(lstm=persistent):
            out = engine.run_lstm_loop(packed, x.to(dev), h0.to(dev), c0.to(dev))
    finally:
        _abi.lstm_forward = real
    torch.cuda.synchronize()
    return taken, out


def _run_default(packed, x, h0, c0):
    """The form the engine picks by itself for this size (persistent where the plan allows it)."""
    from multimodalfilter_amd import _abi

    T, N = x.shape[:2]
    taken, out = _run(packed, x, h0, c0, True)
    assert taken == [1 if T > 0 and _abi.lstm_persistent_plan(N, max(T, 1)) > 0 else 0], taken
    return out


def _bits_equal(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("c", lc.all_cases(), ids=lc.case_id)
def test_recurrence_against_fp64_in_both_forms(c):
    _need_gpu()
    from multimodalfilter_amd import _abi

    family, in_dim, N, T = c
    k = lc.case(*c)
    packed = _packed(in_dim, k.variant, k.seed)
    taken_p, pers = _run(packed, k.x, k.h0, k.c0, True)
    taken_l, launches = _run(packed, k.x, k.h0, k.c0, False)
    plan = _abi.lstm_persistent_plan(N, T)
    assert (plan > 0) == (N <= 256), (plan, N)            # an MI355X has room for the 128 resident workgroups
    assert taken_p == [1 if plan > 0 else 0] and taken_l == [0], (taken_p, taken_l)
    for name, a, b in zip(NAMES, pers, launches):
        assert _bits_equal(a, b), name
    errs = []
    for name, got, want, t32 in zip(NAMES, pers, k.truth, k.fp32):
        assert got.shape == want.shape and bool(torch.isfinite(got).all()), name
        errs.append((name, rel_err(got, want, dims=1), rel_err(t32, want, dims=1)))
        print(f"LSTMERR {family} in_dim={in_dim} N={N} T={T} {name}: engine {errs[-1][1]:.3e} torch_fp32 {errs[-1][2]:.3e}")
    for name, e_engine, e_torch in errs:
        assert e_engine <= lc.bar(e_torch), (name, e_engine, e_torch)


@pytest.mark.parametrize("in_dim", [8, 512])
def test_a_trajectory_does_not_depend_on_its_batch_position(in_dim):
    """N = 257, T = 3 (loop of launches, two column groups): rows 0, 31, 32 (tile edges), 255 and 256 (the last of the first
    column group and the only one of the second) each equal, bit for bit, the same trajectory run alone at N = 1 (the
    persistent form)."""
    _need_gpu()
    k = lc.case("plain", in_dim, 257, 3)
    packed = _packed(in_dim, k.variant, k.seed)
    whole = _run_default(packed, k.x, k.h0, k.c0)
    for row in (0, 31, 32, 255, 256):
        alone = _run_default(packed, k.x[:, row:row + 1], k.h0[:, row:row + 1], k.c0[:, row:row + 1])
        for name, a, w in zip(NAMES, alone, whole):
            assert _bits_equal(a, w[:, row:row + 1].contiguous()), (row, name)


@pytest.mark.parametrize("N", [33, 257])
def test_one_call_equals_two_chained_calls(N):
    """T = 5 in one call against T = 3 followed by T = 2 on the returned ``(hT, cT)``: ``h2``, ``hT``, ``cT`` bit for bit."""
    _need_gpu()
    in_dim, variant = 24, "default"
    packed = _packed(in_dim, variant)
    g = torch.Generator().manual_seed(50 + N)
    x = torch.randn((5, N, in_dim), generator=g)
    h0, c0 = torch.randn((2, N, lc.H), generator=g), torch.randn((2, N, lc.H), generator=g)
    h2, hT, cT = _run_default(packed, x, h0, c0)
    h2a, hTa, cTa = _run_default(packed, x[:3], h0, c0)
    h2b, hTb, cTb = _run_default(packed, x[3:], hTa, cTa)
    assert _bits_equal(torch.cat([h2a, h2b]), h2) and _bits_equal(hTb, hT) and _bits_equal(cTb, cT)
    assert _bits_equal(h2a[-1], hTa[1]) and not _bits_equal(hTa, hT)
    # and the single call is the recurrence (so the equality above is not one of two empty results)
    want = lc.reference(x, h0, c0, lc.tensors(in_dim, variant))
    for name, got, w in zip(NAMES, (h2, hT, cT), want):
        assert rel_err(got, w, dims=1) <= 1e-5, name


@pytest.mark.parametrize("N", [1, 33, 257])
def test_no_steps_pass_the_state_through(N):
    """T = 0: ``hT`` / ``cT`` are bit copies of ``h0`` / ``c0`` (NaN payloads and signed zeros included), ``h2`` is empty."""
    _need_gpu()
    packed = _packed(8, "default")
    g = torch.Generator().manual_seed(60 + N)
    h0, c0 = torch.randn((2, N, lc.H), generator=g), torch.randn((2, N, lc.H), generator=g)
    h0[0, 0, :4] = torch.tensor([float("nan"), -0.0, float("inf"), 1e-42])
    for persistent in (True, False):
        taken, (h2, hT, cT) = _run(packed, torch.zeros((0, N, 8)), h0, c0, persistent)
        assert taken == [0]
        assert h2.shape == (0, N, lc.H) and _bits_equal(hT.cpu(), h0) and _bits_equal(cT.cpu(), c0)


@pytest.mark.parametrize("in_dim", [8, 512])
def test_pack_layout_is_the_documented_one(in_dim):
    """``mmf_lstm_pack`` into a blob pre-filled with NaN against the numpy restatement of ``include/mmf.h``'s layout
    (``_lstm_cases.packed_layout``, itself checked on the CPU): every float written, every bit equal."""
    _need_gpu()
    from multimodalfilter_amd import _abi

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(70 + in_dim)
    shapes = [(2048, in_dim), (2048, 512), (2048,), (2048,), (2048, 512), (2048, 512), (2048,), (2048,)]
    ts = [torch.randn(s, generator=g) for s in shapes]
    n = _abi.lstm_blob_floats(in_dim)
    assert n == 2048 * (in_dim + 512 + 1024 + 2)
    blob = torch.full((n + 64,), float("nan"), device=dev)
    _abi.lstm_pack([t.to(dev) for t in ts], blob, in_dim)
    torch.cuda.synchronize()
    got = blob.cpu().numpy()
    assert np.isnan(got[n:]).all()                     # nothing past the blob
    assert not np.isnan(got[:n]).any()
    want = lc.packed_layout(ts, in_dim)
    assert np.array_equal(got[:n].view(np.int32), want.view(np.int32))


def _valid_call(dev, N=3, T=2, in_dim=8):
    """A valid ``MmfLstmArgs`` (loop of launches) over real device tensors, the outputs pre-filled with a sentinel; ``x`` is
    large enough for any in_dim up to 520.  Returns the struct and the tensors by name."""
    from multimodalfilter_amd import _abi

    g = torch.Generator().manual_seed(80)
    t = {"x": torch.randn((T, N, 520), generator=g).to(dev), "h0": torch.randn((2, N, lc.H), generator=g).to(dev),
         "c0": torch.randn((2, N, lc.H), generator=g).to(dev)}
    for name, shape in (("hT", (2, N, lc.H)), ("cT", (2, N, lc.H)), ("h2", (T, N, lc.H))):
        t[name] = torch.full(shape, SENTINEL, device=dev)
    t["packed"] = _packed(in_dim, "default").blob()
    t["sync"] = torch.full((_abi.lstm_sync_words(N),), 0x55555555, dtype=torch.int32, device=dev)
    a = _abi.MmfLstmArgs()
    a.T, a.N, a.in_dim, a.persistent = T, N, in_dim, 0
    for name in ("x", "h0", "c0", "hT", "cT", "h2", "packed"):
        setattr(a, name, _abi.vp(t[name]))
    a.sync_words, a.n_sync_words = _abi.vp(t["sync"], torch.int32), _abi.lstm_sync_words(N)
    a.range_flag = None
    return a, t


BAD_CALLS = {
    "hT_is_h0": lambda a, t, abi: setattr(a, "hT", abi.vp(t["h0"])),
    "cT_is_c0": lambda a, t, abi: setattr(a, "cT", abi.vp(t["c0"])),
    "sync_words_one_short": lambda a, t, abi: setattr(a, "n_sync_words", abi.lstm_sync_words(a.N) - 1),
    "in_dim_12": lambda a, t, abi: setattr(a, "in_dim", 12),
    "in_dim_520": lambda a, t, abi: setattr(a, "in_dim", 520),
    "N_0": lambda a, t, abi: setattr(a, "N", 0),
}


@pytest.mark.parametrize("bad", sorted(BAD_CALLS))
@pytest.mark.parametrize("persistent", [0, 1])
def test_refused_calls_return_an_error_and_write_nothing(bad, persistent):
    _need_gpu()
    from multimodalfilter_amd import _abi

    dev = torch.device("cuda:0")
    a, t = _valid_call(dev)
    before = {name: v.clone() for name, v in t.items()}
    a.persistent = persistent
    BAD_CALLS[bad](a, t, _abi)
    rc = _abi.load().mmf_lstm_forward(ctypes.byref(a), _abi.stream_of(t["x"]))
    assert rc == -1, rc                                  # MMF_EINVAL
    with pytest.raises(_abi.MmfError, match="argument error"):
        _abi.lstm_forward(a, t["x"])
    torch.cuda.synchronize()
    for name, v in t.items():
        assert torch.equal(v, before[name]), name        # sentinels, inputs and the sync words alike


def test_the_call_the_refusals_are_built_from_is_valid():
    """The same struct without a defect runs and fills every output: each refusal above is down to its one defect."""
    _need_gpu()
    from multimodalfilter_amd import _abi

    dev = torch.device("cuda:0")
    a, t = _valid_call(dev)
    _abi.lstm_forward(a, t["x"])
    torch.cuda.synchronize()
    want = lc.reference(_as_in_dim_8(t["x"]), t["h0"].cpu(), t["c0"].cpu(), lc.tensors(8, "default"))
    for name, w in zip(NAMES, want):
        assert not bool((t[name] == SENTINEL).any()), name
        assert rel_err(t[name], w, dims=1) <= 1e-5, name


def test_no_steps_through_the_c_call_copy_the_state_and_touch_nothing_else():
    """The same struct with T = 0 (x and h2 still real pointers): ``hT`` / ``cT`` become bit copies of ``h0`` / ``c0``; ``h2``
    keeps its sentinel and the sync words what they held -- nothing was launched or zeroed."""
    _need_gpu()
    from multimodalfilter_amd import _abi

    dev = torch.device("cuda:0")
    for persistent in (0, 1):
        a, t = _valid_call(dev)
        sync = t["sync"].clone()
        a.T, a.persistent = 0, persistent
        _abi.lstm_forward(a, t["x"])
        torch.cuda.synchronize()
        assert _bits_equal(t["hT"], t["h0"]) and _bits_equal(t["cT"], t["c0"])
        assert bool((t["h2"] == SENTINEL).all()) and torch.equal(t["sync"], sync)


def _as_in_dim_8(x):
    """What the kernel reads of the ``(T, N, 520)`` buffer at in_dim = 8: its first ``T * N * 8`` floats as ``(T, N, 8)``."""
    T, N = x.shape[:2]
    return x.cpu().reshape(-1)[:T * N * 8].reshape(T, N, 8)

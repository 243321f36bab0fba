"""The LSTM baselines on the MI355X: the eval path (K4 image encoder, K7 encoders + fusion and head, the recurrence of
``csrc/lstm.hip``) against the reference's fixture and an fp64 composition, the persistent form against the loop of
launches bit for bit, the rerun after a persistent launch gives up, and a training step."""
import copy
import os
import warnings

import numpy as np
import pytest
import torch

from _tol import REL_TOL, rel_err

pytestmark = pytest.mark.gpu

OBS = ("image", "gripper_pos", "gripper_sensors")


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")


def _cls(task):
    import multimodalfilter_amd as mmf

    return {"door": mmf.door_models.DoorLSTMFilter, "push": mmf.push_models.PushLSTMFilter}[task]


def _inputs(T, N, seed, dev):
    g = torch.Generator().manual_seed(seed)
    t = {"image": torch.randn((T, N, 32, 32), generator=g), "gripper_pos": torch.randn((T, N, 3), generator=g),
         "gripper_sensors": torch.randn((T, N, 7), generator=g), "controls": torch.randn((T, N, 7), generator=g)}
    return {k: v.to(dev) for k, v in t.items()}


def _call(m, inp):
    return m.forward_loop(observations={k: inp[k] for k in OBS}, controls=inp["controls"])


def _torch_composition(m, inp, hidden):
    """The reference's forward_loop (lstm.py:62-100) on the module's own torch layers, in the module's dtype / device."""
    T, N = inp["image"].shape[:2]
    feat = m.observation_image_layers(inp["image"].reshape(T * N, 1, 32, 32)).reshape(T, N, m.units)
    merged = torch.cat((feat, m.observation_pos_layers(inp["gripper_pos"]), m.observation_sensors_layers(inp["gripper_sensors"]),
                        m.control_layers(inp["controls"])), dim=-1)
    out, hidden = m.lstm(m.fusion_layers(merged), hidden)
    return m.output_layers(out), hidden


@pytest.mark.parametrize("task", ["door", "push"])
def test_lstm_eval_matches_the_reference(task, golden_dir):
    """Two consecutive forward_loop calls (T = 5, then 4) after initialize_beliefs: outputs and (h, c) of both."""
    _need_gpu()
    dev = torch.device("cuda:0")
    z = np.load(os.path.join(golden_dir, "lstm.npz"))
    torch.manual_seed(0)
    m = _cls(task)().to(dev).eval()
    d = m.state_dim
    m.initialize_beliefs(mean=torch.zeros(3, d, device=dev), covariance=torch.eye(d, device=dev)[None].expand(3, d, d))
    assert m.lstm_hidden[0].shape == (2, 3, 512) and m.lstm_hidden[0].device == dev
    for i in range(2):
        inp = {k: torch.from_numpy(z[f"{task}/call{i}/{k}"]).to(dev) for k in OBS + ("controls",)}
        out = _call(m, inp)
        assert out.shape == z[f"{task}/call{i}/out"].shape
        assert rel_err(out, z[f"{task}/call{i}/out"]) <= REL_TOL, i
        assert rel_err(m.lstm_hidden[0], z[f"{task}/call{i}/h"], dims=1) <= REL_TOL, i
        assert rel_err(m.lstm_hidden[1], z[f"{task}/call{i}/c"], dims=1) <= REL_TOL, i


def test_lstm_eval_against_fp64_with_saturated_gates():
    """LSTM weights x 4 (gates saturate), T = 64, N = 37: the engine's error against an fp64 evaluation of the same torch
    modules stays within twice torch's own fp32 CPU error (+ 1e-6) -- a bar taken from the reference's rounding."""
    _need_gpu()
    dev = torch.device("cuda:0")
    torch.manual_seed(11)
    m = _cls("door")()
    with torch.no_grad():
        for p in m.lstm.parameters():
            p.mul_(4.0)
    T, N = 64, 37
    inp = _inputs(T, N, 5, "cpu")
    h0 = (0.5 * torch.randn(2, N, 512), 0.5 * torch.randn(2, N, 512))
    with torch.no_grad():
        ref64 = copy.deepcopy(m).double().eval()
        want, (hw, cw) = _torch_composition(ref64, {k: v.double() for k, v in inp.items()}, tuple(t.double() for t in h0))
        got32, (h32, c32) = _torch_composition(copy.deepcopy(m).eval(), inp, h0)
    g = m.to(dev).eval()
    g.lstm_hidden = tuple(t.to(dev) for t in h0)
    got = _call(g, {k: v.to(dev) for k, v in inp.items()})
    for name, e, t, w in (("out", got, got32, want), ("h", g.lstm_hidden[0], h32, hw), ("c", g.lstm_hidden[1], c32, cw)):
        err_engine, err_torch = rel_err(e, w, dims=1), rel_err(t, w, dims=1)
        assert err_engine <= 2 * err_torch + 1e-6, (name, err_engine, err_torch)


def _run_forms(N, T, seed=0):
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    torch.manual_seed(seed)
    lstm = torch.nn.LSTM(64, 512, 2).to(dev)
    packed = engine.packed_lstm(lstm)
    g = torch.Generator(device=dev).manual_seed(seed + 1)
    x = torch.randn((T, N, 64), generator=g, device=dev)
    h0 = torch.randn((2, N, 512), generator=g, device=dev)
    c0 = torch.randn((2, N, 512), generator=g, device=dev)
    taken = []
    real = _abi.lstm_forward

    def spy(a, like):
        taken.append(int(a.persistent))
        return real(a, like)

    _abi.lstm_forward = spy
    try:
        with engine.persistent_forms(lstm=True):
            pers = engine.run_lstm_loop(packed, x, h0, c0)
        with engine.persistent_forms(lstm=False):
            launches = engine.run_lstm_loop(packed, x, h0, c0)
    finally:
        _abi.lstm_forward = real
    with torch.no_grad():
        want, (hw, cw) = lstm(x, (h0, c0))
    return taken, pers, launches, (want, hw, cw)


@pytest.mark.parametrize("N,T", [(1, 1), (32, 17), (48, 17), (256, 9)])
def test_persistent_lstm_gives_the_bits_of_the_loop_of_launches(N, T):
    _need_gpu()
    from multimodalfilter_amd import _abi

    taken, pers, launches, want = _run_forms(N, T)
    assert taken == [1, 0], taken  # the persistent form did run first (plan > 0 for N <= 256)
    assert _abi.lstm_persistent_plan(N, T) > 0
    for a, b in zip(pers, launches):
        assert torch.equal(a, b)
    # and both are the recurrence nn.LSTM computes
    for got, w in zip(pers, want):
        assert rel_err(got, w, dims=1) <= REL_TOL


def test_lstm_beyond_the_persistent_size_runs_as_launches():
    _need_gpu()
    from multimodalfilter_amd import _abi

    taken, pers, launches, want = _run_forms(300, 3)
    assert _abi.lstm_persistent_plan(300, 3) == 0 and taken == [0, 0]
    for a, b in zip(pers, launches):
        assert torch.equal(a, b)
    for got, w in zip(pers, want):
        assert rel_err(got, w, dims=1) <= REL_TOL


def test_persistent_lstm_that_gives_up_is_rerun_as_a_loop_of_launches():
    """As the particle filter's: the first (persistent) C call is followed by scrambled outputs and the abort bit --
    outputs and final state must equal the launch path's bit for bit, one warning, and the next call stays on launches."""
    _need_gpu()
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    N, T = 8, 6
    torch.manual_seed(3)
    f = _cls("door")().to(dev).eval()
    inp = _inputs(T, N, 9, dev)
    d = f.state_dim
    cov = torch.eye(d, device=dev)[None].expand(N, d, d)

    def run(sabotage):
        taken = []
        real = _abi.lstm_forward

        def spy(a, like):
            taken.append(int(a.persistent))
            real(a, like)
            if sabotage and a.persistent:  # what an aborted launch leaves behind: garbage and the abort bit
                torch.cuda.synchronize()
                for name, rows in (("h2", T), ("hT", 2), ("cT", 2)):
                    ctypes_fill(getattr(a, name), rows * N * 512)
                engine.range_flag(dev).bitwise_or_(_abi.FLAG_GAVE_UP)

        _abi.lstm_forward = spy
        try:
            f.initialize_beliefs(mean=torch.zeros(N, d, device=dev), covariance=cov)
            with warnings.catch_warnings(record=True) as caught:
                warnings.simplefilter("always")
                out = _call(f, inp)
                out2 = _call(f, inp)
        finally:
            _abi.lstm_forward = real
        return taken, out, out2, [t.clone() for t in f.lstm_hidden], caught

    with engine.persistent_forms(lstm=False):
        taken_ref, ref, ref2, hid_ref, _ = run(False)
    with engine.persistent_forms(lstm=True):
        taken, out, out2, hid, caught = run(True)
        assert taken_ref == [0, 0]
        assert taken == [1, 0, 0], taken  # aborted persistent call, its rerun, then the next call on launches
        assert torch.equal(out, ref) and torch.equal(out2, ref2)
        assert all(torch.equal(a, b) for a, b in zip(hid, hid_ref))
        assert sum("gave up" in str(w.message) for w in caught) == 1
        assert engine.LSTM_PERSISTENT is False


def ctypes_fill(address: int, n: int):
    """Overwrite ``n`` floats of device memory at ``address`` with NaN bytes (the HIP runtime's own memset)."""
    import ctypes

    hip = ctypes.CDLL("libamdhip64.so")
    hip.hipMemset.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t]
    assert hip.hipMemset(ctypes.c_void_p(address), 0xFF, 4 * n) == 0
    torch.cuda.synchronize()


def test_lstm_training_step_matches_fp64_and_repacks():
    """train() with the autograd backend: ``train.train_filter_step`` gives the loss and gradients of an fp64 CPU run of
    the same modules; after the optimiser step an eval() forward_loop uses the new weights (the blob was re-packed)."""
    _need_gpu()
    from multimodalfilter_amd import engine, train

    dev = torch.device("cuda:0")
    N, L = 8, 4
    torch.manual_seed(21)
    m = _cls("door")()
    ref = copy.deepcopy(m).double().train()
    g = torch.Generator().manual_seed(4)
    batch = {"states": torch.randn((L, N, 3), generator=g), "image": torch.randn((L, N, 32, 32), generator=g),
             "gripper_pos": torch.randn((L, N, 3), generator=g), "gripper_sensors": torch.randn((L, N, 7), generator=g),
             "controls": torch.randn((L, N, 7), generator=g)}
    cov = torch.eye(3) * 0.1

    # fp64 CPU: the reference's loss (torchfilter.train.train_filter: zero state, forward_loop over [1:], MSE)
    b64 = {k: v.double() for k, v in batch.items()}
    hidden = (torch.zeros(2, N, 512, dtype=torch.float64), torch.zeros(2, N, 512, dtype=torch.float64))
    pred, _ = _torch_composition(ref, {k: b64[k][1:] for k in OBS + ("controls",)}, hidden)
    loss_ref = torch.mean((pred - b64["states"][1:]) ** 2)
    loss_ref.backward()

    m = m.to(dev).train()
    eval_before = None
    old = engine.TRAINING_BACKEND
    engine.set_training_backend("autograd")
    try:
        m.eval()
        m.initialize_beliefs(mean=torch.zeros(N, 3, device=dev), covariance=cov.to(dev)[None].expand(N, 3, 3))
        eval_before = _call(m, {k: batch[k][1:].to(dev) for k in OBS + ("controls",)})
        m.train()
        opt = torch.optim.SGD(m.parameters(), lr=0.5)
        grads = {}
        loss = train.train_filter_step(m, {k: v.to(dev) for k, v in batch.items()}, _GradKeeper(opt, m, grads),
                                       initial_covariance=cov.to(dev))
    finally:
        engine.set_training_backend(old)
    lref = float(loss_ref.detach())
    assert abs(loss - lref) <= 1e-4 * max(1.0, abs(lref))
    for (name, p_ref) in ref.named_parameters():
        gr = grads[name]
        scale = float(p_ref.grad.abs().max())
        if scale == 0.0:
            assert float(gr.abs().max()) == 0.0, name
            continue
        assert float((gr.double().cpu() - p_ref.grad).abs().max()) <= 1e-3 * scale, name

    # eval after the step: the new LSTM weights are in use (re-packed), i.e. the engine matches the updated modules
    m.eval()
    m.initialize_beliefs(mean=torch.zeros(N, 3, device=dev), covariance=cov.to(dev)[None].expand(N, 3, 3))
    inp = {k: batch[k][1:].to(dev) for k in OBS + ("controls",)}
    after = _call(m, inp)
    upd = copy.deepcopy(m).cpu().double().eval()
    with torch.no_grad():
        want, _ = _torch_composition(upd, {k: v.double().cpu() for k, v in inp.items()},
                                     (torch.zeros(2, N, 512, dtype=torch.float64), torch.zeros(2, N, 512, dtype=torch.float64)))
    assert rel_err(after, want) <= REL_TOL
    assert not torch.equal(after, eval_before)


class _GradKeeper:
    """An optimiser wrapper that records every parameter's gradient before stepping."""

    def __init__(self, opt, model, store):
        self.opt, self.model, self.store = opt, model, store

    def zero_grad(self, set_to_none=True):
        self.opt.zero_grad(set_to_none=set_to_none)

    def step(self):
        for name, p in self.model.named_parameters():
            self.store[name] = torch.zeros_like(p) if p.grad is None else p.grad.detach().clone()
        self.opt.step()

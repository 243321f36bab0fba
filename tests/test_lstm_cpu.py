"""The LSTM baselines without a GPU: construction against the reference's fixture, the registries, the host-side sizing
of ``mmf_lstm_*``, the argument struct against the header, the packed-blob cache, and the training formulation."""
import ctypes
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TASKS = ("door", "push")


def _golden(golden_dir):
    return np.load(os.path.join(golden_dir, "lstm.npz"))


def _cls(task):
    import multimodalfilter_amd as mmf

    return {"door": mmf.door_models.DoorLSTMFilter, "push": mmf.push_models.PushLSTMFilter}[task]


@pytest.mark.parametrize("task", TASKS)
def test_lstm_filter_matches_the_reference_construction(task, golden_dir):
    z = _golden(golden_dir)
    torch.manual_seed(0)
    m = _cls(task)()
    assert (m.lstm_hidden_dim, m.lstm_num_layers, m.units, m.image_rows, m.image_cols) == (512, 2, 64, 32, 32)
    assert m.state_dim == (3 if task == "door" else 2)
    sd = m.state_dict()
    assert sorted(sd) == list(z[f"{task}/keys"]) and len(sd) == 52
    for k, t in sd.items():
        flat = t.detach().double().flatten()
        got = np.concatenate([[float(flat.sum()), float(flat.abs().sum())], flat[:8].numpy()])
        want = z[f"{task}/fp/{k}"]
        # to fp32 rounding, not bit for bit: torch's vectorised uniform_ (the default initialisers) rounds the last bit
        # differently on CPUs of another vector width, and a reduction's order follows the thread count.  A construction
        # in another order draws other numbers altogether.
        np.testing.assert_allclose(got[2:], want[2:], rtol=1e-6, atol=1e-7, err_msg=k)
        np.testing.assert_allclose(got[1], want[1], rtol=1e-6, err_msg=k)
        np.testing.assert_allclose(got[0], want[0], rtol=0, atol=1e-6 * want[1], err_msg=k)


def test_lstm_filters_are_baselines_not_registered_filters():
    import multimodalfilter_amd as mmf

    for task, prefix in (("door", "Door"), ("push", "Push")):
        name = f"{prefix}LSTMFilter"
        assert mmf.baseline_types(task) == {name: _cls(task)}
        assert name not in mmf.model_types(task)
        assert _cls(task).__name__ == name


@pytest.mark.parametrize("task", TASKS)
def test_training_formulation_reproduces_the_reference_on_cpu(task, golden_dir):
    """The ``use_autograd`` path (torch modules, hidden state carried across calls) against the reference's outputs."""
    from multimodalfilter_amd import engine

    z = _golden(golden_dir)
    torch.manual_seed(0)
    m = _cls(task)().train()
    d = m.state_dim
    old = engine.TRAINING_BACKEND
    engine.set_training_backend("autograd")
    try:
        m.initialize_beliefs(mean=torch.zeros(3, d), covariance=torch.eye(d)[None].expand(3, d, d))
        for i in range(2):
            inp = {k: torch.from_numpy(z[f"{task}/call{i}/{k}"]) for k in ("image", "gripper_pos", "gripper_sensors", "controls")}
            out = m.forward_loop(observations={k: inp[k] for k in ("image", "gripper_pos", "gripper_sensors")},
                                 controls=inp["controls"])
            np.testing.assert_allclose(out.detach().numpy(), z[f"{task}/call{i}/out"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(m.lstm_hidden[0].detach().numpy(), z[f"{task}/call{i}/h"], rtol=0, atol=1e-5)
            np.testing.assert_allclose(m.lstm_hidden[1].detach().numpy(), z[f"{task}/call{i}/c"], rtol=0, atol=1e-5)
    finally:
        engine.set_training_backend(old)


def test_lstm_sizing_needs_no_gpu():
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    for in_dim in (8, 64, 512):
        # per layer 64 workgroups x 32 gate rows x K (K_0 = in_dim + 512, K_1 = 1024), then 2 x 2048 summed biases
        assert lib.mmf_lstm_blob_floats(in_dim) == 2048 * (in_dim + 512) + 2048 * 1024 + 2 * 2048
    assert lib.mmf_lstm_blob_floats(64) == 2048 * 1602
    for bad in (0, -8, 7, 12, 520):
        assert lib.mmf_lstm_blob_floats(bad) == 0
    # [abort word, padded to 16 B][64 progress words][2 layers][2 parities][512][N] 8-byte granules
    for N in (1, 32, 256, 1000):
        assert lib.mmf_lstm_sync_words(N) == 4 + 64 + 2 * 2 * 2 * 512 * N
    assert lib.mmf_lstm_sync_words(0) == 0
    # without a device nothing is eligible; nonsense is refused
    assert lib.mmf_lstm_persistent_plan(32, 256) == 0
    assert lib.mmf_lstm_persistent_plan(0, 5) == -1 and lib.mmf_lstm_persistent_plan(5, 0) == -1
    assert lib.mmf_lstm_persistent_plan(-3, -1) == -1
    args = _abi.MmfLstmArgs()
    assert lib.mmf_lstm_forward(None, None) == -1
    assert lib.mmf_lstm_forward(ctypes.byref(args), None) == -1  # N = 0, null pointers: refused before any HIP call
    assert lib.mmf_lstm_pack(*([None] * 9), 64, None) == -1


def test_lstm_args_struct_matches_the_header(tmp_path):
    """``MmfLstmArgs`` of the binding against the C header (gcc prints ``sizeof`` / ``offsetof``)."""
    import shutil
    import subprocess

    from multimodalfilter_amd import _abi

    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    cls = _abi.MmfLstmArgs
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(MmfLstmArgs));']
    for field, _t in cls._fields_:
        lines.append(f'  printf("{field} %zu\\n", offsetof(MmfLstmArgs, {field}));')
    lines += ["  return 0;", "}"]
    src = tmp_path / "lstm_layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "lstm_layout"
    out = subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for field, _t in cls._fields_:
        assert int(got[field]) == getattr(cls, field).offset, field
    last, last_t = cls._fields_[-1]
    assert getattr(cls, last).offset + ctypes.sizeof(last_t) == ctypes.sizeof(cls)
    assert [n for n, _ in cls._fields_][:4] == ["T", "N", "in_dim", "persistent"]


def test_packed_lstm_blob_is_rebuilt_exactly_when_an_lstm_tensor_changes(monkeypatch):
    """``engine.PackedLstm`` goes through ``utils.cached``: the same blob while the eight tensors are untouched; a new pack
    after an in-place update of any one of them (optimiser step, graph replay's version bump), a replacement
    (``load_state_dict``) -- and not after a change to a parameter outside the LSTM."""
    from multimodalfilter_amd import _abi, engine

    packs = []

    def fake_pack(self, src):
        packs.append(1)
        return torch.zeros(1)

    monkeypatch.setattr(engine.PackedLstm, "_pack", fake_pack)
    m = _cls("door")()
    p = engine.packed_lstm(m.lstm)
    assert engine.packed_lstm(m.lstm) is p
    b = p.blob()
    assert p.blob() is b and len(packs) == 1
    with torch.no_grad():
        m.output_layers[0].weight.add_(1.0)  # not an LSTM tensor
    assert p.blob() is b and len(packs) == 1
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1"]
    for i, name in enumerate(names):
        with torch.no_grad():
            getattr(m.lstm, name).mul_(0.5)
        b2 = p.blob()
        assert b2 is not b and len(packs) == 2 + i, name
        assert p.blob() is b2 and len(packs) == 2 + i, name
        b = b2
    torch.autograd.graph.increment_version(m.lstm.bias_hh_l1)  # what GraphedFilterStep does after a replay
    p.blob()
    assert len(packs) == 2 + len(names)
    m.lstm.load_state_dict({k: v.clone() for k, v in m.lstm.state_dict().items()})
    p.blob()
    assert len(packs) == 3 + len(names)
    assert _abi.LSTM_HIDDEN == 512 and _abi.LSTM_LAYERS == 2


def test_design_quotes_the_committed_lstm_measurement():
    """DESIGN.md's LSTM paragraph and the README's switch table against ``profiles/lstm/bench_lstm.json``: a re-measure
    that is not followed by a doc update fails here, and the default form is the one the A/B found faster."""
    import json

    with open(os.path.join(ROOT, "profiles", "lstm", "bench_lstm.json")) as fh:
        line = json.loads([l for l in fh.read().splitlines() if l.startswith("{")][-1])
    with open(os.path.join(ROOT, "DESIGN.md")) as fh:
        design = fh.read()
    legs = line["legs"]
    for key in ("persistent_N32", "launches_N32", "torch_N32", "persistent_N256", "launches_N256", "torch_N256"):
        assert f"{legs[key] * 1e3:.1f} µs" in design, key
    for p in line["profile"]:
        assert f"{p['lstm_kernel_share_of_gpu_time'] * 100:.0f} %" in design
    from multimodalfilter_amd import engine

    faster = legs["persistent_vs_launches_N32"] < 1.0 and legs["persistent_vs_launches_N256"] < 1.0
    assert ("MMF_LSTM_PERSISTENT=1" in design) == faster
    with open(os.path.join(ROOT, "README.md")) as fh:
        assert "| `MMF_LSTM_PERSISTENT` | 1 |" in fh.read()
    if os.environ.get("MMF_LSTM_PERSISTENT") is None:
        assert engine.LSTM_PERSISTENT == faster

#!/usr/bin/env python3
"""Generate ``tests/golden/lstm.npz`` from the REFERENCE's own LSTM baselines (``crossmodal/door_models/lstm.py``,
``push_models/lstm.py``), imported with ``oracle.capture_golden.import_reference_crossmodal()``.

Runs in the build container only: the reference does not travel, only the vectors written here.  Per task, at
``N = 3``: the inputs of two consecutive ``forward_loop`` calls (``T = 5``, then ``T = 4``) after ``initialize_beliefs``,
the reference's outputs of both calls and its ``lstm_hidden`` after each, the sorted ``state_dict`` keys, and a
fingerprint of every parameter under ``torch.manual_seed(0)`` (sum, absolute sum, first 8 values) -- not the 3.9 M
weights themselves: a model built under the same seed in the reference's order has the same weights.

    python scripts/capture_lstm_golden.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "lstm.npz")
N, T_CALLS = 3, (5, 4)


def make_inputs(rng, T, d_ctrl=7):
    return {"image": rng.standard_normal((T, N, 32, 32)).astype(np.float32),
            "gripper_pos": rng.standard_normal((T, N, 3)).astype(np.float32),
            "gripper_sensors": rng.standard_normal((T, N, 7)).astype(np.float32),
            "controls": rng.standard_normal((T, N, d_ctrl)).astype(np.float32)}


def fingerprint(t: torch.Tensor) -> np.ndarray:
    flat = t.detach().double().flatten()
    return np.concatenate([[float(flat.sum()), float(flat.abs().sum())], flat[:8].numpy()]).astype(np.float64)


def main():
    from oracle.capture_golden import import_reference_crossmodal

    cm = import_reference_crossmodal()
    blob = {}
    for task, cls, d in (("door", cm.door_models.DoorLSTMFilter, 3), ("push", cm.push_models.PushLSTMFilter, 2)):
        torch.manual_seed(0)
        model = cls()
        model.eval()
        sd = model.state_dict()
        keys = sorted(sd)
        blob[f"{task}/keys"] = np.array(keys)
        for k in keys:
            blob[f"{task}/fp/{k}"] = fingerprint(sd[k])
        rng = np.random.RandomState(7 if task == "door" else 8)
        with torch.no_grad():
            model.initialize_beliefs(mean=torch.zeros(N, d), covariance=torch.eye(d)[None].expand(N, d, d))
            for i, T in enumerate(T_CALLS):
                inp = make_inputs(rng, T)
                for k, v in inp.items():
                    blob[f"{task}/call{i}/{k}"] = v
                t = {k: torch.from_numpy(v) for k, v in inp.items()}
                out = model.forward_loop(observations={k: t[k] for k in ("image", "gripper_pos", "gripper_sensors")},
                                         controls=t["controls"])
                assert out.shape == (T, N, d)
                blob[f"{task}/call{i}/out"] = out.numpy()
                blob[f"{task}/call{i}/h"] = model.lstm_hidden[0].numpy()
                blob[f"{task}/call{i}/c"] = model.lstm_hidden[1].numpy()
    np.savez_compressed(OUT, **blob)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()

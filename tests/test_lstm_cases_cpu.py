"""Certifies, without a GPU, what ``test_gpu_lstm_kernel.py`` holds the recurrence kernel to (``_lstm_cases.py``): that the
written-out fp64 recurrence IS ``nn.LSTM`` in fp64, that the small-signal families really run with small cell states, that
torch's fp32 ``nn.LSTM`` -- the yardstick of the GPU test's error rule -- is itself within 1e-5 of the truth, and that the rule
tells the tanh ``2 sigmoid(2x) - 1`` from ``mmf_det_tanh`` on an fp32 emulation of the recurrence.

The caps are conditions on the INPUTS: a seed that breaks one is replaced, the cap stays."""
import numpy as np
import pytest
import torch

import _lstm_cases as lc
from _tol import REL_TOL, rel_err

CASES = lc.all_cases()
NAMES = ("h2", "hT", "cT")


def test_the_case_list_covers_what_it_claims():
    shapes = lc.shapes()
    assert len(shapes) == len(set(shapes)) == 19
    for d in lc.IN_DIMS:
        assert (d, 33, 3) in shapes
        assert {n for dd, n, _ in shapes if dd == d} == set(lc.NS) and {t for dd, _, t in shapes if dd == d} == set(lc.TS)
    for n in lc.NS:
        assert {t for _, nn, t in shapes if nn == n} == set(lc.TS)
    assert len(CASES) == len(set(CASES)) == 4 * 19 + 16
    assert {c[0] for c in CASES} == set(lc.FAMILIES)
    assert all(t == 1 for f, _, _, t in CASES if f == "zero_state")
    # ordered by the weights they run on: each (in_dim, variant) is one contiguous stretch
    keys = [(c[1], lc.VARIANT[c[0]]) for c in CASES]
    assert len([k for i, k in enumerate(keys) if i == 0 or keys[i - 1] != k]) == len(set(keys)) == 12


def test_the_weight_variants():
    base, x4, zb = (lc.tensors(24, v) for v in ("default", "times4", "zero_bias"))
    bound = 1.0 / np.sqrt(lc.H)                      # nn.LSTM: U(-1 / sqrt(hidden), 1 / sqrt(hidden))
    for name, b, s, z in zip(lc.TENSOR_NAMES, base, x4, zb):
        assert b.dtype == torch.float32 and float(b.abs().max()) <= bound and float(b.abs().max()) > 0.9 * bound
        assert torch.equal(s, 4.0 * b)
        assert torch.equal(z, torch.zeros_like(b) if name.startswith("bias") else b)
    assert [tuple(t.shape) for t in base] == [(2048, 24), (2048, 512), (2048,), (2048,), (2048, 512), (2048, 512), (2048,), (2048,)]
    m = lc.module(24, base, torch.float64)
    assert all(torch.equal(getattr(m, n), t.double()) for n, t in zip(lc.TENSOR_NAMES, base))


@pytest.mark.parametrize("c", CASES, ids=lc.case_id)
def test_reference_and_yardstick(c):
    """The written-out recurrence against ``nn.LSTM(...).double()`` on the CPU to 1e-12; torch's fp32 ``nn.LSTM`` against it
    finite and within 1e-5 -- so ``2 x err_torch + 1e-6`` is a bar of a few 1e-6 at most, and the reference itself meets it;
    the regime each family names."""
    family, in_dim, N, T = c
    k = lc.case(*c)
    assert k.x.shape == (T, N, in_dim) and k.h0.shape == k.c0.shape == (2, N, lc.H) and k.x.dtype == torch.float32
    with torch.no_grad():
        want = lc.module(in_dim, k.tensors(), torch.float64)(k.x.double(), (k.h0.double(), k.c0.double()))
    want = (want[0], want[1][0], want[1][1])
    for name, got, w, t32 in zip(NAMES, k.truth, want, k.fp32):
        assert got.shape == w.shape and got.dtype == torch.float64 and bool(torch.isfinite(got).all()), name
        assert rel_err(got, w, dims=1) <= 1e-12, (name, rel_err(got, w, dims=1))
        e = rel_err(t32, got, dims=1)
        assert bool(torch.isfinite(t32).all()) and e <= lc.FP32_CAP, (name, e)
        assert lc.bar(e) <= 0.3 * REL_TOL
    assert np.array_equal(k.cells[:, -1], k.truth[2].numpy()) and torch.equal(k.truth[0][-1], k.truth[1][1])
    if family in lc.SMALL_SIGNAL:
        factor = lc.SMALL_SIGNAL[family]
        assert all(float(b.abs().max()) == 0.0 for n, b in zip(lc.TENSOR_NAMES, k.tensors()) if n.startswith("bias"))
        for layer in range(2):
            med = float(np.median(np.abs(k.cells[layer])))
            assert 0.0 < med < 10.0 * factor, (layer, med)
    if family == "zero_state":
        assert T == 1 and float(k.h0.abs().max()) == 0.0 and float(k.c0.abs().max()) == 0.0
    if family == "saturated":  # a tenth of the first step's gates beyond |pre| = 3, where sigma is within 5 % of 0 or 1
        w_ih, w_hh, b_ih, b_hh = (t.double() for t in k.tensors()[:4])
        pre = k.x[0].double() @ w_ih.T + k.h0[0].double() @ w_hh.T + b_ih + b_hh
        assert float((pre.abs() > 3.0).double().mean()) > 0.1


def test_old_tanh_form_is_the_fused_expression():
    from oracle import strict

    x = np.concatenate([np.linspace(-12, 12, 4001), [1e-4, -1e-4, 0.0]]).astype(np.float32)
    s = strict.det_sigmoid(2.0 * x).astype(np.float64)
    assert np.array_equal(lc.old_det_tanh(x), np.array([np.float32(2.0 * v - 1.0) for v in s]))
    assert np.max(np.abs(lc.old_det_tanh(x) - np.tanh(x.astype(np.float64)))) <= 7e-7     # its documented ABSOLUTE error


@pytest.mark.parametrize("c", [("small_signal_1e-4", 8, 33, 3), ("small_signal_1e-4", 512, 257, 2)], ids=lc.case_id)
def test_the_bar_discriminates_between_the_two_tanh_forms(c):
    """An fp32 emulation of the recurrence (fp64 dot products rounded to fp32, the deterministic sigmoid) with
    ``2 sigmoid(2x) - 1`` for tanh breaches ``2 x err_torch + 1e-6`` on the 1e-4 small-signal case -- by more than the
    project's whole 1e-4 bar -- and meets it with ``mmf_det_tanh``."""
    from oracle import strict

    k = lc.case(*c)
    old = lc.emulate_fp32(k.x, k.h0, k.c0, k.tensors(), lc.old_det_tanh)
    new = lc.emulate_fp32(k.x, k.h0, k.c0, k.tensors(), strict.det_tanh)
    for name, o, n, want, t32 in zip(NAMES, old, new, k.truth, k.fp32):
        limit = lc.bar(rel_err(t32, want, dims=1))
        e_old, e_new = rel_err(o, want, dims=1), rel_err(n, want, dims=1)
        print(f"{lc.case_id(c)} {name}: old tanh {e_old:.3e}, mmf_det_tanh {e_new:.3e}, bar {limit:.3e}")
        assert e_new <= limit, (name, e_new, limit)
        assert e_old > limit and e_old > REL_TOL, (name, e_old, limit)


@pytest.mark.parametrize("c", [("plain", 24, 33, 5), ("saturated", 64, 33, 3), ("small_signal_1e-3", 8, 31, 2), ("zero_state", 8, 1, 1)],
                         ids=lc.case_id)
def test_the_emulation_with_the_new_tanh_meets_the_bar_in_every_family(c):
    """The bar is one an fp32 evaluation with the project's own activations CAN meet, whatever the family."""
    from oracle import strict

    k = lc.case(*c)
    got = lc.emulate_fp32(k.x, k.h0, k.c0, k.tensors(), strict.det_tanh)
    for name, g, want, t32 in zip(NAMES, got, k.truth, k.fp32):
        assert rel_err(g, want, dims=1) <= lc.bar(rel_err(t32, want, dims=1)), name


@pytest.mark.parametrize("in_dim", [8, 512])
def test_packed_layout_restatement(in_dim):
    """``packed_layout`` on tensors whose value IS their position: element ``[g][k][q]`` of a layer's weights must be
    entry (row gate * 512 + 8 g + j, column k) of ``[W_ih | W_hh]``, and the size what ``mmf_lstm_blob_floats`` says."""
    K0 = in_dim + 512
    ts = []
    for l, K_in in enumerate((in_dim, 512)):
        w = (np.arange(2048)[:, None] * 2048 + np.arange(K_in + 512)[None, :] + l * 2 ** 23).astype(np.float32)   # exact: < 2^24
        ts += [w[:, :K_in].copy(), w[:, K_in:].copy(), np.arange(2048, dtype=np.float32), 3.0 * np.arange(2048, dtype=np.float32)]
    blob = lc.packed_layout(ts, in_dim)
    assert blob.shape == (2048 * (K0 + 1024 + 2),) and blob.dtype == np.float32
    for l, g, k, q in ((0, 0, 0, 0), (0, 5, 3, 9), (0, 63, K0 - 1, 31), (1, 0, 0, 0), (1, 17, 600, 22), (1, 63, 1023, 31)):
        K = K0 if l == 0 else 1024
        at = (2048 * K0 if l else 0) + g * 32 * K + k * 32 + q
        row = (q // 8) * 512 + 8 * g + q % 8
        assert blob[at] == row * 2048 + k + l * 2 ** 23, (l, g, k, q)
        assert blob[2048 * (K0 + 1024) + l * 2048 + g * 32 + q] == 4.0 * row

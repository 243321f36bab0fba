"""Input families and references for the recurrence kernel of the LSTM baselines (``csrc/lstm.hip``): pure numpy / torch-CPU,
shared by ``test_lstm_cases_cpu.py`` (which certifies the inputs and the references without a GPU) and
``test_gpu_lstm_kernel.py`` (which runs the kernel on them).

The truth is ``reference``: the two-layer recurrence written out in fp64 numpy -- gate order i, f, g, o of
``W_ih x + b_ih + W_hh h + b_hh``, ``c' = f c + i g``, ``h' = o tanh(c')`` -- which does NOT go through ``nn.LSTM``; the CPU
test pins it to ``nn.LSTM(...).double()`` to 1e-12.  The yardstick of the GPU test's error rule is torch's fp32 CPU
``nn.LSTM`` on the same tensors (``Case.fp32``).  ``emulate_fp32`` is an fp32 evaluation of the same recurrence with the
project's deterministic activations, the tanh exchangeable: it shows without a GPU that the error rule tells the tanh
``2 sigmoid(2x) - 1`` from one that is accurate relatively.

Every case is built once (``functools.lru_cache``) and shared: no test writes to one.  The weights, 10 to 17 MB a set, are kept for
the two most recent ``(in_dim, variant)`` only, so ``all_cases()`` is ordered by them.
"""
import functools
from typing import NamedTuple, Tuple

import numpy as np
import torch

H = 512
LAYERS = 2
IN_DIMS = (8, 24, 64, 512)   # K_0 = 520: 65 k pairs per wave, a tail of 1 in the 32-wide operand batches; 24; the model's; K_0 = 1024
NS = (1, 31, 33, 257)        # one column; one short of / one past a 32-column tile; one column in the second column group
TS = (1, 2, 3, 5)            # 3 and 5 wrap both parity slots and open layer 0's progress wait (s >= 2)
TENSOR_NAMES = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0", "weight_ih_l1", "weight_hh_l1", "bias_ih_l1", "bias_hh_l1")
SMALL_SIGNAL = {"small_signal_1e-3": 1e-3, "small_signal_1e-4": 1e-4}
FAMILIES = ("plain", "saturated") + tuple(SMALL_SIGNAL) + ("zero_state",)
# which weights a family runs on: nn.LSTM's default initialisation as drawn, x 4, or with the four biases zeroed
VARIANT = {"plain": "default", "zero_state": "default", "saturated": "times4", "small_signal_1e-3": "zero_bias", "small_signal_1e-4": "zero_bias"}
FP32_CAP = 1e-5              # torch's fp32 CPU nn.LSTM against the truth, norm-wise: a condition on the INPUTS


def shapes():
    """``(in_dim, N, T)``: a 4 x 4 Latin square (T index = in_dim index + N index mod 4: every pair of values of two axes
    occurs) plus the remaining in_dim at N = 33, T = 3.  So: every in_dim at N = 33, T = 3; every N at every in_dim;
    every T at every N and at every in_dim."""
    out = [(d, n, TS[(i + j) % 4]) for i, d in enumerate(IN_DIMS) for j, n in enumerate(NS)]
    out += [(d, 33, 3) for d in IN_DIMS if (d, 33, 3) not in out]
    return out


def all_cases():
    """``(family, in_dim, N, T)`` of every case, ordered by the weights they run on.  ``zero_state`` is a T = 1 family: it
    takes every ``(in_dim, N)`` of ``shapes()`` once."""
    out = []
    for d in IN_DIMS:
        for variant in ("default", "times4", "zero_bias"):
            for family in FAMILIES:
                if VARIANT[family] != variant:
                    continue
                if family == "zero_state":
                    out += [(family, d, n, 1) for n in NS]
                else:
                    out += [(family, dd, n, t) for dd, n, t in shapes() if dd == d]
    return out


def case_id(c):
    return "{}-in{}-N{}-T{}".format(*c)


@functools.lru_cache(maxsize=2)
def tensors(in_dim, variant, seed=0):
    """The eight tensors of ``nn.LSTM(in_dim, 512, 2)`` (``TENSOR_NAMES`` order, float32) as its constructor initialises
    them under ``torch.manual_seed``, the global generator left as it was; ``variant``: see ``VARIANT``."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(7919 * seed + in_dim)
        m = torch.nn.LSTM(in_dim, H, LAYERS)
    out = []
    for name in TENSOR_NAMES:
        t = getattr(m, name).detach().clone()
        if variant == "times4":
            t *= 4.0
        elif variant == "zero_bias" and name.startswith("bias"):
            t.zero_()
        else:
            assert variant in ("default", "times4", "zero_bias"), variant
        out.append(t)
    return tuple(out)


def module(in_dim, ts, dtype=torch.float32):
    """An ``nn.LSTM(in_dim, 512, 2)`` on the CPU that holds (copies of) the eight tensors ``ts`` in ``dtype``."""
    with torch.random.fork_rng(devices=[]):  # (its constructor draws an initialisation: the global generator stays as it was)
        m = torch.nn.LSTM(in_dim, H, LAYERS)
    with torch.no_grad():
        for name, t in zip(TENSOR_NAMES, ts):
            getattr(m, name).copy_(t)
    return m.to(dtype)


# ------------------------------------------------------------------------------ the recurrence, written out
def _sigmoid64(v):
    e = np.exp(-np.abs(v))
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _recurrence(x, h0, c0, ts, *, pre, sigmoid, tanh, cell, mul):
    """Both layers over the whole sequence.  ``pre(inp, h, w_ih, w_hh, b_ih, b_hh)`` -> ``(N, 2048)`` gate pre-activations;
    ``cell(f, c, i, g)`` -> ``c'``; ``mul(o, t)`` -> ``h'``.  Returns ``h2 (T, N, 512)``, ``hT``, ``cT (2, N, 512)`` and the
    cell states of every step ``(2, T, N, 512)``."""
    T, N = x.shape[:2]
    inp, hT, cT, cells = x, [], [], []
    for l in range(LAYERS):
        w_ih, w_hh, b_ih, b_hh = ts[4 * l:4 * l + 4]
        h, c, hs, cs = h0[l], c0[l], [], []
        for s in range(T):
            p = pre(inp[s], h, w_ih, w_hh, b_ih, b_hh)
            i, f, g, o = (p[:, k * H:(k + 1) * H] for k in range(4))
            c = cell(sigmoid(f), c, sigmoid(i), tanh(g))
            h = mul(sigmoid(o), tanh(c))
            hs.append(h)
            cs.append(c)
        inp = np.stack(hs) if hs else np.zeros((0, N, H), dtype=h0.dtype)
        cells.append(np.stack(cs) if cs else np.zeros((0, N, H), dtype=h0.dtype))
        hT.append(h)
        cT.append(c)
    return inp, np.stack(hT), np.stack(cT), np.stack(cells)


def _np(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=dtype)


def _reference_with_cells(x, h0, c0, ts):
    d = np.float64
    return _recurrence(_np(x, d), _np(h0, d), _np(c0, d), [_np(t, d) for t in ts],
                       pre=lambda a, h, w_ih, w_hh, b_ih, b_hh: a @ w_ih.T + b_ih + h @ w_hh.T + b_hh,
                       sigmoid=_sigmoid64, tanh=np.tanh, cell=lambda f, c, i, g: f * c + i * g, mul=lambda o, t: o * t)


def reference(x, h0, c0, ts):
    """``(h2, hT, cT)`` in fp64 (numpy) of ``x (T, N, in_dim)``, ``h0`` / ``c0 (2, N, 512)`` and the eight tensors."""
    return _reference_with_cells(x, h0, c0, ts)[:3]


def old_det_tanh(v):
    """``fmaf(2, mmf_det_sigmoid(2 v), -1)``, the tanh ``csrc/lstm.hip`` used to evaluate: ``2 s`` is exact, so one rounding
    of the fp64 difference is the fused operation."""
    from oracle import strict

    s = strict.det_sigmoid((np.float32(2.0) * np.asarray(v, dtype=np.float32)).astype(np.float32))
    return (2.0 * s.astype(np.float64) - 1.0).astype(np.float32)


def emulate_fp32(x, h0, c0, ts, tanh):
    """The recurrence in fp32 as the kernel forms it, up to the order of the dot products: each gate pre-activation is the
    fp64 product sum rounded to fp32 plus the fp32 ``b_ih + b_hh``; sigma is ``oracle.strict.det_sigmoid``; ``tanh`` is the
    form under test (float32 array -> float32 array); ``c' = fmaf(f, c, i g)``, ``h' = o tanh(c')``, every result rounded
    to fp32.  Returns ``(h2, hT, cT)`` as float32."""
    from oracle import strict

    f32, f64 = np.float32, np.float64

    def pre(a, h, w_ih, w_hh, b_ih, b_hh):
        dots = (a.astype(f64) @ w_ih.astype(f64).T + h.astype(f64) @ w_hh.astype(f64).T).astype(f32)
        return (dots + (b_ih + b_hh).astype(f32)).astype(f32)

    def cell(f, c, i, g):
        ig = (i * g).astype(f32)
        return (f.astype(f64) * c.astype(f64) + ig.astype(f64)).astype(f32)   # the product of two fp32 is exact in fp64

    return _recurrence(_np(x, f32), _np(h0, f32), _np(c0, f32), [_np(t, f32) for t in ts], pre=pre,
                       sigmoid=lambda v: strict.det_sigmoid(np.ascontiguousarray(v)), tanh=lambda v: tanh(np.ascontiguousarray(v)),
                       cell=cell, mul=lambda o, t: (o * t).astype(f32))[:3]


# ------------------------------------------------------------------------------ the cases
class Case(NamedTuple):
    family: str
    in_dim: int
    variant: str
    seed: int
    x: torch.Tensor                   # (T, N, in_dim) float32
    h0: torch.Tensor                  # (2, N, 512) float32
    c0: torch.Tensor
    truth: Tuple[torch.Tensor, ...]   # (h2, hT, cT) in fp64: ``reference``
    cells: np.ndarray                 # (2, T, N, 512): the truth's cell state after every step
    fp32: Tuple[torch.Tensor, ...]    # (h2, hT, cT) of torch's fp32 CPU nn.LSTM

    def tensors(self):
        return tensors(self.in_dim, self.variant, self.seed)


def _frozen(a):
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(family, in_dim, N, T, seed=0):
    """One case of ``family`` (``FAMILIES``) at ``(in_dim, N, T)``:
    ``plain``: default ``nn.LSTM`` initialisation, ``x``, ``h0``, ``c0`` ~ N(0, 1);  ``saturated``: the same with every LSTM
    tensor x 4;  ``small_signal_F``: default weights, the biases zeroed, ``x``, ``h0``, ``c0`` ~ F N(0, 1);  ``zero_state``:
    ``plain`` with ``h0 = c0 = 0`` at T = 1 (the ``s == 0`` branch of the kernel's operand load and its ``s == T - 1``
    write in the same step)."""
    assert family in FAMILIES and (family != "zero_state" or T == 1), (family, T)
    g = torch.Generator().manual_seed(1 + 104729 * seed + 1009 * FAMILIES.index(family) + 101 * in_dim + 11 * N + T)
    x = torch.randn((T, N, in_dim), generator=g)
    h0 = torch.randn((LAYERS, N, H), generator=g)
    c0 = torch.randn((LAYERS, N, H), generator=g)
    if family in SMALL_SIGNAL:
        x, h0, c0 = (t * SMALL_SIGNAL[family] for t in (x, h0, c0))
    if family == "zero_state":
        h0, c0 = torch.zeros_like(h0), torch.zeros_like(c0)
    variant = VARIANT[family]
    ts = tensors(in_dim, variant, seed)
    h2, hT, cT, cells = _reference_with_cells(x, h0, c0, ts)
    with torch.no_grad():
        o32, (h32, c32) = module(in_dim, ts)(x, (h0, c0))
    truth = tuple(torch.from_numpy(a) for a in (h2, hT, cT))
    return Case(family, in_dim, variant, seed, x, h0, c0, truth, _frozen(cells), (o32, h32, c32))


def bar(err_torch):
    """The engine's error against fp64 may be twice torch's own fp32 CPU error, + 1e-6: the rule of
    ``test_gpu_lstm.py::test_lstm_eval_against_fp64_with_saturated_gates``."""
    return 2.0 * err_torch + 1e-6


# ------------------------------------------------------------------------------ the packed layout
def packed_layout(ts, in_dim):
    """``mmf_lstm_pack``'s blob restated from ``include/mmf.h``: per layer l (K_0 = in_dim + 512, K_1 = 1024), per
    workgroup g < 64, 32 x K_l floats ``[k / 2][k & 1][row q]`` with q = gate * 8 + j standing for row
    ``gate * 512 + 8 g + j`` of ``[W_ih | W_hh]``; then ``b_ih + b_hh`` (an fp32 sum) per layer as ``[g][q]``."""
    ts = [_np(t, np.float32) for t in ts]
    q = np.arange(32)
    parts, biases = [], []
    for l in range(LAYERS):
        w_ih, w_hh, b_ih, b_hh = ts[4 * l:4 * l + 4]
        w = np.concatenate([w_ih, w_hh], axis=1)                       # (2048, K_l)
        K = w.shape[1]
        assert K == (in_dim + H if l == 0 else 2 * H)
        b = (b_ih + b_hh).astype(np.float32)
        for g in range(H // 8):
            rows = (q // 8) * H + 8 * g + q % 8
            block = np.empty((K // 2, 2, 32), dtype=np.float32)
            for k in range(K):
                block[k // 2, k & 1, :] = w[rows, k]
            parts.append(block.ravel())
            biases.append(b[rows])
    return np.concatenate(parts + biases)

"""``mmf_pf_set_nll`` (csrc/pf_set_loss.hip) against the fp64 reference of ``_set_loss_cases``: the mixture log score of a
weighted particle set and its closed-form gradients, held to ``_tol.REL_TOL`` on every case of the family (whose fairness
``test_set_loss_cases_cpu.py`` asserts), with the exact zeros, the exact scaling and the bit-for-bit properties of the header."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _set_loss_cases as lc
from _tol import REL_TOL

DEV = "cuda:0"
SHAPE = {"nll": lambda R, M, d: (R,), "g_states": lambda R, M, d: (R, M, d), "g_logw": lambda R, M, d: (R, M),
         "g_log_scale": lambda R, M, d: (R, d)}


def run_kernel(case, outputs=lc.OUTPUTS, g_nll=None, rows=None):
    """The kernel on a case (``rows``: a slice of its rows) -> ``{name: numpy}`` of the outputs asked for.  Every output is
    allocated with ``GUARD_ROWS`` rows of ``SENTINEL`` behind it, which must come back untouched."""
    from multimodalfilter_amd import _abi

    sl = slice(None) if rows is None else rows
    X, A, Y = (torch.from_numpy(np.ascontiguousarray(case[k][sl])).to(DEV) for k in ("states", "logw", "truth"))
    s = torch.from_numpy(case["scale"]).to(DEV)
    R, M, d = X.shape
    g = None if g_nll is None else torch.from_numpy(np.ascontiguousarray(np.asarray(g_nll, np.float32)[sl])).to(DEV)
    bufs = {name: torch.full((R + lc.GUARD_ROWS,) + SHAPE[name](R, M, d)[1:], lc.SENTINEL, dtype=torch.float32, device=DEV) for name in outputs}
    _abi.pf_set_nll(X, A, Y, s, g, **{name: b[:R] for name, b in bufs.items()})
    out = {}
    for name, b in bufs.items():
        b = b.cpu().numpy()
        assert (b[R:] == np.float32(lc.SENTINEL)).all(), (name, "wrote behind its last row")
        out[name] = b[:R]
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("M", lc.ALL_MS)
def test_set_nll_kernel_matches_the_fp64_reference(M):
    """Forward call (``nll`` alone) and backward call (the three gradients alone) on every case of the family at this ``M``:
    ``nll`` and ``g_log_scale`` under ``rel_err_elementwise(floor=1e-3)``, ``g_states`` and ``g_logw`` under ``rel_err``, all below
    ``REL_TOL``; NaN exactly where the definition puts it; exact zeros at dead particles and on rows whose ``nll`` is NaN."""
    worst = {name: 0.0 for name in lc.OUTPUTS}
    n = 0
    for c in lc.family():
        if c[0] != M:
            continue
        case, ref = lc.family_case(*c)
        got = run_kernel(case, ("nll",))
        got.update(run_kernel(case, ("g_states", "g_logw", "g_log_scale")))
        for name in lc.OUTPUTS:
            err = lc.compare(got[name], ref[name], name, c)
            worst[name] = max(worst[name], err)
            assert err < REL_TOL, (c, name, err)
        dead = ~(case["logw"] > -np.inf)
        assert not got["g_states"][dead].any() and not got["g_logw"][dead].any(), (c, "a dead particle's gradient is not 0")
        gone = np.isnan(ref["nll"])
        for name in ("g_states", "g_logw", "g_log_scale"):
            assert np.isfinite(got[name]).all(), (c, name)
            assert not got[name][gone].any(), (c, name, "a row without an nll has a gradient")
        n += 1
    print(f"M = {M}: {n} cases, worst error per output {worst}")
    assert n >= 7


def test_nan_truth_and_dead_rows_give_nan_and_zero_gradients():
    for variant in ("nan_truth", "dead_row"):
        for M in (30, lc.WAVE_M + 1):
            case, ref = lc.family_case(M, 3, 3, variant, lc.SCALES[0])
            got = run_kernel(case)
            r = 3 // 2
            assert np.isnan(got["nll"][r]) and np.isfinite(np.delete(got["nll"], r)).all()
            assert not got["g_states"][r].any() and not got["g_logw"][r].any() and not got["g_log_scale"][r].any()
            assert got["g_states"][0].any() and got["g_logw"][0].any()


@pytest.mark.parametrize("M", [30, lc.WAVE_M, lc.WAVE_M + 1, lc.BIG_M])
def test_gradients_scale_exactly_by_a_power_of_two_upstream_gradient(M):
    """Without ``g_nll`` the gradients are those of ``g_nll = 1``, bit for bit; with powers of two they are those times ``g``,
    exactly; ``nll`` does not depend on it."""
    c = next(c for c in lc.family() if c[0] == M and c[2] == 3 and c[3] == "plain")
    case, _ = lc.family_case(*c)
    base = run_kernel(case)
    ones = run_kernel(case, g_nll=np.ones(3))
    g = np.asarray([4.0, 0.5, -2.0], np.float32)
    scaled = run_kernel(case, g_nll=g)
    dead = ~(case["logw"] > -np.inf)
    assert dead.any()
    for name in lc.OUTPUTS:
        assert same_bits(base[name], ones[name]), name
        want = base[name] if name == "nll" else base[name] * g.reshape((3,) + (1,) * (base[name].ndim - 1))
        if name in ("g_states", "g_logw"):
            want[dead] = 0.0  # a dead particle's gradient is WRITTEN as 0, not multiplied: +0 whatever the sign of g
        assert same_bits(scaled[name], want.astype(np.float32)), name


@pytest.mark.parametrize("M", [30, lc.WAVE_M + 1])
def test_bits_depend_on_neither_the_outputs_asked_for_nor_the_batch_nor_the_call(M):
    """Any subset of outputs gives the bits of the full call; a row alone (``R = 1``) gives the bits it has inside a batch of
    seven, wherever it stands; two calls give the same bits."""
    import itertools

    case = lc.make_case(M, 3, 7, "dead_particles", lc.SCALES[0])
    g = np.asarray([1.0, 0.3, -1.7, 2.0, 0.9, 1.1, 5.0], np.float32)
    full = run_kernel(case, g_nll=g)
    again = run_kernel(case, g_nll=g)
    for name in lc.OUTPUTS:
        assert same_bits(full[name], again[name]), name
    for k in (1, 2, 3):
        for subset in itertools.combinations(lc.OUTPUTS, k):
            got = run_kernel(case, subset, g_nll=g)
            for name in subset:
                assert same_bits(got[name], full[name]), (subset, name)
    for r in range(7):
        alone = run_kernel(case, g_nll=g, rows=slice(r, r + 1))
        for name in lc.OUTPUTS:
            assert same_bits(alone[name], full[name][r:r + 1]), (r, name)


def test_arguments_are_checked_on_the_host():
    from multimodalfilter_amd import _abi

    case = lc.make_case(30, 3, 3, "plain", lc.SCALES[0])
    X, A, Y, s = (torch.from_numpy(case[k]).to(DEV) for k in ("states", "logw", "truth", "scale"))
    nll = torch.empty(3, device=DEV)
    with pytest.raises(_abi.MmfError):
        _abi.pf_set_nll(X, A, Y, s)                                  # no output
    with pytest.raises(_abi.MmfError):
        _abi.pf_set_nll(X, A, Y, s, g_logw=A)                        # an output over an input
    five = torch.zeros((3, 30, 5), device=DEV)
    with pytest.raises(_abi.MmfError):
        _abi.pf_set_nll(five, A, torch.zeros((3, 5), device=DEV), torch.ones(5, device=DEV), nll=nll)   # d = 5

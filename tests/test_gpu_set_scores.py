"""``mmf_pf_scores_backward`` (csrc/pf_scores_backward.hip) against the fp64 closed form of ``_set_score_cases``: the gradients
of CRPS and the energy score of a weighted particle set, held to ``_tol.REL_TOL`` on every case of the family (whose fairness
``test_set_score_cases_cpu.py`` asserts), with the exact zeros, the exact scaling and the bit-for-bit properties of the header;
and ``engine.ParticleSetScoresFunction`` over it and over ``mmf_pf_scores``."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _set_score_cases as sc
from _tol import REL_TOL

DEV = "cuda:0"
SHAPE = {"g_states": lambda R, M, d: (R, M, d), "g_logw": lambda R, M, d: (R, M)}


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def run_kernel(case, outputs=sc.OUTPUTS, rows=None, times=None):
    """The kernel on a case (``rows``: a slice of its rows; ``times (R)``: factors of the rows' upstream gradients) ->
    ``{name: numpy}`` of the outputs asked for.  Every output is allocated with ``GUARD_ROWS`` rows of ``SENTINEL`` behind
    it, which must come back untouched."""
    from multimodalfilter_amd import _abi

    sl = slice(None) if rows is None else rows
    X, A, Y = (_dev(None if case[k] is None else case[k][sl]) for k in ("states", "logw", "truth"))
    R, M, d = X.shape
    t = np.ones(case["states"].shape[0], np.float32) if times is None else np.asarray(times, np.float32)
    gc = _dev(None if case["g_crps"] is None else (case["g_crps"] * t[:, None])[sl])
    ge = _dev(None if case["g_energy"] is None else (case["g_energy"] * t)[sl])
    bufs = {name: torch.full((R + sc.GUARD_ROWS,) + SHAPE[name](R, M, d)[1:], sc.SENTINEL, dtype=torch.float32, device=DEV) for name in outputs}
    _abi.pf_scores_backward(X, A, None, Y, gc, ge, scale=case["scale"], **{name: b[:R] for name, b in bufs.items()})
    out = {}
    for name, b in bufs.items():
        b = b.cpu().numpy()
        assert (b[R:] == np.float32(sc.SENTINEL)).all(), (name, "wrote behind its last row")
        out[name] = b[:R]
    return out


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def plus_zero(a):
    return not a.view(np.uint32).any()


@pytest.mark.parametrize("M", sc.ALL_MS)
def test_kernel_matches_the_fp64_reference(M):
    """Every case of the family at this ``M``: ``g_states`` under ``rel_err`` over per-particle vectors, ``g_logw`` under
    ``rel_err`` over per-row vectors, both below ``REL_TOL``; NaN nowhere; exact +0 at dead particles, on rows without a live
    particle and in what a NaN truth takes out."""
    worst = {name: 0.0 for name in sc.OUTPUTS}
    n = 0
    for c in sc.family():
        if c[0] != M:
            continue
        case, ref = sc.family_case(*c)
        got = run_kernel(case)
        for name in sc.OUTPUTS:
            err = sc.compare(got[name], ref[name], name, c)
            worst[name] = max(worst[name], err)
            assert err < REL_TOL, (c, name, err)
        dead = ~(sc._weights(case) > 0)
        assert plus_zero(got["g_states"][dead]) and plus_zero(got["g_logw"][dead]), (c, "a dead particle's gradient is not +0")
        gone = dead.all(1)
        assert plus_zero(got["g_states"][gone]) and plus_zero(got["g_logw"][gone]), (c, "a row without a live particle has a gradient")
        nan = np.isnan(case["truth"])
        for r in np.flatnonzero(nan.any(1)):   # no energy term; no crps term in the NaN coordinates: nothing touches those
            assert plus_zero(got["g_states"][r][:, nan[r]]), (c, r, "a NaN-valued term has a gradient")
            if nan[r].all() or case["g_crps"] is None:
                assert plus_zero(got["g_states"][r]) and plus_zero(got["g_logw"][r]), (c, r)
        n += 1
    print(f"M = {M}: {n} cases, worst error per output {worst}")
    assert n >= 8


def test_a_nan_upstream_gradient_of_a_nan_term_contributes_nothing():
    """The upstream gradient of a term whose forward value is NaN is not read into anything, NaN included."""
    case, _ = sc.family_case(65, 3, 3, "nan_truth")
    r = 3 // 2
    k = int(np.flatnonzero(np.isnan(case["truth"][r]))[0])
    base = run_kernel(case)
    poisoned = dict(case, g_crps=case["g_crps"].copy(), g_energy=case["g_energy"].copy())
    poisoned["g_crps"][r, k] = np.nan
    poisoned["g_energy"][r] = np.nan
    got = run_kernel(poisoned)
    for name in sc.OUTPUTS:
        assert same_bits(got[name], base[name]), name
    assert base["g_states"][r].any() and base["g_logw"][r].any()


@pytest.mark.parametrize("M", [30, sc.I_BLOCK + 1, sc.J_TILE + 1])
def test_bits_depend_on_neither_the_outputs_asked_for_nor_the_batch_nor_the_call(M):
    """Two calls give the same bits; a row alone (``R = 1``) gives the bits it has inside a batch of seven, wherever it
    stands; either output alone gives the bits of the call for both."""
    for variant in ("dead_particles", "crps_only", "energy_only"):
        case = sc.make_case(M, 3, 7, variant)
        full = run_kernel(case)
        again = run_kernel(case)
        for name in sc.OUTPUTS:
            assert same_bits(full[name], again[name]), (variant, name)
            alone = run_kernel(case, (name,))
            assert same_bits(alone[name], full[name]), (variant, name, "alone")
        for r in range(7):
            one = run_kernel(case, rows=slice(r, r + 1))
            for name in sc.OUTPUTS:
                assert same_bits(one[name], full[name][r:r + 1]), (variant, r, name)


@pytest.mark.parametrize("M", [30, sc.I_BLOCK, sc.I_BLOCK + 1, sc.BIG_M])
def test_gradients_scale_exactly_by_a_power_of_two_upstream_gradient(M):
    """A row's upstream gradients all times one power of two: its outputs times that, exactly (a zero stays +0)."""
    R = 3 if M < sc.BIG_M else 1
    for variant in ("plain", "scaled"):
        case = sc.make_case(M, 3, R, variant)
        base = run_kernel(case)
        t = np.asarray([4.0, 0.5, -2.0][:R], np.float32)
        scaled = run_kernel(case, times=t)
        for name in sc.OUTPUTS:
            want = (base[name] * t.reshape((R,) + (1,) * (base[name].ndim - 1))).astype(np.float32)
            want[want == 0] = 0.0   # (written as +0 whatever the sign of the factor)
            assert base[name].any() and same_bits(scaled[name], want), (variant, name)


@pytest.mark.parametrize("M", [30, sc.I_BLOCK + 1])
def test_autograd_function_is_the_two_kernels(M):
    """``ParticleSetScoresFunction``: the forward outputs are bit for bit those of ``_abi.pf_scores`` on the same tensors; the
    backward is ``_abi.pf_scores_backward`` with the upstream gradients autograd hands it, and an output that the loss does not
    use arrives as a null pointer (the bits of the call without it)."""
    from multimodalfilter_amd import _abi, engine, train

    case = sc.make_case(M, 3, 3, "scaled")
    X, A, Y = (_dev(case[k]) for k in ("states", "logw", "truth"))
    crps, energy = torch.empty((3, 3), device=DEV), torch.empty((3,), device=DEV)
    _abi.pf_scores(X, A, None, Y, crps, energy, None, case["scale"])
    engine.set_training_backend("hip")
    try:
        for use in ("both", "crps", "energy"):
            x, a = X.clone().requires_grad_(True), A.clone().requires_grad_(True)
            got_c, got_e = train.particle_set_scores(x, a, Y, case["scale"])
            assert torch.equal(got_c.view(torch.int32), crps.view(torch.int32)) and torch.equal(got_e.view(torch.int32), energy.view(torch.int32))
            gc, ge = _dev(case["g_crps"]), _dev(case["g_energy"])
            loss = 0.0
            if use != "energy":
                loss = loss + (got_c * gc).sum()
            if use != "crps":
                loss = loss + (got_e * ge).sum()
            loss.backward()
            want = run_kernel(dict(case, g_crps=None if use == "energy" else case["g_crps"], g_energy=None if use == "crps" else case["g_energy"]))
            assert same_bits(x.grad.cpu().numpy(), want["g_states"]) and same_bits(a.grad.cpu().numpy(), want["g_logw"]), use
        # the wrappers, and a set without leading axes
        x = X[0].clone().requires_grad_(True)
        e = train.particle_set_energy(x, A[0], Y[0], case["scale"])
        c = train.particle_set_crps(x, A[0], Y[0])
        assert e.shape == () and c.shape == (3,) and float(e.detach()) == float(energy[0]) and torch.equal(c, crps[0])
        (e + c.sum()).backward()
        assert bool(torch.isfinite(x.grad).all()) and bool(x.grad.abs().sum() > 0)
    finally:
        engine.set_training_backend(None)


def test_arguments_are_checked_on_the_host():
    from multimodalfilter_amd import _abi

    case = sc.make_case(30, 3, 3, "plain")
    X, A, Y, gc, ge = (_dev(case[k]) for k in ("states", "logw", "truth", "g_crps", "g_energy"))
    gx = torch.empty_like(X)
    with pytest.raises(_abi.MmfError):
        _abi.pf_scores_backward(X, A, None, Y, gc, ge)                              # no output
    with pytest.raises(_abi.MmfError):
        _abi.pf_scores_backward(X, A, None, Y, None, None, g_states=gx)             # no upstream gradient
    with pytest.raises(_abi.MmfError):
        _abi.pf_scores_backward(X, A, None, Y, gc, ge, g_logw=A)                    # an output over an input
    with pytest.raises(_abi.MmfError):
        _abi.pf_scores_backward(X, A, None, Y, gc, ge, g_states=gx, scale=(1.0, 0.0, 1.0))

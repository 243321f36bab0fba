"""The particle-set log score without a GPU: the fp64 reference of ``_set_loss_cases`` against plain fp64 autograd, the zeros
it puts at dead particles and dead rows, the library's torch fallback (``train.particle_set_nll`` on CPU tensors) against it,
what ``train.filter_loss(loss="nll")`` refuses, and the fairness condition of the GPU test's cases."""
import math

import numpy as np
import pytest
import torch

import _set_loss_cases as lc

SHAPES = [(1, 2, 1), (2, 3, 3), (30, 3, 3), (65, 4, 1), (257, 1, 3), (4096, 2, 1)]  # (M, d, R)


@pytest.mark.parametrize("M,d,R", SHAPES)
def test_closed_form_gradients_equal_fp64_autograd(M, d, R):
    """The reference's closed forms against torch autograd in fp64, nothing masked: equal wherever autograd is finite (it
    gives NaN in a row with a dead particle), to 1e-9 of the output's largest entry -- the far and the collapsed case included."""
    checked = 0
    for variant in lc.VARIANTS:
        case = lc.make_case(M, d, R, variant, lc.SCALES[0])
        ref = lc.reference(case)
        with np.errstate(invalid="ignore"):
            got = dict(zip(lc.OUTPUTS, lc.autograd64(case)))
        for name in lc.OUTPUTS:
            fin = np.isfinite(got[name]) & np.isfinite(ref[name])
            if name != "nll":  # (a row whose nll is NaN has zero gradients by definition, autograd has NaN)
                fin &= np.isfinite(ref["nll"]).reshape((R,) + (1,) * (ref[name].ndim - 1))
            if not fin.any():
                continue
            top = max(float(np.abs(ref[name][fin]).max()), 1e-300)
            assert float(np.abs(got[name] - ref[name])[fin].max()) <= 1e-9 * top, (variant, name)
            checked += int(fin.sum())
    assert checked > 0


def test_gradients_are_exactly_zero_at_dead_particles_and_on_dead_rows():
    for variant, M, R in (("dead_particles", 30, 3), ("dead_row", 65, 3), ("nan_truth", 30, 3), ("plain", 257, 1)):
        case = lc.make_case(M, 3, R, variant, lc.SCALES[0])
        ref = lc.reference(case)
        dead = ~(case["logw"] > -np.inf)
        assert dead.any()
        assert not ref["g_states"][dead].any() and not ref["g_logw"][dead].any()
        gone = np.isnan(ref["nll"])
        assert gone.any() == (variant in ("dead_row", "nan_truth"))
        for name in ("g_states", "g_logw", "g_log_scale"):
            assert not ref[name][gone].any(), (variant, name)
            assert np.isfinite(ref[name]).all(), (variant, name)


@pytest.mark.parametrize("M,d,R", SHAPES[:5])
def test_torch_fallback_on_cpu_tensors_matches_the_reference(M, d, R):
    """``train.particle_set_nll`` on CPU tensors (no training backend, no device): the definition in value and in every
    gradient, fp64 to 1e-9; dead particles and dead rows get exact zeros where plain autograd has NaN."""
    from multimodalfilter_amd import train

    for variant in lc.VARIANTS:
        case = lc.make_case(M, d, R, variant, lc.SCALES[1])
        ref = lc.reference(case)
        X, A, Y, s = (torch.from_numpy(case[k]).double() for k in ("states", "logw", "truth", "scale"))
        X.requires_grad_(True)
        A.requires_grad_(True)
        s.requires_grad_(True)
        nll = train.particle_set_nll(X, A, Y, s)
        assert nll.shape == (R,)
        keep = ~torch.isnan(nll)
        assert np.array_equal(keep.numpy(), ~np.isnan(ref["nll"]))
        g = torch.tensor([0.5, 2.0, 1.0])[:R].double()
        gx, ga, gs = torch.autograd.grad((torch.where(keep, nll, torch.zeros_like(nll)) * g).sum(), (X, A, s))
        for name, got, want in (("nll", nll.detach().numpy(), ref["nll"]), ("g_states", gx.numpy(), ref["g_states"] * g.numpy()[:, None, None]),
                                ("g_logw", ga.numpy(), ref["g_logw"] * g.numpy()[:, None]),
                                ("g_scale", gs.numpy(), (ref["g_log_scale"] * g.numpy()[:, None]).sum(0) / case["scale"].astype(np.float64))):
            assert np.isfinite(got[~np.isnan(want)]).all() and got.shape == want.shape, (variant, name)
            fin = ~np.isnan(want)
            if fin.any():
                top = max(float(np.abs(want[fin]).max()), 1e-300)
                assert float(np.abs(got - want)[fin].max()) <= 1e-9 * top, (variant, name)
        dead = ~(case["logw"] > -np.inf)
        assert not gx.numpy()[dead].any() and not ga.numpy()[dead].any(), variant
    # a list of floats serves as the scale, and a set without leading axes is one row
    case = lc.make_case(30, 3, 1, "plain", lc.SCALES[0])
    one = train.particle_set_nll(torch.from_numpy(case["states"][0]), torch.from_numpy(case["logw"][0]), torch.from_numpy(case["truth"][0]),
                                 [float(v) for v in case["scale"]])
    assert one.shape == () and abs(float(one) - lc.reference(case)["nll"][0]) < 1e-4 * abs(lc.reference(case)["nll"][0])


def test_filter_loss_nll_refuses_a_missing_scale_and_a_kalman_filter():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, train

    batch = {"states": torch.zeros(3, 2, 3)}
    engine.set_training_backend("autograd")
    try:
        pf = mmf.door_models.DoorParticleFilter().train()
        with pytest.raises(ValueError, match="nll_scale"):
            train.filter_loss(pf, batch, initial_covariance=torch.eye(3), loss="nll")
        kf = mmf.door_models.DoorKalmanFilter().train()
        with pytest.raises(ValueError, match="Kalman"):
            train.filter_loss(kf, batch, initial_covariance=torch.eye(3), loss="nll", nll_scale=(0.1, 0.1, 0.1))
        with pytest.raises(ValueError, match="callable"):
            train.filter_loss(pf, batch, initial_covariance=torch.eye(3), loss="crps")
        assert pf.keep_training_sets is False and pf.last_training_sets is None
    finally:
        engine.set_training_backend(None)


def test_entry_checks_its_arguments_on_the_host():
    """``mmf_pf_set_nll`` decides on the host, before any HIP call (the pointers here are never dereferenced): null required
    pointers, no output, ``d`` outside 1 .. 4, ``M < 1``, an output over an input or over another output -> ``MMF_EINVAL``;
    ``R == 0`` is a successful no-op."""
    import ctypes

    from multimodalfilter_amd import _abi

    lib = _abi.load()
    bufs = [(ctypes.c_float * 4096)() for _ in range(8)]
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]

    def call(**kw):
        a = _abi.MmfPfSetNllArgs()
        a.R, a.M, a.d = 2, 8, 3
        a.states, a.logw, a.truth, a.scale, a.nll = P[0], P[1], P[2], P[3], P[4]
        for k, v in kw.items():
            setattr(a, k, v)
        return lib.mmf_pf_set_nll(ctypes.byref(a), None)

    for name in ("states", "logw", "truth", "scale"):
        assert call(R=0, **{name: None}) == -1, name
    assert call(R=0, nll=None) == -1                                   # no output at all
    assert call(R=0, d=0) == -1 and call(R=0, d=5) == -1 and call(R=0, M=0) == -1 and call(R=-1) == -1
    assert call(nll=P[1]) == -1 and call(nll=P[3]) == -1               # an output over an input (logw, scale)
    assert call(g_states=P[4]) == -1                                   # an output over another output
    assert call(g_nll=P[5], g_logw=P[5]) == -1                         # over the upstream gradient
    assert call(R=0) == 0 and call(R=0, nll=None, g_states=P[5], g_logw=P[6], g_log_scale=P[7]) == 0
    assert lib.mmf_pf_train_backward_sets(None, P[0], P[1], None) == -1


def test_family_covers_what_the_issue_lists():
    fam = list(lc.family())
    assert len(fam) == len(set(fam))
    assert {c[0] for c in fam} == set(lc.ALL_MS) and {lc.WAVE_M - 1, lc.WAVE_M, lc.WAVE_M + 1, 1, 2, 30, 63, 64, 65, 257, 4096} <= set(lc.ALL_MS)
    for M in lc.MS:
        assert {(d, R, v) for m, d, R, v, _ in fam if m == M} >= {(d, R, v) for d in lc.DIMS for R in lc.RS for v in lc.VARIANTS}
    assert {v for m, _, _, v, _ in fam if m == lc.BIG_M} == set(lc.VARIANTS)
    assert max(c[2] for c in fam) > 256 * lc.ROWS_PER_BLOCK
    from multimodalfilter_amd import _abi

    assert lc.WAVE_M == _abi.SET_NLL_WAVE_M


@pytest.mark.parametrize("M", lc.ALL_MS)
def test_fp32_torch_formulation_stays_within_a_third_of_the_tolerance(M):
    """The fairness condition of ``test_gpu_set_loss.py``: on every case it uses, the same formulation in fp32 torch ops stays
    within ``REL_TOL / 3`` of the fp64 reference, under the metrics the kernel is held to."""
    from _tol import REL_TOL

    assert lc.CAP == REL_TOL / 3
    worst = {name: 0.0 for name in lc.OUTPUTS}
    for c in lc.family():
        if c[0] != M:
            continue
        case, ref = lc.family_case(*c)
        assert lc.well_conditioned(case, ref), c
        got = lc.torch_formulation(case)
        for name in lc.OUTPUTS:
            err = lc.compare(got[name], ref[name], name, c)
            worst[name] = max(worst[name], err)
            assert err < lc.CAP, (c, name, err)
    print(f"M = {M}: worst fp32 error per output {worst}")
    assert math.isfinite(sum(worst.values()))

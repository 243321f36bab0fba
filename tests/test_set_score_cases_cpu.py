"""The gradients of CRPS and the energy score of a particle set without a GPU: the fp64 closed form of ``_set_score_cases``
against plain fp64 autograd, the fairness condition of the GPU test's cases, the library's torch fallback
(``train.particle_set_crps`` / ``particle_set_energy`` on CPU tensors) against the reference with its zero rules, what
``mmf_pf_scores_backward`` refuses on the host, and ``train.filter_loss``'s ``ValueError``s."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _set_score_cases as sc

SHAPES = [(1, 2, 1), (2, 3, 3), (30, 3, 3), (65, 4, 1), (513, 1, 3), (1025, 2, 1)]  # (M, d, R)


@pytest.mark.parametrize("M,d,R", SHAPES)
def test_closed_form_gradients_equal_fp64_autograd(M, d, R):
    """The reference's closed forms against torch autograd of the forward definition in fp64 on the live particles (half of
    the states are duplicates: a pair at distance 0 contributes 0), to 1e-10 of the output's largest entry, on every variant."""
    checked = 0
    for variant in sc.VARIANTS:
        case = sc.make_case(M, d, R, variant)
        ref = sc.reference(case)
        gx, ga = sc.autograd64(case)
        rows = ~np.isnan(case["truth"]).any(1)  # (autograd64 leaves a row with a NaN truth out: its other terms are checked below)
        for name, got in (("g_states", gx), ("g_logw", ga)):
            want = ref[name][rows]
            top = float(np.abs(want).max()) if want.size else 0.0
            if top == 0.0:
                continue
            assert float(np.abs(got[rows] - want).max()) <= 1e-10 * top, (variant, name)
            checked += int(want.size)
    assert checked > 0


def test_a_nan_truth_takes_out_its_own_terms_alone():
    """With ``y_k`` NaN the row's gradients are those of the loss without ``crps[k]`` and without ``energy``: the reference on
    the NaN case equals fp64 autograd on a case with a finite truth there and zero upstream gradients for those terms."""
    case = sc.make_case(30, 3, 3, "nan_truth")
    r, k = 3 // 2, (30 + 3) % 3
    assert np.isnan(case["truth"][r, k])
    ref = sc.reference(case)
    other = {key: (None if v is None else np.array(v, copy=True)) if not isinstance(v, tuple) else v for key, v in case.items()}
    other["truth"][r, k] = 0.25
    other["g_crps"][r, k] = 0.0
    other["g_energy"][r] = 0.0
    gx, ga = sc.autograd64(other)
    assert ref["g_states"][r].any() and not ref["g_states"][r][:, k].any()
    for got, want in ((gx, ref["g_states"]), (ga, ref["g_logw"])):
        assert float(np.abs(got - want).max()) <= 1e-10 * float(np.abs(want).max())
    assert np.isnan(ref["crps"][r, k]) and np.isnan(ref["energy"][r]) and np.isfinite(np.delete(ref["crps"][r], k)).all()


def test_family_covers_what_the_issue_lists():
    fam = list(sc.family())
    assert len(fam) == len(set(fam))
    assert {c[0] for c in fam} == set(sc.ALL_MS) == {1, 2, 30, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4096}
    assert (sc.RUN, sc.I_BLOCK, sc.J_TILE) == (64, 512, 1024)
    for M in sc.SMALL_MS:
        assert {(d, R, v) for m, d, R, v in fam if m == M} >= {(d, R, v) for d in sc.DIMS for R in sc.RS for v in sc.VARIANTS}
    for M in sc.LARGE_MS:
        assert {(d, v) for m, d, R, v in fam if m == M} == {(d, v) for d in sc.DIMS for v in sc.VARIANTS}
        assert {R for m, d, R, v in fam if m == M} == set(sc.RS)
    assert {v for m, _, _, v in fam if m == sc.BIG_M} == set(sc.VARIANTS)
    assert max(c[2] for c in fam) > 1024
    case = sc.draw_case(30, 3, 3)
    for g in (case["g_crps"], case["g_energy"]):
        assert 0.5 <= float(g.min()) and float(g.max()) <= 1.5


@pytest.mark.parametrize("M", sc.ALL_MS)
def test_fp32_torch_formulation_stays_within_a_third_of_the_tolerance(M):
    """The fairness condition of ``test_gpu_set_scores.py``: on every case it uses, the same formulation in fp32 torch ops stays
    within ``REL_TOL / 3`` of the fp64 reference, under the metrics the kernel is held to."""
    from _tol import REL_TOL

    assert sc.CAP == REL_TOL / 3
    worst = {name: 0.0 for name in sc.OUTPUTS}
    for c in sc.family():
        if c[0] != M:
            continue
        case, ref = sc.family_case(*c)
        assert sc.well_conditioned(case, ref), c
        got = sc.torch_formulation(case)
        for name in sc.OUTPUTS:
            err = sc.compare(got[name], ref[name], name, c)
            worst[name] = max(worst[name], err)
            assert err < sc.CAP, (c, name, err)
    print(f"M = {M}: worst fp32 error per output {worst}")
    assert math.isfinite(sum(worst.values()))


@pytest.mark.parametrize("M,d,R", SHAPES[:5])
def test_torch_fallback_on_cpu_tensors_matches_the_reference(M, d, R):
    """``train.particle_set_crps`` / ``particle_set_energy`` / ``particle_set_scores`` on CPU tensors (no training backend, no
    device) in fp64, on the reference's own log-weights: the definition in value and in both gradients to 1e-9; exact zeros at dead particles, on a dead row and
    for the terms a NaN truth takes out, where plain autograd has NaN."""
    from multimodalfilter_amd import train

    for variant in sc.VARIANTS:
        case = sc.make_case(M, d, R, variant)
        ref = sc.reference(case)
        X = torch.from_numpy(case["states"]).double().requires_grad_(True)
        with np.errstate(divide="ignore"):   # the kernels' a - max a, rounded to fp32 as they round it (the reference's weights); dead: -inf
            A = torch.from_numpy(np.log(sc._weights(case))).requires_grad_(True)
        Y = torch.from_numpy(case["truth"]).double()
        if variant == "crps_only":
            crps, energy = train.particle_set_crps(X, A, Y), None
        elif variant == "energy_only":
            crps, energy = None, train.particle_set_energy(X, A, Y, case["scale"])
        else:
            crps, energy = train.particle_set_scores(X, A, Y, case["scale"])
        loss = 0.0
        for got, name, g in ((crps, "crps", case["g_crps"]), (energy, "energy", case["g_energy"])):
            if got is None:
                continue
            want = ref[name]
            assert got.shape == want.shape and np.array_equal(np.isnan(got.detach().numpy()), np.isnan(want)), (variant, name)
            fin = ~np.isnan(want)
            if fin.any():
                assert float(np.abs(got.detach().numpy() - want)[fin].max()) <= 1e-9 * max(float(np.abs(want[fin]).max()), 1e-300), (variant, name)
            loss = loss + (torch.where(torch.isnan(got), torch.zeros_like(got), got) * torch.from_numpy(g).double()).sum()
        gx, ga = torch.autograd.grad(loss, (X, A))
        for name, got in (("g_states", gx.numpy()), ("g_logw", ga.numpy())):
            assert np.isfinite(got).all(), (variant, name)
            assert float(np.abs(got - ref[name]).max()) <= 1e-9 * max(float(np.abs(ref[name]).max()), 1e-300), (variant, name)
        dead = ~(sc._weights(case) > 0)
        assert not gx.numpy()[dead].any() and not ga.numpy()[dead].any(), variant
        if variant in ("dead_row", "nan_truth") and R == 3:
            r = R // 2
            if variant == "dead_row":
                assert not gx.numpy()[r].any() and not ga.numpy()[r].any()
            else:
                assert not gx.numpy()[r][:, np.isnan(case["truth"][r])].any()
    # a set without leading axes is one row, and a scale of the wrong length or sign is refused
    case = sc.make_case(30, 3, 1, "scaled")
    one = train.particle_set_energy(torch.from_numpy(case["states"][0]), torch.from_numpy(case["logw"][0]), torch.from_numpy(case["truth"][0]), case["scale"])
    want = sc.reference(case)["energy"][0]
    assert one.shape == () and abs(float(one) - want) < 1e-4 * abs(want)
    with pytest.raises(ValueError, match="scale"):
        train.particle_set_energy(torch.zeros(2, 3), torch.zeros(2), torch.zeros(3), (1.0, 1.0))
    with pytest.raises(ValueError, match="scale"):
        train.particle_set_energy(torch.zeros(2, 3), torch.zeros(2), torch.zeros(3), (1.0, -1.0, 1.0))


def test_torch_formulation_chunks_do_not_change_the_definition():
    from multimodalfilter_amd import engine

    case = sc.make_case(65, 3, 3, "plain")
    X, A, Y = (torch.from_numpy(case[k]).double() for k in ("states", "logw", "truth"))
    whole = engine.particle_set_scores_torch(X, A, Y, None, chunk=65)
    for chunk in (1, 7, 64):
        parts = engine.particle_set_scores_torch(X, A, Y, None, chunk=chunk)
        for a, b in zip(whole, parts):
            assert float((a - b).abs().max()) < 1e-12


_FIELDS = ("states", "log_a", "log_b", "truth", "g_crps", "g_energy", "g_states", "g_logw", "workspace")


def test_entry_checks_its_arguments_on_the_host():
    """``mmf_pf_scores_backward`` decides on the host, before any HIP call (the pointers here are never dereferenced)."""
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    EINVAL, ETOOLARGE = -1, -2
    bufs = [(ctypes.c_double * (1 << 16))() for _ in range(len(_FIELDS))]
    P = dict(zip(_FIELDS, (ctypes.cast(b, ctypes.c_void_p) for b in bufs)))

    def call(scale=(1.0, 1.0), **over):
        a = _abi.MmfPfScoresBackwardArgs()
        a.R, a.M, a.d, a.workspace_bytes = 2, 8, 2, 8 << 16
        for name in _FIELDS:
            setattr(a, name, P[name])
        for i, s in enumerate(scale):
            a.scale[i] = s
        for k, v in over.items():
            setattr(a, k, v)
        return lib.mmf_pf_scores_backward(ctypes.byref(a), None)

    assert lib.mmf_pf_scores_backward(None, None) == EINVAL
    assert call(R=0) == 0                                                        # a successful no-op
    assert call(R=0, states=None) == EINVAL and call(R=0, truth=None) == EINVAL
    assert call(R=0, log_a=None, log_b=None) == 0                                # either log-weight may be null
    assert call(R=0, g_crps=None) == 0 and call(R=0, g_energy=None) == 0 and call(R=0, g_crps=None, g_energy=None) == EINVAL
    assert call(R=0, g_states=None) == 0 and call(R=0, g_logw=None) == 0 and call(R=0, g_states=None, g_logw=None) == EINVAL
    assert call(R=0, d=0) == EINVAL and call(R=0, d=5) == EINVAL and call(R=0, M=0) == EINVAL and call(R=-1) == EINVAL
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert call((1.0, bad), R=0) == EINVAL, bad
    assert call((1.0, 0.5, -3.0), R=0) == 0                                      # (beyond d: not read)
    # the workspace: none up to 512 particles, needed beyond whichever output is asked for
    assert _abi.pf_scores_backward_workspace_bytes(3, 512, 4) == 0 == _abi.pf_scores_backward_workspace_bytes(0, 513, 2)
    assert _abi.pf_scores_backward_workspace_bytes(1, 513, 2) == (2 + 2 * 513) * 8
    assert _abi.pf_scores_backward_workspace_bytes(3, 16384, 4) == 3 * (32 + 2 * 16384) * 8
    assert call(R=0, M=512, workspace=None, workspace_bytes=0) == 0
    need = _abi.pf_scores_backward_workspace_bytes(2, 513, 2)
    assert call(R=0, M=513, workspace_bytes=need) == 0
    assert call(M=513, workspace=None) == EINVAL and call(M=513, workspace_bytes=need - 8) == EINVAL
    assert call(M=513, g_logw=None, workspace=None) == EINVAL
    assert call(M=513, workspace=ctypes.c_void_p(P["workspace"].value + 4), workspace_bytes=need) == EINVAL   # misaligned
    # aliasing: an output or the workspace over an input or over another output
    for out in ("g_states", "g_logw"):
        for inp in ("states", "log_a", "log_b", "truth", "g_crps", "g_energy"):
            assert call(**{out: P[inp]}) == EINVAL, (out, inp)
    assert call(g_logw=P["g_states"]) == EINVAL
    assert call(M=513, workspace_bytes=need, workspace=P["states"]) == EINVAL
    assert call(M=513, workspace_bytes=need, workspace=P["g_logw"]) == EINVAL
    assert call(R=0, g_logw=P["states"]) == 0                                    # (no rows: nothing overlaps)
    # sizes
    assert call(R=0, M=16385, workspace_bytes=1 << 40) == ETOOLARGE
    assert call(R=0x7fffffff, M=16384, workspace_bytes=1 << 60) == ETOOLARGE     # the grid


def test_binding_refuses_a_scale_of_the_wrong_length():
    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    with pytest.raises(_abi.MmfError, match="scale"):
        _abi.pf_scores_backward(x, None, None, torch.zeros((2, 3)), torch.zeros((2, 3)), None, g_states=torch.zeros_like(x), scale=(1.0, 1.0))


def test_filter_loss_refuses_what_the_set_scores_cannot_serve():
    """``loss="energy"`` on a Kalman filter and under a scale of the wrong length or sign; ``crps_loss`` likewise (on a Kalman
    filter when it is called, with no sets); the valid-values message names the new keyword, and ``"crps"`` as a string stays
    what it was, no keyword."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, train

    batch = {"states": torch.zeros(3, 2, 3)}
    engine.set_training_backend("autograd")
    try:
        pf = mmf.door_models.DoorParticleFilter().train()
        kf = mmf.door_models.DoorKalmanFilter().train()
        with pytest.raises(ValueError, match="Kalman"):
            train.filter_loss(kf, batch, initial_covariance=torch.eye(3), loss="energy")
        with pytest.raises(ValueError, match="scale"):
            train.filter_loss(pf, batch, initial_covariance=torch.eye(3), loss="energy", score_scale=(1.0, 1.0))
        with pytest.raises(ValueError, match="scale"):
            train.filter_loss(pf, batch, initial_covariance=torch.eye(3), loss="energy", score_scale=(1.0, 0.0, 1.0))
        for loss in ("mae", "crps"):
            with pytest.raises(ValueError, match='"mse", "nll", "energy" or a callable'):
                train.filter_loss(pf, batch, initial_covariance=torch.eye(3), loss=loss)
        assert pf.keep_training_sets is False and pf.last_training_sets is None
    finally:
        engine.set_training_backend(None)
    with pytest.raises(ValueError, match="scale"):
        train.crps_loss((1.0, -1.0, 1.0))
    with pytest.raises(ValueError, match="Kalman"):
        train.crps_loss()(torch.zeros(2, 2, 3), None, batch)
    sets = {"states": torch.zeros(2, 2, 4, 3), "log_weights": torch.zeros(2, 2, 4)}
    with pytest.raises(ValueError, match="scale"):
        train.crps_loss((1.0, 1.0))(torch.zeros(2, 2, 3), sets, batch)


def test_crps_loss_is_the_scaled_sum_of_the_sets_crps():
    """``crps_loss(scale)`` on CPU tensors: the mean over steps and trajectories of ``sum_k crps_k / scale_k`` of the reference."""
    from multimodalfilter_amd import train

    case = sc.make_case(30, 3, 3, "plain")
    ref = sc.reference(case)
    with np.errstate(divide="ignore"):
        A = torch.from_numpy(np.log(sc._weights(case)))
    sets = {"states": torch.from_numpy(case["states"]).double()[:, None], "log_weights": A[:, None]}   # (T = 3, N = 1, M, d)
    batch = {"states": torch.cat([torch.zeros(1, 1, 3, dtype=torch.float64), torch.from_numpy(case["truth"]).double()[:, None]])}
    scale = (0.5, 1.0, 2.0)
    for s, want in ((None, ref["crps"].sum(-1).mean()), (scale, (ref["crps"] / np.asarray(scale)).sum(-1).mean())):
        got = float(train.crps_loss(s)(None, sets, batch))
        assert abs(got - want) < 1e-9 * abs(want), (s, got, want)

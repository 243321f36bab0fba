"""Certifies, without a GPU, the inputs ``test_gpu_kalman_kernels.py`` runs the Kalman kernels on (``_kalman_cases.py``):
that they reach the row swaps of ``mmf_ekf::inverse`` -- which no other input of the suite does -- and that the fp32 torch
reference, the yardstick of the GPU test's error rule, is itself close enough to fp64 for that rule to mean something.

The caps are conditions on the INPUTS: a seed that breaks one is replaced, the cap stays."""
import itertools

import numpy as np
import pytest
import torch

import _kalman_cases as kc
import _tol


def _big(ns=kc.NS):
    return [N for N in ns if N >= kc.COVERAGE_MIN_N]


def test_swap_pattern_replays_the_comparisons_on_known_matrices():
    """The replay itself on matrices whose pivoting can be done by hand."""
    assert kc.swap_pattern(np.eye(3)).tolist() == [False, False, False]
    assert kc.swap_pattern([[1.0, 2.0], [2.0, 5.0]]).tolist() == [True]
    assert kc.swap_pattern([[2.0, 1.0], [1.0, 2.0]]).tolist() == [False]
    # column 0: |4| > |1| swaps rows 0, 1; |6| > |4| swaps rows 0, 2 -> rows (6 1 1), (1 5 1), (4 1 5); after elimination
    # column 1 holds 5 - 1/6 and 1 - 4/6: no swap
    assert kc.swap_pattern([[1.0, 5.0, 1.0], [4.0, 1.0, 5.0], [6.0, 1.0, 1.0]]).tolist() == [True, True, False]
    assert kc.swap_pattern(np.zeros((4, 0, 1, 1))).shape == (4, 0, 0)
    # ties do not swap (the kernel compares with >)
    assert kc.swap_pattern([[1.0, 1.0], [-1.0, 3.0]]).tolist() == [False]


@pytest.mark.parametrize("d", [2, 3])
def test_hand_built_matrices_are_spd_and_take_every_pattern(d):
    mats = np.asarray(kc.HAND_BUILT[d])
    assert np.array_equal(mats, mats.transpose(0, 2, 1))
    assert float(np.linalg.eigvalsh(mats).min()) > 0.1
    want = list(itertools.product([False, True], repeat=d * (d - 1) // 2))
    assert [tuple(p) for p in kc.swap_pattern(mats).tolist()] == want


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
@pytest.mark.parametrize("N", _big())
def test_step_cases_cover_the_swaps_of_the_innovation_inverse(N, K, d):
    """Every comparison comes out both true and false; for d = 2, 3 every swap pattern occurs (the hand-built rows see
    to the patterns the random family misses)."""
    Sinn, _, _ = kc.step_inverted_matrices(N, d, K)
    assert float(np.linalg.eigvalsh(Sinn).min()) > 0.0
    pats = kc.swap_pattern(Sinn).reshape(-1, d * (d - 1) // 2)
    assert pats.any(0).all() and (~pats).any(0).all(), (pats.mean(0))
    if d <= 3:
        assert len({tuple(p) for p in pats.tolist()}) == 2 ** (d * (d - 1) // 2)


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("K", [3])
def test_backward_case_covers_the_swaps(K, d):
    """Group C runs at N = 257, K = 3."""
    Sinn, _, _ = kc.step_inverted_matrices(257, d, K)
    pats = kc.swap_pattern(Sinn).reshape(-1, d * (d - 1) // 2)
    assert pats.any(0).all() and (~pats).any(0).all()


@pytest.mark.parametrize("d", [2, 3, 4])
@pytest.mark.parametrize("K", [2, 3, 4])
@pytest.mark.parametrize("N", _big())
def test_fusion_2_inverses_see_swaps(N, K, d):
    _, post, Psum = kc.step_inverted_matrices(N, d, K)
    assert kc.swap_pattern(post).any(), "no posterior inverse swaps"
    assert kc.swap_pattern(Psum).any(), "the inverse of the summed precisions never swaps"


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("K,fusion", kc.STEP_COMBOS)
@pytest.mark.parametrize("N", kc.NS)
def test_fp32_reference_of_the_step_is_within_its_caps(N, K, fusion, d):
    truth = kc.step_reference(N, d, K, fusion, torch.float64)
    fp32 = kc.step_reference(N, d, K, fusion, torch.float32)
    for name, got, want, cap in zip(("mu", "Sigma", "mu_f", "Sigma_f"), fp32, truth,
                                    (kc.CAP_STEP, kc.CAP_STEP, kc.CAP_FUSED, kc.CAP_FUSED)):
        if want is not None:
            assert bool(torch.isfinite(want).all())
            assert _tol.rel_err(got, want) <= cap, (name, _tol.rel_err(got, want))
    assert 3 * kc.CAP_FUSED <= 5.1e-3 and kc.GPU_BAR_CEILING <= 5e-3


@pytest.mark.parametrize("d", kc.SENSOR_DIMS)
@pytest.mark.parametrize("K", kc.SENSOR_KS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("N", kc.NS)
def test_fp32_reference_of_the_fused_sensors_is_within_its_caps(N, mode, K, d):
    c = kc.sensor_case(N, d, K)
    T = c["T"]
    low = np.abs(T[..., np.tril_indices(d)[0], np.tril_indices(d)[1]])
    assert np.array_equal(T, np.tril(T)) and low.min() >= 0.2 and low.max() <= 1.0
    assert (np.diagonal(T, axis1=-2, axis2=-1) > 0).all() and c["w"].min() >= 0.3 and c["w"].max() <= 1.0
    z64, t64, inverted = kc.sensor_reference(N, d, K, mode, torch.float64)
    z32, t32, _ = kc.sensor_reference(N, d, K, mode, torch.float32)
    assert bool(torch.isfinite(t64).all()) and bool(torch.isfinite(t32).all())
    assert _tol.rel_err(z32, z64) <= kc.CAP_STEP, _tol.rel_err(z32, z64)
    assert _tol.rel_err(t32, t64) <= (kc.CAP_FUSED if mode == 2 else kc.CAP_STEP), _tol.rel_err(t32, t64)
    if inverted is not None and N >= kc.COVERAGE_MIN_N:
        pats = kc.swap_pattern(inverted.numpy())
        assert pats.any(0).all() and (~pats).any(0).all()   # Q5's 1e9 upper triangle makes this inverse pivot


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("N", kc.NS)
def test_belief_cases_are_positive_definite_with_condition_at_most_1e3(N, d):
    c = kc.belief_case(N, d)
    ev = np.linalg.eigvalsh(c["Sigma"].astype(np.float64))
    assert ev.min() > 0 and float((ev.max(-1) / ev.min(-1)).max()) <= 1.01e3
    assert np.array_equal(c["Sigma"], c["Sigma"].transpose(0, 2, 1))


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("strategy", kc.STRATEGY_NAMES)
@pytest.mark.parametrize("N", kc.NS)
def test_fp32_yardsticks_of_the_unscented_moments(N, strategy, d):
    """Julier and alpha = 0.5: fp32 torch is within 1e-4 of fp64.  Merwe's default (alpha = 1e-2, ``wm0`` ~ -1e4): the
    sum as written is 10 to 100 times outside, the evaluation about point 0 is at most 3.4e-5 / 1.2e-4 -- the fp32
    yardstick the GPU test uses there."""
    c = kc.moments_case(N, d, strategy)
    wc0, wm0, wi = c["weights"]
    assert abs(wm0 + 2 * d * wi - 1.0) < 1e-9 * max(1.0, abs(wm0))      # the normalisation the about-point-0 form uses
    assert np.abs(c["q_tril"]).max() > 0
    m64, S64 = kc.moments_reference(N, d, strategy, torch.float64)
    m32, S32 = kc.moments_reference(N, d, strategy, torch.float32)
    m0, S0 = kc.moments_about_point0_fp32(N, d, strategy)
    e_m, e_S = _tol.rel_err(m0, m64), _tol.rel_err(S0, S64)
    assert e_m <= 3.4e-5 and e_S <= 1.2e-4, (e_m, e_S)
    if strategy != "merwe_default":
        assert _tol.rel_err(m32, m64) <= 1e-4 and _tol.rel_err(S32, S64) <= 1e-4
    elif N >= kc.COVERAGE_MIN_N:
        assert _tol.rel_err(m32, m64) > max(1e-4, 3 * e_m)      # the weighted sum as written misses the bar already in the mean

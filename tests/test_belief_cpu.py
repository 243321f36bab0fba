"""The belief record (per-step covariance, ESS, log-evidence) where no GPU is needed: the boundary knows the new entry
point and fields, and the calibration metrics of ``evaluation.py`` against closed forms."""
import ctypes
import math

import torch

from multimodalfilter_amd import _abi, evaluation


def test_binding_has_the_belief_entry_point_and_fields():
    assert "mmf_pf_reweight_resample_belief" in _abi.SIGNATURES
    pf = [n for n, _ in _abi.MmfPfLoopArgs._fields_]
    assert pf[-3:] == ["cov_steps", "ess_steps", "log_evidence_steps"]  # appended: the older fields keep their offsets
    # the EKF loop's per-step destination is an argument of an entry point of its own: MmfEkfLoopArgs keeps its size
    assert "mmf_ekf_forward_loop_belief" in _abi.SIGNATURES
    assert [n for n, _ in _abi.MmfEkfLoopArgs._fields_][-1] == "sync_words"
    # the version after the struct layouts changed: the parent's 41 (the LSTM recurrence) + 1
    assert _abi.ABI_VERSION == 42 == _abi.load().mmf_version()


def test_belief_entry_point_rejects_null_and_invalid_arguments():
    lib = _abi.load()
    bufs = [(ctypes.c_float * 64)() for _ in range(10)]
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    f = lib.mmf_pf_reweight_resample_belief
    EINVAL, ETOOLARGE = -1, -2
    ok = lambda **kw: f(kw.get("loglik", P[0]), kw.get("logw_in", P[1]), kw.get("states_in", P[2]), kw.get("u", P[3]),
                        kw.get("estimate", P[4]), kw.get("states_out", P[5]), kw.get("logw_out", P[6]), None,
                        kw.get("N", 0), kw.get("M", 8), kw.get("M_out", 8), kw.get("d", 3), kw.get("mode", 1),
                        kw.get("alpha", 1.0), P[7], P[8], P[9], None)
    assert ok() == 0                                        # an empty batch is a no-op: nothing is dereferenced
    for required in ("loglik", "states_in", "estimate"):
        assert ok(**{required: None}) == EINVAL, required
    assert ok(u=None) == EINVAL and ok(states_out=None) == EINVAL      # resampling needs uniforms and a destination
    assert ok(states_out=P[2]) == EINVAL                               # in-place gather
    assert ok(d=5) == EINVAL and ok(mode=3) == EINVAL and ok(alpha=0.0) == EINVAL
    assert ok(mode=0, alpha=0.5) == EINVAL                             # soft resampling needs a resampling mode
    assert ok(mode=0, logw_in=None) == EINVAL                          # the uniform shortcut belongs to plain resampling
    # the record's reduction rows come out of the same 160 KiB: the stated limits of a recording call
    assert ok(M=20200, M_out=20200) == 0 and ok(M=20300, M_out=20300) == ETOOLARGE
    assert ok(mode=0, M=40500, M_out=40500) == 0 and ok(mode=0, M=40600, M_out=40600) == ETOOLARGE
    # ... while the non-recording call keeps its own
    plain = lambda M, mode: lib.mmf_pf_reweight_resample(P[0], P[1], P[2], P[3], P[4], P[5], P[6], None, 0, M, M, 3, mode, None)
    assert plain(20400, 1) == 0 and plain(40800, 0) == 0
    # the EKF loop with a record: the destination is required, and the struct is checked as mmf_ekf_forward_loop checks it
    a = _abi.MmfEkfLoopArgs()
    assert lib.mmf_ekf_forward_loop_belief(ctypes.byref(a), None, None) == EINVAL
    assert lib.mmf_ekf_forward_loop_belief(None, P[0], None) == EINVAL
    assert lib.mmf_ekf_forward_loop_belief(ctypes.byref(a), P[0], None) == EINVAL  # N = 0, null fields


def test_filters_expose_record_belief_and_lstm_does_not():
    import multimodalfilter_amd as mmf

    for f in (mmf.door_models.DoorParticleFilter(), mmf.door_models.DoorKalmanFilter(),
              mmf.door_models.DoorCrossmodalKalmanFilter(), mmf.door_models.DoorUnimodalKalmanFilter()):
        assert f.record_belief is False and f.last_belief is None, type(f).__name__
    assert not hasattr(mmf.door_models.DoorLSTMFilter(), "record_belief")


def test_metrics_isotropic_closed_form():
    """``C = s^2 I`` and a constant error ``e``: NEES = |e|^2 / s^2, NLL = 0.5 (NEES + 2 d log s + d log 2 pi), and the
    point is inside the ``level`` ellipsoid iff the chi-square CDF at NEES is at most ``level``."""
    T, N = 40, 3
    for d, s, e in ((2, 0.5, [0.3, -0.4]), (3, 2.0, [1.0, 2.0, -2.0])):
        true = torch.zeros(T, N, d, dtype=torch.float64)
        pred = true + torch.tensor(e, dtype=torch.float64)
        cov = (torch.eye(d, dtype=torch.float64) * s * s).expand(T, N, d, d).contiguous()
        want = sum(x * x for x in e) / (s * s)
        got = evaluation.nees(pred, cov, true)
        assert got.shape == (T - evaluation.START_TRUNCATION, N)
        assert torch.allclose(got, torch.full_like(got, want), rtol=1e-12)
        nll = evaluation.gaussian_nll(pred, cov, true)
        assert nll.shape == (N,)
        assert torch.allclose(nll, torch.full_like(nll, 0.5 * (want + 2 * d * math.log(s) + d * math.log(2 * math.pi))), rtol=1e-12)
        # chi-square CDF by hand: d = 2: 1 - exp(-x / 2); d = 3: erf(sqrt(x / 2)) - sqrt(2 x / pi) exp(-x / 2)
        cdf = (1 - math.exp(-want / 2) if d == 2 else
               math.erf(math.sqrt(want / 2)) - math.sqrt(2 * want / math.pi) * math.exp(-want / 2))
        for level in (cdf - 0.01, cdf + 0.01):
            cvr = evaluation.coverage(pred, cov, true, level)
            assert cvr.shape == (N,) and bool((cvr == (1.0 if cdf <= level else 0.0)).all()), (d, level)
    # the burn-in: errors before START_TRUNCATION do not count
    pred[:evaluation.START_TRUNCATION] += 100.0
    assert torch.allclose(evaluation.nees(pred, cov, true), torch.full((T - evaluation.START_TRUNCATION, N), want, dtype=torch.float64))


def test_metrics_on_samples_of_the_belief_are_calibrated():
    """Errors drawn from ``N(0, C)`` itself (fixed generator): NEES is chi-square with ``d`` degrees -- mean ``d``, variance
    ``2 d`` -- so its sample mean lies within 3 standard errors ``sqrt(2 d / n)`` of ``d``; the 95 % coverage is a binomial
    share, within 3 standard errors ``sqrt(0.95 x 0.05 / n)`` of 0.95.  Both bounds follow from the sample count."""
    g = torch.Generator().manual_seed(7)
    T, N = 530, 40
    n = (T - evaluation.START_TRUNCATION) * N
    for d in (2, 3):
        A = torch.randn((T, N, d, d), generator=g, dtype=torch.float64)
        C = A @ A.transpose(-1, -2) + 0.1 * torch.eye(d, dtype=torch.float64)  # a different full covariance per step
        L = torch.linalg.cholesky(C)
        e = (L @ torch.randn((T, N, d, 1), generator=g, dtype=torch.float64))[..., 0]
        true = torch.randn((T, N, d), generator=g, dtype=torch.float64)
        pred = true + e
        mean_nees = float(evaluation.nees(pred, C, true).mean())
        assert abs(mean_nees - d) <= 3 * math.sqrt(2 * d / n), (d, mean_nees)
        cover = float(evaluation.coverage(pred, C, true, 0.95).mean())
        assert abs(cover - 0.95) <= 3 * math.sqrt(0.95 * 0.05 / n), (d, cover)
        # the NLL of a calibrated belief: E = 0.5 (d + E logdet C + d log 2 pi); 3 standard errors of the chi-square part
        nll = float(evaluation.gaussian_nll(pred, C, true).mean())
        logdet = float(torch.logdet(C[evaluation.START_TRUNCATION:]).mean())
        assert abs(nll - 0.5 * (d + logdet + d * math.log(2 * math.pi))) <= 3 * 0.5 * math.sqrt(2 * d / n), (d, nll)

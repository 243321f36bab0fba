"""ESS-triggered (adaptive) resampling where no GPU is needed: the boundary knows the two new entry points without a new ABI
version or struct field, refuses what ``include/mmf.h`` says it refuses, and ``ParticleFilter`` carries the switch."""
import ctypes
import math

import pytest

from multimodalfilter_amd import _abi

EINVAL, ETOOLARGE = -1, -2
_LOOP_FIELDS = [
    "T", "N", "M", "d", "n_meas", "resample_mode", "precision", "n_res_dyn", "n_res_meas", "logw_stride", "dyn_packed",
    "dyn_bias", "meas_packed", "meas_bias", "meas_logw", "noise", "scale_tril", "uniforms", "states_a", "states_b", "logw_a",
    "logw_b", "loglik", "estimates", "range_flag", "final_location", "events", "event_stride", "loglik_steps", "indices_steps",
    "noise_seed", "noise_step0", "noise_traj0", "noise_mode", "soft_alpha", "estimate_argmax", "estimate_scratch",
    "persistent", "n_sync_words", "sync_words", "cov_steps", "ess_steps", "log_evidence_steps"]


def test_binding_has_the_adaptive_entry_points_and_no_new_layout():
    lib = _abi.load()
    for name in ("mmf_pf_reweight_resample_adaptive", "mmf_pf_forward_loop_adaptive"):
        assert name in _abi.SIGNATURES
        assert hasattr(lib, name), name
    # purely additive: the version and the loop struct are the ones of the belief record
    assert _abi.ABI_VERSION == 42 == lib.mmf_version()
    assert [n for n, _ in _abi.MmfPfLoopArgs._fields_] == _LOOP_FIELDS


def test_adaptive_entry_points_reject_null_and_invalid_arguments():
    lib = _abi.load()
    bufs = [(ctypes.c_float * 64)() for _ in range(11)]
    P = [ctypes.cast(b, ctypes.c_void_p) for b in bufs]
    f = lib.mmf_pf_reweight_resample_adaptive
    ok = lambda **kw: f(kw.get("loglik", P[0]), kw.get("logw_in", P[1]), kw.get("states_in", P[2]), kw.get("u", P[3]),
                        kw.get("estimate", P[4]), kw.get("states_out", P[5]), kw.get("logw_out", P[6]), None,
                        kw.get("N", 0), kw.get("M", 8), kw.get("d", 3), kw.get("mode", 1), kw.get("alpha", 1.0),
                        kw.get("thr", 0.5), kw.get("resampled", P[10]), P[7], P[8], P[9], None)
    assert ok() == 0 and ok(mode=2) == 0 and ok(thr=1.0) == 0          # an empty batch is a no-op: nothing is dereferenced
    assert ok(resampled=None) == 0 and ok(logw_in=None) == 0           # optional: the decisions; uniform incoming weights
    assert ok(mode=0) == EINVAL and ok(mode=3) == EINVAL               # a threshold needs a resampling mode
    for required in ("loglik", "states_in", "estimate", "logw_out", "states_out", "u"):
        assert ok(**{required: None}) == EINVAL, required
    assert ok(states_out=P[2]) == EINVAL                               # in-place gather
    for thr in (0.0, -0.5, 1.5, math.nan, math.inf):
        assert ok(thr=thr) == EINVAL, thr
    for alpha in (0.0, -1.0, 1.5, math.nan):
        assert ok(alpha=alpha) == EINVAL, alpha
    assert ok(alpha=0.5) == 0 and ok(alpha=0.5, logw_in=None) == EINVAL  # the uniform shortcut belongs to plain resampling
    assert ok(d=5) == EINVAL and ok(M=0) == EINVAL
    # sum e^2 is reduced through the record's rows in LDS: the limits of a recording call
    assert ok(M=20200) == 0 and ok(M=20300) == ETOOLARGE and ok(M=65537) == ETOOLARGE
    assert ok(M=20200, mode=2) == 0 and ok(M=20300, mode=2) == ETOOLARGE

    g = lib.mmf_pf_forward_loop_adaptive
    a = _abi.MmfPfLoopArgs()
    assert g(None, 0.5, None, None) == EINVAL
    assert g(ctypes.byref(a), 0.5, None, None) == EINVAL               # resample_mode 0
    a.resample_mode = 1
    assert g(ctypes.byref(a), 0.5, None, None) == EINVAL               # N = 0, null fields: as mmf_pf_forward_loop checks them
    for thr in (0.0, 1.5, math.nan):
        assert g(ctypes.byref(a), thr, None, None) == EINVAL, thr


def test_particle_filter_carries_the_threshold_and_lstm_does_not():
    import multimodalfilter_amd as mmf

    for f in (mmf.door_models.DoorParticleFilter(), mmf.door_models.DoorCrossmodalParticleFilter(),
              mmf.push_models.PushCrossmodalParticleFilter()):
        assert f.resample_ess_threshold is None and f.last_resampled is None, type(f).__name__
        f.resample_ess_threshold = 0.5
        assert f.resample_ess_threshold == 0.5
        f.resample_ess_threshold = 1
        assert f.resample_ess_threshold == 1.0
        for bad in (0, 0.0, 1.5, -0.1, math.nan):
            with pytest.raises(AssertionError):
                f.resample_ess_threshold = bad
        assert f.resample_ess_threshold == 1.0                         # a refused value leaves the old one
        f.resample_ess_threshold = None
        assert f.resample_ess_threshold is None
    dyn, meas = mmf.door_models.DoorDynamicsModel(), mmf.door_models.DoorParticleFilter().measurement_model
    g = mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, resample_ess_threshold=0.25)
    assert g.resample_ess_threshold == 0.25
    for bad in (0, 1.5, math.nan):
        with pytest.raises(AssertionError):
            mmf.filters.ParticleFilter(dynamics_model=dyn, measurement_model=meas, resample_ess_threshold=bad)
    lstm = mmf.door_models.DoorLSTMFilter()
    assert not hasattr(lstm, "resample_ess_threshold") and not hasattr(lstm, "last_resampled")

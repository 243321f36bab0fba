"""CPU-side checks of regularised resampling (``include/mmf.h``: ``mmf_pf_regularise``, ``mmf_pf_forward_loop_regularised``,
``mmf_philox_normals_stream``; ``ParticleFilter.regularisation``): the boundary and what it refuses, the feasibility of the
GPU test's case set, the Philox stream against its gcc twin, and the filter's attributes."""
import ctypes
import math
import shutil

import numpy as np
import pytest
import torch

import _regularise_cases as rc
from _tol import REL_TOL

EINVAL = -1

# MmfPfLoopArgs as ABI 42 laid it down: the regularised loop adds symbols and structs of its own
_LOOP_FIELDS = ["T", "N", "M", "d", "n_meas", "resample_mode", "precision", "n_res_dyn", "n_res_meas", "logw_stride",
                "dyn_packed", "dyn_bias", "meas_packed", "meas_bias", "meas_logw", "noise", "scale_tril", "uniforms",
                "states_a", "states_b", "logw_a", "logw_b", "loglik", "estimates", "range_flag", "final_location", "events",
                "event_stride", "loglik_steps", "indices_steps", "noise_seed", "noise_step0", "noise_traj0", "noise_mode",
                "soft_alpha", "estimate_argmax", "estimate_scratch", "persistent", "n_sync_words", "sync_words", "cov_steps",
                "ess_steps", "log_evidence_steps"]


def _buffers(count=8):
    bufs = [(ctypes.c_float * 64)() for _ in range(count)]
    return bufs, [ctypes.cast(b, ctypes.c_void_p) for b in bufs]


# ------------------------------------------------------------------------------------------ 1. the binding
def test_binding_has_the_new_symbols_and_the_old_layouts():
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    for name in ("mmf_pf_regularise", "mmf_pf_forward_loop_regularised", "mmf_philox_normals_stream"):
        assert name in _abi.SIGNATURES and hasattr(lib, name), name
    assert lib.mmf_version() == _abi.ABI_VERSION == 42
    assert [n for n, _ in _abi.MmfPfLoopArgs._fields_] == _LOOP_FIELDS
    assert [n for n, _ in _abi.MmfPfHistory._fields_] == ["states_steps", "logw_in_steps", "logw_in0"]
    assert _abi.PHILOX_STREAM_JITTER == 2
    text = open(rc.os.path.join(rc.ROOT, "include", "mmf_philox.h")).read()
    assert "#define MMF_PHILOX_STREAM_JITTER 2u" in text


def test_kernel_entry_refuses_what_the_header_lists():
    """Every refusal is decided on the host before any HIP call, so the (host) pointers are never dereferenced."""
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    keep, P = _buffers()

    def args(**over):
        a = _abi.MmfPfRegulariseArgs()
        a.N, a.M, a.d, a.scale = 2, 5, 3, 1.0
        a.states, a.cov, a.ess, a.noise, a.mean = P[0], P[1], P[2], P[3], P[4]
        for k, v in over.items():
            if k == "floor":
                for i, f in enumerate(v):
                    a.floor[i] = f
            else:
                setattr(a, k, v)
        return a

    call = lambda a: lib.mmf_pf_regularise(ctypes.byref(a), None)
    assert lib.mmf_pf_regularise(None, None) == EINVAL
    for field in ("states", "cov", "ess", "noise"):               # null required pointers (noise: noise_mode 0)
        assert call(args(**{field: None})) == EINVAL, field
    for d in (0, 5, -1):
        assert call(args(d=d)) == EINVAL, d
    for scale in (0.0, -1.0, math.nan, math.inf):
        assert call(args(scale=scale)) == EINVAL, scale
    for floor in ((-0.1, 0.0, 0.0), (0.0, math.nan, 0.0), (0.0, 0.0, -1e-30)):
        assert call(args(floor=floor)) == EINVAL, floor
    assert call(args(shrink=1, mean=None)) == EINVAL              # shrinkage needs the mean
    for mode in (1, 3, -1):
        assert call(args(noise_mode=mode)) == EINVAL, mode
    assert call(args(M=0)) == EINVAL and call(args(N=-1)) == EINVAL
    # N == 0 is a successful no-op, in either noise mode; counter noise takes no tensor; a floor beyond d is not looked at
    assert call(args(N=0)) == 0
    assert call(args(N=0, noise_mode=2, noise=None)) == 0
    assert call(args(N=0, shrink=1, floor=(0.0, 0.5, 0.0, -1.0))) == 0
    assert lib.mmf_philox_normals_stream(1, 2, 0, 0, None, 2, 5, 3, None) == EINVAL
    assert lib.mmf_philox_normals_stream(1, 2, 0, 0, P[0], 2, 5, 5, None) == EINVAL
    assert lib.mmf_philox_normals_stream(1, 2, 0, 0, P[0], 0, 5, 3, None) == 0
    del keep


def test_loop_entry_refuses_what_the_header_lists():
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    keep, P = _buffers()
    a, h, r = _abi.MmfPfLoopArgs(), _abi.MmfPfHistory(), _abi.MmfPfLoopRegularise()
    f = lib.mmf_pf_forward_loop_regularised
    call = lambda hist=None, thr=0.0, took=None, reg=r: f(ctypes.byref(a), None if hist is None else ctypes.byref(hist), thr, took,
                                                         None if reg is None else ctypes.byref(reg), None)
    assert f(None, None, 0.0, None, ctypes.byref(r), None) == EINVAL
    a.T, a.N, a.M, a.d, a.n_meas, a.resample_mode = 0, 2, 5, 3, 1, 1
    for k in ("dyn_packed", "dyn_bias", "noise", "scale_tril", "uniforms", "states_a", "states_b", "logw_a", "logw_b", "loglik",
              "estimates"):
        setattr(a, k, P[0])
    r.scale, r.noise, r.cov, r.ess = 1.0, P[1], P[2], P[3]
    assert call() == 0                                            # T = 0: nothing to enqueue, every argument in order
    assert call(reg=None) == EINVAL                               # the entry IS the regularised loop
    a.resample_mode = 0
    assert call() == EINVAL                                       # no resampling, nothing to regularise
    a.resample_mode = 1
    for thr in (-0.5, 1.5, math.nan):
        assert call(thr=thr) == EINVAL, thr
    r.cov = None
    assert call() == EINVAL                                       # K1's covariance needs a place: cov_steps or the scratch
    a.cov_steps = P[4]
    assert call() == 0
    r.ess = None
    assert call() == EINVAL
    a.ess_steps = P[5]
    assert call() == 0
    assert call(thr=0.5) == EINVAL                                # the decisions need a place too
    r.resampled = P[6]
    assert call(thr=0.5) == 0
    r.noise = None
    assert call() == EINVAL                                       # a noise tensor, or noise_mode 2
    r.noise_mode = 2
    assert call() == 0
    r.noise_mode = 1
    assert call() == EINVAL
    r.noise_mode = 2
    # with a history: what mmf_pf_forward_loop_history refuses (a history that passes goes on to the runtime -- the copy of
    # the incoming log-weights -- and is the GPU test's)
    assert call(hist=h) == EINVAL
    h.states_steps, h.logw_in0 = P[0], P[1]
    assert call(hist=h) == EINVAL                                 # loglik_steps / indices_steps
    a.loglik_steps = P[2]
    assert call(hist=h) == EINVAL
    a.indices_steps = P[3]
    assert call(hist=h, thr=0.5) == EINVAL                        # the weights travel: logw_in_steps
    a.soft_alpha = 0.5
    assert call(hist=h) == EINVAL
    del keep


# ------------------------------------------------------------------------------------------ 2. the case set is feasible
@pytest.mark.parametrize("M,d", rc.SHAPES)
def test_case_set_is_feasible_in_float32(M, d):
    """The definition evaluated in float32 numpy stays within ``REL_TOL / 2`` of itself in float64 on every case of the GPU
    test -- states, factor and bandwidth --, so a correct fp32 kernel can meet ``REL_TOL``.  Measured: at most 2.9e-5 on the
    states (row by row, ``_regularise_cases.rel_err_rows``), 2.2e-7 on the factor, 1e-7 on the bandwidth."""
    c = rc.make_case(M, d)
    for shrink in (False, True):
        for floor in rc.FLOORS:
            kw = dict(scale=rc.SCALE, floor=floor, shrink=shrink, resampled=c["resampled"])
            want = rc.reference(c["x"], c["mu"], c["C"], c["ess"], c["eps"], dtype=np.float64, **kw)
            got = rc.reference(c["x"], c["mu"], c["C"], c["ess"], c["eps"], dtype=np.float32, **kw)
            errs = (rc.rel_err_rows(got[0], want[0], dims=1), rc.rel_err_rows(got[1][:, None], want[1][:, None]),
                    rc.rel_err_rows(got[2][:, None, None], want[2][:, None, None], dims=1))
            assert max(errs) <= REL_TOL / 2, (shrink, floor, errs)
            # the rows the definition leaves alone, and what it reports for them
            for n in rc.UNCHANGED_ROWS:
                assert np.array_equal(want[0][n], c["x"][n].astype(np.float64)) and not want[1][n].any()
            assert np.isnan(want[2][rc.ROW_NAN_ESS]) and want[2][rc.ROW_KEPT] == 0 and want[2][rc.ROW_NAN_COV] > 0
            moved = np.abs(want[0][rc.ROW_RANK][:, -1] - c["x"][rc.ROW_RANK][:, -1]).max()
            assert (moved > 0) == (floor > 0), (floor, moved)     # a collapsed direction moves only with a floor
            assert (np.abs(want[0][rc.ROW_ZERO] - c["x"][rc.ROW_ZERO]).max() > 0) == (floor > 0)
            assert (want[0][:7] != c["x"][:7]).mean() > 0.99      # the regular rows move


def test_reference_statistics_and_formulas():
    """The restatement is the textbook: Silverman's factor, a Cholesky factor where the matrix is positive definite, and a
    set whose covariance grows by ``1 + h^2`` without shrinkage and stays put with it."""
    assert abs(rc.silverman(100.0, 1, 1.0) - (4.0 / 300.0) ** 0.2) < 1e-15
    assert abs(rc.silverman(50.0, 3, 2.0) - 2.0 * (4.0 / 250.0) ** (1.0 / 7.0)) < 1e-15
    rng = np.random.default_rng(0)
    A = np.eye(3) + 0.3 * rng.standard_normal((3, 3))
    C = A @ A.T
    assert np.allclose(rc.clamped_cholesky(C, np.zeros(3)), np.linalg.cholesky(C), atol=1e-13)
    L = rc.clamped_cholesky(np.diag([1.0, 0.0, 4.0]), np.array([0.0, 0.5, 0.0]))
    assert np.array_equal(L, np.diag([1.0, 0.5, 2.0]))
    assert not rc.clamped_cholesky(np.full((2, 2), np.nan), np.zeros(2)).any()
    M = 200000
    x = rng.standard_normal((1, M, 3)) @ A.T
    mu, Cs = x[0].mean(0)[None], np.cov(x[0].T, bias=True)[None]
    eps = rng.standard_normal((1, M, 3))
    for shrink, growth in ((False, None), (True, 1.0)):
        out, factor, h = rc.reference(x, mu, Cs, np.array([40.0]), eps, scale=1.0, floor=0.0, shrink=shrink)
        growth = 1.0 + h[0] ** 2 if growth is None else growth
        assert np.allclose(np.cov(out[0].T, bias=True), growth * Cs[0], rtol=2e-2, atol=2e-2)
        assert np.allclose(out[0].mean(0), mu[0], atol=1e-2)
        assert np.allclose(factor[0] @ factor[0].T, h[0] ** 2 * Cs[0], rtol=1e-10)


# ------------------------------------------------------------------------------------------ 3. Philox
@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_philox_stream_function_keeps_the_old_bits_and_separates_streams(tmp_path):
    exe = rc.build_philox(tmp_path)
    z0, legacy_equal = rc.philox_normals(exe, 99, 0, 3, 5, 4, 33)
    assert legacy_equal, "mmf_philox_normal4 must be stream 0 of mmf_philox_normal4_stream, bit for bit"
    z2, _ = rc.philox_normals(exe, 99, 2, 3, 5, 4, 33)
    assert z0.shape == z2.shape == (4, 33, 4) and np.isfinite(z0).all() and np.isfinite(z2).all()
    assert not np.array_equal(z0.view(np.uint32), z2.view(np.uint32))
    assert (z0 == z2).mean() < 0.01                               # another stream, not a few other draws
    assert abs(z2.mean()) < 0.2 and 0.8 < z2.std() < 1.2
    from oracle import strict

    if strict.available():  # the twin the rest of the suite uses draws the same stream-0 bits
        strict.build()
        assert np.array_equal(np.asarray(strict.philox_normals(99, 3, 4, 33, 4, traj0=5), dtype=np.float32).view(np.uint32),
                              z0.view(np.uint32))


# ------------------------------------------------------------------------------------------ 4. the filter's attributes
def _filter():
    import multimodalfilter_amd as mmf

    return mmf.door_models.DoorParticleFilter()


def test_filter_defaults_and_refused_values():
    from multimodalfilter_amd import utils

    f = _filter().eval()
    assert f.regularisation is None and f.regularisation_floor == 0.0 and f.regularisation_shrink is False
    assert type(f.regularisation_noise) is utils.NoiseSource and f.regularisation_noise.seed == 1 and f.noise.seed == 0
    assert f.last_regularisation is None and f._regularisation_args() is None
    f.regularisation = 1
    assert f.regularisation == 1.0 and type(f.regularisation) is float
    for bad in (0.0, -1.0, math.nan, math.inf, True, "1.0"):
        with pytest.raises(ValueError, match="^regularisation must be None or a finite float > 0"):
            f.regularisation = bad
    assert f.regularisation == 1.0                                # a refused value changes nothing
    d = f.state_dim
    f.regularisation_floor = 0.05
    f.regularisation_floor = (0.0,) * (d - 1) + (0.1,)
    assert f._regularisation_args() == (1.0, [0.0] * (d - 1) + [0.1], False)
    for bad in (-0.1, math.nan, math.inf, (0.0,) * (d + 1), (0.0,) * (d - 1) + (-1.0,)):
        with pytest.raises(ValueError, match="^regularisation floor must be"):
            f.regularisation_floor = bad
    assert f.regularisation_floor == (0.0,) * (d - 1) + (0.1,)
    f.regularisation = None
    assert f._regularisation_args() is None


def test_filter_refuses_training_mode_and_a_shared_counter_stream():
    import multimodalfilter_amd as mmf

    f = _filter()
    f.train()
    with pytest.raises(RuntimeError, match="^regularisation: the training"):
        f.regularisation = 1.0
    f.eval()
    f.regularisation = 1.0
    f.train()                                                     # switched to training with the switch set: the step raises
    with pytest.raises(RuntimeError, match="^regularisation: the training"):
        f._regularisation_args()
    f._initialized = True
    f.particle_states, f.particle_log_weights = torch.zeros((2, 4, f.state_dim)), torch.zeros((2, 4))
    for step in (f._step, f._step_autograd):                      # whichever path a training-mode forward takes
        with pytest.raises(RuntimeError, match="^regularisation: the training"):
            step({}, torch.zeros((2, 7)))
    f.eval()
    # a counter source of the jitter on the (seed, stream) of the process noise
    assert mmf.CounterNoise.JITTER == 2 and mmf.CounterNoise(3).stream == 0
    f.noise = mmf.CounterNoise(5)
    f.regularisation_noise = mmf.CounterNoise(5, stream=mmf.CounterNoise.JITTER)     # the same seed on the jitter stream: fine
    f.regularisation_noise = mmf.CounterNoise(6)                                     # another seed: fine
    with pytest.raises(ValueError, match=r"^regularisation_noise shares \(seed, stream\) = \(5, 0\)"):
        f.regularisation_noise = mmf.CounterNoise(5)
    assert f.regularisation_noise.seed == 6
    f.noise = mmf.CounterNoise(6)                                 # ... also when the process noise is replaced afterwards
    with pytest.raises(ValueError, match=r"^regularisation_noise shares"):
        f._regularisation_args()
    with pytest.raises(AssertionError):
        mmf.CounterNoise(1, stream=1)                             # stream 1 is the resampling uniforms'

"""The innovation statistics' references and inputs, certified without a GPU (``tests/_innovation_cases.py``), and everything
of the feature that is decided on the host: the binding and the argument checks of ``mmf_ekf_step_innov`` /
``mmf_ekf_forward_loop_innov``, and the refusals and defaults of the two switches."""
import ctypes
import itertools
import math
import os
import re

import numpy as np
import pytest
import torch

import _innovation_cases as ic
from _tol import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _col(t):
    return torch.as_tensor(t)[..., None]  # (K, N) scalars as vectors of length 1: every entry against its own magnitude


# ------------------------------------------------------------------------------ the input conditions
@pytest.mark.parametrize("N,d", list(itertools.product(ic.NS, ic.DIMS)))
def test_step_inputs_are_bimodal_and_keep_the_fp32_yardstick_under_the_caps(N, d):
    """On every step case: no fp64 NIS lies in ``NIS_MARGIN = [6, 24]`` around the gate of 12 -- the inliers are below 6 and
    the outliers above 24, where the construction put them -- so an fp32 evaluation (relative error measured here: under
    2e-6) cannot flip a decision and no GPU comparison ever has to exclude a row; cases of at least 255 rows have both
    classes in every sub-filter; and the fp32 yardstick (``torch.linalg.solve`` / ``slogdet`` in fp32) is within the caps the
    module records of the fp64 truth on every output, gated and ungated -- conditions on the inputs, reseeded where a draw
    breaks one (``RESEED``).  The last line makes the GPU rule's bar ``max(1e-4, 3 x yardstick)`` explicit: 1e-4 for the NIS
    and the log-likelihood of every case."""
    for K, fusion in ic.STEP_COMBOS:
        c = ic.step_case(N, d, K)
        for gate in (None, ic.GATE):
            want = ic.step_reference(N, d, K, fusion, torch.float64, gate)
            yard = ic.step_reference(N, d, K, fusion, torch.float32, gate)
            nis = want["nis"].numpy()
            assert not ((nis >= ic.NIS_MARGIN[0]) & (nis <= ic.NIS_MARGIN[1])).any(), (N, d, K)
            assert np.array_equal(nis > ic.GATE, c["outlier"]), (N, d, K)
            if gate is None:
                assert bool(want["accepted"].all())
            else:
                assert np.array_equal(~want["accepted"].numpy(), c["outlier"])
                assert np.array_equal((yard["nis"] <= gate).numpy(), want["accepted"].numpy())  # fp32 decides the same
            if N >= 255:
                assert c["outlier"].any(axis=1).all() and (~c["outlier"]).any(axis=1).all(), (N, d, K)
            for k in ("nis", "log_likelihood"):
                err = rel_err(_col(yard[k]), _col(want[k]), dims=1)
                assert err < ic.CAP_INNOV and 3.0 * err < 1e-4, (N, d, K, gate, k, err)
            for k in ("mu", "Sigma"):
                err = rel_err(yard[k], want[k])
                assert err < ic.CAP_INNOV, (N, d, K, gate, k, err)
            for k in ("mu_f", "Sigma_f"):
                if fusion:
                    err = rel_err(yard[k], want[k])
                    assert err < ic.CAP_INNOV_FUSED, (N, d, K, fusion, gate, k, err)
            if gate is not None and N >= 255:  # the gate changes the beliefs: the gated reference is another answer
                free = ic.step_reference(N, d, K, fusion, torch.float64, None)
                assert float((free["mu"] - want["mu"]).abs().max()) > 1e-2


def test_step_observations_sit_where_the_construction_put_them():
    """``z = mu- + c chol(S) u``: the fp64 NIS of the float32 observations is ``c^2`` inside its class's range, up to the
    rounding of ``z`` (a relative 1e-5 at most, measured)."""
    for N, d, K in ((257, 1, 4), (255, 3, 2), (257, 4, 4)):
        c = ic.step_case(N, d, K)
        nis = ic.step_reference(N, d, K, 0, torch.float64)["nis"].numpy()
        lo, hi = np.where(c["outlier"], ic.OUTLIER_C2[0], ic.INLIER_C2[0]), np.where(c["outlier"], ic.OUTLIER_C2[1], ic.INLIER_C2[1])
        assert ((nis > lo * (1 - 1e-4)) & (nis < hi * (1 + 1e-4))).all()
        assert not np.array_equal(c["z"], np.array(ic.kc.step_case(N, d, K)["z"]))


# ------------------------------------------------------------------------------ the recursion against an independent truth
def test_summed_log_likelihood_equals_the_dense_joint_log_density():
    """The fp64 Kalman filter's ``sum_t log_likelihood[t]`` per trajectory against ``log N(y_{0:T-1}; m, C)`` of the joint
    Gaussian of all observations, built densely with no recursion: 1e-10 relative."""
    c = ic.lg_case()
    assert c["y"].shape == (6, 5, 2) and c["gate"] is None and bool(c["accepted"].all())
    dense = ic.dense_log_density(ic.LG_D, c["y"])
    summed = c["log_likelihood"].sum(axis=0)
    err = float(np.abs(summed - dense).max() / np.abs(dense).max())
    print(f"recursion vs dense: {err:.3e}", dense)
    assert err < 1e-10
    # another model is another density: the truth notices a shift of the controls by one step
    shifted = ic.kalman_filter(ic.LG_D, np.roll(np.array(c["y"]), 1, axis=0))["log_likelihood"].sum(axis=0)
    assert float(np.abs(shifted - dense).max()) > 1e-2


def test_the_displaced_observations_are_the_rejected_ones_in_fp64():
    """The gated copy: exactly the four displaced observations are rejected by the fp64 filter, every other NIS is at
    least 5 % away from the gate (an fp32 NIS is good to 1e-4 here), and the gate changes the estimates."""
    c, clean = ic.lg_case(displaced=True), ic.lg_case()
    assert c["gate"] == ic.GATE
    rejected = sorted(map(tuple, np.argwhere(~c["accepted"]).tolist()))
    assert rejected == sorted(ic.DISPLACED) and len(rejected) == 4
    assert (np.abs(c["nis"] / ic.GATE - 1.0) > 0.05).all()
    assert float(c["nis"][~c["accepted"]].min()) > 2.0 * ic.NIS_MARGIN[1]
    moved = np.abs(np.array(c["y"]) - np.array(clean["y"])).sum(-1) > 0
    assert sorted(map(tuple, np.argwhere(moved).tolist())) == sorted(ic.DISPLACED)
    ungated = ic.kalman_filter(ic.LG_D, np.array(c["y"]))
    assert float(np.abs(ungated["mean"] - c["mean"]).max()) > 0.1
    # a rejected step keeps the prediction: the covariance grows there instead of shrinking
    t, n = ic.DISPLACED[0]
    assert np.trace(c["cov"][t, n]) > np.trace(ungated["cov"][t, n])


# ------------------------------------------------------------------------------ binding and ABI
def test_both_entries_are_bound_and_the_abi_number_stays():
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    assert lib.mmf_version() == _abi.ABI_VERSION == 42
    for name in ("mmf_ekf_step_innov", "mmf_ekf_forward_loop_innov"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    text = open(os.path.join(ROOT, "include", "mmf.h")).read()
    for name in ("mmf_ekf_step_innov", "mmf_ekf_forward_loop_innov"):
        assert re.search(r"^int\s+%s\s*\(" % name, text, re.M), name
    assert len(_abi.SIGNATURES["mmf_ekf_step_innov"][1]) == len(_abi.SIGNATURES["mmf_ekf_step_gated"][1]) + 4
    assert [n for n, _ in _abi.MmfEkfLoopArgs._fields_][-1] == "sync_words"  # the loop's struct has not grown


def test_innov_args_layout_matches_the_header(tmp_path):
    """``_abi.MmfEkfInnovArgs`` against ``include/mmf.h`` as a C compiler lays it out (``sizeof`` / ``offsetof`` from a small
    C program, the header compiled as plain C), field by field."""
    import shutil
    import subprocess

    from multimodalfilter_amd import _abi

    cls = _abi.MmfEkfInnovArgs
    assert [n for n, _ in cls._fields_] == ["nis_gate", "nis_steps", "loglik_steps", "accepted_steps"]
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(MmfEkfInnovArgs));']
    lines += [f'  printf("{f} %zu\\n", offsetof(MmfEkfInnovArgs, {f}));' for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    out = subprocess.run([gcc, "-std=c99", "-o", str(exe), str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(line.split() for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f, t in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f
    last, last_t = cls._fields_[-1]
    assert getattr(cls, last).offset + ctypes.sizeof(last_t) == ctypes.sizeof(cls)  # no field hides behind the last


_STEP_NAMES = ("A", "mu_pred", "q_tril", "z", "r_tril", "fuse_w", "mu", "Sigma", "mu_f", "Sigma_f")


def _step_call(lib, keep, N=4, d=3, K=2, fusion=1, gate=-1.0, **over):
    """``mmf_ekf_step_innov`` over host buffers of 16 KiB each, far apart: the checks are made before any HIP call and never
    dereference them.  ``over``: operand name -> replacement (``None``: null)."""
    P = {k: ctypes.cast(keep[k], ctypes.c_void_p) for k in keep}
    P.update(over)
    return lib.mmf_ekf_step_innov(*[P[k] for k in _STEP_NAMES], N, d, K, fusion, 0, P["feedback_gate"], ctypes.c_float(gate),
                                  P["nis"], P["loglik"], P["accepted"], None)


def test_step_entry_argument_checks_need_no_gpu():
    """Every ``MMF_EINVAL`` and no-op case of ``mmf_ekf_step_innov``, with host pointers only."""
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    keep = {k: (ctypes.c_float * 4096)() for k in _STEP_NAMES + ("feedback_gate", "nis", "loglik", "accepted")}
    assert _step_call(lib, keep, N=0) == 0                                      # nothing to do: a successful no-op
    assert _step_call(lib, keep, N=0, nis=None, loglik=None, accepted=None) == 0
    assert _step_call(lib, keep, N=-1) == EINVAL
    for d in (0, 5):
        assert _step_call(lib, keep, N=0, d=d) == EINVAL, d
    for K in (0, 5):
        assert _step_call(lib, keep, N=0, K=K) == EINVAL, K
    for fusion in (-1, 3):
        assert _step_call(lib, keep, N=0, fusion=fusion) == EINVAL
    for k in ("A", "mu_pred", "q_tril", "z", "r_tril", "mu", "Sigma", "fuse_w", "mu_f", "Sigma_f"):
        assert _step_call(lib, keep, N=0, **{k: None}) == EINVAL, k           # (fuse_w / mu_f / Sigma_f: fusion 1 needs them)
    assert _step_call(lib, keep, N=0, fusion=0, fuse_w=None, mu_f=None, Sigma_f=None, feedback_gate=None) == 0
    assert _step_call(lib, keep, N=0, gate=float("nan")) == EINVAL
    at = lambda k, off=0: ctypes.c_void_p(ctypes.addressof(keep[k]) + off)
    for out, inp in (("nis", "z"), ("loglik", "A"), ("accepted", "r_tril"), ("mu", "mu_pred"), ("Sigma", "A"), ("mu_f", "fuse_w"),
                     ("nis", "loglik"), ("accepted", "nis"), ("nis", "mu"), ("loglik", "Sigma"), ("Sigma_f", "z")):
        assert _step_call(lib, keep, **{out: at(inp)}) == EINVAL, (out, inp)    # an output on top of an input / another output
    assert _step_call(lib, keep, nis=at("z", 8)) == EINVAL                      # ... or only partly on top of it
    assert _step_call(lib, keep, N=0, nis=at("z")) == 0                         # (empty ranges overlap nothing)


def _loop_args(T=3, N=4, d=3, K=2, fusion=1):
    from multimodalfilter_amd import _abi

    a, i, keep = _abi.MmfEkfLoopArgs(), _abi.MmfEkfInnovArgs(), {}
    a.T, a.N, a.d, a.K, a.fusion, a.feedback, a.n_res_dyn, a.precision = T, N, d, K, fusion, 0, 3, _abi.PREC_F32
    page = lambda k: ctypes.cast(keep.setdefault(k, (ctypes.c_float * 8192)()), ctypes.c_void_p)
    for k in ("q_tril", "z", "r_tril", "fuse_w", "mu", "Sigma", "mu_pred", "A", "Sigma_f", "estimates"):
        setattr(a, k, page(k))
    for k in range(_abi.LOOP_MAX_MEAS):
        a.dyn_packed[k], a.dyn_bias[k] = page(f"packed{k}"), page(f"bias{k}")
    i.nis_gate = -1.0
    i.nis_steps, i.loglik_steps, i.accepted_steps = page("nis"), page("loglik"), page("accepted")
    return a, i, keep


def test_loop_entry_argument_checks_need_no_gpu():
    """Every ``MMF_EINVAL`` and no-op case of ``mmf_ekf_forward_loop_innov``, with host pointers only."""
    from multimodalfilter_amd import _abi

    lib = _abi.load()
    call = lambda a, i, steps=None: lib.mmf_ekf_forward_loop_innov(ctypes.byref(a), ctypes.byref(i), steps, None)
    a, i, keep = _loop_args()
    assert lib.mmf_ekf_forward_loop_innov(None, ctypes.byref(i), None, None) == EINVAL
    assert lib.mmf_ekf_forward_loop_innov(ctypes.byref(a), None, None, None) == EINVAL
    for T, N in ((0, 4), (3, 0), (0, 0)):                                       # nothing to do: a successful no-op
        a, i, keep = _loop_args(T=T, N=N)
        a.persistent = 1                                                         # (ignored)
        assert call(a, i) == 0, (T, N)
        i.nis_steps = i.loglik_steps = i.accepted_steps = None                   # any of the three may be null
        assert call(a, i) == 0
    for kw in ({"T": -1}, {"N": -1}, {"d": 0}, {"d": 5}, {"K": 0}, {"K": 5}, {"fusion": 3}, {"fusion": -1}):
        a, i, keep = _loop_args(**{"T": 0, **kw})
        assert call(a, i) == EINVAL, kw
    for k in ("q_tril", "z", "r_tril", "fuse_w", "mu", "Sigma", "mu_pred", "A", "Sigma_f", "estimates"):
        a, i, keep = _loop_args(T=0)
        setattr(a, k, None)
        assert call(a, i) == EINVAL, k
    a, i, keep = _loop_args(T=0)
    a.dyn_bias[1] = None
    assert call(a, i) == EINVAL
    a, i, keep = _loop_args(T=0)
    i.nis_gate = float("nan")
    assert call(a, i) == EINVAL
    for out, inp in (("nis_steps", "z"), ("loglik_steps", "r_tril"), ("accepted_steps", "fuse_w"), ("nis_steps", "mu"),
                     ("loglik_steps", "Sigma"), ("accepted_steps", "estimates"), ("nis_steps", "A"), ("loglik_steps", "q_tril")):
        a, i, keep = _loop_args()
        setattr(i, out, getattr(a, inp))                                         # a record on top of an operand of the loop
        assert call(a, i) == EINVAL, (out, inp)
    a, i, keep = _loop_args()
    i.loglik_steps = ctypes.c_void_p(i.nis_steps + 16)                           # ... or partly on top of another record
    assert call(a, i) == EINVAL
    a, i, keep = _loop_args()
    steps = ctypes.cast((ctypes.c_float * 8192)(), ctypes.c_void_p)
    i.accepted_steps = steps                                                     # ... or on top of Sigma_steps
    assert call(a, i, steps) == EINVAL


# ------------------------------------------------------------------------------ the switches: defaults and refusals
def _kalman_filters():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import filters

    dyn, sensor = ic.rc.lg_filter_models(2, "cpu")
    types = mmf.model_types("door")
    return {"ekf": filters.VirtualSensorExtendedKalmanFilter(dynamics_model=dyn, virtual_sensor_model=sensor).eval(),
            "ukf": filters.VirtualSensorUnscentedKalmanFilter(dynamics_model=dyn, virtual_sensor_model=sensor).eval(),
            "crossmodal": types["DoorCrossmodalKalmanFilter"]().eval(), "unimodal": types["DoorUnimodalKalmanFilter"]().eval()}


def test_defaults_on_all_four_filter_classes():
    from multimodalfilter_amd import base_models, filters

    fs = _kalman_filters()
    assert isinstance(fs["crossmodal"], base_models.CrossmodalKalmanFilter) and isinstance(fs["unimodal"], base_models.UnimodalKalmanFilter)
    assert type(fs["ukf"]) is filters.VirtualSensorUnscentedKalmanFilter
    for name, f in fs.items():
        assert f.record_innovations is False and f.innovation_gate is None and f.last_innovations is None, name
        assert "record_innovations" not in f.state_dict() and not any("innovation" in k for k in f.state_dict()), name
    for name in ("crossmodal", "unimodal"):  # the smoothing line stays closed for the fused filters
        assert not hasattr(fs[name], "record_history") and not hasattr(fs[name], "default_smooth_method")
        for sub in fs[name].filter_models:
            assert sub.record_innovations is False and sub.innovation_gate is None


def test_innovation_gate_refuses_anything_but_none_or_a_positive_float():
    for name, f in _kalman_filters().items():
        for bad in (0, 0.0, -1.0, "12", True, float("nan"), float("inf"), [12.0]):
            with pytest.raises(ValueError, match="innovation_gate"):
                f.innovation_gate = bad
            assert f.innovation_gate is None, (name, bad)
        f.innovation_gate = 12
        assert f.innovation_gate == 12.0 and isinstance(f.innovation_gate, float)
        f.innovation_gate = None
        assert f.innovation_gate is None


def test_training_mode_refuses_either_switch_by_name():
    from multimodalfilter_amd import engine

    was = engine.TRAINING_BACKEND
    engine.set_training_backend("autograd")
    try:
        for name, f in _kalman_filters().items():
            f.train()
            fused = name in ("crossmodal", "unimodal")
            ctrl = torch.zeros((2, 3, 7 if fused else 1))
            obs = torch.zeros((2, 3, 2))
            for switch, value in (("record_innovations", True), ("innovation_gate", 12.0)):
                setattr(f, switch, value)
                with pytest.raises(RuntimeError, match=switch):
                    f.forward_loop(observations=obs, controls=ctrl)
                with pytest.raises(RuntimeError, match=switch):
                    f(observations=obs[0], controls=ctrl[0])
                setattr(f, switch, False if switch == "record_innovations" else None)
            f.eval()
    finally:
        engine.set_training_backend(was)


def test_run_filter_refuses_a_filter_without_the_switch_before_it_runs():
    import inspect

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    p = inspect.signature(evaluation.run_filter).parameters["return_innovations"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(evaluation.fit_process_noise).parameters["return_log_likelihood"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    types = mmf.model_types("door")
    without = [types["DoorParticleFilter"](), types["DoorCrossmodalParticleFilter"](), mmf.door_models.DoorLSTMFilter()]
    for f in without:
        with pytest.raises(ValueError, match="return_innovations"):  # (traj=None: it never gets as far as the data)
            evaluation.run_filter(f, None, return_innovations=True)
    with pytest.raises(ValueError, match="return_log_likelihood"):
        evaluation.fit_process_noise(types["DoorParticleFilter"](), None, return_log_likelihood=True)
    with pytest.raises(TypeError, match="return_innovations"):
        evaluation.fit_process_noise(types["DoorKalmanFilter"](), None, return_innovations=True)


def test_innovation_summary_on_hand_made_records():
    from multimodalfilter_amd import base, evaluation

    nis = torch.tensor([[1.0, 3.0, 50.0], [2.0, 2.0, 2.0]])
    ll = torch.tensor([[-1.0, -2.0, -30.0], [-1.5, -1.5, -1.5]])
    acc = torch.tensor([[True, True, False], [True, True, True]])
    single = evaluation.innovation_summary(base.belief_record(nis=nis, log_likelihood=ll, accepted=acc, sub_filters=None), 2)
    assert math.isclose(float(single["mean_nis"]), 10.0) and math.isclose(float(single["nis_over_dim"]), 5.0)
    assert math.isclose(float(single["accepted_fraction"]), 5.0 / 6.0) and math.isclose(float(single["log_likelihood"]), -7.5)
    fused = evaluation.innovation_summary(base.belief_record(nis=nis[None], log_likelihood=ll[None], accepted=acc[None], sub_filters=2), 2)
    assert fused["mean_nis"].tolist() == [18.0, 2.0] and fused["log_likelihood"].tolist() == [-3.0, -4.5]
    assert torch.allclose(fused["accepted_fraction"], torch.tensor([2.0 / 3.0, 1.0], dtype=torch.float64))
    with pytest.raises(ValueError, match="record_innovations"):
        evaluation.innovation_summary(base.belief_record(covariance=nis), 2)
    with pytest.raises(ValueError, match="dim"):
        evaluation.innovation_summary(base.belief_record(nis=nis, log_likelihood=ll, accepted=acc, sub_filters=None), 0)

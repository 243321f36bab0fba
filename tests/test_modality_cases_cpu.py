"""CPU-side checks of the modality attribution (``include/mmf.h``: "Per-modality attribution"): the fp64 reference of
``tests/_modality_cases.py`` satisfies the identities the header lists, on the whole family; the family's inputs meet the cap
(the same definition in fp32 torch ops stays within ``REL_TOL / 3`` of the reference); the struct of the binding is the
header's, field by field; ``mmf_pf_modalities`` refuses on the host what it must; ``evaluation.modality_summary`` /
``modality_errors`` on hand-made records; and the ``ValueError``s of ``ParticleFilter.belief_modalities`` and
``evaluation.run_filter(return_modalities=)`` that need no device."""
import ctypes
import inspect
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import _modality_cases as mc
import _smooth_cases as sc
from _tol import REL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("states", "log_w", "modality_logw")
_OUTPUTS = mc.OUTPUTS
_POINTERS = _INPUTS + _OUTPUTS


# ------------------------------------------------------------------------------------------ 1. the reference's identities
@pytest.mark.parametrize("M", mc.MS)
def test_the_reference_satisfies_the_identities_of_the_definition(M):
    tol = 1e-9
    for M_, d, R, K, variant in mc.family():
        if M_ != M:
            continue
        case, ref = mc.family_case(M, d, R, K, variant)
        what = (M, d, R, K, variant)
        le, rho, ess, mean, div, ov = (ref[k] for k in mc.OUTPUTS)
        b = np.zeros((R, K)) if case["beta"] is None else case["beta"].astype(np.float64)
        for r in range(R):
            if np.isnan(le[r]).all():                                 # a set without a live particle: NaN everywhere
                assert variant == "dead_row" and r == R // 2, what
                assert all(np.isnan(ref[k][r]).all() for k in mc.OUTPUTS), what
                continue
            has = le[r] > -np.inf
            assert not np.isnan(le[r]).any() and bool((rho[r][~has[:K]] == 0).all()), what
            assert np.isnan(ess[r][~has]).all() and np.isnan(mean[r][~has]).all() and np.isnan(div[r][~has[:K]]).all(), what
            assert np.isnan(ov[r][~has[:K]]).all() and np.isnan(ov[r][:, ~has[:K]]).all(), what
            if not has[K]:                                            # every modality blacked out
                assert not has.any(), what
                continue
            assert abs(rho[r].sum() - 1.0) < tol, what                # the responsibilities sum to 1
            on = has[:K]
            assert np.allclose((rho[r][on, None] * mean[r][:K][on]).sum(0), mean[r][K], rtol=0, atol=1e-9), what  # W = sum rho_k W^k
            assert bool((div[r][on] >= -tol).all()) and bool((div[r][on] <= -np.log(rho[r][on]) + tol).all()), what
            assert bool((ess[r][has] >= 1 - tol).all()) and bool((ess[r][has] <= M + tol).all()), what
            o = ov[r][np.ix_(on, on)]
            assert bool((o == o.T).all()) and bool((o <= 1 + tol).all()) and bool((o >= 0).all()), what
            assert np.allclose(np.diag(o), 1.0, rtol=0, atol=tol), what
            if K == 1:
                assert abs(rho[r, 0] - 1.0) < tol and abs(div[r, 0]) < tol and abs(le[r, 0] + b[r, 0] - le[r, 1]) < tol, what
                if case["beta"] is None:
                    assert le[r, 0] == le[r, 1], what
            if variant == "identical":
                soft = np.exp(b[r] - np.log(np.exp(b[r]).sum()))
                assert np.allclose(rho[r], soft, rtol=0, atol=tol) and np.allclose(div[r], 0, atol=tol) and np.allclose(o, 1, atol=tol), what
            if variant == "disjoint" and K >= 2:
                assert not (has[0] and has[1]) or ov[r, 0, 1] == 0.0, what
                if K == 2 and has[0] and has[1]:
                    assert np.allclose(div[r], -np.log(rho[r]), rtol=0, atol=1e-9), what
            if variant == "blackout" and r == R // 2:
                assert not has[K - 1] and le[r, K - 1] == -np.inf, what


def test_the_reference_gives_a_log_weight_of_minus_infinity_no_share():
    for K in (1, 2, 3):
        case = dict(mc.make_case(65, 3, 3, K, "plain"))
        beta = case["beta"].copy()
        beta[:, 0] = -np.inf
        beta[1] = -np.inf
        case["beta"] = beta
        ref = mc.reference(case)
        rho, le = ref["responsibility"], ref["log_evidence"]
        assert bool((rho[:, 0] == 0).all()) and bool((rho[1] == 0).all()) and not np.isnan(rho).any()
        assert bool(np.isfinite(le[:, :K]).all()) and le[1, K] == -np.inf and bool(np.isfinite(le[[0, 2], K]).all()) == (K > 1)
        assert np.isnan(ref["divergence"][1]).all() and np.isnan(ref["mean"][1, K]).all() and np.isnan(ref["ess"][1, K])
        if K > 1:
            assert np.allclose(rho[[0, 2]].sum(-1), 1.0, rtol=0, atol=1e-12)
        import torch
        errs = mc.compare(case, mc.torch_formulation(case, dtype=torch.float64), ref, f"K={K}")
        assert max(errs.values()) < 1e-10, errs


def test_the_family_covers_every_variant_at_every_size_and_the_edges_of_the_plan():
    fam = list(mc.family())
    assert len(fam) == len(set(fam))
    for M in mc.MS:
        assert {v for M_, _, _, _, v in fam if M_ == M} == set(mc.VARIANTS), M
        assert (M, 4, 1, 4, "plain") in fam or M <= mc.SMALL
    for M in (64 * mc.RUN_PT, 64 * mc.RUN_PT + 1, 128 * mc.RUN_PT, 128 * mc.RUN_PT + 1, mc.THREADS * mc.RUN_PT, mc.THREADS * mc.RUN_PT + 1,
              2 * mc.THREADS * mc.RUN_PT, 2 * mc.THREADS * mc.RUN_PT + 1):
        assert M in mc.MS, M                                          # one wave | two | three; one batch | two | three
    assert {K for _M, _d, _R, K, _v in fam} == set(mc.KS)
    assert {(K, d) for M, d, _, K, _ in fam if M <= mc.SMALL} == {(K, d) for K in mc.KS for d in mc.DIMS}


# ------------------------------------------------------------------------------------------ 2. the cap on the inputs
@pytest.mark.parametrize("M", mc.MS)
def test_fp32_torch_formulation_stays_within_the_cap_on_the_family(M):
    worst = {}
    for M_, d, R, K, variant in mc.family():
        if M_ != M:
            continue
        case, ref = mc.family_case(M, d, R, K, variant)
        errs = mc.compare(case, mc.torch_formulation(case), ref, f"M={M} d={d} R={R} K={K} {variant}")
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
    print(f"M={M}: fp32 torch formulation, worst " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()) + f" (cap {mc.CAP:.1e})")
    for k, e in worst.items():
        assert e <= mc.CAP, (M, k, e)
    assert mc.CAP == REL_TOL / 3


def test_fp64_torch_formulation_is_the_reference():
    import torch

    for M, d, R, K, variant in ((65, 3, 3, 2, "plain"), (257, 4, 3, 4, "blackout"), (64, 2, 3, 3, "dead_row"), (255, 1, 1, 2, "disjoint"),
                                (63, 3, 3, 3, "nan_loglik"), (256, 2, 1, 4, "uniform")):
        case, ref = mc.family_case(M, d, R, K, variant)
        errs = mc.compare(case, mc.torch_formulation(case, dtype=torch.float64), ref, variant)
        assert max(errs.values()) < 1e-10, (variant, errs)


# ------------------------------------------------------------------------------------------ 3. struct, header, binding
def test_struct_header_and_binding_are_tied(tmp_path):
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == _abi.ABI_VERSION == 42
    text = open(os.path.join(ROOT, "include", "mmf.h")).read()
    assert int(re.search(r"^#define MMF_LOOP_MAX_MEAS\s+(\d+)", text, re.M).group(1)) == _abi.LOOP_MAX_MEAS == mc.MAX_K
    assert _abi.SUMMARY_MAX_M == mc.MAX_M == 16384
    body = re.search(r"typedef struct MmfPfModalitiesArgs \{(.*?)\} MmfPfModalitiesArgs;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*(?:\[\w+\])?\s*[,;]", body)
    cls = _abi.MmfPfModalitiesArgs
    assert names == [f for f, _ in cls._fields_], names
    assert _abi.SIGNATURES["mmf_pf_modalities"] == (ctypes.c_int, [ctypes.POINTER(cls), ctypes.c_void_p])
    assert hasattr(lib, "mmf_pf_modalities")
    section = text[text.index("Per-modality attribution"):text.index("typedef struct MmfPfModalitiesArgs")]
    assert "crossmodal/base_models/crossmodal_pf.py:106-139" in section
    gcc = shutil.which("gcc")
    if gcc is None:
        pytest.skip("no gcc")
    lines = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{os.path.join(ROOT, "include", "mmf.h")}"', "int main(void) {",
             '  printf("size %zu\\n", sizeof(MmfPfModalitiesArgs));']
    lines += [f'  printf("{f} %zu\\n", offsetof(MmfPfModalitiesArgs, {f}));' for f, _ in cls._fields_]
    lines += ["  return 0;", "}"]
    (tmp_path / "layout.c").write_text("\n".join(lines))
    out = subprocess.run([gcc, "-std=c99", "-o", str(tmp_path / "layout"), str(tmp_path / "layout.c")], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    got = dict(line.split() for line in subprocess.run([str(tmp_path / "layout")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(cls)
    for f, _ in cls._fields_:
        assert int(got[f]) == getattr(cls, f).offset, f


# ------------------------------------------------------------------------------------------ 4. the entry point's host checks
def _args(alias=None, logliks=2, **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it (R = M = d = K = 2: the largest output,
    ``mean``, is 12 floats); ``logliks``: how many of the four columns are set; ``alias``: as for ``alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfModalitiesArgs, _POINTERS, **{**dict(R=2, M=2, d=2, K=2, logw_stride=2), **over})
    a._columns = [(ctypes.c_float * 16)() for _ in range(logliks)]
    for k, b in enumerate(a._columns):
        a.loglik[k] = ctypes.cast(b, ctypes.c_void_p)
    return sc.alias_host_args(a, _POINTERS, alias)


def _call(alias=None, logliks=2, **over):
    return sc.lib().mmf_pf_modalities(ctypes.byref(_args(alias, logliks, **over)), None)


def test_modalities_refuses_null_arguments():
    assert sc.lib().mmf_pf_modalities(None, None) == EINVAL
    assert _call(states=None) == EINVAL and _call(logliks=1) == EINVAL and _call(logliks=0) == EINVAL
    assert _call(R=0) == 0 and _call(R=0, log_w=None, modality_logw=None) == 0     # no rows: a successful no-op
    assert _call(R=0, logliks=1) == EINVAL                                         # (still an invalid call)


def test_modalities_refuses_a_number_of_modalities_outside_1_to_4():
    for bad in (0, -1, 5, 64):
        assert _call(K=bad, logliks=4) == EINVAL and _call(R=0, K=bad, logliks=4) == EINVAL, bad
    for K in (1, 2, 3, 4):
        assert _call(R=0, K=K, logliks=K, logw_stride=K) == 0, K
    assert _call(logw_stride=1) == EINVAL and _call(R=0, logw_stride=1, modality_logw=None) == 0   # a stride below K, read or not


def test_modalities_refuses_a_state_dimension_outside_1_to_4_no_particles_and_negative_rows():
    assert _call(d=0) == EINVAL and _call(d=5) == EINVAL and _call(d=-1) == EINVAL
    assert _call(M=0) == EINVAL and _call(M=-2) == EINVAL and _call(R=-1) == EINVAL
    assert _call(R=0, d=4, M=1) == 0 and _call(R=0, d=1) == 0


def test_modalities_refuses_a_call_without_outputs():
    assert _call(**{k: None for k in _OUTPUTS}) == EINVAL
    for out in _OUTPUTS:
        assert _call(R=0, **{k: None for k in _OUTPUTS if k != out}) == 0, out   # any one output is a request


def test_modalities_refuses_an_output_on_top_of_an_input_or_another_output():
    for out in _OUTPUTS:
        for target in _INPUTS + tuple(o for o in _OUTPUTS if o != out):
            assert _call({out: (target, 0)}) == EINVAL, (out, target)
    assert _call({"mean": ("states", 28)}) == EINVAL and _call({"ess": ("overlap", 8)}) == EINVAL  # partly on top
    a = _args()
    a.overlap = ctypes.c_void_p(ctypes.addressof(a._columns[1]))                  # on top of a log-likelihood column
    assert sc.lib().mmf_pf_modalities(ctypes.byref(a), None) == EINVAL
    assert _call({"mean": ("states", 0)}, R=0) == 0   # (no rows: the arrays are empty)


def test_modalities_refuses_too_many_particles_and_a_grid_beyond_32_bits():
    assert _call(M=16385) == ETOOLARGE and _call(M=1 << 20) == ETOOLARGE
    assert _call(M=16385, states=None) == EINVAL                        # an invalid call is invalid whatever its size
    assert _call(R=0, M=16384, d=4) == 0 and _call(R=0, M=16385) == ETOOLARGE


def test_the_binding_refuses_cpu_tensors_and_a_bad_number_of_modalities():
    import torch

    from multimodalfilter_amd import _abi

    x, l = torch.zeros((2, 4, 3)), torch.zeros((2, 4))
    with pytest.raises(_abi.MmfError):
        _abi.pf_modalities(x, None, [l, l], None, responsibility=torch.zeros((2, 2)))
    for bad in ([], [l] * 5):
        with pytest.raises(_abi.MmfError, match="modalities"):
            _abi.pf_modalities(x, None, bad, None, responsibility=torch.zeros((2, max(1, len(bad)))))


# ------------------------------------------------------------------------------------------ 5. the Python refusals
def _history(T, N, M, d, **extra):
    import torch

    from multimodalfilter_amd import base

    return base.history_record(states=torch.zeros((T, N, M, d)), log_likelihoods=torch.zeros((T, N, M)), log_weights_in=torch.zeros((T, N, M)),
                               ancestors=None, resampled=None, controls=None, **extra)


def test_belief_modalities_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base, base_models

    assert list(inspect.signature(mmf.filters.ParticleFilter.belief_modalities).parameters) == ["self"]  # no of=
    f = mmf.door_models.DoorCrossmodalParticleFilter().eval()
    assert f.last_modalities is None
    with pytest.raises(ValueError, match="^belief_modalities needs a history"):
        f.belief_modalities()
    pf = mmf.door_models.DoorParticleFilter().eval()
    pf.last_history = _history(2, 2, 4, 3)
    with pytest.raises(ValueError, match="CrossmodalParticleFilterMeasurementModel.*fuses nothing"):
        pf.belief_modalities()
    f.last_history = _history(2, 2, 4, 3)                             # a history some other code left: no observations
    with pytest.raises(ValueError, match="holds no observations"):
        f.belief_modalities()
    obs = {"image": torch.zeros((2, 2, 32, 32)), "gripper_pos": torch.zeros((2, 2, 3)), "gripper_sensors": torch.zeros((2, 2, 7))}
    f.last_history = h = _history(2, 2, 4, 3, observations=obs, enabled_models=(True, False))
    with pytest.raises(ValueError, match=r"enabled_models = \[True, True\] now, \[True, False\] when"):
        f.belief_modalities()
    f.last_history = _history(1, 1, mc.MAX_M + 1, 3, observations=obs, enabled_models=(True, True))
    with pytest.raises(ValueError, match="16384"):
        f.belief_modalities()
    f.last_history = h
    f.measurement_model.enabled_models = [True, False]
    with pytest.raises(_abi.MmfError):                                # in order: the call reaches the device code, which
        f.belief_modalities()                                         # refuses host memory -- there is no torch fallback
    assert f.last_modalities is None and f.last_history is h and pf.last_modalities is None

    # a crossmodal model over measurement models that are not fused networks has no log-likelihoods to evaluate apart
    class Plain(base.ParticleFilterMeasurementModel):
        def __init__(self):
            super().__init__(state_dim=3)

        def forward(self, *, states, observations):
            return states.sum(-1)

    meas = base_models.CrossmodalParticleFilterMeasurementModel(measurement_models=[Plain(), Plain()], crossmodal_weight_model=None, state_dim=3)
    with pytest.raises(ValueError, match="not fused networks"):
        meas.modality_log_likelihoods(torch.zeros((2, 4, 3)), {})


def test_run_filter_modalities_switch_and_refusals():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert sig["return_modalities"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_modalities"].default is False
    names = list(sig)
    assert names.index("return_modes") < names.index("return_modalities") < names.index("return_quantiles")
    for ctor, why in ((mmf.door_models.DoorParticleFilter, "fuses no modalities"), (mmf.door_models.DoorLSTMFilter, "fuses no modalities"),
                      (mmf.door_models.DoorKalmanFilter, "separate change"), (mmf.door_models.DoorCrossmodalKalmanFilter, "separate change"),
                      (mmf.push_models.PushUnimodalKalmanFilter, "separate change")):
        f = ctor().eval()
        with pytest.raises(ValueError, match=f"return_modalities needs a crossmodal particle filter.*{why}"):
            evaluation.run_filter(f, {}, return_modalities=True)      # (before the run: the trajectories are never read)
        assert getattr(f, "record_history", False) is False


# ------------------------------------------------------------------------------------------ 6. modality_summary, modality_errors
def _hand_made_record(beta=True):
    import torch

    from multimodalfilter_amd import base

    nan = math.nan
    rho = torch.tensor([[[0.9, 0.1], [0.5, 0.5]], [[0.2, 0.8], [nan, nan]], [[1.0, 0.0], [0.25, 0.75]]])       # (T=3, N=2, K=2)
    le = torch.tensor([[[-1.0, -3.0, -0.5], [-2.0, -2.0, -1.0]], [[-4.0, -2.0, -1.5], [nan, nan, nan]],
                       [[-1.0, -math.inf, -1.0], [-3.0, -1.0, -0.5]]])
    div = torch.tensor([[[0.1, 2.0], [0.5, 0.5]], [[1.5, 0.2], [nan, nan]], [[0.0, nan], [1.0, 0.25]]])
    ov = torch.stack([torch.stack([torch.tensor([[1.0, o], [o, 1.0]]) for o in row]) for row in ((0.5, 1.0), (0.25, nan), (nan, 0.75))])
    ov[2, 0] = torch.tensor([[1.0, nan], [nan, nan]])
    mean = torch.zeros((3, 2, 3, 2))
    mean[..., 0, :] = torch.tensor([3.0, 4.0])
    mean[..., 1, :] = torch.tensor([0.0, 1.0])
    mean[2, 0, 1] = nan
    logw = torch.log(torch.tensor([[[0.5, 0.5], [0.25, 0.75]], [[0.5, 0.5], [0.5, 0.5]], [[0.75, 0.25], [0.5, 0.5]]])) if beta else None
    return base.belief_record(responsibility=rho, log_evidence=le, divergence=div, overlap=ov, mean=mean, log_weights=logw, modalities=(0, 1))


def test_modality_summary_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    assert inspect.signature(evaluation.modality_summary).parameters["start"].default == evaluation.START_TRUNCATION == 30
    rec = _hand_made_record()
    s = evaluation.modality_summary(rec, start=0)
    assert set(s) == {"responsibility", "dominant", "log_evidence", "divergence", "overlap", "prior"}
    close = lambda got, want: torch.allclose(got.double(), torch.tensor(want, dtype=torch.float64), rtol=1e-6, atol=1e-7)
    assert close(s["responsibility"], [(0.9 + 0.5 + 0.2 + 1.0 + 0.25) / 5, (0.1 + 0.5 + 0.8 + 0.0 + 0.75) / 5])
    assert close(s["dominant"], [3 / 5, 2 / 5])                       # the tie (0.5, 0.5) goes to the lowest index; the NaN step is left out
    assert close(s["log_evidence"], [(-1 - 2 - 4 - 1 - 3) / 5, (-3 - 2 - 2 - 1) / 4, (-0.5 - 1 - 1.5 - 1 - 0.5) / 5])  # -inf left out
    assert close(s["divergence"], [(0.1 + 0.5 + 1.5 + 0.0 + 1.0) / 5, (2.0 + 0.5 + 0.2 + 0.25) / 4])
    assert close(s["overlap"], [[1.0, (0.5 + 1.0 + 0.25 + 0.75) / 4], [(0.5 + 1.0 + 0.25 + 0.75) / 4, 1.0]])
    assert close(s["prior"], [(0.5 + 0.25 + 0.5 + 0.5 + 0.75 + 0.5) / 6, (0.5 + 0.75 + 0.5 + 0.5 + 0.25 + 0.5) / 6])
    late = evaluation.modality_summary(rec, start=2)
    assert close(late["responsibility"], [(1.0 + 0.25) / 2, 0.75 / 2]) and close(late["dominant"], [0.5, 0.5])
    assert close(evaluation.modality_summary(_hand_made_record(beta=False), start=0)["prior"], [0.5, 0.5])
    with pytest.raises(ValueError, match="^modality_summary: the record has no responsibility"):
        evaluation.modality_summary(base.belief_record(crps=torch.zeros((3, 2, 2))))


def test_modality_errors_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    rec = _hand_made_record()
    true = torch.zeros((3, 2, 2))
    true[1, 1] = torch.tensor([3.0, 0.0])
    e = evaluation.modality_errors(rec, true)
    assert e.shape == (3, 2, 3)
    assert torch.equal(e[0, 0], torch.tensor([5.0, 1.0, 0.0])) and torch.equal(e[1, 1], torch.tensor([4.0, math.sqrt(10.0), 3.0]))
    assert torch.isnan(e[2, 0, 1]) and e[2, 0, 0] == 5.0 and int(torch.isnan(e).sum()) == 1
    for bad in (true[:2], true[..., :1], None, true.numpy()):
        with pytest.raises(ValueError, match="^modality_errors: true must be a"):
            evaluation.modality_errors(rec, bad)
    with pytest.raises(ValueError, match="^modality_errors: the record has no mean"):
        evaluation.modality_errors(base.belief_record(mean=torch.zeros((3, 2, 2))), true)

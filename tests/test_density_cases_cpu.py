"""CPU-side checks of the particle-posterior density (``include/mmf.h``: ``MmfPfDensityArgs`` / ``mmf_pf_density``;
``ParticleFilter.belief_density``; ``evaluation.gaussian_log_density`` / ``gaussian_entropy`` / ``density_summary`` /
``run_filter(return_density=)``): the fp64 reference of ``_density_cases`` is held to closed forms and to the symmetries of a
kernel density, its family is certified against the fp32 formulation, the Gaussian closed forms are held to
``torch.distributions``, and the entry point's and the Python layers' refusals are reached on the host before any HIP call
or device work."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _density_cases as dc
import _quantile_cases as qc
import _score_cases as sk
import _smooth_cases as sc
from _filter_stubs import _Recorded
from _tol import REL_TOL

EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("states", "log_a", "log_b", "truth")
_OUTPUTS = ("log_density", "log_score", "entropy", "mode", "mode_index", "bandwidth_out")
_POINTERS = _INPUTS + _OUTPUTS + ("workspace",)
LOG_2PI = math.log(2.0 * math.pi)


# ------------------------------------------------------------------------------------------ 1. the definition, closed forms
def _rows(X, W, y, rule, bandwidth=None, min_bandwidth=None):
    X = np.asarray(X, np.float32)
    floor = None if min_bandwidth is None else (min_bandwidth,) * X.shape[-1]
    return dc.reference_rows(X, np.asarray(W, np.float64), None if y is None else np.asarray(y, np.float32), rule, bandwidth, floor)


def test_one_particle_with_a_fixed_bandwidth_is_the_gaussian_log_pdf():
    for d in sk.DIMS:
        rng = np.random.default_rng(d)
        x, y = rng.standard_normal((1, 1, d)).astype(np.float32), rng.standard_normal((1, d)).astype(np.float32)
        h = np.asarray(dc.FIXED[:d], np.float32).astype(np.float64)
        ref = _rows(x, [[0.7]], y, "fixed", dc.FIXED[:d])
        z = (y[0].astype(np.float64) - x[0, 0]) / h
        want = -0.5 * (z ** 2).sum() - np.log(h).sum() - 0.5 * d * LOG_2PI
        at_self = -np.log(h).sum() - 0.5 * d * LOG_2PI
        assert abs(ref["log_score"][0] - want) <= 1e-13 * max(1.0, abs(want))
        assert abs(ref["log_density"][0, 0] - at_self) <= 1e-13 and abs(ref["entropy"][0] + at_self) <= 1e-13
        assert np.array_equal(ref["bandwidth"][0], h)


def test_one_particle_under_a_rule_has_the_floor_as_its_bandwidth():
    for rule in ("silverman", "scott"):
        ref = _rows(np.ones((1, 1, 3)), [[2.0]], None, rule, min_bandwidth=0.25)
        assert np.array_equal(ref["bandwidth"], np.full((1, 3), 0.25)) and ref["log_score"] is None
        assert abs(ref["log_density"][0, 0] - (-3 * math.log(0.25) - 1.5 * LOG_2PI)) <= 1e-13


def test_the_rules_of_thumb_on_a_hand_computed_set():
    x = np.asarray([[[0.0], [2.0], [4.0], [9.0]]])                          # the last particle is dead
    ref = _rows(x, [[1.0, 2.0, 1.0, 0.0]], None, "silverman", min_bandwidth=1e-6)
    n_eff, sigma = 16.0 / 6.0, math.sqrt(2.0)                               # W = (1/4, 1/2, 1/4): mean 2, variance 2
    assert abs(ref["bandwidth"][0, 0] - sigma * (4.0 / (3.0 * n_eff)) ** 0.2) <= 1e-14
    assert ref["log_density"][0, 3] == -np.inf and np.isfinite(ref["log_density"][0, :3]).all()
    ref = _rows(x, [[1.0, 2.0, 1.0, 0.0]], None, "scott", min_bandwidth=1e-6)
    assert abs(ref["bandwidth"][0, 0] - sigma * n_eff ** -0.2) <= 1e-14


def test_symmetries_of_the_reference():
    rng = np.random.default_rng(11)
    # two symmetric particles have equal densities
    ref = _rows([[[-1.5, 0.5], [1.5, -0.5]]], [[1.0, 1.0]], [[0.0, 0.0]], "silverman", min_bandwidth=1e-6)
    assert abs(ref["log_density"][0, 0] - ref["log_density"][0, 1]) <= 1e-14
    for rule in dc.RULES:
        for M, d in ((5, 1), (33, 3), (64, 4)):
            X = rng.standard_normal((2, M, d)).astype(np.float32)
            W = np.exp(rng.standard_normal((2, M)))
            W[:, 1] = 0.0
            y = rng.standard_normal((2, d)).astype(np.float32)
            bw = dc.FIXED[:d] if rule == "fixed" else None
            ref = dc.reference_rows(X, W, y, rule, bw, (1e-6,) * d)
            # translating states and truth (by an amount exact in fp32) leaves everything unchanged
            moved = dc.reference_rows(X.astype(np.float64) + 8.0, W, y.astype(np.float64) + 8.0, rule, bw, (1e-6,) * d)
            # scaling states, truth and fixed bandwidths by 2 shifts every log by -d log 2 (and the entropy by + d log 2)
            twice = dc.reference_rows(2.0 * X, W, 2.0 * y, rule, None if bw is None else tuple(2.0 * h for h in bw), (1e-6,) * d)
            for k in ("log_density", "log_score", "entropy", "bandwidth"):
                assert np.allclose(moved[k], ref[k], rtol=1e-11, atol=1e-11), (rule, M, d, k)
            shift = d * math.log(2.0)
            assert np.allclose(twice["log_density"], ref["log_density"] - shift, rtol=1e-12, atol=1e-12)
            assert np.allclose(twice["log_score"], ref["log_score"] - shift, rtol=1e-12, atol=1e-12)
            assert np.allclose(twice["entropy"], ref["entropy"] + shift, rtol=1e-12, atol=1e-12)
            assert np.allclose(twice["bandwidth"], 2.0 * ref["bandwidth"], rtol=1e-14)
            assert (ref["log_density"][:, 1] == -np.inf).all()


def test_the_reference_is_a_true_log_sum_exp():
    """A truth 50 sigma off, and a collapsed set with the truth 1.0 away from it under the floor 1e-6: finite, and what the
    closed form of the nearest particle says."""
    X = np.zeros((1, 64, 2), np.float32)
    ref = _rows(X, np.ones((1, 64)), [[1.0, 0.0]], "silverman", min_bandwidth=1e-6)
    h = float(np.float32(1e-6))
    want = -0.5 / h ** 2 - 2 * math.log(h) - LOG_2PI
    assert np.isfinite(ref["log_score"][0]) and abs(ref["log_score"][0] - want) <= 1e-12 * abs(want)
    case, ref = dc.family_case(65, 3, 3, "nan_truth", "silverman")
    assert np.isnan(ref["log_score"][1]) and np.isfinite(np.delete(ref["log_score"], 1)).all()
    assert np.isfinite(ref["entropy"]).all() and np.isfinite(ref["bandwidth"]).all()
    case, ref = dc.family_case(65, 3, 3, "dead_row", "scott")
    assert all(np.isnan(ref[k][1]).all() for k in ("log_density", "log_score", "entropy", "bandwidth"))
    assert np.isinf(np.delete(ref["log_density"], 1, 0)).any() and not np.isnan(np.delete(ref["log_density"], 1, 0)).any()


# ------------------------------------------------------------------------------------------ 2. the family is certified
@pytest.mark.parametrize("M", sk.ALL_MS)
def test_the_fp32_formulation_is_within_the_cap_on_the_family(M):
    """A condition on the INPUTS: where fp32 torch ops cannot hold ``CAP = REL_TOL / 3`` against fp64, the kernel could not
    be asked for ``REL_TOL`` either.  Every case is held to it, none is skipped."""
    worst, cases = {}, 0
    for case_id in dc.family():
        if case_id[0] != M:
            continue
        case, ref = dc.family_case(*case_id)
        got = {k: (None if v is None else v.numpy()) for k, v in dc.torch_formulation(case).items()}
        errs = {"log_density": dc.log_err(got["log_density"], ref["log_density"], "log_density"),
                "entropy": dc.log_err(got["entropy"], ref["entropy"], "entropy"),
                "bandwidth": dc.bandwidth_err(got["bandwidth"], ref["bandwidth"], "bandwidth")}
        if case["truth"] is None:
            assert ref["log_score"] is None and got["log_score"] is None
        else:
            errs["log_score"] = dc.log_err(got["log_score"], ref["log_score"], "log_score")
        errs["mode"] = dc.check_mode(case["states"], qc.weights64(case), got["log_density"], got["mode_index"], got["mode"],
                                     ref["log_density"], str(case_id))
        print(f"{case_id}: fp32 formulation against fp64 " + ", ".join(f"{k} {e:.2e}" for k, e in errs.items()) + f" (cap {dc.CAP:.0e})")
        assert max(errs.values()) < dc.CAP, (case_id, errs)
        for k, e in errs.items():
            worst[k] = max(worst.get(k, 0.0), e)
        cases += 1
    assert cases >= len(dc.VARIANTS)
    print(f"M={M}: worst over {cases} cases " + ", ".join(f"{k} {e:.2e}" for k, e in worst.items()))


def test_the_family_covers_what_the_definition_distinguishes():
    seen = set(dc.family())
    assert dc.CAP <= REL_TOL / 3
    assert {c[0] for c in seen} == set(sk.ALL_MS) and "scaled" not in {c[3] for c in seen}
    for M in sk.ALL_MS:
        assert {c[3] for c in seen if c[0] == M} == set(dc.VARIANTS)
        assert {c[4] for c in seen if c[0] == M} == set(dc.RULES)
        assert {c[1] for c in seen if c[0] == M and c[3] == "plain"} == set(sk.DIMS)
        assert {c[2] for c in seen if c[0] == M} == set(sk.RS)
    # the family's own weights leave 1 to 3 effective particles; the moderate ones nearly all of them
    n_eff = lambda case: 1.0 / ((qc.weights64(case) / qc.weights64(case).sum(-1, keepdims=True)) ** 2).sum(-1)
    assert n_eff(dc.make_case(256, 2, 3, "plain")).max() < 16 and n_eff(dc.make_case(256, 2, 3, "moderate")).min() > 128


# ------------------------------------------------------------------------------------------ 3. the Gaussian closed forms
def test_gaussian_log_density_and_entropy_against_torch_distributions():
    import torch

    from multimodalfilter_amd import evaluation

    g = torch.Generator().manual_seed(9)
    T, N, d = 40, 3, 3
    mu = torch.randn((T, N, d), generator=g, dtype=torch.float64)
    A = torch.randn((T, N, d, d), generator=g, dtype=torch.float64)
    cov = A @ A.transpose(-1, -2) + 0.05 * torch.eye(d, dtype=torch.float64)
    y = mu + torch.randn((T, N, d), generator=g, dtype=torch.float64)
    mvn = torch.distributions.MultivariateNormal(mu, covariance_matrix=cov)
    got = evaluation.gaussian_log_density(mu, cov, y)
    assert got.shape == (T, N) and got.dtype == torch.float64
    assert torch.allclose(got, mvn.log_prob(y), rtol=1e-12, atol=1e-12)
    ent = evaluation.gaussian_entropy(cov)
    assert ent.shape == (T, N) and torch.allclose(ent, mvn.entropy(), rtol=1e-12, atol=1e-12)
    for start in (0, 30):
        assert torch.allclose(evaluation.gaussian_nll(mu, cov, y, start=start), -got[start:].mean(0), rtol=1e-12, atol=1e-12)
    got32 = evaluation.gaussian_log_density(mu.float(), cov.float(), y.float())
    assert got32.dtype == torch.float32 and torch.allclose(got32.double(), got, rtol=1e-4, atol=1e-4)


def test_density_summary_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    log_score = torch.tensor([[-1.0], [math.nan], [-4.0], [-math.inf]])  # (T = 4, N = 1)
    entropy = torch.tensor([[0.5], [math.nan], [1.5], [2.5]])
    got = evaluation.density_summary(base.belief_record(log_score=log_score, entropy=entropy), start=0)
    assert got == {"log_score": -2.5, "entropy": 1.5}
    got = evaluation.density_summary(base.belief_record(entropy=entropy), start=2)
    assert got == {"entropy": 2.0}
    assert inspect.signature(evaluation.density_summary).parameters["start"].default == evaluation.START_TRUNCATION
    with pytest.raises(ValueError, match="entropy"):
        evaluation.density_summary(base.belief_record(log_score=log_score))


# ------------------------------------------------------------------------------------------ 4. the entry point's host checks
def _args(alias=None, bandwidth=(1.0, 1.0), min_bandwidth=(1e-6, 1e-6), **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfDensityArgs, _POINTERS, **{**dict(R=2, M=2, d=2, rule=1, workspace_bytes=64), **over})
    for i, h in enumerate(bandwidth):
        a.bandwidth[i] = h
    for i, h in enumerate(min_bandwidth):
        a.min_bandwidth[i] = h
    return sc.alias_host_args(a, _POINTERS, alias)


def test_density_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == 42
    call = lambda alias=None, **over: lib.mmf_pf_density(ctypes.byref(_args(alias, **over)), None)
    assert lib.mmf_pf_density(None, None) == EINVAL
    assert call(states=None) == EINVAL
    assert call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(M=0) == EINVAL and call(M=-2) == EINVAL and call(R=-1) == EINVAL
    assert call(rule=-1) == EINVAL and call(rule=3) == EINVAL
    nothing = {k: None for k in _OUTPUTS}
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        for rule in (1, 2):  # the rules read the floor, not the bandwidth
            assert call(rule=rule, min_bandwidth=(1.0, bad)) == EINVAL and call(rule=rule, min_bandwidth=(bad, 2.0)) == EINVAL, bad
            assert call(rule=rule, bandwidth=(bad, bad), R=0) == 0, bad
        assert call(rule=0, bandwidth=(1.0, bad)) == EINVAL and call(rule=0, bandwidth=(bad, 2.0)) == EINVAL, bad
        assert call(rule=0, min_bandwidth=(bad, bad), R=0) == 0, bad
    assert call(rule=0, bandwidth=(0.5, 2.0, 0.0, math.nan), R=0) == 0   # (beyond d nothing is read)
    assert call(**nothing) == EINVAL                                     # nothing requested
    assert call(truth=None) == EINVAL                                    # log_score without a truth
    assert call(truth=None, log_score=None, R=0) == 0
    for out in _OUTPUTS:
        assert call(R=0, **{k: None for k in _OUTPUTS if k != out}) == 0, out   # any one output is a request
        for target in _INPUTS + tuple(o for o in _OUTPUTS if o != out):
            assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"log_density": ("states", 28)}) == EINVAL and call({"mode": ("entropy", 4)}) == EINVAL  # partly on top
    assert call(M=16385) == ETOOLARGE and call(M=1 << 20) == ETOOLARGE
    assert call(M=16385, states=None) == EINVAL                         # an invalid call is invalid whatever its size
    assert call(R=1 << 27, M=16384) == ETOOLARGE                         # R * workgroups per row beyond a 32-bit grid
    # successful no-ops: no rows (the arrays are empty, so nothing is needed and nothing overlaps)
    assert call(R=0) == 0 and call(R=0, M=16384, d=4, min_bandwidth=(1.0,) * 4) == 0 and call(R=0, M=16385) == ETOOLARGE
    assert call(R=0, log_a=None, log_b=None) == 0
    assert call(R=0, workspace=None, workspace_bytes=0, M=4096) == 0
    assert call({"log_density": ("states", 0)}, R=0) == 0


def test_density_workspace_formula_and_refusals_on_the_host():
    """16 bytes per workgroup of a row beyond one.  With ``M > 512`` the arrays no longer fit the 16-float host buffers, but
    every check below is decided on pointer values alone, before any HIP call."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    ws = _abi.pf_density_workspace_bytes
    assert ws(0, 513, 2) == 0 and ws(1, 0, 2) == 0 and ws(1, 513, 0) == 0
    for M in (1, 2, 511, 512):
        assert ws(3, M, 4) == 0
    for M in (513, 1024, 1025, 4096, 16384):
        for R in (1, 3):
            assert ws(R, M, 1) == ws(R, M, 4) == 16 * R * -(-M // 512)
    R, M, d = 1, 513, 1
    need = ws(R, M, d)
    big = [(ctypes.c_float * (R * M * (d + 1) + 64))() for _ in _POINTERS]

    def call(**over):
        a = _abi.MmfPfDensityArgs()
        for name, b in zip(_POINTERS, big):
            setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
        a.R, a.M, a.d, a.rule, a.workspace_bytes = R, M, d, 2, need
        a.min_bandwidth[0] = 1e-6
        for k, v in over.items():
            setattr(a, k, v)
        a._keep = big
        return lib.mmf_pf_density(ctypes.byref(a), None)

    base = ctypes.addressof(big[_POINTERS.index("workspace")])
    assert call(workspace=None) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    assert call(workspace=ctypes.c_void_p(base + 4)) == EINVAL       # not 8-byte aligned
    for target in _INPUTS + _OUTPUTS:
        assert call(workspace=ctypes.cast(big[_POINTERS.index(target)], ctypes.c_void_p)) == EINVAL, target
    assert call(R=0) == 0


def test_the_binding_refuses_cpu_tensors():
    import torch

    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_density(x, None, None, None, min_bandwidth=(1e-6,) * 3, entropy=torch.zeros((2,)))
    with pytest.raises(_abi.MmfError, match="min_bandwidth"):
        _abi.pf_density(x, None, None, None, min_bandwidth=(1e-6,) * 2, entropy=torch.zeros((2,)))
    with pytest.raises(_abi.MmfError, match="bandwidth"):
        _abi.pf_density(x, None, None, None, rule="fixed", entropy=torch.zeros((2,)))
    with pytest.raises(_abi.MmfError, match="rule"):
        _abi.pf_density(x, None, None, None, rule="epanechnikov", entropy=torch.zeros((2,)))
    assert _abi.DENSITY_MAX_M == 16384 == dc.MAX_M and _abi.DENSITY_RULES == {"fixed": 0, "silverman": 1, "scott": 2}


# ------------------------------------------------------------------------------------------ 5. the Python refusals
def test_belief_density_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    sig = inspect.signature(mmf.filters.ParticleFilter.belief_density).parameters
    assert list(sig) == ["self", "truth", "of", "bandwidth", "min_bandwidth"] and sig["truth"].default is None
    assert sig["of"].kind is inspect.Parameter.KEYWORD_ONLY and sig["of"].default == "filtered"
    assert sig["bandwidth"].default == "silverman" and sig["min_bandwidth"].default == 1e-6
    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_density is None
    with pytest.raises(ValueError, match="^belief_density needs a history"):
        pf.belief_density()
    with pytest.raises(ValueError, match=r"^belief_density\(of='smoothed'\) needs a smoothed record"):
        pf.belief_density(of="smoothed")
    with pytest.raises(ValueError, match="of must be"):
        pf.belief_density(of="predicted")

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    truth = torch.zeros((T, N, d))
    before = (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores)
    f.last_smoothed = base.belief_record(covariance=torch.zeros((T, N, d, d)), unique=torch.zeros((T, N), dtype=torch.int32), lag=None)
    with pytest.raises(ValueError, match=r"belief_density\(of='smoothed'\).*no per-step weights"):
        f.belief_density(truth, of="smoothed")
    f.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_density(truth, of="smoothed")
    f.last_smoothed = before[1]
    for bad in (torch.zeros((T, N)), torch.zeros((T + 1, N, d)), torch.zeros((T, N, d + 1)), np.zeros((T, N, d))):
        with pytest.raises(ValueError, match="truth"):
            f.belief_density(bad)
    for bad in ((), (1.0, 1.0), (1.0,) * 4, (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, math.nan, 1.0), (1.0, math.inf, 1.0),
                ("1", 1.0, 1.0), (True, 1.0, 1.0), 2.0, "epanechnikov", None):
        with pytest.raises(ValueError, match="bandwidth must be 'silverman', 'scott' or 3"):
            f.belief_density(truth, bandwidth=bad)
    for bad in ((), (1.0, 1.0), (1.0, 0.0, 1.0), 0.0, -1.0, math.nan, math.inf, True, "1e-6", None):
        with pytest.raises(ValueError, match="min_bandwidth"):
            f.belief_density(truth, min_bandwidth=bad)
    big = base.history_record(states=torch.zeros((1, 1, dc.MAX_M + 1, 1)), log_likelihoods=torch.zeros((1, 1, dc.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="16384"):
        f.belief_density()
    f.last_history = before[0]
    assert f.last_density is None and (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores) == before
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    for kw in (dict(), dict(bandwidth="scott", min_bandwidth=(1e-3, 1e-4, 1e-5)), dict(bandwidth=(0.5, 2.0, 1.0))):
        with pytest.raises(_abi.MmfError):
            f.belief_density(truth, **kw)
        with pytest.raises(_abi.MmfError):
            f.belief_density(**kw)
    assert f.last_density is None


def test_run_filter_density_of_a_gaussian_belief_and_refusal_of_a_point_estimate():
    import torch

    from multimodalfilter_amd import evaluation

    g = torch.Generator().manual_seed(3)
    T, N, d = 5, 2, 3
    states = torch.randn((T + 1, N, d), generator=g)
    traj = dict(states=states, image=torch.zeros((T + 1, N, 1)), gripper_pos=torch.zeros((T + 1, N, 1)),
                gripper_sensors=torch.zeros((T + 1, N, 1)), controls=torch.zeros((T + 1, N, 1)))
    est = states[1:] + 0.3 * torch.randn((T, N, d), generator=g)
    A = torch.randn((T, N, d, d), generator=g)
    cov = A @ A.transpose(-1, -2) + 0.1 * torch.eye(d)

    kf = _Recorded(est, cov)
    assert evaluation.run_filter(kf, traj) is est and evaluation.run_filter(kf, traj, return_density=False) is est
    out, rec = evaluation.run_filter(kf, traj, return_density=True)
    assert out is est and kf.record_belief is False                       # the switch is put back, the belief is not returned
    assert set(vars(rec)) == {"log_score", "entropy", "mode", "of"} and rec.of == "filtered" and rec.mode is est
    assert torch.equal(rec.log_score, evaluation.gaussian_log_density(est, cov, states[1:])) and rec.log_score.shape == (T, N)
    assert torch.equal(rec.entropy, evaluation.gaussian_entropy(cov))
    out = evaluation.run_filter(kf, traj, return_belief=True, return_scores=True, return_density=True)
    assert len(out) == 4 and out[1] is kf.last_belief and hasattr(out[2], "crps") and torch.equal(out[3].log_score, rec.log_score)
    got = evaluation.density_summary(rec, start=1)
    assert set(got) == {"log_score", "entropy"} and abs(got["log_score"] - float(rec.log_score[1:].double().mean())) < 1e-12

    point = _Recorded(est)
    with pytest.raises(ValueError, match="return_density.*no density"):
        evaluation.run_filter(point, traj, return_density=True)
    with pytest.raises(ValueError, match="density_bandwidth"):
        evaluation.run_filter(kf, traj, return_density=True, density_bandwidth=(1.0, 1.0))  # not d of them


def test_run_filter_switch_and_refusals():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert sig["return_density"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_density"].default is False
    assert sig["density_bandwidth"].kind is inspect.Parameter.KEYWORD_ONLY and sig["density_bandwidth"].default == "silverman"
    pf = mmf.door_models.DoorParticleFilter().eval()
    for kw in (dict(smooth_method="map"), dict(smooth_lag=3), dict(smooth_lag=None), dict(smooth_method="ancestry", smooth_lag=0)):
        with pytest.raises(ValueError, match="return_density"):
            evaluation.run_filter(pf, {}, return_density=True, **kw)  # (before the run: the trajectories are never read)
    for bad in ((1.0, 0.0, 1.0), (1.0, math.nan, 1.0), (), "abc", 3.0, None):
        with pytest.raises(ValueError, match="density_bandwidth"):
            evaluation.run_filter(pf, {}, return_density=True, density_bandwidth=bad)
    for given in ((1.0, 1.0, 1.0), "scott", "silverman"):
        with pytest.raises(ValueError, match="density_bandwidth.*without\\s+return_density"):
            evaluation.run_filter(pf, {}, density_bandwidth=given)
    lstm = mmf.door_models.DoorLSTMFilter().eval()
    with pytest.raises(ValueError, match="return_density"):
        evaluation.run_filter(lstm, {}, return_density=True)
    assert pf.record_history is False and pf.record_belief is False and pf.last_density is None

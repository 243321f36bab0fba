"""CPU-side checks of the particle-posterior scores (``include/mmf.h``: ``MmfPfScoresArgs`` / ``mmf_pf_scores``;
``ParticleFilter.belief_scores``; ``evaluation.gaussian_crps`` / ``score_summary`` / ``run_filter(return_scores=)``): the
family of ``_score_cases`` is certified against the fp32 formulation, the fp64 reference obeys the identities of the scores,
the Gaussian closed form is held to a numerical integral, and the entry point's and the Python layers' refusals are reached
on the host before any HIP call or device work."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _quantile_cases as qc
import _score_cases as sk
import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2
_POINTERS = ("states", "log_a", "log_b", "truth", "crps", "energy", "spread", "workspace")


@pytest.fixture(autouse=True, scope="module")
def _the_entry_these_tests_describe():
    """The family and the reference of this module define ONE entry point: without the binding, the method and the
    evaluation functions there is nothing they are the reference of."""
    from multimodalfilter_amd import _abi, evaluation, filters

    assert hasattr(_abi, "MmfPfScoresArgs") and callable(getattr(_abi, "pf_scores", None))
    assert callable(getattr(filters.ParticleFilter, "belief_scores", None))
    assert callable(getattr(evaluation, "gaussian_crps", None)) and callable(getattr(evaluation, "score_summary", None))


# ------------------------------------------------------------------------------------------ 1. the family is certified
@pytest.mark.parametrize("M", sk.ALL_MS)
def test_the_fp32_formulation_is_within_the_cap_on_the_family(M):
    """A condition on the INPUTS: where fp32 torch ops cannot hold ``CAP = REL_TOL / 3`` against fp64, the kernel could not
    be asked for ``REL_TOL`` either.  Every case is held to it, none is skipped."""
    worst = 0.0
    cases = 0
    for M_, d, R, variant in sk.family():
        if M_ != M:
            continue
        case, (crps, energy, spread) = sk.family_case(M, d, R, variant)
        t_crps, t_energy, t_spread = sk.torch_formulation(case)
        errs = [sk.compare(t_spread.numpy(), spread, "spread")]
        if case["truth"] is None:
            assert crps is None and energy is None and t_crps is None and t_energy is None
        else:
            errs += [sk.compare(t_crps.numpy(), crps, "crps"), sk.compare(t_energy.numpy(), energy, "energy")]
        print(f"M={M} d={d} R={R} {variant}: fp32 formulation against fp64 {max(errs):.3e} (cap {sk.CAP:.0e})")
        assert max(errs) < sk.CAP, (M, d, R, variant, errs)
        worst = max(worst, max(errs))
        cases += 1
    assert cases >= len(sk.VARIANTS)
    print(f"M={M}: worst {worst:.3e} over {cases} cases")


def test_the_family_covers_what_the_definition_distinguishes():
    seen = set(sk.family())
    assert {m for m, *_ in seen} == set(sk.ALL_MS) and set(sk.MS) <= set(sk.ALL_MS)
    for M in sk.ALL_MS:
        assert {v for m, _, _, v in seen if m == M} == set(sk.VARIANTS)
        assert {d for m, d, _, v in seen if m == M and v == "plain"} == set(sk.DIMS)
    for edge in (sk.I_BLOCK, sk.J_TILE):
        assert {edge - 1, edge, edge + 1} <= set(sk.ALL_MS)
    # NaN exactly where the definition puts it
    case, (crps, energy, spread) = sk.family_case(65, 3, 3, "dead_row")
    assert np.isnan(crps[1]).all() and np.isnan(energy[1]) and np.isnan(spread[1]).all()
    assert np.isfinite(np.delete(crps, 1, 0)).all() and np.isfinite(np.delete(spread, 1, 0)).all()
    case, (crps, energy, spread) = sk.family_case(65, 3, 3, "nan_truth")
    k = int(np.flatnonzero(np.isnan(case["truth"][1]))[0])
    assert np.isnan(crps[1, k]) and np.isnan(energy[1]) and np.isfinite(np.delete(crps[1], k)).all()
    assert np.isfinite(spread).all() and np.isfinite(np.delete(energy, 1)).all()
    case, (crps, energy, spread) = sk.family_case(65, 3, 3, "no_truth")
    assert crps is None and energy is None and np.isfinite(spread).all()
    case, _ = sk.family_case(65, 3, 3, "plain")
    assert np.isnan(case["states"]).any() and np.isinf(case["log_b"]).any()  # dead particles carry NaN rows


# ------------------------------------------------------------------------------------------ 2. identities of the reference
@pytest.mark.parametrize("M", [1, 2, 65, 257])
def test_identities_of_the_scores_in_fp64(M):
    for d in sk.DIMS:
        for variant in ("plain", "uniform", "scaled"):
            case, (crps, energy, spread) = sk.family_case(M, d, 3, variant)
            assert bool((crps >= -1e-15).all()) and bool((energy >= -1e-15).all()) and bool((spread >= 0).all())
            if M == 1:  # a point mass: the absolute / Euclidean error, no spread
                e = case["states"][:, 0, :].astype(np.float64) - case["truth"]
                assert np.array_equal(spread, np.zeros_like(spread))
                assert np.allclose(crps, np.abs(e), rtol=1e-15, atol=0)
                assert np.allclose(energy, np.sqrt(((e / sk._scale64(case)) ** 2).sum(-1)), rtol=1e-15, atol=0)
            if d == 1 and case["scale"] is None:
                assert np.allclose(energy, crps[:, 0], rtol=1e-13, atol=1e-16)
                assert np.allclose(spread[:, 1], spread[:, 0], rtol=1e-13, atol=1e-16)
            # every particle twice with half its weight: the same distribution, the same scores
            twice = dict(case, states=np.concatenate([case["states"]] * 2, axis=1))
            W = np.concatenate([qc.weights64(case)] * 2, axis=1) * 0.5
            c2, e2, s2 = sk.reference_rows(twice["states"], W, case["truth"], sk._scale64(case))
            for a, b in ((c2, crps), (e2, energy), (s2, spread)):
                assert np.allclose(a, b, rtol=1e-12, atol=1e-15)


def test_crps_of_equal_weights_is_the_order_statistics_formula():
    """An independent route to the pair sum in one dimension: ``sum_ml |x_m - x_l| = 2 sum_i (2 i - n + 1) x_(i)``."""
    case, (crps, energy, spread) = sk.family_case(257, 2, 3, "uniform")
    for r in range(3):
        for k in range(2):
            x = np.sort(case["states"][r, :, k].astype(np.float64))
            n = len(x)
            gini = 2.0 * ((2.0 * np.arange(n) - n + 1) * x).sum() / n ** 2
            assert abs(gini - spread[r, k]) <= 1e-12 * max(1.0, gini)
            assert abs(np.abs(x - case["truth"][r, k]).mean() - 0.5 * gini - crps[r, k]) <= 1e-12


# ------------------------------------------------------------------------------------------ 3. the Gaussian closed form
def _crps_by_quadrature(mu, sigma, y, n):
    """``int (F(x) - 1[x >= y])^2 dx`` by the trapezoid rule on ``n`` intervals, the two sides of the jump at ``y`` apart."""
    lo, hi = min(mu - 12.0 * sigma, y) - 1e-9, max(mu + 12.0 * sigma, y) + 1e-9
    Phi = lambda x: 0.5 * (1.0 + np.vectorize(math.erf)((x - mu) / (sigma * math.sqrt(2.0))))
    left, right = np.linspace(lo, y, n + 1), np.linspace(y, hi, n + 1)
    trapezoid = lambda f, x: float((0.5 * (f[1:] + f[:-1]) * np.diff(x)).sum())
    return trapezoid(Phi(left) ** 2, left) + trapezoid((Phi(right) - 1.0) ** 2, right)


def test_gaussian_crps_against_a_trapezoid_integral():
    import torch

    from multimodalfilter_amd import evaluation

    rng = np.random.default_rng(5)
    T, N, d = 3, 2, 3
    mu = rng.standard_normal((T, N, d))
    A = rng.standard_normal((T, N, d, d))
    cov = A @ np.swapaxes(A, -1, -2) + 0.05 * np.eye(d)
    y = mu + 2.0 * rng.standard_normal((T, N, d)) * np.sqrt(np.einsum("tnkk->tnk", cov))
    y[0, 0, 0] = mu[0, 0, 0]          # on the mean: sigma (sqrt(2) - 1) / sqrt(pi)
    cov[1, 1, :, 2] = cov[1, 1, 2, :] = 0.0  # sigma = 0: a point mass in dimension 2
    got = evaluation.gaussian_crps(torch.from_numpy(mu), torch.from_numpy(cov), torch.from_numpy(y))
    assert got.shape == (T, N, d) and got.dtype == torch.float64
    got = got.numpy()
    assert got[1, 1, 2] == abs(y[1, 1, 2] - mu[1, 1, 2])
    sigma0 = math.sqrt(cov[0, 0, 0, 0])
    assert abs(got[0, 0, 0] - sigma0 * (math.sqrt(2.0) - 1.0) / math.sqrt(math.pi)) <= 1e-14
    for idx in np.ndindex(T, N, d):
        sigma = math.sqrt(cov[idx + (idx[-1],)])
        if sigma == 0.0:
            continue
        fine, coarse = (_crps_by_quadrature(mu[idx], sigma, y[idx], n) for n in (20000, 10000))
        tol = 10.0 * abs(fine - coarse)  # ten times what halving the grid step changes
        assert tol < 1e-5 * sigma, (idx, tol)  # (the grid is fine enough for the comparison to mean something)
        assert abs(got[idx] - fine) <= tol, (idx, got[idx], fine, tol)
    # fp32 in, fp32 out
    got32 = evaluation.gaussian_crps(torch.from_numpy(mu).float(), torch.from_numpy(cov).float(), torch.from_numpy(y).float())
    assert got32.dtype == torch.float32 and np.allclose(got32.numpy(), got, rtol=1e-4, atol=1e-6)


def test_score_summary_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    crps = torch.tensor([[[1.0, 2.0]], [[3.0, math.nan]], [[5.0, 6.0]]])  # (T = 3, N = 1, d = 2)
    energy = torch.tensor([[1.0], [math.nan], [4.0]])
    spread = torch.tensor([[[0.5, 1.0, 2.0]], [[0.5, 1.0, 2.0]], [[1.5, 1.0, 4.0]]])
    got = evaluation.score_summary(base.belief_record(crps=crps, energy=energy, spread=spread), start=0)
    assert set(got) == {"crps", "energy", "spread"}
    assert torch.equal(got["crps"], torch.tensor([3.0, 4.0])) and got["energy"] == 2.5
    assert torch.allclose(got["spread"], torch.tensor([2.5 / 3, 1.0, 8.0 / 3]))
    got = evaluation.score_summary(base.belief_record(crps=crps), start=1)
    assert set(got) == {"crps"} and torch.equal(got["crps"], torch.tensor([4.0, 6.0]))
    assert inspect.signature(evaluation.score_summary).parameters["start"].default == evaluation.START_TRUNCATION
    with pytest.raises(ValueError, match="crps"):
        evaluation.score_summary(base.belief_record(energy=energy))


# ------------------------------------------------------------------------------------------ 4. the entry point's host checks
def _args(alias=None, scale=(1.0, 1.0), **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfScoresArgs, _POINTERS, **{**dict(R=2, M=2, d=2, workspace_bytes=64), **over})
    for i, s in enumerate(scale):
        a.scale[i] = s
    return sc.alias_host_args(a, _POINTERS, alias)


def test_scores_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == 42
    call = lambda alias=None, scale=(1.0, 1.0), **over: lib.mmf_pf_scores(ctypes.byref(_args(alias, scale, **over)), None)
    assert lib.mmf_pf_scores(None, None) == EINVAL
    assert call(states=None) == EINVAL
    assert call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(M=0) == EINVAL and call(M=-2) == EINVAL and call(R=-1) == EINVAL
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(scale=(1.0, bad)) == EINVAL and call(scale=(bad, 2.0)) == EINVAL, bad
    assert call(scale=(0.5, 2.0, 0.0, math.nan), R=0) == 0            # (beyond d the scale is not read)
    assert call(crps=None, energy=None, spread=None) == EINVAL       # nothing requested
    assert call(truth=None) == EINVAL and call(truth=None, crps=None) == EINVAL and call(truth=None, energy=None) == EINVAL
    outs, ins = ("crps", "energy", "spread"), ("states", "log_a", "log_b", "truth")
    for out in outs:
        for target in ins + tuple(o for o in outs if o != out):
            assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"spread": ("states", 28)}) == EINVAL and call({"crps": ("energy", 4)}) == EINVAL  # partly on top
    assert call(M=16385) == ETOOLARGE and call(M=1 << 20) == ETOOLARGE
    assert call(M=16385, states=None) == EINVAL                     # an invalid call is invalid whatever its size
    # a row beyond one workgroup needs the workspace: present, large enough, aligned, and clear of everything else
    need = _abi.pf_scores_workspace_bytes(0, 513, 2), _abi.pf_scores_workspace_bytes(1, 513, 2)
    assert need == (0, 2 * 11 * 8) and _abi.pf_scores_workspace_bytes(1, 512, 2) == 0
    assert _abi.pf_scores_workspace_bytes(3, 16384, 4) == 3 * 32 * 11 * 8
    assert call(R=1 << 27, M=16384) == ETOOLARGE                     # R * workgroups per row beyond a 32-bit grid
    # successful no-ops: no rows (the arrays are empty, so nothing is needed and nothing overlaps)
    assert call(R=0) == 0 and call(R=0, M=16384, d=4, scale=(1.0,) * 4) == 0 and call(R=0, M=16385) == ETOOLARGE
    assert call(R=0, log_a=None, log_b=None) == 0 and call(R=0, truth=None, crps=None, energy=None) == 0
    assert call(R=0, workspace=None, workspace_bytes=0, M=4096) == 0
    assert call({"crps": ("states", 0)}, R=0) == 0


def test_scores_workspace_refusals_on_the_host():
    """With ``M > 512`` the arrays no longer fit the 16-float host buffers, but every check below is decided on pointer
    values alone, before any HIP call."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    R, M, d = 1, 513, 1
    need = _abi.pf_scores_workspace_bytes(R, M, d)
    big = [(ctypes.c_float * (R * M * (d + 1) + 64))() for _ in _POINTERS]

    def call(**over):
        a = _abi.MmfPfScoresArgs()
        for name, b in zip(_POINTERS, big):
            setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
        a.R, a.M, a.d, a.workspace_bytes = R, M, d, need
        a.scale[0] = 1.0
        for k, v in over.items():
            setattr(a, k, v)
        a._keep = big
        return lib.mmf_pf_scores(ctypes.byref(a), None)

    base = ctypes.addressof(big[_POINTERS.index("workspace")])
    assert call(workspace=None) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    assert call(workspace=ctypes.c_void_p(base + 4)) == EINVAL       # not 8-byte aligned
    for target in ("states", "log_a", "log_b", "truth", "crps", "energy", "spread"):
        assert call(workspace=ctypes.cast(big[_POINTERS.index(target)], ctypes.c_void_p)) == EINVAL, target
    assert call(R=0) == 0


def test_the_binding_refuses_cpu_tensors():
    import torch

    from multimodalfilter_amd import _abi

    x = torch.zeros((2, 4, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_scores(x, None, None, torch.zeros((2, 3)), torch.zeros((2, 3)), torch.zeros((2,)), torch.zeros((2, 4)))
    with pytest.raises(_abi.MmfError, match="scale"):
        _abi.pf_scores(x, None, None, None, None, None, torch.zeros((2, 4)), scale=(1.0, 1.0))
    assert _abi.SCORES_MAX_M == 16384 == sk.MAX_M


# ------------------------------------------------------------------------------------------ 5. the Python refusals
def test_belief_scores_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_scores is None
    with pytest.raises(ValueError, match="belief_scores needs a history"):
        pf.belief_scores(torch.zeros((1, 1, 3)))
    with pytest.raises(ValueError, match="smoothed record"):
        pf.belief_scores(torch.zeros((1, 1, 3)), of="smoothed")
    with pytest.raises(ValueError, match="of must be"):
        pf.belief_scores(torch.zeros((1, 1, 3)), of="predicted")
    with pytest.raises(TypeError):
        pf.belief_scores()  # the truth is required

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    truth = torch.zeros((T, N, d))
    before = (f.last_history, f.last_smoothed, f.last_quantiles)
    f.last_smoothed = base.belief_record(covariance=torch.zeros((T, N, d, d)), unique=torch.zeros((T, N), dtype=torch.int32), lag=None)
    with pytest.raises(ValueError, match=r"belief_scores\(of='smoothed'\).*no per-step weights"):
        f.belief_scores(truth, of="smoothed")
    f.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_scores(truth, of="smoothed")
    f.last_smoothed = before[1]
    for bad in (None, torch.zeros((T, N)), torch.zeros((T + 1, N, d)), torch.zeros((T, N, d + 1)), np.zeros((T, N, d))):
        with pytest.raises(ValueError, match="truth"):
            f.belief_scores(bad)
    for bad in ((), (1.0, 1.0), (1.0,) * 4, (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, math.nan, 1.0), (1.0, math.inf, 1.0),
                ("1", 1.0, 1.0), (True, 1.0, 1.0), 2.0):
        with pytest.raises(ValueError, match="scale"):
            f.belief_scores(truth, scale=bad)
    big = base.history_record(states=torch.zeros((1, 1, sk.MAX_M + 1, 1)), log_likelihoods=torch.zeros((1, 1, sk.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="16384"):
        f.belief_scores(torch.zeros((1, 1, 1)))
    f.last_history = before[0]
    assert f.last_scores is None and (f.last_history, f.last_smoothed, f.last_quantiles) == before
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    with pytest.raises(_abi.MmfError):
        f.belief_scores(truth, scale=(0.5, 2.0, 1.0))
    assert f.last_scores is None


def test_belief_quantiles_keeps_its_messages_through_the_shared_helper():
    import torch

    import multimodalfilter_amd as mmf

    pf = mmf.door_models.DoorParticleFilter().eval()
    with pytest.raises(ValueError, match="^belief_quantiles needs a history: set record_history and run forward_loop"):
        pf.belief_quantiles((0.5,))
    with pytest.raises(ValueError, match=r"^belief_quantiles\(of='smoothed'\) needs a smoothed record: call smooth"):
        pf.belief_quantiles((0.5,), of="smoothed")


class _Recorded:
    """A stand-in filter on the CPU: ``forward_loop`` returns fixed estimates (``run_filter`` is duck-typed); with a
    covariance it keeps a belief record like a Kalman filter, without one it is a point estimator like the LSTM baselines."""

    def __init__(self, est, cov=None):
        self._est, self._cov = est, cov
        if cov is not None:
            self.record_belief, self.last_belief = False, None

    def initialize_beliefs(self, *, mean, covariance):
        pass

    def forward_loop(self, *, observations, controls):
        if self._cov is not None:
            from multimodalfilter_amd import base

            self.last_belief = base.belief_record(covariance=self._cov) if self.record_belief else None
        return self._est


def test_run_filter_scores_of_a_gaussian_belief_and_of_a_point_estimate():
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
    assert evaluation.run_filter(kf, traj) is est
    out, rec = evaluation.run_filter(kf, traj, return_scores=True)
    assert out is est and kf.record_belief is False                       # the switch is put back, the belief is not returned
    assert set(vars(rec)) == {"crps", "of", "scale"} and rec.of == "filtered" and rec.scale == (1.0,) * d
    assert torch.equal(rec.crps, evaluation.gaussian_crps(est, cov, states[1:])) and bool((rec.crps > 0).all())
    out = evaluation.run_filter(kf, traj, return_belief=True, return_scores=True)
    assert len(out) == 3 and out[1] is kf.last_belief and torch.equal(out[2].crps, rec.crps)
    assert set(evaluation.score_summary(rec, start=0)) == {"crps"}

    point = _Recorded(est)
    scale = (0.5, 2.0, 4.0)
    out, rec = evaluation.run_filter(point, traj, return_scores=True, score_scale=scale)
    e = est - states[1:]
    assert out is est and set(vars(rec)) == {"crps", "energy", "of", "scale"} and rec.scale == scale
    assert torch.equal(rec.crps, e.abs())
    assert torch.allclose(rec.energy, torch.sqrt(((e / torch.tensor(scale)) ** 2).sum(-1)), rtol=1e-6, atol=0)
    got = evaluation.score_summary(rec, start=1)
    assert set(got) == {"crps", "energy"} and torch.allclose(got["crps"], e[1:].abs().mean((0, 1)))
    with pytest.raises(ValueError, match="score_scale"):
        evaluation.run_filter(point, traj, return_scores=True, score_scale=(1.0, 1.0))  # not d of them


def test_run_filter_switch_and_refusals():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert sig["return_scores"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_scores"].default is False
    assert sig["score_scale"].kind is inspect.Parameter.KEYWORD_ONLY and sig["score_scale"].default is None
    assert list(sig)[-3:] == ["return_quantiles", "return_scores", "score_scale"]
    pf = mmf.door_models.DoorParticleFilter().eval()
    for kw in (dict(smooth_method="map"), dict(smooth_lag=3), dict(smooth_lag=None), dict(smooth_method="ancestry", smooth_lag=0)):
        with pytest.raises(ValueError, match="return_scores"):
            evaluation.run_filter(pf, {}, return_scores=True, **kw)  # (before the run: the trajectories are never read)
    for bad in ((1.0, 0.0, 1.0), (1.0, math.nan, 1.0), (), "abc", 3.0):
        with pytest.raises(ValueError, match="score_scale"):
            evaluation.run_filter(pf, {}, return_scores=True, score_scale=bad)
    with pytest.raises(ValueError, match="score_scale"):
        evaluation.run_filter(pf, {}, score_scale=(1.0, 1.0, 1.0))
    assert pf.record_history is False and pf.record_belief is False and pf.last_scores is None

"""CPU-side checks of the particle-posterior modes (``include/mmf.h``: ``MmfPfModesArgs`` / ``mmf_pf_modes``;
``ParticleFilter.belief_modes``; ``evaluation.mode_errors`` / ``mode_summary`` / ``run_filter(return_modes=)``): the fp64
reference of ``_mode_cases`` is held to the answers known by construction and to a bimodal set, its random family is certified
against the same definition in numpy fp32 (the condition on the INPUTS behind the cap on certified differences), struct,
header and binding are tied, and the entry point's and the Python layers' refusals are reached on the host before any HIP call
or device work."""
import ctypes
import inspect
import math
import os
import re

import numpy as np
import pytest

import _density_cases as dc
import _mode_cases as mc
import _score_cases as sk
import _smooth_cases as sc
from _tol import REL_TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("states", "log_a", "log_b", "log_density", "bandwidth")
_OUTPUTS = ("parent", "labels", "count", "index", "modes", "mass", "mean")
_POINTERS = _INPUTS + _OUTPUTS + ("workspace",)
CPU_BY_MS = tuple(M for M in mc.BY_MS if M <= 1025)  # (the reference is O(M^2); the chain alone goes to 4096)


# ------------------------------------------------------------------------------------------ 1. the cap: a condition on the inputs
@pytest.mark.parametrize("M", sk.ALL_MS)
def test_numpy_fp32_links_differ_from_fp64_on_at_most_the_cap_of_every_random_case(M):
    """The definition in numpy fp32 -- the difference, times the fp32 reciprocal, the squares summed in order -- against fp64:
    at most ``CAP_FP32`` of the particles of a case may link differently, and every difference must be certified; so a
    kernel in the same arithmetic can be asked for ``MAX_CERTIFIED``."""
    cases = differing = particles = 0
    for case_id in mc.random_family():
        if case_id[0] != M:
            continue
        case, ref = mc.random_case(*case_id), mc.random_reference(*case_id)
        got = mc.parents(case, np.float32)
        certified, n = mc.check_parents(case, ref["parent"], got, str(case_id), cap=mc.CAP_FP32)
        differing, particles, cases = differing + certified, particles + n, cases + 1
    print(f"M={M}: {differing} differing links among {particles} participating particles of {cases} cases")
    assert cases >= len(dc.VARIANTS) - len(mc.TRUTH_VARIANTS)


def test_lattice_cases_are_exact_in_fp32_and_do_not_move_with_the_shift():
    for M, d, R in mc.lattice_family():
        case, ref = mc.lattice_case(M, d, R), mc.lattice_reference(M, d, R)
        assert np.array_equal(mc.parents(case, np.float32), ref["parent"]), (M, d, R)
        moved = mc.lattice_case(M, d, R, shift=mc.LATTICE_SHIFT)
        assert np.array_equal(moved["log_density"], case["log_density"]) and moved["link_radius"] == case["link_radius"]
        assert np.array_equal(mc.parents(moved), ref["parent"]) and np.array_equal(mc.parents(moved, np.float32), ref["parent"])
        part = mc.takes_part(case)
        assert 0 < (~part).sum() or M < 8
        assert (ref["parent"][~part] == -1).all() and (ref["labels"][~part] == -1).all()
        ties = sum(len(np.unique(case["log_density"][r][part[r]])) < part[r].sum() for r in range(R))
        assert ties == R or M < 17  # (16 levels: exact ties everywhere)


def test_the_random_family_cycles_the_radius_and_the_number_of_modes():
    seen = list(mc.random_family())
    assert {c[0] for c in seen} == set(sk.ALL_MS) and not {c[3] for c in seen} & set(mc.TRUTH_VARIANTS)
    for M in sk.ALL_MS:
        mine = [mc.random_case(*c) for c in seen if c[0] == M and (M > sk.SMALL or c[1] == 3)]
        assert {c["link_radius"] for c in mine} == set(mc.TAUS) and {c["max_modes"] for c in mine} == set(mc.KS), M
    assert mc.LDS_MASS_M - 1 in mc.BY_MS and mc.LDS_MASS_M in mc.BY_MS and mc.LDS_MASS_M + 1 in mc.BY_MS and mc.MAX_M in mc.BY_MS
    for M in (1, 2, 63, 64, 65, 511, 512, 513, 1023, 1024, 1025, 4096):
        assert M in mc.BY_MS


# ------------------------------------------------------------------------------------------ 2. the reference, by construction
def _hold_construction(kind, M):
    case, exp = mc.constructed_case(kind, M)
    ref = mc.reference(case)
    what = f"{kind} M={M}"
    if "parent" in exp:
        assert np.array_equal(ref["parent"][0], exp["parent"]), what
    assert np.array_equal(ref["labels"][0], exp["labels"]) and int(ref["count"][0]) == exp["count"], what
    n = len(exp["index"])
    assert n == min(exp["count"], case["max_modes"]) and np.array_equal(ref["index"][0, :n], exp["index"]), (what, ref["index"])
    assert (ref["index"][0, n:] == -1).all() and (ref["mass"][0, n:] == 0).all() and np.isnan(ref["mean"][0, n:]).all()
    # 2^-40 is the grain of the integer masses
    assert np.abs(ref["mass"][0, :n] - exp["mass"]).max() <= 1e-11 * M, (what, ref["mass"], exp["mass"])
    assert np.abs(ref["mean"][0, :n] - exp["mean"]).max() <= 1e-10 * max(1.0, np.abs(exp["mean"]).max()), (what, ref["mean"], exp["mean"])
    assert mc.check_forest(case, {k: ref[k] for k in mc.OUTPUTS}, what) == 0.0


@pytest.mark.parametrize("kind", mc.CONSTRUCTIONS)
def test_the_reference_gives_the_answers_known_by_construction(kind):
    for M in CPU_BY_MS:
        _hold_construction(kind, M)


def test_the_reference_walks_a_chain_of_4096_within_a_second():
    import time

    t0 = time.perf_counter()
    _hold_construction("chain", 4096)
    took = time.perf_counter() - t0
    print(f"chain of 4096: reference and checks in {took:.2f} s")


@pytest.mark.parametrize("tau", [1.0, 2.0, 3.0, 4.0])
def test_a_bimodal_set_has_exactly_its_two_modes(tau):
    """90 + 210 particles, sigma = 0.1, centres 2 apart, d = 3, Silverman's bandwidths: two modes with 90 and 210 members.
    The centres are 2 apart along the diagonal, so every dimension sees both of them and gets a bandwidth of about 0.23: a
    cluster is half a bandwidth wide and the two are 8.7 bandwidths apart.  (With the centres apart along one axis the rule
    gives the other two dimensions 0.04, a cluster is 2.3 bandwidths wide there and a radius of 1 finds 38 local maxima:
    a product kernel with one bandwidth per dimension at work, not an error.)"""
    rng = np.random.default_rng(5)
    c = np.ones(3) / math.sqrt(3.0)
    X = np.concatenate([rng.normal(0.0, 0.1, (90, 3)) - c, rng.normal(0.0, 0.1, (210, 3)) + c])[None].astype(np.float32)
    ref = dc.reference_rows(X, np.ones((1, 300)), None, "silverman", None, (1e-6,) * 3)
    case = dict(states=X, log_a=None, log_b=None, log_density=ref["log_density"].astype(np.float32),
                bandwidth=ref["bandwidth"].astype(np.float32), link_radius=tau, max_modes=4)
    got = mc.reference(case)
    assert int(got["count"][0]) == 2 and got["index"][0, 0] >= 90 > got["index"][0, 1] >= 0 and (got["index"][0, 2:] == -1).all()
    assert (got["labels"][0, :90] == got["index"][0, 1]).all() and (got["labels"][0, 90:] == got["index"][0, 0]).all()
    assert np.abs(got["mass"][0] - np.asarray([0.7, 0.3, 0.0, 0.0])).max() <= 1e-11
    assert np.abs(got["mean"][0, 0] - X[0, 90:].astype(np.float64).mean(0)).max() <= 1e-12
    assert np.abs(got["mean"][0, 1] - X[0, :90].astype(np.float64).mean(0)).max() <= 1e-12


def test_the_rules_refuse_what_they_must():
    case, ref = mc.lattice_case(65, 2, 1), mc.lattice_reference(65, 2, 1)
    part = mc.takes_part(case)[0]
    linked = np.flatnonzero(part & (ref["parent"][0] >= 0))
    roots = np.flatnonzero(part & (ref["parent"][0] < 0))
    bad = ref["parent"].copy()
    bad[0, linked[0]] = -1                                     # a root where the reference links well inside the radius
    with pytest.raises(AssertionError):
        mc.check_parents(case, ref["parent"], bad)
    bad = ref["parent"].copy()
    bad[0, roots[0]] = linked[0]                               # a link from the row's top particle: not above it
    with pytest.raises(AssertionError):
        mc.check_parents(case, ref["parent"], bad)
    bad = ref["parent"].copy()
    bad[0, np.flatnonzero(~part)[0]] = 0                       # a dead particle with a parent
    with pytest.raises(AssertionError):
        mc.check_parents(case, ref["parent"], bad)
    got = {k: ref[k].copy() for k in mc.OUTPUTS}
    assert mc.check_forest(case, got, exact_index=True) == 0.0
    for k, edit in (("labels", lambda a: a.__setitem__((0, linked[0]), linked[0])), ("count", lambda a: a.__setitem__(0, a[0] + 1)),
                    ("mass", lambda a: a.__setitem__((0, 0), a[0, 0] * 0.5)), ("modes", lambda a: a.__setitem__((0, 0, 0), 9.0)),
                    ("index", lambda a: a.__setitem__((0, 0), linked[0]))):
        broken = {n: v.copy() for n, v in got.items()}
        edit(broken[k])
        with pytest.raises(AssertionError):
            assert mc.check_forest(case, broken) <= REL_TOL


# ------------------------------------------------------------------------------------------ 3. struct, header, binding
def test_struct_header_and_binding_are_tied():
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == _abi.ABI_VERSION == 42
    text = open(os.path.join(ROOT, "include", "mmf.h")).read()
    assert int(re.search(r"^#define MMF_PF_MODES_MAX\s+(\d+)", text, re.M).group(1)) == _abi.MODES_MAX == mc.MAX_MODES == 8
    assert int(re.search(r"^#define MMF_PF_MODES_LDS_MASS_M\s+(\d+)", text, re.M).group(1)) == _abi.MODES_LDS_MASS_M == mc.LDS_MASS_M
    assert _abi.MODES_MAX_M == mc.MAX_M == 16384
    body = re.search(r"typedef struct MmfPfModesArgs \{(.*?)\} MmfPfModesArgs;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = re.findall(r"(\w+)\s*[,;]", body)
    assert names == [f for f, _ in _abi.MmfPfModesArgs._fields_], names
    assert _abi.SIGNATURES["mmf_pf_modes"][0] is ctypes.c_int and _abi.SIGNATURES["mmf_pf_modes_workspace_bytes"][0] is ctypes.c_size_t
    assert "mmf_pf_modes" in re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "Particle-posterior modes" in text


# ------------------------------------------------------------------------------------------ 4. the entry point's host checks
def _args(alias=None, **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfModesArgs, _POINTERS, **{**dict(R=2, M=2, d=2, max_modes=2, link_radius=3.0, workspace_bytes=64), **over})
    return sc.alias_host_args(a, _POINTERS, alias)


def _call(alias=None, **over):
    return sc.lib().mmf_pf_modes(ctypes.byref(_args(alias, **over)), None)


def test_modes_refuses_null_arguments():
    assert sc.lib().mmf_pf_modes(None, None) == EINVAL
    for k in ("states", "log_density", "bandwidth"):
        assert _call(**{k: None}) == EINVAL, k
    assert _call(R=0) == 0 and _call(R=0, log_a=None, log_b=None) == 0


def test_modes_refuses_a_state_dimension_outside_1_to_4():
    assert _call(d=0) == EINVAL and _call(d=5) == EINVAL and _call(d=-1) == EINVAL
    assert _call(R=0, d=4, M=1) == 0 and _call(R=0, d=1) == 0


def test_modes_refuses_no_particles_and_negative_rows():
    assert _call(M=0) == EINVAL and _call(M=-2) == EINVAL and _call(R=-1) == EINVAL


def test_modes_refuses_a_number_of_modes_outside_1_to_8():
    assert _call(max_modes=0) == EINVAL and _call(max_modes=9) == EINVAL and _call(max_modes=-1) == EINVAL
    assert _call(R=0, max_modes=1) == 0 and _call(R=0, max_modes=8) == 0 and _call(R=0, max_modes=9) == EINVAL


def test_modes_refuses_a_link_radius_that_is_not_finite_and_positive():
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert _call(link_radius=bad) == EINVAL and _call(R=0, link_radius=bad) == EINVAL, bad
    assert _call(R=0, link_radius=1e-3) == 0 and _call(R=0, link_radius=1e30) == 0


def test_modes_refuses_a_call_without_outputs():
    assert _call(**{k: None for k in _OUTPUTS}) == EINVAL
    for out in _OUTPUTS:
        assert _call(R=0, **{k: None for k in _OUTPUTS if k != out}) == 0, out   # any one output is a request


def test_modes_refuses_a_workspace_that_is_missing_too_small_or_misaligned():
    from multimodalfilter_amd import _abi

    ws = _abi.pf_modes_workspace_bytes
    assert ws(0, 513, 2) == 0 and ws(1, 0, 2) == 0 and ws(1, 513, 0) == 0
    for M in (1, 2, 511, 512, 513, 4096, mc.LDS_MASS_M):
        for R in (1, 3):
            assert ws(R, M, 1) == ws(R, M, 4) == (4 * R * M + 7) // 8 * 8, (R, M)
    for M in (mc.LDS_MASS_M + 1, mc.MAX_M):
        for R in (1, 3):
            assert ws(R, M, 1) == ws(R, M, 4) == 8 * R * M + (4 * R * M + 7) // 8 * 8, (R, M)
    need = ws(2, 2, 2)
    assert need == 16
    assert _call(workspace=None) == EINVAL and _call(workspace_bytes=need - 1) == EINVAL and _call(workspace_bytes=0) == EINVAL
    a = _args()
    a.workspace = ctypes.c_void_p(ctypes.addressof(a._buffers[_POINTERS.index("workspace")]) + 4)
    assert sc.lib().mmf_pf_modes(ctypes.byref(a), None) == EINVAL         # not 8-byte aligned
    assert _call(R=0, workspace=None, workspace_bytes=0, M=4096) == 0


def test_modes_refuses_an_output_on_top_of_an_input_or_another_output():
    for out in _OUTPUTS + ("workspace",):
        for target in _INPUTS + tuple(o for o in _OUTPUTS if o != out):
            assert _call({out: (target, 0)}) == EINVAL, (out, target)
    assert _call({"labels": ("states", 28)}) == EINVAL and _call({"mean": ("mass", 8)}) == EINVAL  # partly on top
    assert _call({"parent": ("states", 0)}, R=0) == 0   # (no rows: the arrays are empty)


def test_modes_refuses_too_many_particles_and_a_grid_beyond_32_bits():
    assert _call(M=16385) == ETOOLARGE and _call(M=1 << 20) == ETOOLARGE
    assert _call(M=16385, states=None) == EINVAL                        # an invalid call is invalid whatever its size
    assert _call(R=1 << 27, M=16384) == ETOOLARGE
    assert _call(R=0, M=16384, d=4) == 0 and _call(R=0, M=16385) == ETOOLARGE


def test_the_binding_refuses_cpu_tensors_and_a_bad_number_of_modes():
    import torch

    from multimodalfilter_amd import _abi

    x, ld, h = torch.zeros((2, 4, 3)), torch.zeros((2, 4)), torch.ones((2, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_modes(x, None, None, ld, h, count=torch.zeros((2,), dtype=torch.int32))
    for bad in (0, 9):
        with pytest.raises(_abi.MmfError, match="max_modes"):
            _abi.pf_modes(x, None, None, ld, h, max_modes=bad, count=torch.zeros((2,), dtype=torch.int32))


# ------------------------------------------------------------------------------------------ 5. the Python refusals
def test_belief_modes_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    sig = inspect.signature(mmf.filters.ParticleFilter.belief_modes).parameters
    assert list(sig) == ["self", "of", "max_modes", "link_radius", "bandwidth", "min_bandwidth"] and sig["of"].default == "filtered"
    assert sig["of"].kind is inspect.Parameter.POSITIONAL_OR_KEYWORD and sig["max_modes"].kind is inspect.Parameter.KEYWORD_ONLY
    assert sig["max_modes"].default == 4 and sig["link_radius"].default == 3.0
    assert sig["bandwidth"].default == "silverman" and sig["min_bandwidth"].default == 1e-6
    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_modes is None
    with pytest.raises(ValueError, match="^belief_modes needs a history"):
        pf.belief_modes()
    with pytest.raises(ValueError, match=r"^belief_modes\(of='smoothed'\) needs a smoothed record"):
        pf.belief_modes("smoothed")
    with pytest.raises(ValueError, match="of must be"):
        pf.belief_modes(of="predicted")

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    before = (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores, f.last_density)
    f.last_smoothed = base.belief_record(covariance=torch.zeros((T, N, d, d)), unique=torch.zeros((T, N), dtype=torch.int32), lag=None)
    with pytest.raises(ValueError, match=r"belief_modes\(of='smoothed'\).*no per-step weights"):
        f.belief_modes("smoothed")
    f.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_modes("smoothed")
    f.last_smoothed = before[1]
    for bad in (0, 9, -1, 2.0, True, "4", None):
        with pytest.raises(ValueError, match="max_modes must be an integer in 1 .. 8"):
            f.belief_modes(max_modes=bad)
    for bad in (0.0, -1.0, math.nan, math.inf, True, "3", None, (3.0,)):
        with pytest.raises(ValueError, match="link_radius must be a positive finite float"):
            f.belief_modes(link_radius=bad)
    for bad in ((), (1.0, 1.0), (1.0, 0.0, 1.0), 2.0, "epanechnikov", None):
        with pytest.raises(ValueError, match="^belief_modes: bandwidth must be 'silverman', 'scott' or 3"):
            f.belief_modes(bandwidth=bad)
    for bad in ((), (1.0, 1.0), 0.0, math.nan, True, None):
        with pytest.raises(ValueError, match="^belief_modes: min_bandwidth"):
            f.belief_modes(min_bandwidth=bad)
    big = base.history_record(states=torch.zeros((1, 1, mc.MAX_M + 1, 1)), log_likelihoods=torch.zeros((1, 1, mc.MAX_M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    f.last_history = big
    with pytest.raises(ValueError, match="16384"):
        f.belief_modes()
    f.last_history = before[0]
    assert f.last_modes is None and (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores, f.last_density) == before
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    for kw in (dict(), dict(max_modes=8, link_radius=1, bandwidth="scott"), dict(bandwidth=(0.5, 2.0, 1.0))):
        with pytest.raises(_abi.MmfError):
            f.belief_modes(**kw)
    assert f.last_modes is None and f.last_density is None


def test_run_filter_modes_switch_and_refusals():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert sig["return_modes"].kind is inspect.Parameter.KEYWORD_ONLY and sig["return_modes"].default is None
    assert sig["modes_link_radius"].kind is inspect.Parameter.KEYWORD_ONLY and sig["modes_link_radius"].default == 3.0
    pf = mmf.door_models.DoorParticleFilter().eval()
    for kw in (dict(smooth_method="map"), dict(smooth_lag=3), dict(smooth_lag=None), dict(smooth_method="ancestry", smooth_lag=0)):
        with pytest.raises(ValueError, match="return_modes"):
            evaluation.run_filter(pf, {}, return_modes=4, **kw)  # (before the run: the trajectories are never read)
    for bad in (0, 9, 2.5, True, "4", (4,)):
        with pytest.raises(ValueError, match="return_modes must be None or"):
            evaluation.run_filter(pf, {}, return_modes=bad)
    for bad in (0.0, -2.0, math.nan, math.inf, "3", None):
        with pytest.raises(ValueError, match="modes_link_radius must be"):
            evaluation.run_filter(pf, {}, return_modes=4, modes_link_radius=bad)
    for given in (3.0, 1.5):
        with pytest.raises(ValueError, match="modes_link_radius.*without return_modes"):
            evaluation.run_filter(pf, {}, modes_link_radius=given)
    lstm = mmf.door_models.DoorLSTMFilter().eval()
    with pytest.raises(ValueError, match="return_modes.*no modes"):
        evaluation.run_filter(lstm, {}, return_modes=4)
    assert pf.record_history is False and pf.record_belief is False and pf.last_modes is None


# ------------------------------------------------------------------------------------------ 6. mode_errors, mode_summary
def _hand_made_record():
    import torch

    from multimodalfilter_amd import base

    nan = math.nan
    # T = 3, N = 1, K = 2, d = 2: two modes, one mode, none
    modes = torch.tensor([[[[0.0, 0.0], [3.0, 4.0]]], [[[1.0, 1.0], [nan, nan]]], [[[nan, nan], [nan, nan]]]])
    mass = torch.tensor([[[0.75, 0.25]], [[1.0, 0.0]], [[0.0, 0.0]]])
    count = torch.tensor([[2], [1], [0]], dtype=torch.int32)
    true = torch.tensor([[[3.0, 0.0]], [[1.0, 3.0]], [[0.0, 0.0]]])
    return base.belief_record(modes=modes, mass=mass, count=count), true


def test_mode_errors_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    rec, true = _hand_made_record()
    got = evaluation.mode_errors(rec, true)
    assert set(got) == {"top", "best", "best_rank"}
    assert got["top"][:2, 0].tolist() == [3.0, 2.0] and math.isnan(float(got["top"][2, 0]))
    assert got["best"][:2, 0].tolist() == [3.0, 2.0] and math.isnan(float(got["best"][2, 0]))
    assert got["best_rank"][:, 0].tolist() == [0, 0, -1]
    far = evaluation.mode_errors(rec, torch.tensor([[[3.0, 3.0]], [[1.0, 3.0]], [[0.0, 0.0]]]))
    assert far["best"][0, 0] == 1.0 and far["best_rank"][0, 0] == 1 and abs(float(far["top"][0, 0]) - math.sqrt(18.0)) < 1e-6
    scaled = evaluation.mode_errors(rec, true, scale=(3.0, 1.0))
    assert scaled["top"][:2, 0].tolist() == [1.0, 2.0]
    for bad in ((1.0,), (1.0, 0.0), (1.0, math.nan), "ab", 2.0):
        with pytest.raises(ValueError, match="scale"):
            evaluation.mode_errors(rec, true, scale=bad)
    with pytest.raises(ValueError, match="true must be"):
        evaluation.mode_errors(rec, true[:2])
    with pytest.raises(ValueError, match="no modes"):
        evaluation.mode_errors(base.belief_record(mass=rec.mass), true)


def test_mode_summary_against_hand_computed_values():
    from multimodalfilter_amd import base, evaluation

    rec, true = _hand_made_record()
    got = evaluation.mode_summary(rec, start=0)
    assert got == {"count": 1.0, "top_mass": (0.75 + 1.0 + 0.0) / 3, "multimodal": 1.0 / 3}
    got = evaluation.mode_summary(rec, true, start=0)
    assert set(got) == {"count", "top_mass", "multimodal", "top_rmse", "best_rmse"}
    assert abs(got["top_rmse"] - math.sqrt((9.0 + 4.0) / 2)) < 1e-12 and abs(got["best_rmse"] - math.sqrt((9.0 + 4.0) / 2)) < 1e-12
    assert evaluation.mode_summary(rec, start=1) == {"count": 0.5, "top_mass": 0.5, "multimodal": 0.0}
    assert inspect.signature(evaluation.mode_summary).parameters["start"].default == evaluation.START_TRUNCATION
    with pytest.raises(ValueError, match="count"):
        evaluation.mode_summary(base.belief_record(modes=rec.modes))


def test_run_filter_gives_a_gaussian_belief_its_one_mode():
    import torch

    from multimodalfilter_amd import evaluation
    from _filter_stubs import _Recorded

    g = torch.Generator().manual_seed(3)
    T, N, d = 5, 2, 3
    states = torch.randn((T + 1, N, d), generator=g)
    traj = dict(states=states, image=torch.zeros((T + 1, N, 1)), gripper_pos=torch.zeros((T + 1, N, 1)),
                gripper_sensors=torch.zeros((T + 1, N, 1)), controls=torch.zeros((T + 1, N, 1)))
    est = states[1:] + 0.3 * torch.randn((T, N, d), generator=g)
    A = torch.randn((T, N, d, d), generator=g)
    kf = _Recorded(est, A @ A.transpose(-1, -2) + 0.1 * torch.eye(d))
    assert evaluation.run_filter(kf, traj) is est and evaluation.run_filter(kf, traj, return_modes=None) is est
    out, rec = evaluation.run_filter(kf, traj, return_modes=3)
    assert out is est and kf.record_belief is False
    assert set(vars(rec)) == {"modes", "mean", "mass", "count", "of", "max_modes"} and rec.of == "filtered" and rec.max_modes == 3
    assert rec.modes.shape == (T, N, 3, d) and torch.equal(rec.modes[:, :, 0], est) and bool(torch.isnan(rec.modes[:, :, 1:]).all())
    assert torch.equal(rec.mean[:, :, 0], est) and bool((rec.mass[:, :, 0] == 1).all()) and bool((rec.mass[:, :, 1:] == 0).all())
    assert rec.count.dtype == torch.int32 and bool((rec.count == 1).all())
    errors = evaluation.mode_errors(rec, states[1:])
    assert torch.equal(errors["top"], errors["best"]) and bool((errors["best_rank"] == 0).all())
    assert torch.allclose(errors["top"], torch.linalg.vector_norm(est - states[1:], dim=-1))
    summary = evaluation.mode_summary(rec, states[1:], start=1)
    assert summary["count"] == 1.0 and summary["top_mass"] == 1.0 and summary["multimodal"] == 0.0
    out = evaluation.run_filter(kf, traj, return_belief=True, return_scores=True, return_density=True, return_modes=1)
    assert len(out) == 5 and out[1] is kf.last_belief and hasattr(out[2], "crps") and hasattr(out[3], "entropy")
    assert out[4].modes.shape == (T, N, 1, d)
    point = _Recorded(est)
    with pytest.raises(ValueError, match="return_modes.*no modes"):
        evaluation.run_filter(point, traj, return_modes=2)

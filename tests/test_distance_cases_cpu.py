"""CPU-side checks of the particle-posterior distances (``include/mmf.h``: ``MmfPfDistanceArgs`` / ``mmf_pf_distance``;
``ParticleFilter.belief_distance``; ``evaluation.compare_filters`` / ``distance_summary``): the family of ``_distance_cases``
is certified against its own fp32 formulation and against the margin that bounds the cancellation of the energy distance,
the fp64 reference obeys the identities of the distances, and the entry point's and the Python layers' refusals are reached on
the host before any HIP call or device work."""
import ctypes
import inspect
import math

import numpy as np
import pytest

import _distance_cases as dc
import _smooth_cases as sc

EINVAL, ETOOLARGE = -1, -2
_INPUTS = ("states_a", "log_a_a", "log_b_a", "states_b", "log_a_b", "log_b_b")
_OUTPUTS = ("wasserstein", "cramer", "ks", "energy", "terms")
_POINTERS = _INPUTS + _OUTPUTS + ("workspace",)


@pytest.fixture(autouse=True, scope="module")
def _the_entry_these_tests_describe():
    """The family and the reference of this module define ONE entry point: without the binding, the method and the
    evaluation functions there is nothing they are the reference of."""
    from multimodalfilter_amd import _abi, evaluation, filters

    assert hasattr(_abi, "MmfPfDistanceArgs") and callable(getattr(_abi, "pf_distance", None))
    assert callable(getattr(filters.ParticleFilter, "belief_distance", None))
    assert callable(getattr(evaluation, "compare_filters", None)) and callable(getattr(evaluation, "distance_summary", None))


def _margin(terms):
    """``(2 t0 - t1 - t2) / ((t1 + t2) / 2)`` of the live rows, the least of them (inf without spread or without a live row)."""
    ok = ~np.isnan(terms[:, 0])
    if not ok.any():
        return math.inf
    num, den = 2 * terms[ok, 0] - terms[ok, 1] - terms[ok, 2], 0.5 * (terms[ok, 1] + terms[ok, 2])
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(den > 0, num / den, np.inf).min())


# ------------------------------------------------------------------------------------------ 1. the family is certified
@pytest.mark.parametrize("Ma,Mb", dc.PAIRS)
def test_the_fp32_yardstick_is_within_the_cap_and_the_energy_margin_holds_on_the_family(Ma, Mb):
    """Two conditions on the INPUTS, every case held to both and none skipped: the definition evaluated in fp32 stays within
    ``CAP = REL_TOL / 3`` of fp64 on every output -- so the GPU bar ``max(REL_TOL, 3 x yardstick)`` is ``REL_TOL`` -- and
    ``2 terms[0] - terms[1] - terms[2] >= 0.1 x (terms[1] + terms[2]) / 2`` in fp64, with which the cancellation inside
    ``energy`` amplifies the error of ``terms`` by no more than about 20.  A draw that breaks one is replaced (``RESEED``)."""
    worst, least, cases = 0.0, math.inf, 0
    for key in dc.family():
        if key[:2] != (Ma, Mb):
            continue
        case, ref, yard = dc.family_case(*key)
        m = _margin(ref["terms"])
        print(f"{key}: yardstick " + ", ".join(f"{k} {e:.2e}" for k, e in yard.items()) + f"; margin {m:.3f}")
        assert max(yard.values()) < dc.CAP, (key, yard)
        assert m >= dc.ENERGY_MARGIN, (key, m)
        assert dc.bar(max(yard.values())) == 1e-4
        worst, least, cases = max(worst, max(yard.values())), min(least, m), cases + 1
    assert cases >= len(dc.VARIANTS)
    print(f"({Ma}, {Mb}): worst yardstick error {worst:.3e} (cap {dc.CAP:.0e}), least margin {least:.3f} over {cases} cases")


def test_the_family_covers_what_the_definition_distinguishes():
    seen = set(dc.family())
    assert {k[:2] for k in seen} == set(dc.PAIRS)
    for pair in dc.PAIRS:
        assert {k[4] for k in seen if k[:2] == pair} == set(range(len(dc.VARIANTS)))
        assert {k[2] for k in seen if k[:2] == pair and k[4] == 0} == set(dc.DIMS)
    for key in dc.RESEED:
        assert key in seen, key
    # NaN exactly where the definition puts it: the dead row of either side, in every output
    for v in (6, 7):
        assert "dead_row" in dc.VARIANTS[v][:2]
        case, ref, _ = dc.family_case(64, 64, 3, 5, v)
        for k in dc.OUTPUTS:
            assert np.isnan(ref[k][2]).all() and np.isfinite(np.delete(ref[k], 2, 0)).all(), (v, k)
    case, ref, _ = dc.family_case(64, 64, 3, 5, 0)
    assert np.isnan(case["a"]["states"]).any() and np.isinf(case["b"]["log_b"]).any()  # dead particles carry NaN rows
    assert all(np.isfinite(ref[k]).all() for k in dc.OUTPUTS)
    assert bool((ref["ks"] > 0).all()) and bool((ref["ks"] <= 1).all())
    assert dc.family_case(64, 64, 3, 5, 8)[0]["scale"] == dc.SCALE[:3]


# ------------------------------------------------------------------------------------------ 2. identities of the reference
def _pair_form(x, wx, y, wy):
    """``2 E|x - y| - E|x - x'| - E|y - y'|`` of one coordinate under normalised weights, dense, in fp64."""
    e = lambda p, wp, q, wq: float(wp @ np.abs(p[:, None] - q[None, :]) @ wq)
    return 2.0 * e(x, wx, y, wy) - e(x, wx, x, wx) - e(y, wy, y, wy)


@pytest.mark.parametrize("Ma,Mb", [(1, 37), (37, 300), (64, 64), (300, 37)])
def test_twice_the_cramer_distance_is_the_pair_form_of_the_coordinate(Ma, Mb):
    """``2 int (F_a - F_b)^2 dx = 2 E|x - y| - E|x - x'| - E|y - y'|`` per coordinate.  The two sides differ by the
    ``2^-24`` truncation of the fixed-point weights on the one and the plain weights on the other: held to 1e-4 of the
    value itself (measured: 1e-5; 4e-6 of the form's largest term, ``2 E|x - y|``)."""
    worst = own = 0.0
    for d in dc.DIMS:
        for v in (0, 1, 4):
            case = dc.make_case(Ma, Mb, d, 3, v)
            ref = dc.reference(case, outputs=("cramer",))
            Wa, Wb = dc._weights(case["a"], np.float64), dc._weights(case["b"], np.float64)
            for r in range(Wa.shape[0]):
                la, lb = Wa[r] > 0, Wb[r] > 0
                wa, wb = Wa[r][la] / Wa[r][la].sum(), Wb[r][lb] / Wb[r][lb].sum()
                for k in range(d):
                    x, y = case["a"]["states"][r][la, k].astype(np.float64), case["b"]["states"][r][lb, k].astype(np.float64)
                    want = _pair_form(x, wa, y, wb)
                    size = 2.0 * float(wa @ np.abs(x[:, None] - y[None, :]) @ wb)
                    gap = abs(2.0 * ref["cramer"][r, k] - want) / abs(want)
                    own, worst = max(own, gap), max(worst, abs(2.0 * ref["cramer"][r, k] - want) / size)
                    assert gap <= 1e-4, (Ma, Mb, d, v, r, k, gap)
    print(f"({Ma}, {Mb}): 2 cramer against the pair form, worst {worst:.3e} of 2 E|x - y|, {own:.3e} of itself")


def test_two_point_masses():
    """``wasserstein = cramer = |x - y|`` per coordinate, ``ks = 1``, ``energy = sqrt(2 |x - y|_2)``."""
    rng = np.random.default_rng(11)
    for d in dc.DIMS:
        x, y = rng.standard_normal((4, 1, d)).astype(np.float32), rng.standard_normal((4, 1, d)).astype(np.float32)
        side = lambda s: dict(states=s, log_a=None, log_b=None)
        ref = dc.reference(dict(a=side(x), b=side(y), scale=None))
        e = np.abs(x[:, 0].astype(np.float64) - y[:, 0])
        assert np.allclose(ref["wasserstein"], e, rtol=1e-15, atol=0) and np.allclose(ref["cramer"], e, rtol=1e-15, atol=0)
        assert np.array_equal(ref["ks"], np.ones_like(e))
        norm = np.sqrt((e ** 2).sum(-1))
        assert np.allclose(ref["energy"], np.sqrt(2.0 * norm), rtol=1e-14, atol=0)
        assert np.allclose(ref["terms"], np.stack([norm, 0 * norm, 0 * norm], -1), rtol=1e-15, atol=0)
        same = dc.reference(dict(a=side(x), b=side(x), scale=None))
        assert all(np.array_equal(same[k], np.zeros_like(same[k])) for k in dc.OUTPUTS)


def test_equal_size_uniform_sets_in_one_dimension_are_matched_in_order():
    """With ``n`` equally weighted particles on either side the optimal transport pairs the order statistics."""
    rng = np.random.default_rng(12)
    for n in (2, 37, 300):
        x, y = rng.standard_normal((3, n, 1)).astype(np.float32), (1.2 * rng.standard_normal((3, n, 1)) + 0.5).astype(np.float32)
        side = lambda s: dict(states=s, log_a=None, log_b=None)
        ref = dc.reference(dict(a=side(x), b=side(y), scale=None), outputs=("wasserstein",))
        want = np.abs(np.sort(x[:, :, 0].astype(np.float64), axis=1) - np.sort(y[:, :, 0].astype(np.float64), axis=1)).mean(1)
        assert np.allclose(ref["wasserstein"][:, 0], want, rtol=1e-12, atol=0), n


def test_a_shifted_copy_is_its_shift_away():
    """``B = A + c`` under A's weights: ``wasserstein[k] = |c_k|`` (to the rounding of ``x + c`` to float32)."""
    for Ma, d, v in ((37, 3, 0), (64, 4, 4), (300, 2, 0)):
        case = dc.make_case(Ma, Ma, d, 3, v)
        c = np.asarray([0.25, -1.5, 3.0, -0.125][:d], np.float32)
        case = dict(case, b=dict(case["a"], states=case["a"]["states"] + c))
        ref = dc.reference(case, outputs=("wasserstein", "ks"))
        assert np.allclose(ref["wasserstein"], np.abs(c.astype(np.float64))[None], rtol=1e-6, atol=0), (Ma, d, v)
        assert bool((ref["ks"] > 0).all())


# ------------------------------------------------------------------------------------------ 3. the entry point's host checks
def _args(alias=None, scale=(1.0, 1.0), **over):
    """Sizes at which every array fits the 16-float buffer ``host_args`` gives it; ``alias``: as for
    ``_smooth_cases.alias_host_args``."""
    from multimodalfilter_amd import _abi

    a = sc.host_args(_abi.MmfPfDistanceArgs, _POINTERS, **{**dict(R=2, Ma=2, Mb=2, d=2, workspace_bytes=64), **over})
    for i, s in enumerate(scale):
        a.scale[i] = s
    return sc.alias_host_args(a, _POINTERS, alias)


def test_distance_refuses_bad_arguments_on_the_host():
    """Every refusal of the header with its return code, decided before any HIP call: the pointers are host memory and never
    dereferenced, and the stream is null."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    assert lib.mmf_version() == 42
    call = lambda alias=None, scale=(1.0, 1.0), **over: lib.mmf_pf_distance(ctypes.byref(_args(alias, scale, **over)), None)
    assert lib.mmf_pf_distance(None, None) == EINVAL
    assert call(states_a=None) == EINVAL and call(states_b=None) == EINVAL
    assert call(d=0) == EINVAL and call(d=5) == EINVAL and call(d=-1) == EINVAL
    assert call(Ma=0) == EINVAL and call(Mb=0) == EINVAL and call(Ma=-2) == EINVAL and call(Mb=-2) == EINVAL and call(R=-1) == EINVAL
    for bad in (0.0, -1.0, math.nan, math.inf, -math.inf):
        assert call(scale=(1.0, bad)) == EINVAL and call(scale=(bad, 2.0)) == EINVAL, bad
    assert call(scale=(0.5, 2.0, 0.0, math.nan), R=0) == 0            # (beyond d the scale is not read)
    assert call(**{k: None for k in _OUTPUTS}) == EINVAL             # nothing requested
    for k in _OUTPUTS:                                               # any one output alone is a request
        assert call(R=0, **{o: None for o in _OUTPUTS if o != k}) == 0, k
    for out in _OUTPUTS:
        for target in _INPUTS + tuple(o for o in _OUTPUTS if o != out):
            assert call({out: (target, 0)}) == EINVAL, (out, target)
    assert call({"terms": ("states_b", 28)}) == EINVAL and call({"cramer": ("ks", 4)}) == EINVAL  # partly on top
    # one limit for the whole entry: the union of both sets
    assert call(Ma=16384, Mb=1) == ETOOLARGE and call(Ma=1, Mb=16384) == ETOOLARGE and call(Ma=8193, Mb=8192) == ETOOLARGE
    assert call(Ma=1 << 30, Mb=1 << 30) == ETOOLARGE and call(Ma=(1 << 31) - 1, Mb=(1 << 31) - 1) == ETOOLARGE
    assert call(Ma=16385, Mb=1, states_a=None) == EINVAL             # an invalid call is invalid whatever its size
    assert call(Ma=16384, Mb=1, energy=None, terms=None) == ETOOLARGE and call(Ma=16384, Mb=1, wasserstein=None, cramer=None, ks=None) == ETOOLARGE
    assert call(R=1 << 30, d=4, scale=(1.0,) * 4) == ETOOLARGE       # R * d beyond a 32-bit grid
    assert call(R=1 << 27, Ma=16000, Mb=384, workspace_bytes=1 << 40) == ETOOLARGE  # R * workgroups of a plan likewise
    # successful no-ops: no rows (the arrays are empty, so nothing is needed and nothing overlaps)
    assert call(R=0) == 0 and call(R=0, Ma=16000, Mb=384, d=4, scale=(1.0,) * 4) == 0 and call(R=0, Ma=16000, Mb=385) == ETOOLARGE
    assert call(R=0, log_a_a=None, log_b_a=None, log_a_b=None, log_b_b=None) == 0
    assert call(R=0, workspace=None, workspace_bytes=0, Ma=4096, Mb=300) == 0
    assert call({"cramer": ("states_a", 0)}, R=0) == 0
    # the size queries
    W = _abi.pf_distance_workspace_bytes
    assert W(1, 512, 512, 3) == 0 and W(0, 513, 600, 3) == 0 and W(1, 0, 600, 3) == 0 and W(1, 513, 0, 3) == 0
    assert W(1, 513, 600, 2) == (2 + 2) * 3 * 8 and W(5, 37, 1025, 4) == 5 * (1 + 3) * 3 * 8 and W(2, 16000, 384, 1) == 2 * (32 + 1) * 3 * 8


def test_distance_workspace_refusals_on_the_host():
    """With ``Ma > 512`` the arrays no longer fit the 16-float host buffers, but every check below is decided on pointer
    values alone, before any HIP call."""
    from multimodalfilter_amd import _abi

    lib = sc.lib()
    R, Ma, Mb, d = 1, 513, 40, 1
    need = _abi.pf_distance_workspace_bytes(R, Ma, Mb, d)
    assert need == (2 + 1) * 3 * 8
    big = [(ctypes.c_float * (R * Ma * (d + 1) + 64))() for _ in _POINTERS]

    def call(**over):
        a = _abi.MmfPfDistanceArgs()
        for name, b in zip(_POINTERS, big):
            setattr(a, name, ctypes.cast(b, ctypes.c_void_p))
        a.R, a.Ma, a.Mb, a.d, a.workspace_bytes = R, Ma, Mb, d, need
        a.scale[0] = 1.0
        for k, v in over.items():
            setattr(a, k, v)
        a._keep = big
        return lib.mmf_pf_distance(ctypes.byref(a), None)

    base = ctypes.addressof(big[_POINTERS.index("workspace")])
    assert call(workspace=None) == EINVAL and call(workspace_bytes=need - 1) == EINVAL and call(workspace_bytes=0) == EINVAL
    assert call(workspace=ctypes.c_void_p(base + 4)) == EINVAL       # not 8-byte aligned
    for target in _INPUTS + _OUTPUTS:
        assert call(workspace=ctypes.cast(big[_POINTERS.index(target)], ctypes.c_void_p)) == EINVAL, target
    assert call(R=0) == 0
    # the pair kernel's workspace is not needed by the CDF outputs alone
    assert call(R=0, workspace=None, workspace_bytes=0, energy=None, terms=None) == 0


def test_lds_bytes_are_monotone_and_fit_a_cu():
    from multimodalfilter_amd import _abi

    L = _abi.pf_distance_lds_bytes
    sizes = [L(M - M // 3, M // 3) for M in range(3, 16385)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[0] == 64 * 8
    assert sizes[-1] == L(16000, 384) == (16384 + 256) * 8 <= 160 * 1024
    assert L(255, 257) == (512 + 64) * 8 and L(257, 256) == (1024 + 256) * 8      # one wave up to 512 slots, 256 threads beyond
    assert L(37, 300) == L(300, 37) == L(1, 336)                                   # a function of the union alone
    assert L(0, 5) == 0 and L(5, 0) == 0 and L(-1, -1) == 0 and L(16384, 16384) == sizes[-1]
    assert _abi.DISTANCE_MAX_M == 16384 == dc.MAX_UNION


def test_the_binding_refuses_cpu_tensors():
    import torch

    from multimodalfilter_amd import _abi

    x, y = torch.zeros((2, 4, 3)), torch.zeros((2, 5, 3))
    with pytest.raises(_abi.MmfError):
        _abi.pf_distance(x, None, None, y, None, None, wasserstein=torch.zeros((2, 3)), energy=torch.zeros((2,)))
    with pytest.raises(_abi.MmfError, match="scale"):
        _abi.pf_distance(x, None, None, y, None, None, energy=torch.zeros((2,)), scale=(1.0, 1.0))


# ------------------------------------------------------------------------------------------ 4. the Python refusals
def test_belief_distance_refusals_come_before_any_device_work():
    import torch

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, base

    pf = mmf.door_models.DoorParticleFilter().eval()
    assert pf.last_distance is None
    with pytest.raises(ValueError, match="^belief_distance needs a history: set record_history and run forward_loop"):
        pf.belief_distance()
    with pytest.raises(ValueError, match=r"^belief_distance\(of='smoothed'\) needs a smoothed record: call smooth"):
        pf.belief_distance(of="smoothed")
    with pytest.raises(ValueError, match="of must be"):
        pf.belief_distance(of="predicted")
    with pytest.raises(ValueError, match="other_of must be"):
        pf.belief_distance(other_of="predicted")
    with pytest.raises(ValueError, match="other must be a ParticleFilter"):
        pf.belief_distance(mmf.door_models.DoorKalmanFilter())
    with pytest.raises(TypeError):
        pf.belief_distance(pf, "filtered")  # of, other_of and scale are keyword-only

    made = sc.cpu_filter_with_history()
    f, (T, N, M, d) = made.f, made.dims
    g = sc.cpu_filter_with_history(M=9, seed=78).f
    before = (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores, g.last_history, g.last_smoothed)
    with pytest.raises(ValueError, match=r"^belief_distance\(of='smoothed'\) needs a smoothed record"):
        f.belief_distance(g, other_of="smoothed")  # the other side's refusal has the same text
    g.last_smoothed = base.belief_record(indices=torch.zeros((T, N), dtype=torch.int32), log_posterior=torch.zeros(N), lag=None,
                                         method="map")
    with pytest.raises(ValueError, match="not a\\s+distribution"):
        f.belief_distance(g, other_of="smoothed")
    g.last_smoothed = base.belief_record(covariance=torch.zeros((T, N, d, d)), unique=torch.zeros((T, N), dtype=torch.int32), lag=None)
    with pytest.raises(ValueError, match=r"belief_distance\(of='smoothed'\).*no per-step weights"):
        f.belief_distance(g, other_of="smoothed")
    g.last_smoothed = before[5]
    for shape in ((T + 1, N, 9, d), (T, N + 1, 9, d), (T, N, 9, d - 1)):
        other = sc.cpu_filter_with_history(*shape).f
        with pytest.raises(ValueError, match=rf"\(T, N, d\) = \({T}, {N}, {d}\).*\({shape[0]}, {shape[1]}, {shape[3]}\)"):
            f.belief_distance(other)
    for bad in ((), (1.0, 1.0), (1.0,) * 4, (1.0, 0.0, 1.0), (1.0, -2.0, 1.0), (1.0, math.nan, 1.0), (1.0, math.inf, 1.0),
                ("1", 1.0, 1.0), (True, 1.0, 1.0), 2.0):
        with pytest.raises(ValueError, match="scale"):
            f.belief_distance(g, scale=bad)
    big = base.history_record(states=torch.zeros((T, N, dc.MAX_UNION - M + 1, d)), log_likelihoods=torch.zeros((T, N, dc.MAX_UNION - M + 1)),
                              log_weights_in=None, ancestors=None, resampled=None, controls=None)
    g.last_history = big
    with pytest.raises(ValueError, match=rf"{M} \+ {dc.MAX_UNION - M + 1} particles.*16384"):
        f.belief_distance(g)
    g.last_history = before[4]
    assert f.last_distance is None and g.last_distance is None
    assert (f.last_history, f.last_smoothed, f.last_quantiles, f.last_scores, g.last_history, g.last_smoothed) == before
    # and with everything in order the call reaches the library, which refuses host memory: there is no torch fallback
    with pytest.raises(_abi.MmfError):
        f.belief_distance(g, scale=(0.5, 2.0, 1.0))
    with pytest.raises(_abi.MmfError):
        f.belief_distance()
    assert f.last_distance is None


def test_compare_filters_refuses_before_either_filter_runs():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    pf, other = mmf.door_models.DoorParticleFilter().eval(), mmf.door_models.DoorParticleFilter().eval()
    kf, lstm = mmf.door_models.DoorKalmanFilter().eval(), mmf.door_models.DoorLSTMFilter().eval()
    for a, b, name in ((kf, pf, "filter_a"), (pf, kf, "filter_b"), (lstm, pf, "filter_a"), (pf, lstm, "filter_b")):
        with pytest.raises(ValueError, match=rf"compare_filters: {name} must be a particle filter.*no particle set"):
            evaluation.compare_filters(a, b, {})  # (before the run: the trajectories are never read)
    with pytest.raises(ValueError, match="one object"):
        evaluation.compare_filters(pf, pf, {})
    for bad in ("ancestry", "map", "rts", "filtered", 3):
        with pytest.raises(ValueError, match="smooth_method must be None, 'marginal' or 'simulation'"):
            evaluation.compare_filters(pf, other, {}, smooth_method=bad)
    for method in (None, "marginal"):
        with pytest.raises(ValueError, match="smooth_draws"):
            evaluation.compare_filters(pf, other, {}, smooth_method=method, smooth_draws=8)
    for kw in (dict(return_belief=True), dict(return_scores=True), dict(smooth_lag=3), dict(no_such=1)):
        with pytest.raises(ValueError, match="run_filter_kwargs"):
            evaluation.compare_filters(pf, other, {}, **kw)
    for f in (pf, other):
        assert f.record_history is False and f.record_belief is False and f.last_distance is None and f.last_history is None
    sig = inspect.signature(evaluation.compare_filters).parameters
    assert list(sig) == ["filter_a", "filter_b", "traj", "smooth_method", "smooth_draws", "scale", "run_filter_kwargs"]
    assert sig["smooth_method"].default is None and sig["scale"].default is None
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("smooth_method", "smooth_draws", "scale"))


def test_distance_summary_against_hand_computed_values():
    import torch

    from multimodalfilter_amd import base, evaluation

    nan = math.nan
    w = torch.tensor([[[1.0, 2.0]], [[3.0, nan]], [[5.0, 6.0]]])  # (T = 3, N = 1, d = 2)
    c = torch.tensor([[[0.5, 1.0]], [[nan, nan]], [[1.5, 3.0]]])
    ks = torch.tensor([[[0.25, 0.5]], [[0.75, 1.0]], [[0.5, 0.0]]])
    energy = torch.tensor([[1.0], [nan], [4.0]])
    rec = base.belief_record(wasserstein=w, cramer=c, ks=ks, energy=energy, terms=torch.zeros((3, 1, 3)), of="filtered",
                             other_of="smoothed", scale=(1.0, 1.0), particles=(6, 9))
    got = evaluation.distance_summary(rec, start=0)
    assert set(got) == {"wasserstein", "cramer", "ks", "energy"}
    assert torch.equal(got["wasserstein"], torch.tensor([3.0, 4.0])) and torch.equal(got["cramer"], torch.tensor([1.0, 2.0]))
    assert torch.equal(got["ks"], torch.tensor([0.5, 0.5])) and got["energy"] == 2.5
    got = evaluation.distance_summary(rec, start=2)
    assert torch.equal(got["wasserstein"], torch.tensor([5.0, 6.0])) and got["energy"] == 4.0
    assert inspect.signature(evaluation.distance_summary).parameters["start"].default == evaluation.START_TRUNCATION
    with pytest.raises(ValueError, match="wasserstein"):
        evaluation.distance_summary(base.belief_record(energy=energy))
    with pytest.raises(ValueError, match="wasserstein"):
        evaluation.distance_summary(base.belief_record(crps=w))  # a score record is not a distance record


def test_run_filter_is_what_it_was():
    from multimodalfilter_amd import evaluation

    sig = inspect.signature(evaluation.run_filter).parameters
    assert list(sig) == ["filter_model", "traj", "initial_cov_scale", "measurement_initialize", "return_belief", "smooth_lag",
                         "smooth_method", "smooth_draws", "smooth_transition_moments", "return_innovations", "return_density",
                         "density_bandwidth", "return_modes", "modes_link_radius", "return_modalities", "return_quantiles",
                         "return_scores", "score_scale"]
    assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for name, p in sig.items() if name not in ("filter_model", "traj"))
    assert not any("distance" in name for name in sig)

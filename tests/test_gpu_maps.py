"""Belief maps on the GPU: ``mmf_pf_raster`` (``csrc/pf_raster.hip``) against the fp64 definition of ``tests/_raster_cases.py``
on its whole family, its bit-for-bit identities (two calls, a row alone, a translated set), a window far from every particle,
and ``ParticleFilter.belief_maps`` end to end on small real filters: the density of the predicted, filtered and smoothed sets,
the bandwidths of ``belief_density``, and the likelihood maps against the networks evaluated where the maps say they were.

The bar of a map: ``rel_err_elementwise(floor=1e-3) <= REL_TOL`` per row, every cell against max(its own value, 1e-3 of the
row's largest cell), NaN exactly on the rows where the definition puts it (``_raster_cases.map_err``); of a log-likelihood:
``|got - want| <= REL_TOL max(1, |want|)`` (``_density_cases.log_err``, the measure of ``test_gpu_modalities.py``).  Every
figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _raster_cases as rc
import _smooth_cases as sc
import _summary_gpu as sg
from _density_cases import log_err
from _summary_gpu import N, _filter_run, _same_bits
from _tol import REL_TOL

pytestmark = pytest.mark.gpu

OUTPUTS = ("density",)


def _run(case, want=OUTPUTS, rows=None):
    """``_abi.pf_raster`` on a case (or on ``rows`` of it) with the map between guard rows -> ``dict`` of device tensors."""
    from multimodalfilter_amd import _abi

    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    X, la, lb, c, h = (sc.to_device(pick(case[k])) for k in ("states", "log_a", "log_b", "center", "bandwidth"))
    R, M, d = X.shape
    Gx, Gy = case["cells"]

    def call(out):
        _abi.pf_raster(X, la, lb, c, h, out["density"], dims=case["dims"], step=case["step"])

    return sg.guarded_call(call, R, {"density": (Gy, Gx)}, want, OUTPUTS, f"M={M} d={d} R={R} cells={case['cells']}")


def _hold(case, ref, got, what):
    err = rc.map_err(N(got["density"]), ref, what)
    print(f"{what}: density {err:.3e} (bar {REL_TOL:.0e})")
    assert err <= REL_TOL, (what, err)
    return err


# ------------------------------------------------------------------------------------------ 1. the kernel against the definition
@pytest.mark.parametrize("M", rc.ALL_MS)
def test_kernel_holds_the_definition_on_the_family(M):
    """Guard rows intact (``guarded_call``); NaN exactly on the dead, NaN-centre and bad-bandwidth rows (``map_err``)."""
    cases, worst = 0, 0.0
    for case_id in rc.family():
        if case_id[0] != M:
            continue
        case, ref = rc.family_case(*case_id)
        got = _run(case)
        err = rc.map_err(N(got["density"]), ref, str(case_id))
        assert err <= REL_TOL, (case_id, err)
        nan = np.isnan(N(got["density"])).all((1, 2))
        assert nan.tolist() == rc.nan_rows(case).tolist(), case_id
        worst, cases = max(worst, err), cases + 1
    assert cases >= len(rc.VARIANTS)
    print(f"M={M}: density against fp64, worst over {cases} cases {worst:.3e} (bar {REL_TOL:.0e})")


def test_kernel_at_the_particle_limit():
    """Every wave stages 64 times; a 128 x 128 map is four workgroups."""
    case = rc.make_case(rc.MAX_M, 3, 1, "plain", (128, 128), (2, 0))
    _hold(case, rc.reference(case), _run(case), f"M={rc.MAX_M} 128 x 128")


# ------------------------------------------------------------------------------------------ 2. bit-for-bit identities
BIT_MS = [1, 65, 255, 257, 513, 4096]


@pytest.mark.parametrize("M", BIT_MS)
def test_two_calls_and_a_row_alone_give_the_same_bits(M):
    for d, variant, cells, dims in ((2, "plain", (33, 31), (1, 0)), (3, "dead_row", (128, 2), (2, 0)), (4, "nan_center", (65, 63), (3, 0)),
                                    (3, "bad_bandwidth", (128, 128), (0, 1))):
        case = rc.make_case(M, d, 3, variant, cells, dims)
        sg.assert_repeatable(_run, case, OUTPUTS, range(3), (M, d, variant, cells))


@pytest.mark.parametrize("M", [1, 65, 300, 1025])
def test_a_translated_set_has_the_same_bits(M):
    """States and centre on a dyadic lattice, shifted by 1024 along both map dimensions: the offsets from the centre are
    formed first and are exact either way, so the map does not know where the origin is."""
    rng = np.random.default_rng(M)
    for d, cells, dims in ((2, (33, 31), (1, 0)), (3, (64, 64), (2, 0)), (4, (128, 5), (1, 3))):
        X = (rng.integers(-256, 257, (3, M, d)) / 64.0).astype(np.float32)
        la = rng.standard_normal((3, M)).astype(np.float32)
        c = (rng.integers(-64, 65, (3, 2)) / 64.0).astype(np.float32)
        h = rng.uniform(0.3, 0.9, (3, 2)).astype(np.float32)
        case = dict(states=X, log_a=la, log_b=None, center=c, bandwidth=h, dims=dims, cells=cells, step=(0.11, 0.07))
        moved = dict(case, states=X.copy(), center=c + np.float32(1024.0))
        moved["states"][..., list(dims)] += np.float32(1024.0)
        assert ((moved["states"][..., list(dims)] - np.float32(1024.0)) == X[..., list(dims)]).all()  # (exact on the lattice)
        here, there = _run(case), _run(moved)
        assert _same_bits(here["density"], there["density"]), (M, d, cells)
        _hold(case, rc.reference(case), here, f"lattice M={M} d={d} cells={cells}")


def test_a_window_fifty_bandwidths_from_every_particle_is_finite_and_not_negative():
    rng = np.random.default_rng(50)
    for M, cells in ((1, (2, 2)), (65, (33, 31)), (1000, (128, 128))):
        X = rng.standard_normal((3, M, 3)).astype(np.float32)
        h = np.full((3, 2), 0.25, np.float32)
        reach = np.abs(X).max() + 50.0 * 0.25
        span = np.asarray(cells) * 0.05
        c = np.float32([[reach + span[0], 0.0], [0.0, -reach - span[1]], [reach + span[0], reach + span[1]]])
        case = dict(states=X, log_a=None, log_b=None, center=c, bandwidth=h, dims=(0, 2), cells=cells, step=(0.05, 0.05))
        got = N(_run(case)["density"])
        assert np.isfinite(got).all() and (got >= 0.0).all(), (M, cells)
        assert got.max() < 1e-30 and rc.reference(case).max() < 1e-200


# ------------------------------------------------------------------------------------------ 3. through the filter
def _record_case(states, log_a, log_b, rec):
    T, N_, M, d = states.shape
    case = sg._case_of(states, log_a, log_b, None, dims=rec.dims, cells=rec.cells, step=rec.step)
    del case["truth"]
    case.update(center=N(rec.center).reshape(T * N_, 2), bandwidth=N(rec.bandwidth).reshape(T * N_, 2))
    return case


def _hold_record(f, center, of, sets, what, **kw):
    """``belief_maps`` on a window of 24 of the smallest bandwidths around ``center`` against the definition on the record's own
    sets; the bandwidths are ``belief_density``'s bit for bit (the smoothed and filtered ones: ``"predicted"`` has none there)."""
    states, log_a, log_b = sets
    T, N_, M, d = states.shape
    kept = f.last_density
    f.belief_maps(center, (1.0, 1.0), of=of, **{**kw, "cells": 4})            # (for the bandwidths alone)
    span = tuple(float(24.0 * f.last_maps.bandwidth[..., k].min()) for k in range(2))
    density = f.belief_maps(center, span, of=of, **kw)
    torch.cuda.synchronize()
    rec = f.last_maps
    Gx, Gy = rec.cells
    assert rec.density is density and density.shape == (T, N_, Gy, Gx) and rec.of == of and f.last_density is kept
    assert set(vars(rec)) == {"density", "mass", "center", "step", "dims", "cells", "span", "bandwidth", "of", "rule"}
    assert rec.mass.shape == (T, N_) and rec.center.shape == rec.bandwidth.shape == (T, N_, 2) and rec.span == span
    assert rec.step == tuple(float(np.float32(s / g)) for s, g in zip(span, rec.cells))
    assert torch.equal(rec.center, center[..., list(rec.dims)])
    case = _record_case(states, log_a, log_b, rec)
    ref = rc.reference(case)
    assert (N(rec.bandwidth) >= np.asarray(span, np.float32) / 64).all() and (ref.max((1, 2)) >= 1e-30).all(), what
    assert (N(rec.bandwidth) >= 1e4 * np.spacing(np.abs(N(rec.center)))).all(), what  # (the reference's cell centres are fp32)
    err = rc.map_err(N(density).reshape(T * N_, Gy, Gx), ref, what)
    mass = ref.sum((1, 2)) * rec.step[0] * rec.step[1]
    e_mass = float(np.abs(N(rec.mass).reshape(-1) - mass).max())
    print(f"{what}: density {err:.3e} (bar {REL_TOL:.0e}), mass {mass.min():.3f} .. {mass.max():.3f} off by {e_mass:.2e}")
    assert err <= REL_TOL and e_mass <= REL_TOL
    if of != "predicted":
        f.belief_density(of=of, **{k: v for k, v in kw.items() if k in ("bandwidth", "min_bandwidth")})
        assert _same_bits(rec.bandwidth, f.last_density.bandwidth[..., list(rec.dims)].contiguous()), what
        f.last_density = kept
    return rec


def _grid_of(rec, center):
    """The grid states of a record's likelihood maps: ``dims`` at the cell centres, every other dimension at ``center``'s."""
    from multimodalfilter_amd import evaluation

    T, N_, d = center.shape
    Gx, Gy = rec.cells
    x, y = evaluation.map_axes(rec)
    g = center[:, :, None, None, :].repeat(1, 1, Gy, Gx, 1)
    g[..., rec.dims[0]] = x[:, :, None, :]
    g[..., rec.dims[1]] = y[:, :, :, None]
    return g.reshape(T * N_, Gy * Gx, d)


@pytest.mark.parametrize("M", [64, 300])
def test_belief_maps_on_the_door_crossmodal_filter(M):
    from multimodalfilter_amd import evaluation
    from multimodalfilter_amd.utils import ReplayNoise

    f, forward, traj, (T, N_, _, d) = _filter_run("DoorCrossmodalParticleFilter", M, owner="maps")
    est = forward().clone()
    h = f.last_history
    before = {k: getattr(h, k).clone() for k in ("states", "log_likelihoods", "log_weights_in", "ancestors") if getattr(h, k) is not None}
    f.belief_density()
    f.belief_modalities()
    others = ("last_smoothed", "last_quantiles", "last_scores", "last_density", "last_modes", "last_modalities", "last_distance",
              "last_forecast", "last_belief")
    kept = {k: getattr(f, k) for k in others}
    f.last_maps = None
    _hold_record(f, est, "filtered", (h.states, h.log_weights_in, h.log_likelihoods), f"door M={M} filtered", dims=(2, 0), cells=(33, 31))
    _hold_record(f, est, "predicted", (h.states, h.log_weights_in, None), f"door M={M} predicted", dims=(0, 1))
    _hold_record(f, traj["states"][1:], "filtered", (h.states, h.log_weights_in, h.log_likelihoods), f"door M={M} filtered, scott",
                 bandwidth="scott", min_bandwidth=(1e-3, 1e-4, 1e-5), dims=(1, 2), cells=(128, 65))

    # likelihood maps: an odd grid centred on a recorded particle, so the middle cell IS that particle
    p = (h.log_weights_in + h.log_likelihoods).argmax(dim=-1)                        # a live particle of every set
    at = torch.gather(h.states, 2, p[..., None, None].expand(T, N_, 1, d))[:, :, 0].contiguous()
    Gx, Gy, dims = 5, 7, (2, 0)
    f.belief_maps(at, (0.2, 0.1), dims=dims, cells=(Gx, Gy), likelihoods=True)
    torch.cuda.synchronize()
    rec, mod = f.last_maps, f.last_modalities
    K = 2
    assert set(vars(rec)) >= {"log_likelihood", "modalities", "log_weights"} and rec.modalities == mod.modalities == (0, 1)
    assert rec.log_likelihood.shape == (T, N_, K + 1, Gy, Gx) and _same_bits(rec.log_weights, mod.log_weights)
    x, y = (N(a) for a in evaluation.map_axes(rec))
    assert (x[..., Gx // 2] == N(at)[..., dims[0]]).all() and (y[..., Gy // 2] == N(at)[..., dims[1]]).all()
    middle = N(rec.log_likelihood[:, :, :K, Gy // 2, Gx // 2]).astype(np.float64)      # (T, N, K)
    own = N(torch.gather(mod.log_likelihoods, 3, p[None, ..., None].expand(K, T, N_, 1))[..., 0]).astype(np.float64)
    e_mid = log_err(middle, own.transpose(1, 2, 0), "the middle cell against the particle's own l_k")
    flat = {k: v.reshape((T * N_,) + tuple(v.shape[2:])) for k, v in h.observations.items()}
    fused = f.measurement_model(states=_grid_of(rec, at), observations=flat)
    e_fused = log_err(N(rec.log_likelihood[:, :, K]).reshape(T * N_, Gy * Gx).astype(np.float64), N(fused).astype(np.float64),
                      "the fused map against the measurement model on the grid")
    print(f"door M={M}: middle cell against belief_modalities {e_mid:.3e}, fused map against the model {e_fused:.3e} (bar {REL_TOL:.0e})")
    assert e_mid <= REL_TOL and e_fused <= REL_TOL
    summary = evaluation.map_summary(rec, traj["states"][1:], start=0)
    assert set(summary) == {"mass", "peak_error", "agreement"} and summary["agreement"].shape == (K + 1,)
    assert 0.0 <= summary["mass"] < float("inf")  # (a Riemann sum: with cells wider than a bandwidth it can exceed 1)
    assert bool(((summary["agreement"] >= 0) & (summary["agreement"] <= 1 + 1e-6)).all())

    # nothing else moved: the history, every other record, the estimates and the noise stream
    assert f.last_history is h and all(getattr(f, k) is v for k, v in kept.items())
    for k, v in before.items():
        assert torch.equal(getattr(h, k), v), k
    after = f.noise.uniform((4, 5), like=h.states).clone()  # where the noise stream stands after the calls ...
    assert torch.equal(forward(), est)
    assert torch.equal(f.noise.uniform((4, 5), like=h.states), after)  # ... is where it stands without them
    f.last_history = h

    # smoothed: the marginal smoother's weights over the history's states, then 16 equally weighted draws per step
    mean = f.smooth(method="marginal").clone()
    s = f.last_smoothed
    weights = s.weights.clone()
    _hold_record(f, mean, "smoothed", (h.states, torch.log(weights), None), f"door M={M} marginal", dims=(0, 2), cells=(63, 65))
    assert f.last_smoothed is s and torch.equal(s.weights, weights)
    S = 16
    f.noise = ReplayNoise(uniforms=[torch.rand((T, N_, S), generator=torch.Generator().manual_seed(5))])
    f.smooth(method="simulation", num_draws=S)
    s = f.last_smoothed
    _hold_record(f, s.trajectories[:, :, 0].contiguous(), "smoothed", (s.trajectories, None, None), f"door M={M} simulation",
                 dims=(1, 0), cells=32)
    assert f.last_smoothed is s and f.last_history is h
    for k, v in before.items():
        assert torch.equal(getattr(h, k), v), k
    for method in ("ancestry", "map"):
        f.smooth(method=method)
        maps = f.last_maps
        with pytest.raises(ValueError, match="of='smoothed'"):
            f.belief_maps(est, (1.0, 1.0), of="smoothed")
        assert f.last_maps is maps


def test_belief_maps_on_the_push_filter():
    """``d = 2`` and a measurement model that fuses nothing: one likelihood map, from the observations it is handed."""
    from multimodalfilter_amd.utils import ReplayNoise

    f, forward, traj, (T, N_, M, d) = _filter_run("PushParticleFilter", 64, owner="maps")
    est = forward().clone()
    h = f.last_history
    assert d == 2 and getattr(h, "observations", None) is None
    _hold_record(f, est, "filtered", (h.states, h.log_weights_in, h.log_likelihoods), "push filtered", dims=(1, 0), cells=(65, 63))
    _hold_record(f, est, "predicted", (h.states, h.log_weights_in, None), "push predicted", cells=(2, 128))
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    p = (h.log_weights_in + h.log_likelihoods).argmax(dim=-1)
    at = torch.gather(h.states, 2, p[..., None, None].expand(T, N_, 1, d))[:, :, 0].contiguous()
    with pytest.raises(ValueError, match="pass observations="):
        f.belief_maps(at, (0.2, 0.2), cells=(7, 5), likelihoods=True)
    f.belief_maps(at, (0.2, 0.2), cells=(7, 5), likelihoods=True, observations=obs)
    torch.cuda.synchronize()
    rec = f.last_maps
    assert rec.log_likelihood.shape == (T, N_, 1, 5, 7) and rec.modalities == (0,) and rec.log_weights is None
    own = N(torch.gather(h.log_likelihoods, 2, p[..., None])[..., 0]).astype(np.float64)
    e_mid = log_err(N(rec.log_likelihood[:, :, 0, 2, 3]).astype(np.float64), own, "the middle cell against the particle's own l")
    flat = {k: v.reshape((T * N_,) + tuple(v.shape[2:])) for k, v in obs.items()}
    whole = f.measurement_model(states=_grid_of(rec, at), observations=flat)
    e_map = log_err(N(rec.log_likelihood[:, :, 0]).reshape(T * N_, 35).astype(np.float64), N(whole).astype(np.float64), "the map")
    print(f"push: middle cell against the history's log-likelihood {e_mid:.3e}, map against the model {e_map:.3e} (bar {REL_TOL:.0e})")
    assert e_mid <= REL_TOL and e_map <= REL_TOL
    assert torch.equal(forward(), est)
    h = f.last_history
    mean = f.smooth(method="marginal").clone()
    _hold_record(f, mean, "smoothed", (h.states, torch.log(f.last_smoothed.weights), None), "push marginal", cells=(31, 33))
    S = 16
    f.noise = ReplayNoise(uniforms=[torch.rand((T, N_, S), generator=torch.Generator().manual_seed(5))])
    f.smooth(method="simulation", num_draws=S)
    s = f.last_smoothed
    # (16 draws can agree in a dimension, where the rule of thumb gives its floor, and the fp32 cell centres of the reference
    # are half an ulp of the coordinate off: that is 6e-8 / h of a bandwidth, times |t| <= 3.7 in the exponent of a cell that
    # counts.  A floor of 0.05 keeps it near 5e-6)
    _hold_record(f, s.trajectories[:, :, 0].contiguous(), "smoothed", (s.trajectories, None, None), "push simulation", dims=(1, 0),
                 min_bandwidth=5e-2)

"""Particle-posterior distances on the GPU: ``mmf_pf_distance`` (``csrc/pf_distance.hip``) against the fp64 definition of
``tests/_distance_cases.py`` on its whole family, at the particle limit, its bit-for-bit identities (two calls, a row pair
alone, any subset of the outputs, a set against itself, a permutation), its symmetry, near-identical sets, dead particles, and
``ParticleFilter.belief_distance`` / ``evaluation.compare_filters`` end to end on small real filters.

The bar: ``_tol.rel_err(got, fp64) < max(REL_TOL, 3 x the fp32 yardstick's own error)`` on every output, with NaN exactly
where the definition puts it.  Every figure is printed before it is asserted."""
import numpy as np
import pytest
import torch

import _distance_cases as dc
import _smooth_cases as sc
from _summary_gpu import N, _filter_run, _same_bits, assert_repeatable, assert_subsets_match_full, guarded_call
from _tol import REL_TOL

pytestmark = pytest.mark.gpu

OUTPUTS = dc.OUTPUTS
CDF = dc.CDF_OUTPUTS


def _run(case, want=OUTPUTS, rows=None):
    """``_abi.pf_distance`` on a case (or on ``rows`` of it) with every output between guard rows; the outputs not in ``want``
    are handed over as null and their buffers must come back untouched -> ``dict`` of device tensors (``None`` for those)."""
    from multimodalfilter_amd import _abi

    pick = (lambda x: x) if rows is None else (lambda x: None if x is None else x[rows])
    a, b = ([sc.to_device(pick(side[k])) for k in ("states", "log_a", "log_b")] for side in (case["a"], case["b"]))
    R, Ma, d = a[0].shape
    Mb = b[0].shape[1]
    tails = {"wasserstein": (d,), "cramer": (d,), "ks": (d,), "energy": (), "terms": (3,)}
    return guarded_call(lambda out: _abi.pf_distance(*a, *b, scale=case["scale"], **out), R, tails, want, OUTPUTS,
                        f"Ma={Ma} Mb={Mb} d={d} R={R}")


def _hold(ref, yard, got, what, outputs=OUTPUTS):
    """The outputs against the reference at the house rule; returns the errors."""
    errs = {k: dc.compare(N(got[k]), ref[k], f"{what} {k}") for k in outputs}
    bars = {k: dc.bar(yard[k]) for k in outputs}
    print(f"{what}: " + ", ".join(f"{k} {errs[k]:.3e} (bar {bars[k]:.1e})" for k in outputs))
    for k in outputs:
        assert errs[k] < bars[k], (what, k, errs[k], bars[k])
    return errs


def _with_yardstick(case, outputs=OUTPUTS):
    ref = dc.reference(case, outputs=outputs)
    yard = dc.reference(case, np.float32, outputs=outputs)
    return ref, {k: dc.compare(yard[k], ref[k], k) for k in outputs}


# ------------------------------------------------------------------------------------------ 1. the kernels against the definition
@pytest.mark.parametrize("Ma,Mb", dc.PAIRS)
def test_kernels_hold_the_definition_on_the_family(Ma, Mb):
    for key in dc.family():
        if key[:2] != (Ma, Mb):
            continue
        case, ref, yard = dc.family_case(*key)
        _hold(ref, yard, _run(case), f"Ma={Ma} Mb={Mb} d={key[2]} R={key[3]} {dc.VARIANTS[key[4]]}")


def test_cdf_kernel_at_the_particle_limit():
    """``Ma + Mb = 16384``: 256 threads with 64 slots each, 130 KiB of LDS.  Only the CDF outputs are asked for (their
    reference is ``O(M log M)``); the pair kernel is skipped by its null outputs, whose buffers ``_run`` finds untouched."""
    Ma, Mb, d = 16000, 384, 3
    assert Ma + Mb == dc.MAX_UNION
    case = dc.make_case(Ma, Mb, d, 1)
    ref, yard = _with_yardstick(case, CDF)
    got = _run(case, CDF)
    assert got["energy"] is None and got["terms"] is None
    _hold(ref, yard, got, f"Ma={Ma} Mb={Mb} d={d}", CDF)


PLAN_PAIRS = ((100, 100), (2000, 49), (4000, 97))  # unions of 200, 2049 and 4097 slots


@pytest.mark.parametrize("Ma,Mb", PLAN_PAIRS)
def test_cdf_kernel_on_the_plans_between_the_family_and_the_limit(Ma, Mb):
    """The smallest unions that the sort plan gives ``<64, 4>`` (129 .. 256 slots), ``<256, 16>`` (2049 .. 4096) and
    ``<256, 32>`` (4097 .. 8192), which no pair of the family reaches.  Only the CDF outputs are asked for, as at the limit."""
    d = 3
    case = dc.make_case(Ma, Mb, d, 1)
    ref, yard = _with_yardstick(case, CDF)
    got = _run(case, CDF)
    assert got["energy"] is None and got["terms"] is None
    _hold(ref, yard, got, f"Ma={Ma} Mb={Mb} d={d}", CDF)


# ------------------------------------------------------------------------------------------ 2. bit-for-bit identities
# (the last three: the smallest unions of the CDF kernel's <64, 4>, <256, 16> and <256, 32>)
@pytest.mark.parametrize("Ma,Mb", [(1, 37), (64, 64), (255, 257), (257, 256), (513, 600), (300, 1025)] + list(PLAN_PAIRS))
def test_two_calls_and_a_row_pair_alone_give_the_same_bits(Ma, Mb):
    for d, v in ((1, 0), (3, 6), (4, 8)):
        assert_repeatable(_run, dc.make_case(Ma, Mb, d, 5, v), OUTPUTS, (0, 2, 4), (Ma, Mb, d, v))


@pytest.mark.parametrize("Ma,Mb", [(37, 300), (513, 600)])
def test_every_subset_of_the_outputs_writes_only_what_was_asked_for(Ma, Mb):
    """All 30 proper non-empty subsets: what is written has the bits of the full call (the untouched buffers are checked
    inside ``_run``), whichever of the two kernels the subset leaves out."""
    assert_subsets_match_full(_run, dc.make_case(Ma, Mb, 3, 3, 0), OUTPUTS, what=(Ma, Mb))


@pytest.mark.parametrize("M", [37, 600])
def test_a_set_against_itself_is_exactly_zero(M):
    """The same arrays as A and as B: every CDF difference is an integer zero, and the three expectations of the energy
    distance are one device function with one dealing, so ``2 t - t - t`` is exactly 0."""
    for d, v in ((1, 0), (3, 0), (4, 8), (2, 3)):
        case = dc.make_case(M, M, d, 3, v)
        case = dict(case, b=case["a"])
        got = _run(case)
        for k in ("wasserstein", "cramer", "ks", "energy"):
            assert bool((got[k] == 0).all()), (M, d, v, k, N(got[k]))
        t = got["terms"]
        assert _same_bits(t[:, 0], t[:, 1]) and _same_bits(t[:, 0], t[:, 2]) and bool((t > 0).all())


@pytest.mark.parametrize("Ma,Mb", [(37, 300), (513, 600)])
def test_a_permutation_of_one_set_leaves_the_cdf_outputs_bit_for_bit(Ma, Mb):
    rng = np.random.default_rng(5)
    for d, v in ((2, 0), (3, 4)):
        case = dc.make_case(Ma, Mb, d, 3, v)
        perm = rng.permutation(Mb)
        moved = dict(case, b={k: (None if x is None else np.ascontiguousarray(x[:, perm])) for k, x in case["b"].items()})
        got, other = _run(case), _run(moved)
        for k in CDF:
            assert _same_bits(got[k], other[k]), (Ma, Mb, d, v, k)
        for k in ("energy", "terms"):
            e = dc.compare(N(other[k]), N(got[k]).astype(np.float64), k)
            print(f"Ma={Ma} Mb={Mb} d={d}: {k} under a permutation of B {e:.3e}")
            assert e < REL_TOL, (Ma, Mb, d, v, k, e)


# ------------------------------------------------------------------------------------------ 3. symmetry
@pytest.mark.parametrize("Ma,Mb", [(1, 37), (37, 300), (257, 256), (513, 600), (1025, 64)])
def test_the_distance_is_symmetric(Ma, Mb):
    for d, v in ((1, 0), (3, 0), (4, 8), (2, 4)):
        case = dc.make_case(Ma, Mb, d, 3, v)
        ab, ba = _run(case), _run(dc.swapped(case))
        ba["terms"] = ba["terms"][:, [0, 2, 1]]
        errs = {k: dc.compare(N(ba[k]), N(ab[k]).astype(np.float64), k) for k in OUTPUTS}
        print(f"Ma={Ma} Mb={Mb} d={d} {dc.VARIANTS[v]}: d(B, A) against d(A, B) " + ", ".join(f"{k} {e:.3e}" for k, e in errs.items()))
        for k, e in errs.items():
            assert e < REL_TOL, (Ma, Mb, d, v, k, e)
        for k in CDF:  # (|D| and D^2 do not see the sign, and the sort of the union does not see the roles)
            assert _same_bits(ab[k], ba[k]), (Ma, Mb, d, v, k)


# ------------------------------------------------------------------------------------------ 4. near-identical sets
def test_near_identical_sets_are_resolved_by_the_cdf_outputs():
    """``B = A + c`` under A's weights, ``|c|_2 = 1e-3`` beside a spread of order 1.  ``wasserstein[k]`` is ``|c_k|``,
    ``cramer``, ``ks`` and ``terms`` meet the bar against fp64.  ``energy`` does NOT, and is not asked to: ``energy^2 = 2 t0 -
    t1 - t2`` is a difference of three sums of order 1 that agree to 1e-3 and are each good to about 1e-7 (the fp32 pair
    terms), so the difference is good to about 1e-4 of itself at best and the fp32 yardstick itself is 4e-4 away from fp64
    here.  What holds of a cancelling difference is its range: ``terms[0] <= terms[1] + |c|_2`` by the triangle inequality
    (``|x - (x' + c)| <= |x - x'| + |c|``) and ``terms[2] = terms[1]``, hence ``0 <= energy <= sqrt(2 |c|_2)``; the factor
    ``1 + 1e-3`` leaves room for the rounding of the bound itself."""
    M, d = 300, 3
    case = dc.make_case(M, M, d, 3, 0)
    c = np.asarray([6e-4, -6.4e-4, 4.8e-4], np.float32)
    norm = float(np.sqrt((c.astype(np.float64) ** 2).sum()))
    assert abs(norm - 1e-3) < 1e-9
    case = dict(case, b=dict(case["a"], states=case["a"]["states"] + c))
    ref, yard = _with_yardstick(case)
    got = _run(case)
    _hold(ref, yard, got, f"near-identical M={M} d={d}", CDF + ("terms",))
    shift = np.broadcast_to(np.abs(c.astype(np.float64)), (3, d))
    e = dc.compare(N(got["wasserstein"]), shift, "wasserstein against |c|")
    energy = N(got["energy"]).astype(np.float64)
    print(f"wasserstein against |c_k| {e:.3e}; energy {energy} (fp64 {ref['energy']}, bound {np.sqrt(2 * norm):.6f})")
    assert e < REL_TOL
    assert bool((energy >= 0).all()) and bool((energy <= np.sqrt(2.0 * norm) * (1.0 + 1e-3)).all())


# ------------------------------------------------------------------------------------------ 5. dead particles
@pytest.mark.parametrize("Ma,Mb", [(37, 300), (513, 600)])
def test_dead_particles_change_nothing(Ma, Mb):
    """NaN state rows at ``-inf`` weights scattered into both sets against the same sets without them: the CDF outputs bit
    for bit (a dead particle takes the padding's key), the pair outputs within the bar (the dealing moves)."""
    rng = np.random.default_rng(9)
    d, R = 3, 3
    lean = dc.make_case(Ma, Mb, d, R, 1)  # (uniform, plain): no dead particle in A; B's own stay on both sides
    fat = {"scale": None}
    for name, extra in (("a", 11), ("b", 70)):
        side = lean[name]
        M = side["states"].shape[1]
        X = np.full((R, M + extra, d), np.nan, np.float32)
        la = np.full((R, M + extra), -np.inf, np.float32)
        lb = np.zeros((R, M + extra), np.float32)
        for r in range(R):
            keep = np.sort(rng.choice(M + extra, M, replace=False))
            X[r, keep] = side["states"][r]
            la[r, keep] = 0.0 if side["log_a"] is None else side["log_a"][r]
            lb[r, keep] = 0.0 if side["log_b"] is None else side["log_b"][r]
        fat[name] = dict(states=X, log_a=la, log_b=lb)
    got, other = _run(lean), _run(fat)
    for k in CDF:
        assert _same_bits(got[k], other[k]), (Ma, Mb, k)
    for k in ("energy", "terms"):
        e = dc.compare(N(other[k]), N(got[k]).astype(np.float64), k)
        print(f"Ma={Ma} Mb={Mb}: {k} with dead particles scattered in {e:.3e}")
        assert e < REL_TOL, (Ma, Mb, k, e)
    assert bool(torch.isfinite(other["terms"]).all())


# ------------------------------------------------------------------------------------------ 6. through the filters
T_, N_ = 12, 5


def _side(states, log_a, log_b):
    T, n, M, d = states.shape
    flat = lambda x, tail: None if x is None else x.detach().cpu().numpy().reshape((T * n,) + tail)
    return dict(states=flat(states, (M, d)), log_a=flat(log_a, (M,)), log_b=flat(log_b, (M,)))


def _hold_record(rec, a, b, what, scale=None, rows=None):
    """A distance record against the definition on the two sides' own arrays.  ``wasserstein``, ``cramer``, ``ks`` and
    ``terms`` at the bar.  ``energy`` at the bar on the steps that keep the family's margin (``2 t0 - t1 - t2 >= 0.1 (t1 +
    t2) / 2``); on every step ``energy^2`` to the resolution of a difference of three sums that are each good to the bar:
    ``|energy^2 - fp64| <= bar (2 t0 + t1 + t2)`` -- recorded sets can be as close as they like (a smoothed set is the
    filtered one at the last step), and there a relative error of the difference means nothing.  ``rows``: the row pairs
    (of the ``T N``) that are held, all of them by default."""
    rows = slice(None) if rows is None else rows
    cut = lambda side: {k: (None if x is None else x[rows]) for k, x in side.items()}
    case = dict(a=cut(a), b=cut(b), scale=scale)
    ref, yard = _with_yardstick(case, CDF + ("terms", "energy"))
    R, d = ref["wasserstein"].shape
    got = {k: getattr(rec, k).reshape((-1,) + ref[k].shape[1:])[rows] for k in OUTPUTS}
    _hold(ref, yard, got, what, CDF + ("terms",))
    t, energy = ref["terms"], N(got["energy"]).astype(np.float64)
    assert bool((np.isnan(energy) == np.isnan(ref["energy"])).all())
    ok = ~np.isnan(ref["energy"])
    total = 2 * t[ok, 0] + t[ok, 1] + t[ok, 2]
    gap = np.abs(energy[ok] ** 2 - ref["energy"][ok] ** 2) / total
    print(f"{what}: energy^2 against fp64, worst {gap.max():.3e} of 2 t0 + t1 + t2 (bar {dc.bar(yard['terms']):.1e})")
    assert bool((gap < dc.bar(yard["terms"])).all())
    wide = ok & (np.nan_to_num(ref["energy"]) ** 2 >= dc.ENERGY_MARGIN * 0.5 * (t[:, 1] + t[:, 2]))
    if wide.any():
        e = dc.compare(energy[wide], ref["energy"][wide], "energy")
        print(f"{what}: energy on the {int(wide.sum())} of {R} steps with the margin {e:.3e}")
        assert e < dc.bar(yard["terms"])
    return ref


def _two_filters():
    fa, run_a, traj, shape_a = _filter_run("DoorCrossmodalParticleFilter", 64, N_, T_, owner="distance a")
    fb, run_b, _, shape_b = _filter_run("DoorCrossmodalParticleFilter", 100, N_, T_, owner="distance b")
    assert fa is not fb and shape_a == (T_, N_, 64, 3) and shape_b == (T_, N_, 100, 3)
    return fa, run_a, fb, run_b, traj


def test_belief_distance_between_two_real_filters():
    """64 particles against 100 on the same trajectories: the record equals the definition on the two histories; nothing
    else moves on either filter, and no noise is drawn."""
    fa, run_a, fb, run_b, traj = _two_filters()
    est_a, est_b = run_a().clone(), run_b().clone()
    ha, hb = fa.last_history, fb.last_history
    fa.belief_quantiles((0.5,))
    kept = (fa.last_quantiles, fa.last_scores, fa.last_smoothed, fb.last_quantiles, fb.last_smoothed)
    fa.last_distance = fb.last_distance = None
    w = fa.belief_distance(fb)
    rec = fa.last_distance
    assert fb.last_distance is None and rec.wasserstein is w
    assert set(vars(rec)) == {"wasserstein", "cramer", "ks", "energy", "terms", "of", "other_of", "scale", "particles"}
    assert (rec.of, rec.other_of, rec.scale, rec.particles) == ("filtered", "filtered", (1.0, 1.0, 1.0), (64, 100))
    assert w.shape == rec.cramer.shape == rec.ks.shape == (T_, N_, 3) and rec.energy.shape == (T_, N_) and rec.terms.shape == (T_, N_, 3)
    a = _side(ha.states, ha.log_weights_in, ha.log_likelihoods)
    b = _side(hb.states, hb.log_weights_in, hb.log_likelihoods)
    _hold_record(rec, a, b, "64 against 100, filtered")
    assert bool(torch.isfinite(w).all()) and bool((rec.ks >= 0).all()) and bool((rec.ks <= 1).all()) and bool((rec.energy >= 0).all())
    scale = (0.5, 2.0, 4.0)
    again = fa.belief_distance(fb, scale=scale)
    assert fa.last_distance.scale == scale and torch.equal(again, w) and torch.equal(fa.last_distance.cramer, rec.cramer)
    assert not torch.equal(fa.last_distance.energy, rec.energy)
    _hold_record(fa.last_distance, a, b, "64 against 100, scaled", scale)
    # the other way round: the roles swapped, the same distance
    fb.belief_distance(fa)
    assert fb.last_distance.particles == (100, 64) and torch.equal(fb.last_distance.wasserstein, w)
    # a filter against itself
    fa.belief_distance()
    zero = fa.last_distance
    assert all(bool((getattr(zero, k) == 0).all()) for k in ("wasserstein", "cramer", "ks", "energy")) and zero.particles == (64, 64)
    assert (fa.last_quantiles, fa.last_scores, fa.last_smoothed, fb.last_quantiles, fb.last_smoothed) == kept
    assert fa.last_history is ha and fb.last_history is hb
    after = fa.noise.uniform((4, 5), like=ha.states).clone()  # where the noise stream stands after the calls ...
    assert torch.equal(run_a(), est_a) and torch.equal(run_b(), est_b)
    assert torch.equal(fa.noise.uniform((4, 5), like=ha.states), after)  # ... is where it stands without them


def test_belief_distance_of_the_filtered_against_the_smoothed_sets():
    """How far the future moved the belief: ``of="filtered"`` against ``other_of="smoothed"`` after the marginal smoother
    (the history's states under the smoothed weights) and after backward simulation (16 drawn paths, equally weighted)."""
    from multimodalfilter_amd.utils import ReplayNoise

    f, run, traj, (T, n, M, d) = _filter_run("DoorCrossmodalParticleFilter", 64, N_, T_, owner="distance a")
    run()
    h = f.last_history
    a = _side(h.states, h.log_weights_in, h.log_likelihoods)
    mean = f.smooth(method="marginal").clone()
    s = f.last_smoothed
    weights = s.weights.clone()
    f.belief_distance(of="filtered", other_of="smoothed")
    rec = f.last_distance
    assert (rec.of, rec.other_of, rec.particles) == ("filtered", "smoothed", (M, M))
    assert f.last_smoothed is s and torch.equal(s.weights, weights) and f.last_history is h
    # the marginal smoother's last step IS the filter's: one distribution, told apart only by the rounding of log(weights) --
    # up to 2^-24 x 88 = 5e-6 of a weight, once for the smoother's normalisation and once for the logarithm, so no CDF value
    # moves by more than 1.1e-5.  Differences of that kind are rounding noise on either side of the comparison with fp64
    # (the reference's exp is not the device's to the ulp), so the last step is held to that bound and the steps before it
    # to the definition
    _hold_record(rec, a, _side(h.states, torch.log(weights), None), "filtered against marginal-smoothed", rows=slice(0, (T - 1) * n))
    print(f"last step: ks {float(rec.ks[-1].max()):.3e}, wasserstein {float(rec.wasserstein[-1].max()):.3e}; step 0: ks {float(rec.ks[0].max()):.3e}")
    assert float(rec.ks[-1].max()) < 2e-5 and bool(torch.isfinite(rec.energy[-1]).all()) and float(rec.ks[0].max()) > 1e-3
    f.belief_distance(of="smoothed", other_of="filtered")
    assert torch.equal(f.last_distance.wasserstein, rec.wasserstein) and f.last_distance.of == "smoothed"
    assert torch.equal(f.smooth(method="marginal"), mean)

    S = 16
    f.noise = ReplayNoise(uniforms=[torch.rand((T, n, S), generator=torch.Generator().manual_seed(5))])
    f.smooth(method="simulation", num_draws=S)
    s = f.last_smoothed
    f.belief_distance(of="filtered", other_of="smoothed")
    assert f.last_distance.particles == (M, S) and f.last_smoothed is s
    _hold_record(f.last_distance, a, _side(s.trajectories, None, None), "filtered against backward simulation")
    for method in ("ancestry", "map"):
        f.smooth(method=method)
        kept = f.last_distance
        with pytest.raises(ValueError, match="of='smoothed'"):
            f.belief_distance(other_of="smoothed")
        assert f.last_distance is kept


def test_compare_filters_is_the_two_runs_and_the_one_call():
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation

    fa, _, fb, _, traj = _two_filters()
    seed = lambda: (setattr(fa, "noise", mmf.NoiseSource(7)), setattr(fb, "noise", mmf.NoiseSource(8)))
    seed()
    fa.record_history = fb.record_history = False
    plain_a, plain_b = evaluation.run_filter(fa, traj).clone(), evaluation.run_filter(fb, traj).clone()
    seed()
    est_a, est_b, rec = evaluation.compare_filters(fa, fb, traj)
    assert torch.equal(est_a, plain_a) and torch.equal(est_b, plain_b) and rec is fa.last_distance
    assert fa.record_history is False and fb.record_history is False and fa.record_belief is False and fb.record_belief is False
    assert (rec.of, rec.other_of, rec.particles) == ("filtered", "filtered", (64, 100))
    ha, hb = fa.last_history, fb.last_history
    _hold_record(rec, _side(ha.states, ha.log_weights_in, ha.log_likelihoods), _side(hb.states, hb.log_weights_in, hb.log_likelihoods),
                 "compare_filters")
    fa.belief_distance(fb)  # the separate call on what the two runs left
    for k in OUTPUTS:
        assert torch.equal(getattr(fa.last_distance, k), getattr(rec, k)), k
    summary = evaluation.distance_summary(rec, start=2)
    assert set(summary) == {"wasserstein", "cramer", "ks", "energy"} and summary["wasserstein"].shape == (3,)
    assert torch.allclose(summary["cramer"], rec.cramer[2:].double().mean((0, 1)).float(), rtol=1e-6) and summary["energy"] > 0
    # history switched on by the caller stays on
    fa.record_history = True
    seed()
    evaluation.compare_filters(fa, fb, traj, scale=(0.5, 2.0, 4.0))
    assert fa.record_history is True and fb.record_history is False and fa.last_distance.scale == (0.5, 2.0, 4.0)
    fa.record_history = False
    # smoothed against smoothed
    seed()
    sm_a, sm_b, srec = evaluation.compare_filters(fa, fb, traj, smooth_method="marginal")
    assert (srec.of, srec.other_of) == ("smoothed", "smoothed") and fa.last_smoothed.method == "marginal" == fb.last_smoothed.method
    seed()
    assert torch.equal(sm_a, evaluation.run_filter(fa, traj, smooth_method="marginal"))
    ha, hb = fa.last_history, fb.last_history
    _hold_record(srec, _side(ha.states, torch.log(fa.last_smoothed.weights), None), _side(hb.states, torch.log(fb.last_smoothed.weights), None),
                 "compare_filters, marginal")
    seed()
    _, _, drec = evaluation.compare_filters(fa, fb, traj, smooth_method="simulation", smooth_draws=8)
    assert drec.particles == (8, 8) and drec.of == "smoothed"
    _hold_record(drec, _side(fa.last_smoothed.trajectories, None, None), _side(fb.last_smoothed.trajectories, None, None),
                 "compare_filters, simulation")
    assert fa.record_history is False and fb.record_history is False

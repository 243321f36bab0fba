"""ESS-triggered (adaptive) resampling on the GPU (``include/mmf.h``: ``mmf_pf_reweight_resample_adaptive``,
``mmf_pf_forward_loop_adaptive``; ``ParticleFilter.resample_ess_threshold`` / ``last_resampled``).

The strict C twin has no adaptive path, so the definition is checked by COMPOSITION: per trajectory an adaptive call must
reproduce, bit for bit, either what mode 0 or what the resampling mode of the existing ``mmf_pf_reweight_resample_belief``
writes, according to the decision recomputed from the recorded ESS bits; the execution forms (step by step, loop of
launches, persistent launch) must agree with each other bit for bit; the two ends of the threshold reproduce the
never- and the always-resampling filter; the training path selects per trajectory; and on a linear-Gaussian system the
adaptive filter is held to the always-resampling filter's own Monte-Carlo distance from the Kalman mean."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import models as om

from _tol import REL_TOL, rel_err


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


def _keeps(ess: torch.Tensor, thr: float, M: int) -> torch.Tensor:
    """The definition: a trajectory is kept iff ``ess >= fl32(thr * M)`` (the product rounded once in fp32)."""
    floor = np.float32(thr) * np.float32(M)
    assert floor.dtype == np.float32
    return ess >= float(floor)


# ------------------------------------------------------------------------------------------ 1. K1 composition
_VARIANTS = {"systematic-uniform": (1, 1.0, False), "systematic-weighted": (1, 1.0, True),
             "multinomial-weighted": (2, 1.0, True), "soft-weighted": (1, 0.5, True)}
_SHAPES = [(M, d) for M in (30, 300, 1025, 20000) for d in (2, 3)] + [(300, 1), (1025, 4)]


@pytest.mark.parametrize("rec", [False, True], ids=["plain", "record"])
@pytest.mark.parametrize("M,d", _SHAPES)
@pytest.mark.parametrize("variant", list(_VARIANTS))
def test_adaptive_k1_is_mode0_or_the_resampler_per_trajectory(variant, M, d, rec):
    """Every output row of the adaptive call equals the row of the mode-0 call (kept: identity ancestors, the rows as
    they came) or of the variant's resampling call (both ``mmf_pf_reweight_resample_belief``), as the decision
    recomputed from the recorded ESS bits says; the estimate and the record equal both.  M = 1025: a ragged float4
    chunk; M = 20,000: the CDF-search kernel also for plain systematic resampling.  thr = 1.0 documents the tie rule:
    uniform weights and a flat likelihood have ess == M exactly and are KEPT."""
    from multimodalfilter_amd import _abi

    dev = _dev()
    mode, alpha, weighted = _VARIANTS[variant]
    N = 12
    g = torch.Generator().manual_seed(1000 * mode + M + d)
    scale = torch.tensor([0.0, 0.3, 1.2, 4.0]).repeat(N // 4)
    loglik = (scale[:, None] * torch.randn((N, M), generator=g)).to(dev)
    if weighted:  # the flat-likelihood rows get a mild spread, so they stay above 0.5 M
        lw = torch.where(scale[:, None] == 0, 0.2, 0.5) * torch.randn((N, M), generator=g)
        logw_in = torch.log_softmax(lw, dim=1).to(dev)
    else:
        logw_in = torch.full((N, M), float(np.float32(-math.log(M))), device=dev)
    states = torch.randn((N, M, d), generator=g).to(dev)
    u = torch.rand((N,) if mode == 1 else (N, M), generator=g).to(dev)

    def out():
        return dict(est=torch.full((N, d), math.nan, device=dev), so=torch.full((N, M, d), math.nan, device=dev),
                    lw=torch.full((N, M), math.nan, device=dev), idx=torch.full((N, M), -1, dtype=torch.int32, device=dev),
                    cov=torch.full((N, d, d), math.nan, device=dev), ess=torch.full((N,), math.nan, device=dev),
                    lev=torch.full((N,), math.nan, device=dev))

    keep0, res = out(), out()
    _abi.pf_reweight_resample_belief(loglik, logw_in, states, None, keep0["est"], keep0["so"], keep0["lw"], None, 0,
                                     cov=keep0["cov"], ess=keep0["ess"], log_evidence=keep0["lev"])
    _abi.pf_reweight_resample_belief(loglik, logw_in, states, u, res["est"], res["so"], res["lw"], res["idx"], mode, alpha,
                                     cov=res["cov"], ess=res["ess"], log_evidence=res["lev"])
    assert torch.equal(keep0["so"], states)
    for k in ("est", "cov", "ess", "lev"):  # one record, whichever kernel writes it
        assert torch.equal(keep0[k], res[k]), k
    ident = torch.arange(M, dtype=torch.int32, device=dev)[None].expand(N, M)

    for thr in (0.5, 1.0):
        keeps = _keeps(res["ess"], thr, M)
        print(f"{variant} M={M} d={d} thr={thr}: kept {int(keeps.sum())} of {N}; ess/M {[round(float(e) / M, 3) for e in res['ess']]}")
        if thr == 0.5:
            assert N // 4 <= int(keeps.sum()) <= N - N // 4, keeps
        elif not weighted:  # the tie: ess == M exactly is kept
            assert torch.equal(res["ess"][scale == 0], torch.full((N // 4,), float(M), device=dev))
            assert bool(keeps[scale == 0].all()) and int(keeps.sum()) == N // 4
        got = out()
        took = torch.full((N,), -1, dtype=torch.int32, device=dev)
        kw = dict(cov=got["cov"], ess=got["ess"], log_evidence=got["lev"]) if rec else {}
        _abi.pf_reweight_resample_adaptive(loglik, logw_in, states, u, got["est"], got["so"], got["lw"], got["idx"], mode,
                                           alpha, ess_threshold=thr, resampled=took, **kw)
        assert torch.equal(took, (~keeps).to(torch.int32)), (thr, took, res["ess"])
        for k in ("so", "lw"):
            assert torch.equal(got[k][keeps], keep0[k][keeps]), (thr, k, "kept")
            assert torch.equal(got[k][~keeps], res[k][~keeps]), (thr, k, "resampled")
        assert torch.equal(got["idx"][keeps], ident[keeps]) and torch.equal(got["idx"][~keeps], res["idx"][~keeps])
        for k in ("est",) + (("cov", "ess", "lev") if rec else ()):
            assert torch.equal(got[k], res[k]), (thr, k)
        if not weighted:  # null logw_in IS the uniform -log M; the decisions and the ancestors are optional outputs
            again = out()
            _abi.pf_reweight_resample_adaptive(loglik, None, states, u, again["est"], again["so"], again["lw"], None, mode,
                                               alpha, ess_threshold=thr, **({"ess": again["ess"]} if rec else {}))
            for k in ("est", "so", "lw"):
                assert torch.equal(again[k], got[k]), (thr, k, "null logw_in")


# ------------------------------------------------------------------------------------------ whole filters
_TARGET_STD = 1.2   # synthetic.calibrate_measurement_heads: ESS/M ~ exp(-1.44) = 0.24 one step after uniform weights
_THR = 0.1


def _calibrated_filter(cls, N, M, T, dev, seed=17):
    """An eval-mode filter with calibrated measurement heads and ``T`` steps of observations / controls."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    tname = "door" if cls.startswith("Door") else "push"
    d = om.TASKS[tname].state_dim
    torch.manual_seed(3)
    f = mmf.model_types(tname)[cls]().to(dev).eval()
    f.num_particles = M
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=seed).items()}
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cal = traj["states"][0][:, None, :] + 0.3 * torch.randn((N, 256, d), device=dev)
    synthetic.calibrate_measurement_heads(f, {k: v[0] for k, v in obs.items()}, cal, target_std=_TARGET_STD)
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
    return f, d, traj, obs, traj["controls"][1:], cov


def _share_in_band(took, what):
    """About half the trajectory-steps resample at thr = 0.1 with a log-normal weight spread of std 1.2 (ESS/M ~ 0.24
    after one step from uniform weights: kept; ~ 0.06 after two: resampled)."""
    share = float(took.float().mean())
    print(f"{what}: {share:.3f} of the trajectory-steps resample (target_std {_TARGET_STD}, thr {_THR})")
    assert 0.1 <= share <= 0.9, share


@pytest.mark.parametrize("variant", ["plain", "soft", "multinomial", "argmax", "records"])
def test_adaptive_native_step_loop_equals_stepwise(variant):
    """``mmf_pf_forward_loop_adaptive`` against T separate ``forward`` calls on the same pre-drawn randomness: estimates,
    final belief, decisions, records and ancestors are identical bits, and the decisions are the definition applied to the
    recorded ESS (recorded by the step-by-step run; the loop records only in the last variant, so the kernels without the
    record must take the same decisions as those with it)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi

    dev = _dev()
    N, M, T = 5, 300, 6
    f, d, traj, obs, ctrl, cov = _calibrated_filter("DoorCrossmodalParticleFilter", N, M, T, dev)
    f.resample_ess_threshold = _THR
    f.soft_resample_alpha = 0.5 if variant == "soft" else 1.0
    f.resample_mode = "multinomial" if variant == "multinomial" else "systematic"
    f.estimation_method = "argmax" if variant == "argmax" else "weighted_average"
    g = torch.Generator(device=dev).manual_seed(5)
    eps0 = torch.randn((N, M, d), generator=g, device=dev)
    eps = torch.randn((T, N, M, d), generator=g, device=dev)
    us = torch.rand((T, N, M) if variant == "multinomial" else (T, N), generator=g, device=dev)

    f.record_belief = f.record_indices = True
    f.noise = mmf.StackedNoise(eps0, eps, us)
    f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
    step, took, beliefs, idx = [], [], [], []
    for t in range(T):
        step.append(f(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]))
        assert f.last_resampled.shape == (N,) and f.last_resampled.dtype == torch.bool
        took.append(f.last_resampled)
        beliefs.append(f.last_belief)
        idx.append(f.last_resample_indices)
    step, took, idx = torch.stack(step), torch.stack(took), torch.stack(idx)
    ess = torch.stack([b.ess for b in beliefs])
    s_ref, w_ref = f.particle_states.clone(), f.particle_log_weights.clone()
    assert torch.equal(took, ~_keeps(ess, _THR, M))
    _share_in_band(took, f"stepwise {variant}")
    ident = torch.arange(M, dtype=torch.int32, device=dev).expand(T, N, M)
    assert torch.equal(idx[~took], ident[~took])  # a kept trajectory's ancestors are itself

    f.record_belief = f.record_indices = variant == "records"
    calls = []
    real = _abi.pf_forward_loop
    _abi.pf_forward_loop = lambda *a, **k: (calls.append(k.get("ess_threshold")), real(*a, **k))[1]
    try:
        f.noise = mmf.StackedNoise(eps0, eps, us)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        loop = f.forward_loop(observations=obs, controls=ctrl)
    finally:
        _abi.pf_forward_loop = real
    assert calls and calls[0] == _THR, "the fused particle filter must take the native adaptive loop"
    assert torch.equal(loop, step)
    assert torch.equal(f.particle_states, s_ref) and torch.equal(f.particle_log_weights, w_ref)
    assert f.last_resampled.shape == (T, N) and torch.equal(f.last_resampled, took)
    if variant == "records":
        assert torch.equal(f.last_belief.ess, ess)
        assert torch.equal(f.last_belief.covariance, torch.stack([b.covariance for b in beliefs]))
        assert torch.equal(f.last_belief.log_evidence, torch.stack([b.log_evidence for b in beliefs]))
        assert torch.equal(f.last_resample_indices, idx)
    # the belief stays usable for further single steps
    f.noise = mmf.StackedNoise(None, eps[:1], us[:1])
    f(observations={k: v[0] for k, v in obs.items()}, controls=ctrl[0])


@pytest.mark.parametrize("rec", [False, True], ids=["plain", "record"])
@pytest.mark.parametrize("cls,N,M,T,precision,noise", [
    ("DoorCrossmodalParticleFilter", 32, 300, 9, "f16x3", "tensor"),
    ("PushCrossmodalParticleFilter", 7, 300, 5, "f32", "philox"),
    ("DoorParticleFilter", 5, 77, 5, "f16x3", "tensor"),
])
def test_adaptive_persistent_step_loop_equals_loop_of_launches(cls, N, M, T, precision, noise, rec):
    """The persistent launch with the adaptive branch in its K1 role against the loop of launches: every output and the
    decisions are identical bits, from a non-uniform incoming belief, twice in a row (odd and even T: the carried
    log-weights end in either buffer)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    old_prec = engine.DEFAULT_PRECISION
    engine.set_default_precision(precision)
    try:
        f, d, traj, obs, ctrl, cov = _calibrated_filter(cls, N, M, T + 1, dev)  # one step without resampling, then T
        f.record_belief = rec
        g = torch.Generator(device=dev).manual_seed(5)
        eps0 = torch.randn((N, M, d), generator=g, device=dev)
        eps = torch.randn((T + 3, N, M, d), generator=g, device=dev)
        us = torch.rand((T + 3, N), generator=g, device=dev)

        def run():
            taken = []
            real = _abi.pf_forward_loop
            _abi.pf_forward_loop = lambda a, *r, **k: (taken.append((int(a.persistent), k.get("ess_threshold"))), real(a, *r, **k))[1]
            try:
                f.noise = mmf.CounterNoise(99) if noise == "philox" else mmf.StackedNoise(eps0, eps, us)
                f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
                f.resample, f.resample_ess_threshold = False, None   # one step without resampling: non-uniform log-weights
                first = f.forward_loop(observations={k: v[:1] for k, v in obs.items()}, controls=ctrl[:1])
                f.resample, f.resample_ess_threshold = None, _THR
                a = f.forward_loop(observations={k: v[1:] for k, v in obs.items()}, controls=ctrl[1:])
                out = [first, a, f.last_resampled.clone(), f.particle_states.clone(), f.particle_log_weights.clone()]
                if rec:
                    out += [f.last_belief.covariance.clone(), f.last_belief.ess.clone(), f.last_belief.log_evidence.clone()]
                b = f.forward_loop(observations={k: v[1:3] for k, v in obs.items()}, controls=ctrl[1:3])  # again: even T
                out += [b, f.last_resampled.clone(), f.particle_states.clone(), f.particle_log_weights.clone()]
                return taken, out
            finally:
                _abi.pf_forward_loop = real

        with engine.persistent_forms(pf=False):
            ref = run()
        with engine.persistent_forms(pf=True):
            got = run()
        assert ref[0] == [(0, None), (0, _THR), (0, _THR)], ref[0]
        assert got[0] == [(0, None), (1, _THR), (1, _THR)], got[0]   # the persistent form was taken
        for i, (x, y) in enumerate(zip(ref[1], got[1])):
            assert torch.equal(x, y), i
        assert got[1][2].shape == (T, N) and bool(torch.isfinite(got[1][1]).all())
        if rec:
            assert torch.equal(got[1][2], ~_keeps(got[1][6], _THR, M))
        _share_in_band(got[1][2], f"persistent {cls} {N} x {M}")
    finally:
        engine.set_default_precision(old_prec)


def test_threshold_limits_reproduce_the_never_and_the_always_resampling_filter():
    """thr = 1e-6: ess >= 1 > 1e-6 M at M = 300, so nobody ever resamples and the run is the ``resample=False`` run, bit
    for bit.  thr = 1: only exactly uniform weights are kept, which calibrated models never produce, so the run is the
    always-resampling run.  Separate, identically seeded noise objects."""
    import multimodalfilter_amd as mmf

    dev = _dev()
    N, M, T = 5, 300, 6
    f, d, traj, obs, ctrl, cov = _calibrated_filter("DoorCrossmodalParticleFilter", N, M, T, dev)
    g = torch.Generator(device=dev).manual_seed(5)
    eps0 = torch.randn((N, M, d), generator=g, device=dev)
    eps = torch.randn((T, N, M, d), generator=g, device=dev)
    us = torch.rand((T, N), generator=g, device=dev)

    def run(resample, thr):
        f.resample, f.resample_ess_threshold = resample, thr
        f.noise = mmf.StackedNoise(eps0.clone(), eps.clone(), us.clone())
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        return est, f.particle_states.clone(), f.particle_log_weights.clone(), f.last_resampled

    never, always = run(False, None), run(True, None)
    assert never[3] is None and always[3] is None
    assert not torch.equal(never[0], always[0])
    low, high = run(True, 1e-6), run(True, 1.0)
    assert low[3].shape == (T, N) and not bool(low[3].any())
    assert bool(high[3].all())
    for x, y in zip(never[:3], low[:3]):
        assert torch.equal(x, y)
    for x, y in zip(always[:3], high[:3]):
        assert torch.equal(x, y)
    off = run(False, 0.5)  # the threshold only has meaning on steps that resample
    assert not bool(off[3].any()) and torch.equal(off[0], never[0])


# ------------------------------------------------------------------------------------------ linear-Gaussian user models
def _system(d=3, seed=0, r_scale=1.0):
    g = torch.Generator().manual_seed(seed)
    A = torch.eye(d) * 0.9 + 0.05 * torch.randn(d, d, generator=g)
    B = 0.1 * torch.randn(d, 7, generator=g)
    L = torch.diag(torch.tensor([0.2, 0.1, 0.15][:d]))
    Rt = torch.diag(torch.tensor([0.3, 0.25, 0.2][:d])) * r_scale
    return A, B, L, Rt


def _kalman_means(A, B, L, Rt, mu, S, us, zs):
    """Closed-form Kalman filter in fp64, batched over trajectories that share ``S``: ``(T, N, d)`` posterior means."""
    A, B, L, Rt, mu, S, us, zs = (t.double() for t in (A, B, L, Rt, mu, S, us, zs))
    Q, R = L @ L.T, Rt @ Rt.T
    out = []
    for u, z in zip(us, zs):
        mu = mu @ A.T + u @ B.T
        S = A @ S @ A.T + Q
        K = S @ torch.inverse(S + R)
        mu = mu + (z - mu) @ K.T
        S = (torch.eye(len(Q), dtype=torch.float64) - K) @ S
        out.append(mu.clone())
    return torch.stack(out)


def _user_models(A, B, L, Rt, dev):
    from multimodalfilter_amd import base

    class LinearDynamics(base.DynamicsModel):
        def __init__(self):
            super().__init__(state_dim=A.shape[0])
            self.A, self.B, self.L = A.to(dev), B.to(dev), L.to(dev)

        def forward(self, *, initial_states, controls):
            R, d = initial_states.shape
            return initial_states @ self.A.T + controls @ self.B.T, self.L[None].expand(R, d, d)

    class GaussianLik(base.ParticleFilterMeasurementModel):
        def __init__(self):
            super().__init__(state_dim=A.shape[0])
            self.Rinv = torch.inverse(Rt @ Rt.T).to(dev)

        def forward(self, *, states, observations):
            e = observations["z"][:, None, :] - states
            return -0.5 * torch.einsum("nmi,ij,nmj->nm", e, self.Rinv, e)

    return LinearDynamics, GaussianLik


def test_adaptive_training_step_selects_per_trajectory():
    """``train()``, ``resample=True``, soft alpha = 0.5, autograd backend, thr = 0.1: K1 supplies the ancestors and the
    decisions, torch re-derives the survivors and ``torch.where`` selects per trajectory.  Forward: the eval-mode adaptive
    step on the same randomness, to the tolerances of the soft-resampling training test (1e-4 on means and on the
    log-weights of particles with the same ancestor; at most 1e-3 of the ancestors differ -- a last-ulp difference between
    the torch and the kernel arithmetic moves a position across a CDF boundary).  Backward: the gradient w.r.t. the
    incoming log-weights of a KEPT trajectory is the one of a ``resample=False`` step on that trajectory alone."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine

    dev = _dev()
    d, N, M = 3, 6, 1024
    A, B, L, Rt = _system(d, r_scale=3.0)
    Dyn, Lik = _user_models(A, B, L, Rt, dev)
    g = torch.Generator().manual_seed(9)
    x = (0.2 * torch.randn((N, 1, d), generator=g) + 0.3 * torch.randn((N, M, d), generator=g)).to(dev)
    # mild incoming weights (kept: ESS/M well above 0.1) and collapsed ones (ESS/M ~ exp(-4): resampled), alternating
    spread = torch.tensor([0.3, 2.0]).repeat(N // 2)
    lw0 = torch.log_softmax(spread[:, None] * torch.randn((N, M), generator=g), dim=1).to(dev)
    ctrl = torch.randn((N, 7), generator=g).to(dev)
    z = (0.3 * torch.randn((N, d), generator=g)).to(dev)
    eps = torch.randn((N, M, d), generator=g).to(dev)
    u = torch.rand((N,), generator=g).to(dev)

    def make(train, resample, thr):
        f = mmf.filters.ParticleFilter(dynamics_model=Dyn(), measurement_model=Lik(), num_particles=M, resample=resample,
                                       soft_resample_alpha=0.5, resample_ess_threshold=thr).to(dev)
        f.train(train)
        f._initialized = True
        return f

    fe = make(False, True, _THR)
    fe.record_indices = True
    fe.particle_states, fe.particle_log_weights = x.clone(), lw0.clone()
    fe.noise = mmf.ReplayNoise([eps], [u])
    est_e = fe(observations={"z": z}, controls=ctrl)
    took = fe.last_resampled
    assert took.tolist() == [False, True] * (N // 2), took

    engine.set_training_backend("autograd")
    try:
        ft = make(True, True, _THR)
        lw_leaf = lw0.clone().requires_grad_(True)
        ft.particle_states, ft.particle_log_weights = x.clone(), lw_leaf
        ft.noise = mmf.ReplayNoise([eps], [u])
        est_t = ft(observations={"z": z}, controls=ctrl)
        assert torch.equal(ft.last_resampled, took)
        assert rel_err(est_t, est_e, dims=1) < REL_TOL, rel_err(est_t, est_e, dims=1)
        keep = ~took
        assert rel_err(ft.particle_states[keep], fe.particle_states[keep], dims=1) < REL_TOL
        assert float((ft.particle_log_weights[keep].detach() - fe.particle_log_weights[keep]).abs().max()) < 1e-4
        same = ((ft.particle_states[took] - fe.particle_states[took]).abs() <= 1e-4 * fe.particle_states[took].abs().clamp_min(1.0)).all(-1)
        assert int((~same).sum()) <= 1e-3 * int(took.sum()) * M, int((~same).sum())
        assert float((ft.particle_log_weights[took].detach() - fe.particle_log_weights[took])[same].abs().max()) < 1e-4
        assert float(torch.logsumexp(ft.particle_log_weights.detach(), dim=1).abs().max()) < 1e-4

        # a loss over the KEPT trajectories' outgoing belief and estimate
        c = torch.randn((N, M), generator=g).to(dev)
        loss = lambda f, est, rows, crow: (f.particle_log_weights[rows] * crow).sum() + est[rows].square().sum()
        (grad,) = torch.autograd.grad(loss(ft, est_t, keep, c[keep]), lw_leaf)
        assert float(grad[took].abs().max()) == 0.0  # (nothing of the loss touches them)
        for n in torch.nonzero(keep).flatten().tolist():
            fr = make(True, False, None)
            leaf = lw0[n:n + 1].clone().requires_grad_(True)
            fr.particle_states, fr.particle_log_weights = x[n:n + 1].clone(), leaf
            fr.noise = mmf.ReplayNoise([eps[n:n + 1]], [])
            est_r = fr(observations={"z": z[n:n + 1]}, controls=ctrl[n:n + 1])
            (want,) = torch.autograd.grad(loss(fr, est_r, slice(0, 1), c[n:n + 1]), leaf)
            assert float(want.abs().max()) > 0
            assert rel_err(grad[n:n + 1], want, dims=1) < REL_TOL, (n, rel_err(grad[n:n + 1], want, dims=1))
    finally:
        engine.set_training_backend(None)


def test_adaptive_filter_is_no_further_from_the_kalman_mean_than_the_always_resampling_one():
    """Linear-Gaussian system, N = 16, M = 2000, T = 20, 8 noise seeds: the RMS distance of the posterior means from the
    closed-form Kalman means.  Reference: the always-resampling engine filter on the same seeds; the adaptive filter
    (thr = 0.5) must stay within its mean + 3 standard deviations over the seeds.  Measured on MI355X (this test prints
    both): always-resampling 0.01913 +- 0.00150, adaptive 0.02022 +- 0.00141 with 0.767 of the
    trajectory-steps resampling; bound 0.02362."""
    import multimodalfilter_amd as mmf

    dev = _dev()
    d, N, M, T = 3, 16, 2000, 20
    A, B, L, Rt = _system(d)
    Dyn, Lik = _user_models(A, B, L, Rt, dev)
    g = torch.Generator().manual_seed(11)
    us = torch.randn((T, N, 7), generator=g)
    mu0 = 0.2 * torch.randn((N, d), generator=g)
    S0 = 0.1 * torch.eye(d)
    xs, zs = mu0 + torch.randn((N, d), generator=g) @ torch.linalg.cholesky(S0).T, []
    for t in range(T):  # data drawn from the model itself
        xs = xs @ A.T + us[t] @ B.T + torch.randn((N, d), generator=g) @ L.T
        zs.append(xs + torch.randn((N, d), generator=g) @ Rt.T)
    zs = torch.stack(zs)
    kal = _kalman_means(A, B, L, Rt, mu0, S0, us, zs)

    def rms(thr, seed):
        f = mmf.filters.ParticleFilter(dynamics_model=Dyn(), measurement_model=Lik(), num_particles=M,
                                       resample_ess_threshold=thr)
        f.eval()
        f.noise = mmf.NoiseSource(seed)
        f.initialize_beliefs(mean=mu0.to(dev), covariance=S0[None].expand(N, d, d).to(dev))
        est = f.forward_loop(observations={"z": zs.to(dev)}, controls=us.to(dev)).cpu().double()
        share = None if thr is None else float(f.last_resampled.float().mean())
        return float((est - kal).pow(2).sum(-1).mean().sqrt()), share

    always = np.array([rms(None, seed)[0] for seed in range(8)])
    adaptive = [rms(0.5, seed) for seed in range(8)]
    shares = [s for _, s in adaptive]
    adaptive = np.array([r for r, _ in adaptive])
    bound = always.mean() + 3.0 * always.std(ddof=1)
    print(f"RMS distance from the Kalman mean over 8 seeds: always-resampling {always.mean():.5f} +- {always.std(ddof=1):.5f}, "
          f"adaptive (thr 0.5) {adaptive.mean():.5f} +- {adaptive.std(ddof=1):.5f}; bound {bound:.5f}; "
          f"share of resampling trajectory-steps {np.mean(shares):.3f}")
    assert 0.0 < np.mean(shares) < 1.0      # it is the adaptive filter that is being measured
    assert adaptive.mean() <= bound, (adaptive.mean(), bound)

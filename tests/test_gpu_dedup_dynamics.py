"""The dynamics network once per distinct resampled ancestor (``engine.PF_DEDUP``; ``include/mmf.h``:
``mmf_pf_forward_loop_dedup``, ``mmf_pf_resample_runs``, ``mmf_pf_dynamics_runs``): the change is exact, so every comparison
is ``torch.equal`` -- the path ON against OFF through ``forward_loop``, and K1's run table against what numpy derives from the
ancestors the existing K1 returns.  Shapes are the smallest at which the path can go wrong: one tile per trajectory
(M = 64), a partly filled last tile (M = 192), K1's single full chunk with tiles beyond ``n_runs`` (M = 4096), K1's
two-chunk scan carry (M = 8192); loops of T = 1 (never uses the path), 2 (each kernel once) and 5, run back to back so the
belief is carried across calls."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_SEGMENTS = (1, 2, 5)  # consecutive forward_loop calls of these lengths
_T = sum(_SEGMENTS)


def _dev():
    if not torch.cuda.is_available():
        pytest.skip("needs an MI355X")
    return torch.device("cuda", 0)


def _setup(task, N, M, dev, head_scale=None, seed=17):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    cls = "DoorCrossmodalParticleFilter" if task == "door" else "PushCrossmodalParticleFilter"
    torch.manual_seed(3)
    f = mmf.model_types(task)[cls]().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    f.num_particles, f.resample_mode = M, "systematic"
    d = f.state_dim
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=_T, N=N, seed=seed).items()}
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    if head_scale is not None:  # the measurement heads: 0 -> flat weights, large -> one survivor
        with torch.no_grad():
            for m in f.measurement_model.measurement_models:
                m.shared_layers[4].weight.mul_(head_scale)
                m.shared_layers[4].bias.mul_(head_scale)
    cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
    g = torch.Generator(device=dev).manual_seed(5)
    rnd = (torch.randn((N, M, d), generator=g, device=dev), torch.randn((_T, N, M, d), generator=g, device=dev),
           torch.rand((_T, N), generator=g, device=dev))
    return f, d, traj, obs, traj["controls"][1:], cov, rnd


def _run(f, traj, obs, ctrl, cov, rnd, noise, on, *, segments=_SEGMENTS):
    """The filter over ``segments`` with the path ``on`` / off -> (every compared tensor, whether each call got a workspace)."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    took = []
    real = _abi.pf_forward_loop
    _abi.pf_forward_loop = lambda a, *r, **k: (took.append((int(a.persistent), k.get("dedup") is not None)), real(a, *r, **k))[1]
    saved = engine.PF_DEDUP
    engine.PF_DEDUP = on
    out = []
    try:
        with engine.persistent_forms(pf=False):
            f.noise = mmf.CounterNoise(99) if noise == "philox" else mmf.StackedNoise(rnd[0].clone(), rnd[1], rnd[2])
            f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
            t0 = 0
            for T in segments:
                est = f.forward_loop(observations={k: v[t0:t0 + T] for k, v in obs.items()}, controls=ctrl[t0:t0 + T])
                out += [est.clone(), f.particle_states.clone(), f.particle_log_weights.clone()]
                if f.record_indices:
                    out += [f.last_resample_indices.clone(), f.last_log_likelihoods.clone()]
                if f.record_belief:
                    out += [f.last_belief.covariance.clone(), f.last_belief.ess.clone(), f.last_belief.log_evidence.clone()]
                t0 += T
    finally:
        engine.PF_DEDUP = saved
        _abi.pf_forward_loop = real
    return out, took


def _compare(f, traj, obs, ctrl, cov, rnd, noise, *, segments=_SEGMENTS):
    ref, took_off = _run(f, traj, obs, ctrl, cov, rnd, noise, False, segments=segments)
    got, took_on = _run(f, traj, obs, ctrl, cov, rnd, noise, True, segments=segments)
    assert took_off == [(0, False)] * len(segments), took_off
    assert took_on == [(0, T >= 2) for T in segments], took_on  # the path was taken where a step can consume a table
    assert len(ref) == len(got)
    for i, (x, y) in enumerate(zip(ref, got)):
        assert x.shape == y.shape and torch.equal(x, y), i
        assert bool(torch.isfinite(x.float()).all()), i
    return got


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("precision", ["f16x3", "f32"])
@pytest.mark.parametrize("N,M", [(3, 64), (3, 192), (2, 4096), (1, 8192)])
@pytest.mark.parametrize("task", ["door", "push"])
def test_dedup_on_equals_off_through_forward_loop(task, N, M, precision, noise):
    from multimodalfilter_amd import engine

    dev = _dev()
    old = engine.DEFAULT_PRECISION
    engine.set_default_precision(precision)
    try:
        f, d, traj, obs, ctrl, cov, rnd = _setup(task, N, M, dev)
        f.record_indices = True
        got = _compare(f, traj, obs, ctrl, cov, rnd, noise)
        idx = got[-2]  # ancestors of the last call's steps
        distinct = (1 + (torch.sort(idx, dim=-1)[0].diff(dim=-1) != 0).sum(-1)).float() / M
        print(f"{task} {N} x {M} {precision} {noise}: distinct ancestors / M in [{float(distinct.min()):.3f}, {float(distinct.max()):.3f}]")
        f.record_indices = False  # and without the per-step records (the timed path)
        _compare(f, traj, obs, ctrl, cov, rnd, noise)
    finally:
        engine.set_default_precision(old)


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("N,M", [(3, 192), (2, 4096)])
def test_dedup_collapsed_weights_one_run_feeds_every_slot(N, M, noise):
    """Measurement heads scaled up until one ancestor owns every slot: ``n_runs`` = 1, one lane feeds M slots, every tile
    but the first is empty; and particle 0 has no offspring there."""
    dev = _dev()
    f, d, traj, obs, ctrl, cov, rnd = _setup("door", N, M, dev, head_scale=1.0e6)
    f.record_indices = True
    got = _compare(f, traj, obs, ctrl, cov, rnd, noise)
    idx = got[-2]
    lo, hi = idx.min(-1)[0], idx.max(-1)[0]
    assert bool((lo == hi).any()), "no (step, trajectory) collapsed onto one ancestor"
    assert bool((idx[..., 0] != 0).any()), "particle 0 kept offspring everywhere"


@pytest.mark.parametrize("noise", ["tensor", "philox"])
@pytest.mark.parametrize("N,M", [(3, 192), (2, 4096)])
def test_dedup_flat_weights_every_run_has_length_one(N, M, noise):
    """Heads scaled to 0: ``n_runs`` = M, every run has length 1 (the identity ancestors: particle 0 owns slot 0)."""
    dev = _dev()
    f, d, traj, obs, ctrl, cov, rnd = _setup("door", N, M, dev, head_scale=0.0)
    f.record_indices = True
    got = _compare(f, traj, obs, ctrl, cov, rnd, noise)
    idx = got[-2]
    assert torch.equal(idx, torch.arange(M, dtype=torch.int32, device=dev).expand_as(idx))


@pytest.mark.parametrize("variant", ["record_belief", "argmax"])
def test_dedup_with_belief_record_and_argmax_estimates(variant):
    dev = _dev()
    f, d, traj, obs, ctrl, cov, rnd = _setup("door", 3, 192, dev)
    if variant == "argmax":
        f.estimation_method = "argmax"
    else:
        f.record_belief = True
    _compare(f, traj, obs, ctrl, cov, rnd, "tensor")


def test_dedup_leaves_the_other_loops_alone():
    """Soft, adaptive, multinomial and no resampling get no workspace (and a persistent launch is a persistent launch)."""
    from multimodalfilter_amd import _abi, engine

    dev = _dev()
    f, d, traj, obs, ctrl, cov, rnd = _setup("door", 3, 192, dev)
    g = torch.Generator(device=dev).manual_seed(6)
    um = torch.rand((_T, 3, 192), generator=g, device=dev)

    def taken(**kw):
        for k, v in kw.items():
            setattr(f, k, v)
        _, took = _run(f, traj, obs, ctrl, cov, (rnd[0], rnd[1], um if f.resample_mode == "multinomial" else rnd[2]), "tensor", True,
                       segments=(5,))
        return took

    assert taken() == [(0, True)]
    assert taken(soft_resample_alpha=0.5) == [(0, False)]
    assert taken(soft_resample_alpha=1.0, resample_ess_threshold=0.5) == [(0, False)]
    assert taken(resample_ess_threshold=None, resample_mode="multinomial") == [(0, False)]
    assert taken(resample_mode="systematic", resample=False) == [(0, False)]


def _table_from_ancestors(idx, M):
    """numpy: rank / run_anc / run_start / n_runs of one trajectory's ancestors (non-decreasing)."""
    starts = np.concatenate([[True], idx[1:] != idx[:-1]])
    rank = np.cumsum(starts) - 1
    first = np.nonzero(starts)[0]
    return rank.astype(np.int32), idx[first].astype(np.int32), np.concatenate([first, [M]]).astype(np.int32), int(starts.sum())


@pytest.mark.parametrize("weights", ["random", "collapsed"])
@pytest.mark.parametrize("N,M", [(3, 192), (1, 8192)])
@pytest.mark.parametrize("d", [2, 3])
def test_run_table_of_k1_equals_numpy_on_the_existing_k1s_ancestors(N, M, d, weights):
    from multimodalfilter_amd import _abi

    dev = _dev()
    g = torch.Generator(device=dev).manual_seed(11 + M + d)
    ll = torch.randn((N, M), generator=g, device=dev) * (1.2 if weights == "random" else 1.0e4)
    lw = torch.full((N, M), -float(np.log(M)), device=dev)
    xs = torch.randn((N, M, d), generator=g, device=dev)
    u = torch.rand((N,), generator=g, device=dev)
    est0, so, lo, io = (torch.empty((N, d), device=dev), torch.empty((N, M, d), device=dev), torch.empty((N, M), device=dev),
                        torch.empty((N, M), dtype=torch.int32, device=dev))
    _abi.pf_reweight_resample(ll, lw, xs, u, est0, so, lo, io, 1)
    i32 = dict(dtype=torch.int32, device=dev)
    est1, io1 = torch.empty((N, d), device=dev), torch.empty((N, M), **i32)
    rank, anc, start, n_runs = (torch.full((N, M), -7, **i32), torch.full((N, M + 1), -7, **i32),
                                torch.full((N, M + 1), -7, **i32), torch.full((N,), -7, **i32))
    _abi.pf_resample_runs(ll, lw, xs, u, est1, io1, rank, anc, start, n_runs)
    assert torch.equal(est0, est1) and torch.equal(io, io1)
    idx = io.cpu().numpy()
    for n in range(N):
        assert (np.diff(idx[n]) >= 0).all()
        r, a, s, k = _table_from_ancestors(idx[n], M)
        assert int(n_runs[n]) == k, (n, int(n_runs[n]), k)
        assert np.array_equal(rank[n].cpu().numpy(), r)
        assert np.array_equal(anc[n, :k].cpu().numpy(), a)
        assert np.array_equal(start[n, :k + 1].cpu().numpy(), s)
        if weights == "collapsed":
            assert k <= 2  # (two only if the two largest log-likelihoods tie in fp32)
    # the uniform-weight shortcut of the loop's later steps (null logw_in) gives the same table
    rank2, anc2, start2, n2 = torch.empty_like(rank), torch.full_like(anc, -7), torch.full_like(start, -7), torch.empty_like(n_runs)
    _abi.pf_resample_runs(ll, None, xs, u, est1, None, rank2, anc2, start2, n2)
    assert torch.equal(rank, rank2) and torch.equal(anc, anc2) and torch.equal(start, start2) and torch.equal(n_runs, n2)

"""Training a particle filter on the CRPS and the energy score of its particle sets: the native recursion with the sets as
differentiable outputs against the step-by-step paths, on ``test_gpu_set_loss_training.py``'s ``Problem`` and with its bars
(1e-5 relative on the loss, ``GRAD_TOL`` on every gradient); the ``"hip"`` against the ``"autograd"`` backend; the graphed
step; descent; and the loss against what ``belief_scores`` reports in evaluation."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from _tol import REL_TOL, rel_err_elementwise
from test_gpu_set_loss_training import DEV, Problem, assert_same_training_signal, mse

SCALE = (0.5, 1.0, 2.0)


def energy_all(pred, sets, target):
    from multimodalfilter_amd import train

    return train.particle_set_energy(sets["states"], sets["log_weights"], target, SCALE[:target.shape[-1]]).mean()


def crps_and_mse(pred, sets, target):
    from multimodalfilter_amd import train

    return train.particle_set_crps(sets["states"], sets["log_weights"], target).sum(-1).mean() + 0.1 * mse(pred, sets, target)


@pytest.mark.parametrize("tname,cls,N,M,T,chunk_rows", [
    ("door", "DoorCrossmodalParticleFilter", 6, 30, 5, 32768),    # the reference's training size class: one chunk
    ("door", "DoorCrossmodalParticleFilter", 5, 300, 3, 600),     # several ragged chunks of trajectories
    ("push", "PushUnimodalParticleFilter", 4, 64, 4, 128),
])
def test_native_recursion_matches_stepwise_on_the_energy_score(tname, cls, N, M, T, chunk_rows):
    """The mean energy score over every step's set: the native recursion (sets as outputs, their gradients injected by
    ``mmf_pf_train_backward_sets``) against the step-by-step K6 path."""
    p = Problem(tname, cls, N, M, T)
    want = p.run(energy_all, native=False, chunk_rows=chunk_rows)
    got = p.run(energy_all, native=True, chunk_rows=chunk_rows)
    assert_same_training_signal(got, want, f"{cls} {N}x{M}x{T}")


def test_native_recursion_matches_stepwise_on_crps_plus_mse():
    """``sum_k crps_k + 0.1 mse`` through the sets and the estimates at once; the energy terms of the backward are not asked for."""
    p = Problem("door", "DoorCrossmodalParticleFilter", 6, 30, 5)
    want = p.run(crps_and_mse, native=False)
    got = p.run(crps_and_mse, native=True)
    assert_same_training_signal(got, want, "crps + 0.1 mse")


def test_hip_stepwise_matches_the_autograd_backend_on_the_energy_score():
    """The two kernels of the loss (and K6 under them) against the torch formulation throughout, both step by step."""
    p = Problem("door", "DoorCrossmodalParticleFilter", 6, 30, 5)
    want = p.run(energy_all, native=False, backend="autograd")
    got = p.run(energy_all, native=False, backend="hip")
    assert_same_training_signal(got, want, "hip against autograd")


def test_graphed_step_replays_the_eager_step_on_the_energy_score():
    """``GraphedFilterStep(loss="energy")`` against ``train_filter_step(loss="energy")``: eight steps on changing batches, the
    losses and the final weights bit for bit."""
    import copy

    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, synthetic, train

    dev = torch.device(DEV)
    N, M, L, d = 8, 30, 6, 3
    batches = [{k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=L - 1, N=N, seed=3 + i).items()} for i in range(3)]
    cov = torch.eye(d, device=dev) * 0.1
    torch.manual_seed(0)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).train()
    f.num_particles = M
    g = copy.deepcopy(f)
    of, og = torch.optim.SGD(f.parameters(), lr=1e-3), torch.optim.SGD(g.parameters(), lr=1e-3)
    f.noise, g.noise = mmf.NoiseSource(seed=5), mmf.NoiseSource(seed=5)
    engine.set_training_backend("hip")
    try:
        step = train.GraphedFilterStep(g, og, initial_covariance=cov, noise=g.noise, eager_steps=2, loss="energy", score_scale=SCALE)
        eager = [train.train_filter_step(f, batches[i % 3], of, initial_covariance=cov, noise=f.noise, loss="energy", score_scale=SCALE)
                 for i in range(8)]
        graphed = [step(batches[i % 3]) for i in range(8)]
        assert step.graph is not None
    finally:
        engine.set_training_backend(None)
    assert graphed == eager
    for (n, p), q in zip(f.named_parameters(), g.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    assert f.keep_training_sets is False and g.keep_training_sets is False


def test_sgd_on_the_energy_score_descends():
    """Six SGD steps of ``train_filter_step(loss="energy")`` on one batch with replayed noise lower the energy score of that
    batch; ``loss=train.crps_loss(scale)`` is the scaled sum of what ``particle_set_crps`` gives."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, synthetic, train

    dev = torch.device(DEV)
    d, L, N, M = 3, 5, 6, 30
    batch = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=L - 1, N=N, seed=3).items()}
    cov = torch.eye(d, device=dev) * 0.1
    torch.manual_seed(1)
    f = mmf.door_models.DoorParticleFilter().to(dev).train()
    f.num_particles = M
    eps_init = torch.randn((N, d))
    eps = [torch.randn((N, M, d)) for _ in range(L)]
    opt = torch.optim.SGD(f.parameters(), lr=1e-3)
    replay = lambda: dict(initial_covariance=cov, noise=mmf.ReplayNoise([eps_init.clone()], []))
    engine.set_training_backend("hip")
    try:
        losses = []
        for _ in range(6):
            f.noise = mmf.ReplayNoise([e.clone() for e in eps], [])
            losses.append(train.train_filter_step(f, batch, opt, loss="energy", score_scale=SCALE, **replay()))
        seen = {}

        def crps_scaled(pred, sets, b):
            seen["crps"] = train.particle_set_crps(sets["states"], sets["log_weights"], b["states"][1:]).detach()
            return pred.sum() * 0.0

        f.noise = mmf.ReplayNoise([e.clone() for e in eps], [])
        train.filter_loss(f, batch, loss=crps_scaled, **replay())
        f.noise = mmf.ReplayNoise([e.clone() for e in eps], [])
        got = float(train.filter_loss(f, batch, loss=train.crps_loss(SCALE), **replay()).detach())
    finally:
        engine.set_training_backend(None)
    print("energy score per step:", losses)
    assert all(l == l for l in losses) and losses[-1] < losses[0]
    want = float((seen["crps"].double() / torch.tensor(SCALE, dtype=torch.float64, device=dev)).sum(-1).mean())
    assert abs(got - want) < 1e-5 * abs(want), (got, want)


def test_the_training_loss_is_the_score_that_evaluation_reports():
    """Train on what you evaluate: on the filtered sets of an evaluation run's history, ``particle_set_scores`` is
    ``belief_scores``' ``crps`` and ``energy``.  The evaluation run adds the two log-weights inside the kernel; the training
    path is handed their sum."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine, synthetic, train

    dev = torch.device(DEV)
    N, M, T, d = 5, 300, 6, 3
    traj = synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=11)
    obs = {k: v[1:].to(dev) for k, v in synthetic.observations_of(traj).items()}
    torch.manual_seed(2)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval()
    f.num_particles = M
    f.noise = mmf.NoiseSource(seed=7)
    f.record_history = True
    f.initialize_beliefs(mean=traj["states"][0].to(dev), covariance=(torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev))
    f.forward_loop(observations=obs, controls=traj["controls"][1:].to(dev))
    h = f.last_history
    truth = traj["states"][1:].to(dev).contiguous()
    f.belief_scores(truth, scale=SCALE)
    want_c, want_e = f.last_scores.crps, f.last_scores.energy
    engine.set_training_backend("hip")
    try:
        got_c, got_e = train.particle_set_scores(h.states, h.log_weights_in + h.log_likelihoods, truth, SCALE)
    finally:
        engine.set_training_backend(None)
    assert got_c.shape == want_c.shape == (T, N, d) and got_e.shape == want_e.shape == (T, N)
    assert bool(torch.isfinite(want_c).all()) and bool(torch.isfinite(want_e).all())
    for name, got, want in (("crps", got_c, want_c), ("energy", got_e, want_e)):
        err = rel_err_elementwise(got, want, floor=1e-3)
        print(f"particle_set_scores against belief_scores, {name}:", err)
        assert err < REL_TOL, name

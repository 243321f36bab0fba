"""Training a particle filter on the log score of its particle sets: the native recursion with the sets as differentiable
outputs (``engine.PfTrainLoopFunction`` -> ``mmf_pf_train_backward_sets``) against the step-by-step paths, with the bars of
``test_gpu_training.py::test_native_training_recursion_matches_stepwise`` (1e-5 relative on the loss, ``GRAD_TOL`` on every
gradient, measured as that test measures it); the default path bit for bit; the graphed step; descent; and the loss against
what ``belief_density`` reports in evaluation."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import models as om

from _tol import REL_TOL, rel_err_elementwise, scalar_rel

GRAD_TOL = 5e-3  # test_gpu_training.py's fp32-against-fp32 tolerance (a pre-activation at rounding distance from zero may flip)
SCALE = (0.3, 0.2, 0.25)
DEV = "cuda:0"


def _data(task, T, N, seed):
    g = torch.Generator().manual_seed(seed)
    d = task.state_dim
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1),
           "gripper_pos": torch.randn((T, N, 3), generator=g),
           "gripper_sensors": torch.randn((T, N, 7), generator=g)}
    return obs, torch.randn((T, N, 7), generator=g), torch.randn((N, d), generator=g), \
        torch.randn((T, N, d), generator=g), g


def _scale(d):
    return torch.tensor(SCALE[:d], device=DEV)


def nll_all(pred, sets, target):
    from multimodalfilter_amd import train

    return train.particle_set_nll(sets["states"], sets["log_weights"], target, _scale(target.shape[-1])).mean()


def nll_of_step(t):
    def loss(pred, sets, target):
        from multimodalfilter_amd import train

        return train.particle_set_nll(sets["states"][t], sets["log_weights"][t], target[t], _scale(target.shape[-1])).mean()
    return loss


def mse(pred, sets, target):
    return torch.mean((pred - target) ** 2)


def mixed(pred, sets, target):
    return mse(pred, sets, target) + 0.1 * nll_all(pred, sets, target)


class Problem:
    """One model, one batch and one set of pre-drawn noise, run under whatever path, backend and loss."""

    def __init__(self, tname, cls, N, M, T):
        import multimodalfilter_amd as mmf

        task = om.TASKS[tname]
        d = task.state_dim
        obs, ctrl, x0, target, g = _data(task, T, N, 31)
        self.eps0 = torch.randn((N, M, d), generator=g)
        self.eps = [torch.randn((N, M, d), generator=g) for _ in range(T)]
        self.cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(DEV)
        self.obs, self.ctrl = {k: v.to(DEV) for k, v in obs.items()}, ctrl.to(DEV)
        self.x0, self.target = x0.to(DEV), target.to(DEV)
        torch.manual_seed(3)
        self.f = mmf.model_types(tname)[cls]().to(DEV).train()
        self.f.num_particles = M

    def run(self, loss_fn, *, native, backend="hip", keep=True, chunk_rows=None, init_grad=True):
        """``(loss, parameter gradients, d loss / d initial states, d loss / d initial log-weights)`` on exact-fp32 products
        (both paths, as in the test this file mirrors)."""
        import multimodalfilter_amd as mmf
        from multimodalfilter_amd import engine

        f = self.f
        old_chunk, old_prec = engine.TRAIN_CHUNK_ROWS, engine.DEFAULT_PRECISION
        engine.set_training_backend(backend)
        if chunk_rows is not None:
            engine.TRAIN_CHUNK_ROWS = chunk_rows
        engine.set_default_precision("f32")
        try:
            f.use_native_loop = native
            f.keep_training_sets = keep
            f.zero_grad(set_to_none=True)
            f.noise = mmf.ReplayNoise([self.eps0] + self.eps, [])
            f.initialize_beliefs(mean=self.x0, covariance=self.cov)
            s0 = w0 = None
            if init_grad:
                s0 = f.particle_states.detach().clone().requires_grad_(True)
                w0 = f.particle_log_weights.detach().clone().requires_grad_(True)
                f.particle_states, f.particle_log_weights = s0, w0
            pred = f.forward_loop(observations=self.obs, controls=self.ctrl)
            sets = f.last_training_sets
            assert (sets is not None) == keep
            if keep:
                T, (N, M, d) = pred.shape[0], f.particle_states.shape
                assert sets["states"].shape == (T, N, M, d) and sets["log_weights"].shape == (T, N, M)
                assert sets["states"].requires_grad and sets["log_weights"].requires_grad
            loss = loss_fn(pred, sets, self.target)
            loss.backward()
            grads = {n: p.grad.detach().clone() for n, p in f.named_parameters() if p.grad is not None}
            return (float(loss.detach()), grads, None if s0 is None else s0.grad.detach().clone(),
                    None if w0 is None else w0.grad.detach().clone())
        finally:
            engine.set_training_backend(None)
            engine.TRAIN_CHUNK_ROWS = old_chunk
            engine.set_default_precision(old_prec)
            f.use_native_loop, f.keep_training_sets = True, False


def assert_same_training_signal(got, want, what):
    """The bars of ``test_native_training_recursion_matches_stepwise``: the loss to 1e-5 relative; every parameter gradient within
    ``GRAD_TOL`` of the larger of its own scale and 1e-3 of the model's largest gradient entry; the gradients of the initial
    belief within ``GRAD_TOL`` of their own scale."""
    (l1, g1, s1, w1), (l0, g0, s0, w0) = got, want
    print(what, "loss", l1, l0)
    assert scalar_rel(l1, l0) < 1e-5, (what, l1, l0)
    assert set(g0) == set(g1) and len(g0) > 20, what
    top = max(float(v.abs().max()) for v in g0.values())
    assert top > 0.0
    worst = max((float((g0[k] - g1[k]).abs().max()) / max(1e-3 * top, float(g0[k].abs().max())), k) for k in g0)
    print(what, "largest relative gradient difference:", worst)
    assert worst[0] < GRAD_TOL, (what, worst)
    for name, a, b in (("d_states0", s1, s0), ("d_logw0", w1, w0)):
        if b is None:
            continue
        assert float(b.abs().max()) > 0.0, (what, name)
        err = float((a - b).abs().max()) / float(b.abs().max())
        print(what, name, err)
        assert err < GRAD_TOL, (what, name, err)


@pytest.mark.parametrize("tname,cls,N,M,T,chunk_rows", [
    ("door", "DoorCrossmodalParticleFilter", 6, 30, 5, 32768),    # the reference's training size class: one chunk
    ("door", "DoorCrossmodalParticleFilter", 5, 300, 3, 600),     # several ragged chunks of trajectories; a row is a workgroup's
    ("push", "PushUnimodalParticleFilter", 4, 64, 4, 128),
    ("door", "DoorParticleFilter", 3, 100, 3, 100),               # single measurement network, no modality weights
])
def test_native_recursion_matches_stepwise_on_the_set_nll(tname, cls, N, M, T, chunk_rows):
    """The mean ``particle_set_nll`` over every step's set: the native recursion (sets as outputs, their gradients injected by
    ``mmf_pf_train_backward_sets``) against the step-by-step K6 path (the sets stacked, torch autograd between the steps)."""
    p = Problem(tname, cls, N, M, T)
    want = p.run(nll_all, native=False, chunk_rows=chunk_rows)
    got = p.run(nll_all, native=True, chunk_rows=chunk_rows)
    assert_same_training_signal(got, want, f"{cls} {N}x{M}x{T}")


def test_hip_stepwise_matches_the_autograd_backend_on_the_set_nll():
    """The HIP kernel of the loss (and K6 under it) against the torch formulation throughout, both step by step."""
    p = Problem("door", "DoorCrossmodalParticleFilter", 6, 30, 5)
    want = p.run(nll_all, native=False, backend="autograd")
    got = p.run(nll_all, native=False, backend="hip")
    assert_same_training_signal(got, want, "hip against autograd")


@pytest.mark.parametrize("which,T", [("last", 4), ("first", 4), ("only", 1)])
def test_set_gradients_enter_the_recursion_at_their_own_step(which, T):
    """A loss on ONE step's set -- the last (where the recursion has no later log-weight gradient to add to), the first, and the
    only one of ``T = 1``: a gradient dropped or injected at another step is an O(1) difference."""
    p = Problem("door", "DoorCrossmodalParticleFilter", 4, 30, T)
    loss = nll_of_step(-1 if which == "last" else 0)
    want = p.run(loss, native=False)
    got = p.run(loss, native=True)
    assert_same_training_signal(got, want, f"{which} step of {T}")


def test_native_recursion_matches_stepwise_on_a_mixed_loss():
    """``mse + 0.1 nll`` through the estimates and the sets at once (what Kloss et al. recommend)."""
    p = Problem("door", "DoorCrossmodalParticleFilter", 6, 30, 5)
    want = p.run(mixed, native=False)
    got = p.run(mixed, native=True)
    assert_same_training_signal(got, want, "mse + 0.1 nll")


def test_default_path_keeps_its_bits(monkeypatch):
    """An MSE loss with ``keep_training_sets`` on (the sets handed out, no gradient returned for them) gives every parameter
    gradient of the run with the switch off, bit for bit; and ``mmf_pf_train_backward_sets(args, null, null)`` in place of
    ``mmf_pf_train_backward`` gives those bits too."""
    from multimodalfilter_amd import _abi

    p = Problem("door", "DoorCrossmodalParticleFilter", 6, 30, 5)
    off = p.run(mse, native=True, keep=False)
    on = p.run(mse, native=True, keep=True)
    calls = []

    def through_sets(args, like):
        calls.append(1)
        _abi.pf_train_backward_sets(args, None, None, like)

    monkeypatch.setattr(_abi, "pf_train_backward", through_sets)
    sets_null = p.run(mse, native=True, keep=False)
    assert calls == [1]
    for other, what in ((on, "keep_training_sets"), (sets_null, "backward_sets(null, null)")):
        assert other[0] == off[0], what
        assert set(other[1]) == set(off[1]) and len(off[1]) > 20
        for k in off[1]:
            assert torch.equal(other[1][k], off[1][k]), (what, k)
        assert torch.equal(other[2], off[2]) and torch.equal(other[3], off[3]), what


def test_graphed_step_replays_the_eager_step_on_the_set_nll():
    """``GraphedFilterStep(loss="nll")`` against ``train_filter_step(loss="nll")``, as
    ``test_graphed_training_step_replays_the_eager_step`` compares them for SGD: eight steps on changing batches, the losses and
    the final weights bit for bit."""
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
        step = train.GraphedFilterStep(g, og, initial_covariance=cov, noise=g.noise, eager_steps=2, loss="nll", nll_scale=SCALE)
        eager = [train.train_filter_step(f, batches[i % 3], of, initial_covariance=cov, noise=f.noise, loss="nll", nll_scale=SCALE)
                 for i in range(8)]
        graphed = [step(batches[i % 3]) for i in range(8)]
        assert step.graph is not None
    finally:
        engine.set_training_backend(None)
    assert graphed == eager
    for (n, p), q in zip(f.named_parameters(), g.parameters()):
        assert torch.equal(p.detach(), q.detach()), n
    assert f.keep_training_sets is False and g.keep_training_sets is False


def test_sgd_on_the_set_nll_descends():
    """A few SGD steps of ``train_filter_step(loss="nll")`` on one batch with replayed noise lower the NLL of that batch."""
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
    engine.set_training_backend("hip")
    try:
        losses = []
        for _ in range(6):
            f.noise = mmf.ReplayNoise([e.clone() for e in eps], [])
            losses.append(train.train_filter_step(f, batch, opt, initial_covariance=cov, noise=mmf.ReplayNoise([eps_init.clone()], []),
                                                  loss="nll", nll_scale=(0.5, 0.5, 0.5)))
    finally:
        engine.set_training_backend(None)
    print("nll per step:", losses)
    assert all(l == l for l in losses) and losses[-1] < losses[0]


def test_the_training_loss_is_the_log_score_that_evaluation_reports():
    """Train on what you evaluate: on the filtered sets of an evaluation run's history, ``particle_set_nll`` with a fixed scale
    is ``-belief_density(truth, bandwidth=scale)``'s ``log_score``.  The recorded log-likelihoods are brought within 5 nats of
    each other first, so that no weight rule of the summaries matters."""
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
    ll = h.log_likelihoods
    h.log_likelihoods = (ll - ll.amax(-1, keepdim=True)).clamp_min(-5.0).contiguous()
    truth = traj["states"][1:].to(dev).contiguous()
    f.belief_density(truth, bandwidth=SCALE)
    want = -f.last_density.log_score
    engine.set_training_backend("hip")
    try:
        got = train.particle_set_nll(h.states, h.log_weights_in + h.log_likelihoods, truth, SCALE)
    finally:
        engine.set_training_backend(None)
    assert got.shape == want.shape == (T, N) and bool(torch.isfinite(want).all())
    err = rel_err_elementwise(got, want, floor=1e-3)
    print("particle_set_nll against -log_score:", err, "values", float(want.min()), float(want.max()))
    assert err < REL_TOL

"""The belief record -- per-step posterior covariance, effective sample size and log-evidence written by the native loops
(``record_belief`` / ``last_belief``; ``include/mmf.h``: ``mmf_pf_reweight_resample_belief``, ``MmfPfLoopArgs.cov_steps``,
``mmf_ekf_forward_loop_belief``) -- against fp64 references, its own invariants, itself across the execution forms (bit for
bit) and the CPU oracle.  Bar: ``tests/_tol.py`` (1e-4 of every matrix's own Frobenius norm)."""
import warnings

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import models as om
from oracle.tf.base import ReplayNoise

from _tol import REL_TOL, rel_err


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")


def _moments64(a, x):
    """fp64 reference: ``a (N, M)`` unnormalised log-weights, ``x (N, M, d)`` -> covariance, ess, log-evidence."""
    a, x = a.double(), x.double()
    lev = torch.logsumexp(a, dim=1)
    w = torch.exp(a - lev[:, None])
    mu = torch.sum(w[:, :, None] * x, dim=1)
    dx = x - mu[:, None, :]
    return torch.einsum("nm,nmi,nmj->nij", w, dx, dx), 1.0 / torch.sum(w * w, dim=1), lev


def _k1(mode, alpha, ll, lw, xs, u, M_out, record):
    from multimodalfilter_amd import _abi

    N, M, d = xs.shape
    dev = xs.device
    E = lambda *s, dt=torch.float32: torch.empty(s, dtype=dt, device=dev)
    est = E(N, d)
    so = E(N, M_out, d) if mode != 0 else None
    need_lw = mode == 0 or alpha < 1.0 or lw is not None
    lo = E(N, M_out) if need_lw else None
    idx = E(N, M_out, dt=torch.int32) if mode != 0 else None
    cov, ess, lev = (E(N, d, d), E(N), E(N)) if record else (None, None, None)
    _abi.pf_reweight_resample_belief(ll, lw, xs, u, est, so, lo, idx, mode, alpha, cov=cov, ess=ess, log_evidence=lev,
                                     M_out=M_out)
    torch.cuda.synchronize()
    return est, so, lo, idx, cov, ess, lev


# (label, mode, alpha, non-uniform logw_in): mode 1 / alpha 1 is the search-free kernel (M <= 20,000 and its LDS fits), the
# others -- and M = 20,000 -- the CDF-search kernel
_VARIANTS = [("systematic-uniform", 1, 1.0, False), ("systematic-weighted", 1, 1.0, True), ("none", 0, 1.0, True),
             ("multinomial", 2, 1.0, True), ("soft", 1, 0.5, True)]
# every variant at every M of the sweep, and M_out != M once (plain systematic resampling; mode 0 has no M_out)
_K1_CASES = [v + (M, M) for v in _VARIANTS for M in (300, 4096, 20000)] + [_VARIANTS[0] + (4096, 1000)]


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("label,mode,alpha,weighted,M,M_out", _K1_CASES, ids=[f"{c[0]}-{c[4]}-{c[5]}" for c in _K1_CASES])
def test_k1_record_against_fp64(label, mode, alpha, weighted, M, M_out, d):
    """One trajectory per (cloud width, log-likelihood scale) of {1e-3, 1e-2, 0.3} x {0.5, 5, 50} around an O(1) mean -- ESS
    from ~M/2 down to 1 --: ``cov``, ``ess``, ``log_evidence`` against numpy-style fp64 from the same fp32 inputs, and the
    estimate / survivors / ancestors of the recording call bit-identical to the non-recording one.  A raw-moment kernel
    (``E[x x^T] - mu mu^T`` in fp32) fails this by orders of magnitude at width 1e-3."""
    _need_gpu()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * d + M + mode)
    widths, scales = (1e-3, 1e-2, 0.3), (0.5, 5.0, 50.0)
    N = len(widths) * len(scales)
    width = torch.tensor([w for w in widths for _ in scales])
    scale = torch.tensor([s for _ in widths for s in scales])
    mean = torch.randn((N, 1, d), generator=g) + torch.sign(torch.randn((N, 1, d), generator=g))
    xs = (mean + width[:, None, None] * torch.randn((N, M, d), generator=g)).float()
    ll = (scale[:, None] * torch.randn((N, M), generator=g)).float()
    lw = torch.log_softmax(torch.randn((N, M), generator=g), dim=1).float() if weighted else None
    u = torch.rand((N,) if mode == 1 else (N, M_out), generator=g).float() if mode != 0 else None
    to = lambda t: None if t is None else t.to(dev).contiguous()
    args = (mode, alpha, to(ll), to(lw), to(xs), to(u), M_out)
    got = _k1(*args, record=True)
    ref = _k1(*args, record=False)
    for name, a, b in zip(("estimate", "states_out", "logw_out", "indices"), got[:4], ref[:4]):
        assert (a is None) == (b is None) and (a is None or torch.equal(a, b)), f"{name} changed by recording"
    a64 = ll.double() + (lw.double() if weighted else -np.log(float(M)))
    cov64, ess64, lev64 = _moments64(a64, xs)
    cov, ess, lev = (t.cpu() for t in got[4:])
    errs = rel_err(cov, cov64), rel_err(ess, ess64, dims=1), rel_err(lev, lev64, dims=1)
    print(f"{label} M={M} d={d}: cov {errs[0]:.2e} ess {errs[1]:.2e} log_evidence {errs[2]:.2e}; "
          f"ess range {float(ess64.min()):.2f} .. {float(ess64.max()):.1f}")
    assert errs[0] <= REL_TOL, f"covariance rel err {errs[0]:.3e}"
    assert errs[1] <= 1e-4 and errs[2] <= 1e-4, errs
    # ess and log_evidence are scalars per trajectory: every ONE of them, not only the batch's norm
    assert float(((ess - ess64).abs() / ess64).max()) <= 1e-4
    assert float(((lev - lev64).abs() / lev64.abs().clamp_min(1e-3 * float(lev64.abs().max()))).max()) <= 1e-4
    # properties: symmetric bit for bit, positive semi-definite to -1e-4 x trace, 1 <= ess <= M
    assert torch.equal(cov, cov.transpose(-1, -2))
    eig = torch.linalg.eigvalsh(cov.double())
    assert bool((eig.min(dim=-1).values >= -1e-4 * torch.diagonal(cov.double(), dim1=-2, dim2=-1).sum(-1)).all())
    assert bool((ess >= 1.0 - 1e-6).all()) and bool((ess <= M * (1.0 + 1e-6)).all())


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M", [300, 4096])
def test_k1_record_uniform_and_collapsed_weights(mode, M):
    """Uniform weights: ``ess == M`` to 1e-6 relative, ``log_evidence`` = the common log-likelihood.  One particle holding all
    the weight (the others ``-inf``): ``ess == 1`` and the zero matrix, exactly."""
    _need_gpu()
    dev = torch.device("cuda:0")
    N, d = 4, 3
    g = torch.Generator().manual_seed(M + mode)
    xs = (1.0 + 0.01 * torch.randn((N, M, d), generator=g)).to(dev)
    u = None if mode == 0 else torch.rand((N,) if mode == 1 else (N, M), generator=g).to(dev)
    lw = torch.full((N, M), -float(np.log(M)), device=dev)
    ll = torch.full((N, M), -1.25, device=dev)
    *_, cov, ess, lev = _k1(mode, 1.0, ll, lw, xs, u, M, record=True)
    assert float((ess / M - 1.0).abs().max()) <= 1e-6
    # (-log M - 1.25) + log(M): a handful of fp32 roundings at the size of the largest intermediate -- eight ulps of it
    assert float((lev + 1.25).abs().max()) <= 8 * 2.0 ** -23 * (np.log(M) + 1.25)
    cov64, _, _ = _moments64((ll + lw).cpu(), xs.cpu())
    assert rel_err(cov.cpu(), cov64) <= REL_TOL
    ll = torch.full((N, M), -float("inf"), device=dev)
    holder = torch.tensor([0, 1, M // 2, M - 1], device=dev)
    ll[torch.arange(N, device=dev), holder] = torch.tensor([0.0, -3.0, 2.5, 40.0], device=dev)
    est, *_, cov, ess, lev = _k1(mode, 1.0, ll, lw, xs, u, M, record=True)
    assert torch.equal(ess, torch.ones_like(ess)) and torch.equal(cov, torch.zeros_like(cov))
    assert torch.equal(est, xs[torch.arange(N, device=dev), holder])
    want = ll[torch.arange(N, device=dev), holder].double() - np.log(M)
    assert float((lev.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


# --------------------------------------------------------------------------------------------- forms agree bit for bit
def _same_record(a, b, what):
    assert (a is None) == (b is None), what
    if a is None:
        return
    assert vars(a).keys() == vars(b).keys(), what
    for k in vars(a):
        assert torch.equal(getattr(a, k), getattr(b, k)), f"{what}: {k} differs"


def _stacked(records):
    from multimodalfilter_amd import base

    return base.stack_belief_records(records)


@pytest.mark.parametrize("resample,T,alpha,method", [
    (False, 3, 1.0, "weighted_average"), (False, 4, 1.0, "weighted_average"), (True, 1, 1.0, "weighted_average"),
    (True, 4, 1.0, "weighted_average"), (True, 4, 0.5, "weighted_average"), (True, 3, 0.7, "argmax"),
    (True, 4, 1.0, "argmax"), (False, 3, 1.0, "argmax")])
def test_pf_record_of_stepwise_forward_loop_of_launches_and_persistent_launch_agree(resample, T, alpha, method):
    """The parameter sets of ``test_native_step_loop_equals_stepwise``: ``last_belief`` after T ``forward`` calls (stacked),
    after the loop of launches and -- where the loop is eligible -- after the persistent launch are the same bits; the
    estimates with recording on are the estimates with recording off."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    d, N, M = 3, 5, 300
    g = torch.Generator().manual_seed(23)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1).to(dev),
           "gripper_pos": torch.randn((T, N, 3), generator=g).to(dev),
           "gripper_sensors": torch.randn((T, N, 7), generator=g).to(dev)}
    ctrl = torch.randn((T, N, 7), generator=g).to(dev)
    x0 = torch.randn((N, d), generator=g).to(dev)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev)
    eps0 = torch.randn((N, M, d), generator=g).to(dev)
    eps = torch.randn((T, N, M, d), generator=g).to(dev)
    us = torch.rand((T, N), generator=g).to(dev)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval()
    f.num_particles, f.resample = M, resample
    f.soft_resample_alpha, f.estimation_method = alpha, method

    def start(record):
        f.record_belief = record
        f.noise = mmf.StackedNoise(eps0, eps, us)
        f.initialize_beliefs(mean=x0, covariance=cov)

    start(True)
    step, records = [], []
    for t in range(T):
        step.append(f(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]))
        assert f.last_belief.covariance.shape == (N, d, d) and f.last_belief.ess.shape == (N,)
        records.append(f.last_belief)
    step, records = torch.stack(step), _stacked(records)

    taken = []
    real = _abi.pf_forward_loop
    _abi.pf_forward_loop = lambda a, *r, **k: (taken.append(int(a.persistent)), real(a, *r, **k))[1]
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*persistent.*")  # a give-up warns
            with engine.persistent_forms(pf=False):
                start(True)
                launches = f.forward_loop(observations=obs, controls=ctrl)
                rec_launches = f.last_belief
                start(False)
                plain = f.forward_loop(observations=obs, controls=ctrl)
                assert f.last_belief is None
            with engine.persistent_forms(pf=True):
                start(True)
                persistent = f.forward_loop(observations=obs, controls=ctrl)
                rec_persistent = f.last_belief
                assert engine.PF_PERSISTENT  # (a give-up switches it off)
    finally:
        _abi.pf_forward_loop = real
    eligible = resample and alpha == 1.0 and method == "weighted_average" and _abi.pf_persistent_plan(N, M, 2) > 0
    assert taken == [0, 0, 1 if eligible else 0], taken  # recording does not change which form runs
    assert resample is False or alpha < 1.0 or method == "argmax" or eligible, "5 x 300 must be eligible on a whole MI355X"
    assert rec_launches.covariance.shape == (T, N, d, d) and rec_launches.log_evidence.shape == (T, N)
    assert torch.equal(launches, step) and torch.equal(plain, step) and torch.equal(persistent, step)
    _same_record(rec_launches, records, "loop of launches against stepwise forward")
    _same_record(rec_persistent, records, "second loop against stepwise forward")
    # and they are what the definition says (fp64 from the particles is test 4's business; here: sane)
    assert bool(torch.isfinite(records.covariance).all()) and bool((records.ess >= 1.0 - 1e-6).all())
    assert bool((records.ess <= M * (1.0 + 1e-6)).all())


@pytest.mark.parametrize("cls,N,M,T,precision,noise", [
    ("DoorCrossmodalParticleFilter", 32, 300, 9, "f16x3", "tensor"),
    ("DoorCrossmodalParticleFilter", 32, 300, 6, "f32", "tensor"),
    ("PushCrossmodalParticleFilter", 7, 300, 5, "f16x3", "philox"),
    ("DoorUnimodalParticleFilter", 3, 1000, 4, "f16x3", "tensor"),
    ("DoorParticleFilter", 5, 77, 5, "f16x3", "tensor"),
    ("DoorCrossmodalParticleFilterSeq5", 6, 2048, 3, "f16x3", "philox"),
    ("DoorCrossmodalParticleFilter", 32, 2048, 4, "f16x3", "tensor"),
    ("DoorCrossmodalParticleFilter", 24, 3000, 3, "f32", "philox"),
    ("PushCrossmodalParticleFilter", 24, 3328, 3, "f16x3", "philox"),
])
def test_pf_record_of_persistent_launch_equals_loop_of_launches(cls, N, M, T, precision, noise):
    """The parameter sets of ``test_persistent_step_loop_equals_loop_of_launches`` (both arithmetic modes, both noise
    sources, non-uniform incoming weights, K1's 512 threads standing for up to 1024): the record of ONE persistent launch
    and of the loop of launches are the same bits, the recording run really is the persistent launch (the C call is made
    with ``persistent`` set, the plan is positive, nothing gave up), and recording leaves the estimates alone."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine, synthetic

    dev = torch.device("cuda:0")
    tname = "door" if cls.startswith("Door") else "push"
    d = om.TASKS[tname].state_dim
    old_prec = engine.DEFAULT_PRECISION
    engine.set_default_precision(precision)
    try:
        torch.manual_seed(3)
        f = mmf.model_types(tname)[cls]().to(dev).eval()
        f.num_particles = M
        traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(
            state_dim=d, T=T + 1, N=N, seed=17, image_blackout_ratio=0.4 if cls.endswith("Seq5") else 0.0).items()}
        obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
        ctrl = traj["controls"][1:]
        cov = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
        g = torch.Generator(device=dev).manual_seed(5)
        eps0 = torch.randn((N, M, d), generator=g, device=dev)
        eps = torch.randn((T + 1, N, M, d), generator=g, device=dev)
        us = torch.rand((T + 1, N), generator=g, device=dev)

        def run(record):
            taken = []
            real = _abi.pf_forward_loop
            _abi.pf_forward_loop = lambda a, *r, **k: (taken.append((int(a.persistent), int(a.n_meas))), real(a, *r, **k))[1]
            try:
                f.record_belief = record
                f.noise = mmf.CounterNoise(99) if noise == "philox" else mmf.StackedNoise(eps0, eps, us)
                f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
                f.resample = False  # one step WITHOUT resampling first: the loop then starts from non-uniform log-weights
                first = f.forward_loop(observations={k: v[:1] for k, v in obs.items()}, controls=ctrl[:1])
                rec_first = f.last_belief
                f.resample = None
                a = f.forward_loop(observations={k: v[1:] for k, v in obs.items()}, controls=ctrl[1:])
                return taken, first, a, rec_first, f.last_belief
            finally:
                _abi.pf_forward_loop = real

        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*persistent.*")
            with engine.persistent_forms(pf=False):
                ref = run(True)
            with engine.persistent_forms(pf=True):
                got = run(True)
                assert engine.PF_PERSISTENT, "the persistent launch gave up"
                off = run(False)
        n_meas = got[0][1][1]
        assert _abi.pf_persistent_plan(N, M, n_meas) > 0
        assert [p for p, _ in ref[0]] == [0, 0] and [p for p, _ in got[0]] == [0, 1], (ref[0], got[0])
        assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2])
        assert torch.equal(off[1], got[1]) and torch.equal(off[2], got[2]) and off[3] is None and off[4] is None
        _same_record(ref[3], got[3], "no-resampling step")
        _same_record(ref[4], got[4], "persistent launch against loop of launches")
        assert got[4].covariance.shape == (got[2].shape[0], N, d, d) and got[2].shape[0] >= T - 1
        assert bool(torch.isfinite(got[4].covariance).all())
        assert bool(torch.isfinite(got[4].log_evidence).all()) and bool((got[4].ess >= 1.0 - 1e-6).all())
    finally:
        engine.set_default_precision(old_prec)


def _kalman_stepwise_and_loops(f, obs, ctrl, x0, cov, T):
    """(estimates, stacked stepwise record, per-step public covariance) of T ``forward`` calls with recording on."""
    f.record_belief = True
    f.initialize_beliefs(mean=x0, covariance=cov)
    step, records, public = [], [], []
    for t in range(T):
        step.append(f(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]))
        records.append(f.last_belief)
        if hasattr(f, "filter_models"):
            live = [m for m, on in zip(f.filter_models, f.enabled_models) if on]
            wc = getattr(f, "weighted_covariances", None)
            public.append(wc.clone() if wc is not None else live[0]._belief_covariance.clone())
        else:
            public.append(f.belief_covariance.clone())
    return torch.stack(step), _stacked(records), public


@pytest.mark.parametrize("cls,kw,masked", [
    ("DoorKalmanFilter", {}, False),
    ("PushKalmanFilter", {}, False),
    ("DoorCrossmodalKalmanFilter", {}, False),
    ("DoorCrossmodalKalmanFilter", {"feedback": "belief", "fix_weight_layout": True}, False),
    ("PushCrossmodalKalmanFilter", {}, True),
    ("DoorUnimodalKalmanFilter", {}, False),
    ("PushUnimodalKalmanFilter", {}, True),
    ("DoorCrossmodalKalmanFilter", {"know_image_blackout": True}, False),
    ("DoorCrossmodalKalmanFilter", {"know_image_blackout": True, "feedback": "belief"}, False),
    ("PushCrossmodalKalmanFilter", {"know_image_blackout": True, "feedback": "belief", "fix_weight_layout": True}, False),
    ("DoorCrossmodalKalmanFilter", {"know_image_blackout": True}, True),
])
def test_ekf_record_of_stepwise_forward_and_both_loops_agree(cls, kw, masked):
    """The parameter sets of ``test_native_ekf_loop_equals_stepwise`` (fusion weights, precision fusion, one enabled
    sub-filter, the blackout gate with and without write-back): ``last_belief.covariance[t]`` of the loop of launches and of
    the persistent launch is, bit for bit, the covariance a stepwise run shows after step ``t`` -- the fused one
    (``weighted_covariances``) where the filter publishes it, the only sub-filter's ``belief_covariance`` where nothing is
    fused -- and recording leaves the estimates alone."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    tname = "door" if cls.startswith("Door") else "push"
    d, N, T = om.TASKS[tname].state_dim, 7, 5
    g = torch.Generator().manual_seed(31)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1).to(dev),
           "gripper_pos": torch.randn((T, N, 3), generator=g).to(dev),
           "gripper_sensors": torch.randn((T, N, 7), generator=g).to(dev)}
    ctrl = torch.randn((T, N, 7), generator=g).to(dev)
    x0 = torch.randn((N, d), generator=g).to(dev)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev)
    if kw.get("know_image_blackout"):
        obs["image"][1, 2] = 0.0
        obs["image"][3, 0] = 0.0
        obs["image"][3, 5] = 0.0
    f = mmf.model_types(tname)[cls](**kw).to(dev).eval()
    if masked:
        f.enabled_models = [False, True]
    step, records, public = _kalman_stepwise_and_loops(f, obs, ctrl, x0, cov, T)
    assert records.covariance.shape == (T, N, d, d)
    unimodal_fused = "Unimodal" in cls and not masked  # the information-form fusion publishes no covariance of its own
    if not unimodal_fused:
        for t in range(T):
            assert torch.equal(records.covariance[t], public[t]), f"step {t}: record is not the published covariance"

    taken = []
    real = _abi.ekf_forward_loop
    _abi.ekf_forward_loop = lambda a, *r, **k: (taken.append(int(a.persistent)), real(a, *r, **k))[1]
    try:
        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*persistent.*")
            out = {}
            for form in (False, True):
                with engine.persistent_forms(ekf=form):
                    f.record_belief = True
                    f.initialize_beliefs(mean=x0, covariance=cov)
                    out[form] = (f.forward_loop(observations=obs, controls=ctrl), f.last_belief)
                    assert engine.EKF_PERSISTENT == form
            f.record_belief = False
            f.initialize_beliefs(mean=x0, covariance=cov)
            plain = f.forward_loop(observations=obs, controls=ctrl)
            assert f.last_belief is None
    finally:
        _abi.ekf_forward_loop = real
    K = sum(bool(on) for on in f.enabled_models) if hasattr(f, "filter_models") else 1
    assert taken[:2] == [0, 1 if _abi.ekf_persistent_plan(N, K) > 0 else 0], taken  # recording does not change which form runs
    for form in (False, True):
        assert torch.equal(out[form][0], step)
        _same_record(out[form][1], records, "persistent launch" if form else "loop of launches")
    assert torch.equal(plain, step)


@pytest.mark.parametrize("cls,kw,N,T,precision", [
    ("DoorCrossmodalKalmanFilter", {}, 37, 6, "f16x3"),
    ("DoorCrossmodalKalmanFilter", {"know_image_blackout": True, "feedback": "belief"}, 1027, 5, "f16x3"),
    ("DoorCrossmodalKalmanFilter", {"feedback": "belief", "fix_weight_layout": True}, 64, 4, "f32"),
    ("PushCrossmodalKalmanFilter", {}, 200, 4, "f16x3"),
    ("DoorUnimodalKalmanFilter", {}, 32, 7, "f16x3"),
    ("DoorKalmanFilter", {}, 100, 5, "f16x3"),
    ("DoorCrossmodalKalmanFilter", {}, 4096 + 5, 3, "f16x3"),
])
def test_ekf_record_of_persistent_launch_equals_loop_of_launches(cls, kw, N, T, precision):
    """The parameter sets of ``test_persistent_ekf_loop_equals_loop_of_launches``: per-step covariances of the ONE persistent
    launch (stored from the registers that hold them) and of the 2 T launches are the same bits; estimates unchanged."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, engine

    dev = torch.device("cuda:0")
    tname = "door" if cls.startswith("Door") else "push"
    d = om.TASKS[tname].state_dim
    old_prec = engine.DEFAULT_PRECISION
    engine.set_default_precision(precision)
    try:
        torch.manual_seed(5)
        g = torch.Generator().manual_seed(41)
        obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1).to(dev),
               "gripper_pos": torch.randn((T, N, 3), generator=g).to(dev),
               "gripper_sensors": torch.randn((T, N, 7), generator=g).to(dev)}
        ctrl = torch.randn((T, N, 7), generator=g).to(dev)
        x0 = torch.randn((N, d), generator=g).to(dev)
        cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev)
        if kw.get("know_image_blackout"):
            obs["image"][1, 2] = 0.0
            obs["image"][3, N - 1] = 0.0
        f = mmf.model_types(tname)[cls](**kw).to(dev).eval()

        def run(record):
            taken = []
            real = _abi.ekf_forward_loop
            _abi.ekf_forward_loop = lambda a, *r, **k: (taken.append(int(a.persistent)), real(a, *r, **k))[1]
            try:
                f.record_belief = record
                f.initialize_beliefs(mean=x0, covariance=cov)
                a = f.forward_loop(observations=obs, controls=ctrl)
                rec_a = f.last_belief
                b = f.forward_loop(observations={k: v[:2] for k, v in obs.items()}, controls=ctrl[:2])
                return taken, a, b, rec_a, f.last_belief
            finally:
                _abi.ekf_forward_loop = real

        with warnings.catch_warnings():
            warnings.filterwarnings("error", message=".*persistent.*")
            with engine.persistent_forms(ekf=False):
                ref = run(True)
            with engine.persistent_forms(ekf=True):
                got = run(True)
                assert engine.EKF_PERSISTENT, "the persistent launch gave up"
                off = run(False)
        K = len(f.filter_models) if hasattr(f, "filter_models") else 1
        assert _abi.ekf_persistent_plan(N, K) > 0
        assert ref[0] == [0, 0] and got[0] == [1, 1], (ref[0], got[0])
        assert torch.equal(ref[1], got[1]) and torch.equal(ref[2], got[2])
        assert torch.equal(off[1], got[1]) and torch.equal(off[2], got[2]) and off[3] is None
        _same_record(ref[3], got[3], "first loop")
        _same_record(ref[4], got[4], "second loop")
        assert got[3].covariance.shape == (T, N, d, d) and got[4].covariance.shape == (2, N, d, d)
        assert bool(torch.isfinite(got[3].covariance).all())
        # the last step's record is the belief the loop left
        wc = getattr(f, "weighted_covariances", None)
        if wc is not None:
            assert torch.equal(got[4].covariance[-1], wc)
        elif K == 1:
            assert torch.equal(got[4].covariance[-1], f.belief_covariance)
    finally:
        engine.set_default_precision(old_prec)


def test_ukf_record_is_the_stepwise_belief_covariance():
    """The unscented filter's loop is driven from Python: its record is the per-step ``belief_covariance``, stacked."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import filters

    dev = torch.device("cuda:0")
    d, N, T = 3, 6, 4
    g = torch.Generator().manual_seed(77)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1).to(dev),
           "gripper_pos": torch.randn((T, N, 3), generator=g).to(dev),
           "gripper_sensors": torch.randn((T, N, 7), generator=g).to(dev)}
    ctrl = torch.randn((T, N, 7), generator=g).to(dev)
    x0 = torch.randn((N, d), generator=g).to(dev)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev)
    torch.manual_seed(9)
    ekf = mmf.door_models.DoorKalmanFilter()
    f = filters.VirtualSensorUnscentedKalmanFilter(dynamics_model=ekf.dynamics_model,
                                                   virtual_sensor_model=ekf.virtual_sensor_model).to(dev).eval()
    assert f.record_belief is False and f.last_belief is None
    step, _, public = _kalman_stepwise_and_loops(f, obs, ctrl, x0, cov, T)
    f.initialize_beliefs(mean=x0, covariance=cov)
    loop = f.forward_loop(observations=obs, controls=ctrl)
    assert torch.equal(loop, step) and f.last_belief.covariance.shape == (T, N, d, d)
    for t in range(T):
        assert torch.equal(f.last_belief.covariance[t], public[t])
    f.record_belief = False
    f.initialize_beliefs(mean=x0, covariance=cov)
    assert torch.equal(f.forward_loop(observations=obs, controls=ctrl), step) and f.last_belief is None


# --------------------------------------------------------------------------------------------- against the oracle
@pytest.mark.parametrize("tname,cls", [("door", "DoorCrossmodalParticleFilter"), ("push", "PushCrossmodalParticleFilter")])
def test_particle_filter_record_tracks_oracle(tname, cls):
    """Whole crossmodal particle filters, T = 8, N = 4, M = 256, the oracle's weights and pre-drawn noise as
    ``test_particle_filter_tracks_oracle`` builds them.  The oracle filter is subclassed here to keep the weighted set it
    resamples FROM; covariance / ESS / log-evidence of that set in fp64 are the reference.  Teacher-forced: step ``t`` of the
    engine starts from the oracle's belief of step ``t - 1`` (an ancestor that lands on the other side of a CDF boundary
    hinges on the last ulp of a log-likelihood -- VERDICT N1 -- and would move every later step by ~1 / M).  With
    ``MMF_PRECISION=f32`` the engine is ALSO run free through ``forward_loop``; its steps are compared for as long as its
    ancestors are the oracle's (at least the first)."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine as mmf_engine

    dev = torch.device("cuda:0")
    task = om.TASKS[tname]
    d, N, M, T = task.state_dim, 4, 256, 8
    g = torch.Generator().manual_seed(11)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1),
           "gripper_pos": torch.randn((T, N, 3), generator=g),
           "gripper_sensors": torch.randn((T, N, 7), generator=g)}
    ctrl = torch.randn((T, N, 7), generator=g)
    x0 = torch.randn((N, d), generator=g)
    eps0 = torch.randn((N, M, d), generator=g)
    eps = [torch.randn((N, M, d), generator=g) for _ in range(T)]
    us = [torch.rand((N,), generator=g) for _ in range(T)]

    class Keeping(om.ParticleFilter):
        def _resample(self):
            self.kept.append((self.particle_states.clone(), self.particle_log_weights.clone()))
            super()._resample()

    oracle = Keeping(task, "crossmodal", resample_mode="systematic")
    oracle.kept = []
    oracle.load_state_dict(om.seeded_state_dict(oracle, seed=3, gain=1.0))
    oracle.eval()
    oracle.num_particles = M
    oracle.noise = ReplayNoise([eps0] + eps, us)
    cov0 = (torch.eye(d) * 0.1)[None].expand(N, d, d)
    beliefs, loglik_sums, anc = [], [], []
    with torch.no_grad():
        oracle.initialize_beliefs(mean=x0, covariance=cov0)
        for t in range(T):
            beliefs.append((oracle.particle_states, oracle.particle_log_weights))
            oracle(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t])
            anc.append(oracle.last_resample_indices.clone())
    want_cov, want_ess = [], []
    for states, logw in oracle.kept:  # logw is normalised: its logsumexp is 0, the evidence comes from the step's likelihoods
        c, e, _ = _moments64(logw, states)
        want_cov.append(c)
        want_ess.append(e)
    want_cov, want_ess = torch.stack(want_cov), torch.stack(want_ess)

    eng = mmf.model_types(tname)[cls]()
    eng.load_state_dict(oracle.state_dict())
    eng.to(dev).eval()
    eng.num_particles = M
    eng.record_belief = True
    eng.record_indices = True
    eng.noise = mmf.ReplayNoise([eps0], [])
    eng.initialize_beliefs(mean=x0.to(dev), covariance=cov0.to(dev))
    got_cov, got_ess, got_lev, want_lev = [], [], [], []
    for t in range(T):
        eng.particle_states = beliefs[t][0].to(dev).contiguous()
        eng.particle_log_weights = beliefs[t][1].to(dev).contiguous()
        eng._spare_states = None
        eng.noise = mmf.ReplayNoise([eps[t]], [us[t]])
        eng(observations={k: v[t].to(dev) for k, v in obs.items()}, controls=ctrl[t].to(dev))
        got_cov.append(eng.last_belief.covariance.cpu())
        got_ess.append(eng.last_belief.ess.cpu())
        got_lev.append(eng.last_belief.log_evidence.cpu())
        # the oracle's evidence increment: logsumexp(logw_in + loglik), with ITS log-likelihoods = normalised - in + const;
        # recomputed from the oracle's measurement model on the oracle's propagated particles
        with torch.no_grad():
            ll = oracle.measurement_model(states=oracle.kept[t][0], observations={k: v[t] for k, v in obs.items()})
        want_lev.append(torch.logsumexp(beliefs[t][1].double() + ll.double(), dim=1))
    got_cov, got_ess, got_lev, want_lev = (torch.stack(x) for x in (got_cov, got_ess, got_lev, want_lev))
    errs = rel_err(got_cov, want_cov), rel_err(got_ess, want_ess, dims=1), rel_err(got_lev, want_lev, dims=1)
    print(f"{cls} teacher-forced ({mmf_engine.DEFAULT_PRECISION}): cov {errs[0]:.2e} ess {errs[1]:.2e} log_evidence {errs[2]:.2e}")
    assert errs[0] <= REL_TOL, f"covariance rel err {errs[0]:.3e}"
    assert errs[1] <= REL_TOL and errs[2] <= REL_TOL, errs

    if mmf_engine.DEFAULT_PRECISION == "f32":
        eng.noise = mmf.ReplayNoise([eps0] + eps, us)
        eng.initialize_beliefs(mean=x0.to(dev), covariance=cov0.to(dev))
        eng.forward_loop(observations={k: v.to(dev) for k, v in obs.items()}, controls=ctrl.to(dev))
        same = (eng.last_resample_indices.cpu().long() == torch.stack(anc)).flatten(1).all(dim=1)
        upto = T if bool(same.all()) else int(torch.nonzero(~same)[0]) + 1  # the step that drew another ancestor still started equal
        free = rel_err(eng.last_belief.covariance[:upto].cpu(), want_cov[:upto])
        print(f"{cls} free-running f32: {upto} of {T} steps comparable, cov {free:.2e}")
        assert upto >= 1 and free <= REL_TOL, (upto, free)


@pytest.mark.parametrize("tname,cls,okw", [
    ("door", "DoorKalmanFilter", {}),
    ("door", "DoorCrossmodalKalmanFilter", {}),
    ("push", "PushCrossmodalKalmanFilter", {"feedback": "belief", "fix_weight_layout": True}),
    ("push", "PushUnimodalKalmanFilter", {}),
    ("door", "DoorUnimodalKalmanFilter", {}),
])
def test_kalman_filter_record_tracks_oracle(tname, cls, okw):
    """The cases of ``test_kalman_filters_track_oracle`` (N = 32, T = 6): the per-step posterior covariance of the native loop
    against the oracle's EKF stepped on the CPU -- its ``belief_covariance`` / ``weighted_covariances`` after every step, and
    for the information-form fusion (which the oracle computes but does not keep) the oracle's own formula on its
    sub-filters' covariances.  (Neither key of ``_tol.REFERENCE_FP32_GAP`` is among these cases.)"""
    _need_gpu()
    import multimodalfilter_amd as mmf

    dev = torch.device("cuda:0")
    task = om.TASKS[tname]
    d, N, T = task.state_dim, 32, 6
    g = torch.Generator().manual_seed(5)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1),
           "gripper_pos": torch.randn((T, N, 3), generator=g),
           "gripper_sensors": torch.randn((T, N, 7), generator=g)}
    ctrl = torch.randn((T, N, 7), generator=g)
    x0 = torch.randn((N, d), generator=g)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d)
    oracle = om.build(cls, **okw)
    oracle.load_state_dict(om.seeded_state_dict(oracle, seed=4, gain=1.0))
    oracle.eval()
    want, want_cov = [], []
    with torch.no_grad():
        oracle.initialize_beliefs(mean=x0, covariance=cov)
        for t in range(T):
            want.append(oracle(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]))
            if "Unimodal" in cls:
                prec = torch.stack([torch.inverse(m._belief_covariance + 1e-9) for m in oracle.filter_models])
                want_cov.append(torch.inverse(torch.sum(prec, dim=0) + 1e-9))
            elif hasattr(oracle, "filter_models"):
                want_cov.append(oracle.weighted_covariances.clone())
            else:
                want_cov.append(oracle.belief_covariance.clone())
    eng = mmf.model_types(tname)[cls](**okw)
    eng.load_state_dict(oracle.state_dict())
    eng.to(dev).eval()
    eng.record_belief = True
    eng.initialize_beliefs(mean=x0.to(dev), covariance=cov.to(dev))
    got = eng.forward_loop(observations={k: v.to(dev) for k, v in obs.items()}, controls=ctrl.to(dev))
    assert rel_err(got, torch.stack(want)) < REL_TOL
    err = rel_err(eng.last_belief.covariance, torch.stack(want_cov))
    print(f"{cls}: per-step covariance rel err {err:.2e}")
    assert err <= REL_TOL, f"per-step covariance rel err {err:.3e}"


def test_run_filter_returns_the_record_and_the_metrics_take_it():
    """``evaluation.run_filter(..., return_belief=True)`` and the calibration metrics on device tensors, end to end."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import evaluation, synthetic

    dev = torch.device("cuda:0")
    N, T, d = 6, 40, 3
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=d, T=T + 1, N=N, seed=3).items()}
    torch.manual_seed(1)
    for f in (mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval(), mmf.door_models.DoorCrossmodalKalmanFilter().to(dev).eval()):
        plain = evaluation.run_filter(f, traj)
        if hasattr(f, "noise"):
            f.noise = type(f.noise)(0)  # same draws again
            plain = evaluation.run_filter(f, traj)
            f.noise = type(f.noise)(0)
        est, belief = evaluation.run_filter(f, traj, return_belief=True)
        assert torch.equal(est, plain) and f.record_belief is False
        assert belief.covariance.shape == (est.shape[0], N, d, d) and est.shape[0] >= T
        true = traj["states"][1:]
        jitter = 1e-9 * torch.eye(d, device=dev)
        nll = evaluation.gaussian_nll(est, belief.covariance + jitter, true)
        cvr = evaluation.coverage(est, belief.covariance + jitter, true, 0.95)
        assert nll.shape == (N,) and cvr.shape == (N,) and bool(torch.isfinite(nll).all())
        assert bool(((cvr >= 0) & (cvr <= 1)).all())
        assert evaluation.nees(est, belief.covariance + jitter, true).shape == (est.shape[0] - evaluation.START_TRUNCATION, N)


@pytest.mark.parametrize("backend", ["autograd", "hip"])
def test_training_paths_fill_the_record_with_torch_ops(backend):
    """``train()`` with a training backend: the record comes from detached torch reductions of the particle tensors (fp64),
    step by step -- here against the same reductions made by hand from the belief the step leaves (no resampling while
    training: the belief IS the weighted set), and for the EKF against its ``belief_covariance``; gradients still flow."""
    _need_gpu()
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine

    dev = torch.device("cuda:0")
    d, N, M, T = 3, 4, 30, 3
    g = torch.Generator().manual_seed(3)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1).to(dev),
           "gripper_pos": torch.randn((T, N, 3), generator=g).to(dev),
           "gripper_sensors": torch.randn((T, N, 7), generator=g).to(dev)}
    ctrl = torch.randn((T, N, 7), generator=g).to(dev)
    x0 = torch.randn((N, d), generator=g).to(dev)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d).to(dev)
    engine.set_training_backend(backend)
    try:
        torch.manual_seed(2)
        f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).train()
        f.num_particles, f.record_belief = M, True
        f.initialize_beliefs(mean=x0, covariance=cov)
        est = f.forward_loop(observations=obs, controls=ctrl)
        assert est.requires_grad and f.last_belief.covariance.shape == (T, N, d, d)
        assert not f.last_belief.covariance.requires_grad
        c64, e64, _ = _moments64(f.particle_log_weights.detach().cpu(), f.particle_states.detach().cpu())
        assert rel_err(f.last_belief.covariance[-1].cpu(), c64) <= REL_TOL
        assert rel_err(f.last_belief.ess[-1].cpu(), e64, dims=1) <= REL_TOL
        assert bool(torch.isfinite(f.last_belief.log_evidence).all())
        est.sum().backward()
        k = mmf.door_models.DoorKalmanFilter().to(dev).train()
        k.record_belief = True
        k.initialize_beliefs(mean=x0, covariance=cov)
        out = k.forward_loop(observations=obs, controls=ctrl)
        assert out.requires_grad and k.last_belief.covariance.shape == (T, N, d, d)
        assert torch.equal(k.last_belief.covariance[-1], k.belief_covariance.detach())
    finally:
        engine.set_training_backend(None)

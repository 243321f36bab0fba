"""Innovation statistics and the NIS gate of the Kalman filters on the GPU: ``mmf_ekf_step_innov`` (``csrc/ekf.hip``,
``csrc/ekf_algebra.h``) and ``mmf_ekf_forward_loop_innov`` (``csrc/ekf_loop.hip``) against fp64, bit for bit against the
entry points they extend, and through ``forward`` / ``forward_loop`` / ``evaluation`` of every Kalman filter, on the inputs
``_innovation_cases.py`` builds and ``test_innovation_cases_cpu.py`` certifies.

The error rule is the project's: ``_tol.rel_err(kernel, fp64) < max(1e-4, 3 x _tol.rel_err(fp32 yardstick, fp64))`` -- for the
fusion outputs never above ``GPU_BAR_CEILING``.  The NIS and the log-likelihood are scalars per row: each is held against
``max(|its own value|, 1e-3 of the batch's largest)``.  Every output buffer carries ``GUARD_ROWS`` sentinel rows past its end,
which must come back bit-unchanged.  Each figure is printed before it is asserted (``pytest -s`` shows them)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _innovation_cases as ic
import _kalman_cases as kc
import _tol

INT_SENTINEL = -77


def _dev():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X (run with -m gpu on the GPU box)")
    return torch.device("cuda:0")


def _abi():
    from multimodalfilter_amd import _abi

    _abi.load()
    return _abi


def _d(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _bits(t):
    return t.contiguous().view(torch.int32)


class _Out:
    """An output buffer of ``lead`` rows of shape ``tail`` followed by ``GUARD_ROWS`` guard rows, all filled with the
    sentinel (``init``: the in/out operand's input); ``dtype=torch.int32``: the integer sentinel."""

    def __init__(self, lead, tail=(), init=None, dtype=torch.float32):
        self.rows = int(np.prod(lead))
        self.fill = kc.SENTINEL if dtype == torch.float32 else INT_SENTINEL
        self.full = torch.full((self.rows + kc.GUARD_ROWS,) + tuple(tail), self.fill, device=_dev(), dtype=dtype)
        self.t = self.full[:self.rows].view(tuple(lead) + tuple(tail))
        if init is not None:
            self.t.copy_(init)

    def guard_intact(self):
        g = self.full[self.rows:]
        return torch.equal(_bits(g), _bits(torch.full_like(g, self.fill)))

    def untouched(self):
        return torch.equal(_bits(self.full), _bits(torch.full_like(self.full, self.fill)))


def _raw(name, *args):
    """The C entry point itself (tensors -> device pointers, None -> null, current stream appended)."""
    import ctypes

    abi = _abi()
    conv = [abi.ptr(a, dtype=a.dtype) if isinstance(a, torch.Tensor) else a for a in args]
    conv = [ctypes.c_float(a) if isinstance(a, float) else a for a in conv]
    with torch.cuda.device(_dev()):
        return getattr(abi.load(), name)(*conv, torch.cuda.current_stream().cuda_stream)


def _col(t):
    return torch.as_tensor(t).detach().cpu()[..., None]


def _hold(tag, name, got, truth, yardstick, ceiling=None, dims=None):
    """Print, then assert, ``rel_err(got, fp64) < max(1e-4, 3 rel_err(yardstick, fp64))`` (at most ``ceiling``)."""
    assert bool(torch.isfinite(torch.as_tensor(got)).all()), (tag, name, "not finite")
    err, ref = _tol.rel_err(got, truth, dims), _tol.rel_err(yardstick, truth, dims)
    bar = max(_tol.REL_TOL, 3.0 * ref)
    if ceiling is not None:
        bar = min(bar, ceiling)
    print(f"INNOV {tag} what={name} kernel={err:.3e} fp32={ref:.3e} bar={bar:.3e}")
    assert err < bar, (tag, name, err, ref)


# ------------------------------------------------------------------------------ A: the step kernel
def _step(N, d, K, fusion, gate, want=("nis", "loglik", "accepted"), entry="innov"):
    """One launch on ``ic.step_case(N, d, K)``: ``entry="gated"`` -> ``mmf_ekf_step_gated`` (null gate word), else
    ``mmf_ekf_step_innov`` with NIS gate ``gate`` (``None``: -1, off) and the outputs named in ``want`` (the others null).
    Returns the guarded outputs by name."""
    c = ic.step_case(N, d, K)
    o = {"mu": _Out((K, N), (d,)), "Sigma": _Out((K, N), (d, d), init=_d(c["S0"])), "mu_f": _Out((N,), (d,)), "Sigma_f": _Out((N,), (d, d)),
         "nis": _Out((K, N)), "loglik": _Out((K, N)), "accepted": _Out((K, N), dtype=torch.int32)}
    args = [_d(c["A"]), _d(c["mu_pred"]), _d(c["L"]), _d(c["z"]), _d(c["T"]), _d(c["w"]) if fusion == 1 else None,
            o["mu"].t, o["Sigma"].t, o["mu_f"].t if fusion else None, o["Sigma_f"].t if fusion else None, N, d, K, fusion, 0, None]
    if entry == "gated":
        assert _raw("mmf_ekf_step_gated", *args) == 0
    else:
        extra = [o[k].t if k in want else None for k in ("nis", "loglik", "accepted")]
        assert _raw("mmf_ekf_step_innov", *args, -1.0 if gate is None else float(gate), *extra) == 0
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("d", ic.DIMS)
@pytest.mark.parametrize("K,fusion", ic.STEP_COMBOS)
@pytest.mark.parametrize("N", ic.NS)
def test_innovation_step_against_fp64_and_against_the_plain_step(N, K, fusion, d):
    """Gate off: all four belief outputs are the bits of ``mmf_ekf_step_gated`` and ``accepted`` is all 1.  Gate 12: the
    decisions are the fp64 ones exactly, accepted rows keep the ungated bits, rejected rows of ``mu`` are ``mu_pred`` bit
    for bit, and the NIS, the log-likelihood (recorded for rejected rows too, the same bits with and without the gate),
    the rejected rows of ``Sigma`` and the fused outputs meet the error rule against fp64.  Guard rows survive, outputs
    that were not asked for are not written, and the belief does not depend on which records are asked for."""
    tag = f"N={N} d={d} K={K} fusion={fusion}"
    c = ic.step_case(N, d, K)
    beliefs = ("mu", "Sigma", "mu_f", "Sigma_f")
    plain = _step(N, d, K, fusion, None, entry="gated")
    free = _step(N, d, K, fusion, None)
    for k in beliefs:
        assert torch.equal(free[k].full, plain[k].full), (tag, k)
    assert bool((free["accepted"].t == 1).all())
    t64, t32 = ic.step_reference(N, d, K, fusion, torch.float64), ic.step_reference(N, d, K, fusion, torch.float32)
    _hold(tag, "nis", _col(free["nis"].t), _col(t64["nis"]), _col(t32["nis"]), dims=1)
    _hold(tag, "log_likelihood", _col(free["loglik"].t), _col(t64["log_likelihood"]), _col(t32["log_likelihood"]), dims=1)

    gated = _step(N, d, K, fusion, ic.GATE)
    g64, g32 = (ic.step_reference(N, d, K, fusion, dt, ic.GATE) for dt in (torch.float64, torch.float32))
    acc = gated["accepted"].t.cpu()
    assert bool(((acc == 0) | (acc == 1)).all())
    assert torch.equal(acc == 1, g64["accepted"]), tag
    assert np.array_equal((acc == 0).numpy(), c["outlier"])
    assert torch.equal(gated["nis"].full, free["nis"].full) and torch.equal(gated["loglik"].full, free["loglik"].full)
    ok, rej = (acc == 1).to(_dev()), (acc == 0).to(_dev())
    assert torch.equal(gated["mu"].t[ok], free["mu"].t[ok]) and torch.equal(gated["Sigma"].t[ok], free["Sigma"].t[ok])
    assert torch.equal(gated["mu"].t[rej], _d(c["mu_pred"])[rej]), tag
    if bool(rej.any()):
        r = acc == 0
        _hold(tag, "Sigma[rejected]", gated["Sigma"].t[rej].cpu(), g64["Sigma"][r], g32["Sigma"][r])
        assert not torch.equal(gated["Sigma"].t[rej], free["Sigma"].t[rej])
    _hold(tag, "mu", gated["mu"].t.cpu(), g64["mu"], g32["mu"])
    _hold(tag, "Sigma", gated["Sigma"].t.cpu(), g64["Sigma"], g32["Sigma"])
    if fusion:
        _hold(tag, "mu_f", gated["mu_f"].t.cpu(), g64["mu_f"], g32["mu_f"], ceiling=kc.GPU_BAR_CEILING)
        _hold(tag, "Sigma_f", gated["Sigma_f"].t.cpu(), g64["Sigma_f"], g32["Sigma_f"], ceiling=kc.GPU_BAR_CEILING)
        if N >= 255:  # a rejected sub-filter enters the fusion with its prediction: another fused belief
            assert not torch.equal(gated["mu_f"].t, free["mu_f"].t)
    for o in (plain, free, gated):
        for k, buf in o.items():
            assert buf.guard_intact(), (tag, k)
            if not fusion and k in ("mu_f", "Sigma_f"):
                assert buf.untouched(), (tag, k)
    # null outputs are honoured: nothing is written there and the belief is the same
    for want in ((), ("accepted",), ("nis", "loglik")):
        some = _step(N, d, K, fusion, ic.GATE, want=want)
        for k in beliefs:
            assert torch.equal(some[k].full, gated[k].full), (tag, want, k)
        for k in ("nis", "loglik", "accepted"):
            if k in want:
                assert torch.equal(some[k].full, gated[k].full), (tag, want, k)
            else:
                assert some[k].untouched(), (tag, want, k)


def test_innovation_step_feedback_and_the_gate_word():
    """With write-back (``feedback = 1``) every sub-filter leaves the step with the fused belief of the GATED sub-filter
    beliefs, and the feedback gate word still switches the write-back off: the bits of the ``feedback = 0`` call."""
    N, d, K = 257, 3, 3
    c = ic.step_case(N, d, K)
    dev = _dev()

    def run(feedback, word):
        mu, Sigma = _Out((K, N), (d,)), _Out((K, N), (d, d), init=_d(c["S0"]))
        mu_f, Sigma_f, acc = _Out((N,), (d,)), _Out((N,), (d, d)), _Out((K, N), dtype=torch.int32)
        assert _raw("mmf_ekf_step_innov", _d(c["A"]), _d(c["mu_pred"]), _d(c["L"]), _d(c["z"]), _d(c["T"]), _d(c["w"]), mu.t, Sigma.t,
                    mu_f.t, Sigma_f.t, N, d, K, 1, feedback, word, float(ic.GATE), None, None, acc.t) == 0
        torch.cuda.synchronize()
        return mu, Sigma, mu_f, Sigma_f, acc

    off = run(0, None)
    on = run(1, None)
    for k in range(K):
        assert torch.equal(on[0].t[k], on[2].t) and torch.equal(on[1].t[k], on[3].t)
    assert torch.equal(on[2].full, off[2].full) and torch.equal(on[4].full, off[4].full)
    held = run(1, torch.zeros(1, dtype=torch.int32, device=dev))
    for a, b in zip(held, off):
        assert torch.equal(a.full, b.full)
    for o in on + off:
        assert o.guard_intact()


def test_innovation_step_reports_a_matrix_that_is_not_positive_definite():
    """An innovation covariance that is not positive definite (a negative prior covariance) has no log-determinant: the
    log-likelihood is NaN for that row alone, the others are what they were."""
    N, d, K = 5, 2, 1
    c = ic.step_case(1, d, K)
    rep = lambda k: _d(c[k]).expand((K, N) + tuple(c[k].shape[2:])).contiguous()
    S0 = rep("S0")
    S0[0, 3] = -4.0 * torch.eye(d, device=_dev())
    mu, nis, ll = _Out((K, N), (d,)), _Out((K, N)), _Out((K, N))
    assert _raw("mmf_ekf_step_innov", rep("A"), rep("mu_pred"), _d(c["L"]), rep("z"), rep("T"), None, mu.t, S0, None, None,
                N, d, K, 0, 0, None, -1.0, nis.t, ll.t, None) == 0
    torch.cuda.synchronize()
    bad = torch.isnan(ll.t[0]).cpu()
    assert bad.tolist() == [False, False, False, True, False]
    assert torch.equal(ll.t[0, 0], ll.t[0, 4]) and nis.guard_intact() and ll.guard_intact()


# ------------------------------------------------------------------------------ B: the door task's filters, loop and steps
def _door(cls, seed=7, T=4, N=3):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

    dev = _dev()
    torch.manual_seed(seed)
    f = mmf.model_types("door")[cls]().to(dev).eval()
    traj = {k: v.to(dev) for k, v in synthetic.make_trajectories(state_dim=3, T=T, N=N, seed=3).items()}
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    cov = (torch.eye(3, device=dev) * 0.1)[None].expand(N, 3, 3)
    return f, traj, obs, traj["controls"][1:], cov


def _same_record(a, b):
    assert a.sub_filters == b.sub_filters
    for k in ("nis", "log_likelihood", "accepted"):
        x, y = getattr(a, k), getattr(b, k)
        assert x.shape == y.shape and x.dtype == y.dtype and torch.equal(x, y), k


@pytest.mark.parametrize("cls,K", [("DoorKalmanFilter", None), ("DoorCrossmodalKalmanFilter", 2), ("DoorUnimodalKalmanFilter", 2)])
def test_forward_loop_records_innovations_without_changing_a_bit(cls, K):
    """``T = 4``, ``N = 3``, randomly initialised.  With ``record_innovations`` the estimates and ``last_belief`` (keys and
    bits) are those of the loop without it, under the default form and under ``persistent_forms(ekf=False)``; the record
    has the stated shapes and dtypes and is the stack of the records of ``T`` single ``forward`` calls from the same
    initial belief; the persistent launch is not taken while recording; the gate alone leaves the record too; and with one
    sub-filter disabled ``K`` shrinks."""
    from multimodalfilter_amd import _abi, engine

    T, N = 4, 3
    f, traj, obs, ctrl, cov = _door(cls, T=T, N=N)
    lead = (T, N) if K is None else (T, K, N)

    def loop(record, gate=None, persistent=None):
        f.record_innovations, f.innovation_gate, f.record_belief = record, gate, True
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        seen = []
        real = _abi.ekf_forward_loop
        _abi.ekf_forward_loop = lambda a, *r, **k: (seen.append((int(a.persistent), k.get("innov") is not None)), real(a, *r, **k))[1]
        try:
            with engine.persistent_forms(ekf=persistent):
                est = f.forward_loop(observations=obs, controls=ctrl)
        finally:
            _abi.ekf_forward_loop = real
        assert len(seen) == 1, "the task's Kalman filters take the native loop"
        return est, f.last_belief, f.last_innovations, seen[0]

    def steps(record, gate=None):
        f.record_innovations, f.innovation_gate, f.record_belief = record, gate, True
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov)
        est, recs = [], []
        for t in range(T):
            est.append(f(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]))
            recs.append(f.last_innovations)
        return torch.stack(est), recs

    for persistent in (None, False):
        plain, belief, none, _ = loop(False, persistent=persistent)
        assert none is None
        est, belief_r, rec, (was_persistent, innov) = loop(True, persistent=persistent)
        assert innov and was_persistent == 0
        assert torch.equal(est, plain)
        assert sorted(vars(belief_r)) == sorted(vars(belief)) == ["covariance"]
        assert torch.equal(belief_r.covariance, belief.covariance)
        assert rec.nis.shape == rec.log_likelihood.shape == rec.accepted.shape == lead and rec.sub_filters == K
        assert rec.nis.dtype == rec.log_likelihood.dtype == torch.float32 and rec.accepted.dtype == torch.bool
        assert bool(rec.accepted.all()) and bool(torch.isfinite(rec.nis).all()) and bool(torch.isfinite(rec.log_likelihood).all())
        assert bool((rec.nis >= 0).all())
    est_s, recs = steps(True)
    assert torch.equal(est_s, plain)
    assert all(r.nis.shape == lead[1:] for r in recs)
    _same_record(rec, f._stack_innovation_records(recs))
    assert steps(False)[1] == [None] * T

    # the gate alone: the record is left, measurements are rejected, and loop and steps still agree bit for bit
    gate = float(rec.nis[0].median())  # (of the first step, which the gate has not yet changed: both classes are there)
    est_g, _, rec_g, (_, innov) = loop(False, gate=gate)
    assert innov and rec_g is not None and rec_g.nis.shape == lead
    assert torch.equal(rec_g.accepted, rec_g.nis <= gate) and bool((~rec_g.accepted[0]).any()) and bool(rec_g.accepted[0].any())
    assert torch.equal(rec_g.nis[0], rec.nis[0]) and not torch.equal(est_g, plain)
    est_gs, recs_g = steps(False, gate=gate)
    assert torch.equal(est_gs, est_g)
    _same_record(rec_g, f._stack_innovation_records(recs_g))

    if K is not None:  # one sub-filter disabled: K shrinks
        f.enabled_models = [False, True]
        plain1 = loop(False)[0]
        est1, _, rec1, _ = loop(True)
        assert torch.equal(est1, plain1) and rec1.nis.shape == (T, 1, N) and rec1.sub_filters == 1
        _same_record(rec1, f._stack_innovation_records(steps(True)[1]))
        f.enabled_models = [True, True]
    f.record_innovations, f.innovation_gate, f.record_belief = False, None, False
    assert loop(False)[2] is None


# ------------------------------------------------------------------------------ C: a linear-Gaussian model, user-model path and UKF
@pytest.mark.parametrize("displaced", [False, True])
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_linear_gaussian_loop_against_the_fp64_filter_and_the_dense_density(kind, displaced):
    """``lg_model(2)`` as user models (the Python loop of steps) through the extended filter and through the unscented
    one, whose transform is exact on a linear model: estimates, NIS, log-likelihood and decisions against the fp64 numpy
    filter -- ungated, and with gate 12 on the copy whose four displaced observations must be exactly the rejected ones --
    and the summed log-likelihood against the dense joint density of all observations (no recursion).  The yardstick is
    the same filter in float32 numpy."""
    from multimodalfilter_amd import filters

    dev = _dev()
    d = ic.LG_D
    c = ic.lg_case(displaced)
    yard = ic.kalman_filter(d, c["y"], c["gate"], np.float32, np.array(c["accepted"]))
    dyn, sensor = ic.rc.lg_filter_models(d, dev)
    cls = filters.VirtualSensorExtendedKalmanFilter if kind == "ekf" else filters.VirtualSensorUnscentedKalmanFilter
    f = cls(dynamics_model=dyn, virtual_sensor_model=sensor).to(dev).eval()
    y, u, m0 = (ic._t(c[k], torch.float32).to(dev) for k in ("y", "u", "m_init"))
    P0 = ic._t(c["P_init"], torch.float32).to(dev)[None].expand(ic.LG_N, d, d)
    f.initialize_beliefs(mean=m0, covariance=P0)
    plain = f.forward_loop(observations=y, controls=u)
    assert f.last_innovations is None
    f.record_innovations, f.innovation_gate = True, c["gate"]
    f.initialize_beliefs(mean=m0, covariance=P0)
    est = f.forward_loop(observations=y, controls=u)
    r = f.last_innovations
    tag = f"lg {kind} displaced={displaced}"
    assert r.nis.shape == r.log_likelihood.shape == r.accepted.shape == (ic.LG_T, ic.LG_N) and r.sub_filters is None
    assert np.array_equal(r.accepted.cpu().numpy(), c["accepted"]), tag
    if displaced:
        assert sorted(map(tuple, torch.nonzero(~r.accepted).cpu().tolist())) == sorted(ic.DISPLACED)
        assert not torch.equal(est, plain)
    else:
        assert torch.equal(est, plain) and bool(r.accepted.all())
    T = lambda a: torch.from_numpy(np.array(a))
    _hold(tag, "estimates", est.cpu(), T(c["mean"]), T(yard["mean"]))
    _hold(tag, "covariance", f.belief_covariance.cpu(), T(c["cov"][-1]), T(yard["cov"][-1]))
    _hold(tag, "nis", _col(r.nis), _col(T(c["nis"])), _col(T(yard["nis"])), dims=1)
    _hold(tag, "log_likelihood", _col(r.log_likelihood), _col(T(c["log_likelihood"])), _col(T(yard["log_likelihood"])), dims=1)
    if not displaced:
        dense = T(ic.dense_log_density(d, np.array(c["y"])))
        summed = r.log_likelihood.double().sum(0).cpu()
        _hold(tag, "sum_t log_likelihood vs dense", _col(summed), _col(dense), _col(T(yard["log_likelihood"]).double().sum(0)), dims=1)
    # step by step: the same record
    f.initialize_beliefs(mean=m0, covariance=P0)
    recs = []
    for t in range(ic.LG_T):
        f(observations=y[t], controls=u[t])
        recs.append(f.last_innovations)
        assert recs[-1].nis.shape == (ic.LG_N,)
    _same_record(r, f._stack_innovation_records(recs))


# ------------------------------------------------------------------------------ D: evaluation
def test_run_filter_summary_and_fit_process_noise_with_log_likelihood():
    from multimodalfilter_amd import evaluation

    T, N, d = 12, 5, 3
    f, traj, _, _, _ = _door("DoorKalmanFilter", seed=11, T=T, N=N)
    plain = evaluation.run_filter(f, traj)
    assert f.last_innovations is None
    est, rec = evaluation.run_filter(f, traj, return_innovations=True)
    assert torch.equal(est, plain) and rec.nis.shape == (T, N) and rec.accepted.dtype == torch.bool
    assert f.record_innovations is False and f.innovation_gate is None
    est, belief, rec2 = evaluation.run_filter(f, traj, return_belief=True, return_innovations=True)
    assert torch.equal(est, plain) and belief.covariance.shape == (T, N, d, d)
    _same_record(rec, rec2)
    assert f.record_innovations is False and f.record_belief is False
    s = evaluation.innovation_summary(rec, d)
    assert sorted(s) == ["accepted_fraction", "log_likelihood", "mean_nis", "nis_over_dim"]
    assert all(v.dim() == 0 and bool(torch.isfinite(v)) for v in s.values())
    assert float(s["accepted_fraction"]) == 1.0 and float(s["mean_nis"]) > 0
    assert abs(float(s["log_likelihood"]) - float(rec.log_likelihood.double().sum())) < 1e-9 * abs(float(s["log_likelihood"]))

    f.innovation_gate = float(rec.nis[0].median())  # a switch the caller set stays as the caller set it
    est_g, rec_g = evaluation.run_filter(f, traj, return_innovations=True)
    assert f.innovation_gate == float(rec.nis[0].median()) and f.record_innovations is False
    sg = evaluation.innovation_summary(rec_g, d)
    assert 0.0 < float(sg["accepted_fraction"]) < 1.0
    want = float(rec_g.log_likelihood.double()[rec_g.accepted].sum())
    assert abs(float(sg["log_likelihood"]) - want) < 1e-9 * abs(want)
    f.innovation_gate = None

    fused, _, _, _, _ = _door("DoorCrossmodalKalmanFilter", seed=11, T=T, N=N)
    _, rec_f = evaluation.run_filter(fused, traj, return_innovations=True)
    assert rec_f.nis.shape == (T, 2, N) and rec_f.sub_filters == 2
    sf = evaluation.innovation_summary(rec_f, d)
    assert all(v.shape == (2,) and bool(torch.isfinite(v).all()) for v in sf.values())
    assert torch.allclose(sf["log_likelihood"], rec_f.log_likelihood.double().sum(dim=(0, 2)))

    # EM with its likelihood: the default return is unchanged, the second list has one entry per factor
    twin, _, _, _, _ = _door("DoorKalmanFilter", seed=11, T=T, N=N)
    factors = evaluation.fit_process_noise(twin, traj, iterations=2)
    assert isinstance(factors, list) and len(factors) == 3
    got = evaluation.fit_process_noise(f, traj, iterations=2, return_log_likelihood=True)
    assert isinstance(got, tuple) and len(got) == 2
    factors_l, logliks = got
    assert len(factors_l) == 3 and all(torch.equal(a, b) for a, b in zip(factors_l, factors))
    assert len(logliks) == 2 + 1 and all(isinstance(v, float) and np.isfinite(v) for v in logliks)
    assert abs(logliks[0] - float(s["log_likelihood"])) <= 1e-6 * abs(logliks[0])  # the first factor is the untouched model
    print("INNOV EM log-likelihoods", logliks)
    assert f.record_innovations is False and f.innovation_gate is None
    assert f.record_history is False and f.record_belief is False and f.record_transition_moments is False

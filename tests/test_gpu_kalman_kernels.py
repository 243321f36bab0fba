"""The Kalman kernels (``csrc/ekf.hip``, ``csrc/ekf_algebra.h``, ``csrc/ukf.hip``) where they pivot, cancel and run off a block,
through the C ABI, on the inputs ``_kalman_cases.py`` builds and ``test_kalman_cases_cpu.py`` certifies.

The error rule is that of ``test_k3_matches_oracle_algebra``:
``_tol.rel_err(kernel, fp64) < max(1e-4, 3 x _tol.rel_err(fp32 torch, fp64))`` -- for the fusion outputs and the mode-2
fused-sensor matrix never above 5e-3 (the fp32 reference itself is capped at 1.7e-3 there by the CPU test).  Every output
buffer carries ``GUARD_ROWS`` sentinel rows past its end, which must come back bit-unchanged.  Each figure is printed before it
is asserted (``pytest -s`` shows them; ``profiles/kalman_kernels/README.md`` holds those of one MI355X run)."""

import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import _kalman_cases as kc
from _guarded_gpu import Out as _Out, abi as _abi, bits as _bits, dev as _dev, hold, raw as _raw


def _d(a):
    return torch.from_numpy(np.array(a)).to(_dev())


_hold = functools.partial(hold, "KALMAN")


# ------------------------------------------------------------------------------ A: mmf_ekf_step
def _step(N, d, K, fusion, feedback=0, gate="ungated"):
    """One launch on ``step_case(N, d, K)``; ``gate``: "ungated" -> ``mmf_ekf_step``, a tensor or None -> that gate word
    on ``mmf_ekf_step_gated``.  Returns the four guarded outputs."""
    c = kc.step_case(N, d, K)
    mu, Sigma = _Out((K, N), (d,)), _Out((K, N), (d, d), init=_d(c["S0"]))
    mu_f, Sigma_f = _Out((N,), (d,)), _Out((N,), (d, d))
    args = [_d(c["A"]), _d(c["mu_pred"]), _d(c["L"]), _d(c["z"]), _d(c["T"]), _d(c["w"]) if fusion == 1 else None,
            mu.t, Sigma.t, mu_f.t if fusion else None, Sigma_f.t if fusion else None, N, d, K, fusion, feedback]
    if isinstance(gate, str):
        assert _raw("mmf_ekf_step", *args) == 0
    else:
        assert _raw("mmf_ekf_step_gated", *args, gate) == 0
    torch.cuda.synchronize()
    return mu, Sigma, mu_f, Sigma_f


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("K,fusion", kc.STEP_COMBOS)
@pytest.mark.parametrize("N", kc.NS)
def test_ekf_step_on_the_pivot_family(N, K, fusion, d):
    """Group A: predict + correct and both fusions where the innovation inverse swaps rows (every pattern of d = 2, 3,
    every comparison both ways of d = 4), ``q_tril`` different per k, K up to ``kMaxK``, N around the 256-lane block."""
    c = kc.step_case(N, d, K)
    assert K == 1 or not np.array_equal(c["L"][0], c["L"][1])
    mu, Sigma, mu_f, Sigma_f = _step(N, d, K, fusion)
    truth = kc.step_reference(N, d, K, fusion, torch.float64)
    fp32 = kc.step_reference(N, d, K, fusion, torch.float32)
    tag = f"N={N} d={d} K={K} fusion={fusion}"
    _hold("A", tag, "mu", mu.t.cpu(), truth[0], fp32[0])
    _hold("A", tag, "Sigma", Sigma.t.cpu(), truth[1], fp32[1])
    # Sigma is in/out: every matrix was really overwritten
    assert bool((Sigma.t.cpu() != torch.from_numpy(np.array(c["S0"]))).flatten(2).any(-1).all())
    if fusion:
        _hold("A", tag, "mu_f", mu_f.t.cpu(), truth[2], fp32[2], ceiling=kc.GPU_BAR_CEILING)
        _hold("A", tag, "Sigma_f", Sigma_f.t.cpu(), truth[3], fp32[3], ceiling=kc.GPU_BAR_CEILING)
    else:
        assert mu_f.untouched() and Sigma_f.untouched()
    for o in (mu, Sigma, mu_f, Sigma_f):
        assert o.guard_intact()


# ------------------------------------------------------------------------------ B: mmf_ekf_step_gated
@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("fusion", [1, 2])
def test_ekf_step_gate_word(fusion, d):
    """Group B: with feedback = 1, gate word 0 is the feedback = 0 call and a nonzero or null gate is the ungated
    feedback = 1 call, bit for bit in all four outputs."""
    N, K = 257, 3
    dev = _dev()
    plain0 = _step(N, d, K, fusion, feedback=0)
    plain1 = _step(N, d, K, fusion, feedback=1)
    assert not torch.equal(plain0[0].t, plain1[0].t)      # the write-back changes the sub-filter beliefs
    for k in range(K):
        assert torch.equal(plain1[0].t[k], plain1[2].t) and torch.equal(plain1[1].t[k], plain1[3].t)
    for gate, want in ((torch.zeros(1, dtype=torch.int32, device=dev), plain0),
                       (torch.full((1,), 5, dtype=torch.int32, device=dev), plain1), (None, plain1)):
        got = _step(N, d, K, fusion, feedback=1, gate=gate)
        for g, w in zip(got, want):
            assert torch.equal(g.full, w.full), (fusion, d, None if gate is None else int(gate))
    # the gate never switches the write-back ON
    got = _step(N, d, K, fusion, feedback=0, gate=torch.full((1,), 5, dtype=torch.int32, device=dev))
    for g, w in zip(got, plain0):
        assert torch.equal(g.full, w.full)


# ------------------------------------------------------------------------------ C: mmf_ekf_step_backward
_BWD_N, _BWD_K = 257, 3
_BWD_OUT = ("g_A", "g_mu_pred", "g_z", "g_r_tril", "g_Sigma_in")


def _backward(d, g_mu="case", g_Sigma="case", skip=None):
    """``mmf_ekf_step_backward`` on ``step_case(257, d, 3)``; ``g_mu`` / ``g_Sigma``: "case", "zeros" or None (null);
    ``skip``: the output passed as null.  Returns name -> guarded output (None where skipped)."""
    N, K = _BWD_N, _BWD_K
    c = kc.step_case(N, d, K)

    def grad(which, how):
        if how is None:
            return None
        return _d(c[which]) if how == "case" else torch.zeros(c[which].shape, device=_dev())

    shapes = {"g_A": (d, d), "g_mu_pred": (d,), "g_z": (d,), "g_r_tril": (d, d), "g_Sigma_in": (d, d)}
    outs = {n: (None if n == skip else _Out((K, N), shapes[n])) for n in _BWD_OUT}
    _abi().ekf_step_backward(_d(c["A"]), _d(c["mu_pred"]), _d(c["L"]), _d(c["z"]), _d(c["T"]), _d(c["S0"]),
                             grad("g_mu", g_mu), grad("g_Sigma", g_Sigma),
                             *[None if outs[n] is None else outs[n].t for n in _BWD_OUT])
    torch.cuda.synchronize()
    return outs


def _largest_entry_err(got, want):
    return float((got.double() - want.double()).abs().max()) / max(1e-6, float(want.abs().max()))


@pytest.mark.parametrize("d", kc.DIMS)
def test_ekf_step_backward_with_three_sub_filters(d):
    """Group C: K = 3 with three different ``q_tril`` (picked by ``row / N``) on the pivot family, against fp64 autograd
    through the reference algebra: 1e-4 of the largest entry (the measure of
    ``test_k6_ekf_step_function_matches_fp64_autograd``), or three times fp32 autograd's own error where that misses 1e-4."""
    c = kc.step_case(_BWD_N, d, _BWD_K)
    assert not np.array_equal(c["L"][0], c["L"][1]) and not np.array_equal(c["L"][1], c["L"][2])
    outs = _backward(d)
    want = kc.step_gradients(_BWD_N, d, _BWD_K, torch.float64)
    fp32 = kc.step_gradients(_BWD_N, d, _BWD_K, torch.float32)
    for name, w, f in zip(_BWD_OUT, want, fp32):
        got = outs[name].t.cpu()
        assert bool(torch.isfinite(got).all()), name
        err, ref = _largest_entry_err(got, w), _largest_entry_err(f, w)
        print(f"KALMAN group=C N={_BWD_N} d={d} K={_BWD_K} what={name} kernel={err:.3e} fp32={ref:.3e}")
        assert err < max(1e-4, 3.0 * ref), (name, err, ref)
        assert outs[name].guard_intact(), name


@pytest.mark.parametrize("d", kc.DIMS)
def test_ekf_step_backward_null_arguments(d):
    """Group C: a null ``g_mu`` / ``g_Sigma`` is a zero gradient, bit for bit; every output nulled in turn leaves the
    other four bit-identical."""
    full = _backward(d)
    for kw in ({"g_mu": None}, {"g_Sigma": None}):
        null = _backward(d, **kw)
        zeros = _backward(d, **{k: "zeros" for k in kw})
        for n in _BWD_OUT:
            assert torch.equal(null[n].full, zeros[n].full), (kw, n)
        assert not torch.equal(null["g_A"].t, full["g_A"].t)          # ... and that gradient did matter
    for skip in _BWD_OUT:
        part = _backward(d, skip=skip)
        for n in _BWD_OUT:
            if n != skip:
                assert torch.equal(part[n].full, full[n].full), (skip, n)


# ------------------------------------------------------------------------------ D: mmf_fuse_virtual_sensors
@pytest.mark.parametrize("d", kc.SENSOR_DIMS)
@pytest.mark.parametrize("K", kc.SENSOR_KS)
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("N", kc.NS)
def test_fuse_virtual_sensors(N, mode, K, d):
    """Group D: both modes against ``oracle/models.py``'s formulas in fp64.  Mode 2 (quirk Q5) inverts a matrix whose upper
    triangle is 1e9 K, so that inversion pivots, and its result has entries up to ~1e3; K = 1 is the ``z_0``, ``T T^T``
    special case."""
    c = kc.sensor_case(N, d, K)
    z_out, tril_out = _Out((N,), (d,)), _Out((N,), (d, d))
    _abi().fuse_virtual_sensors(_d(c["z"]), _d(c["T"]), _d(c["w"]) if mode == 1 else None, z_out.t, tril_out.t, mode)
    torch.cuda.synchronize()
    z64, t64, _ = kc.sensor_reference(N, d, K, mode, torch.float64)
    z32, t32, _ = kc.sensor_reference(N, d, K, mode, torch.float32)
    tag = f"N={N} d={d} K={K} mode={mode}"
    _hold("D", tag, "z_out", z_out.t.cpu(), z64, z32)
    _hold("D", tag, "tril_out", tril_out.t.cpu(), t64, t32, ceiling=kc.GPU_BAR_CEILING if mode == 2 else None)
    if mode == 2 and K == 1:
        assert torch.equal(z_out.t.cpu(), torch.from_numpy(np.array(c["z"][0])))
    assert z_out.guard_intact() and tril_out.guard_intact()


# ------------------------------------------------------------------------------ E: mmf_ukf_sigma_points
def _sigma_points(mu, Sigma, scale, flag):
    N, d = mu.shape
    pts = _Out((N,), (2 * d + 1, d))
    not_pd = torch.full((1,), flag, dtype=torch.int32, device=_dev())
    _abi().ukf_sigma_points(_d(mu), _d(Sigma), scale, pts.t, not_pd)
    torch.cuda.synchronize()
    return pts, int(not_pd.item())


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("scale", kc.SIGMA_SCALES)
@pytest.mark.parametrize("N", kc.NS)
def test_ukf_sigma_points(N, scale, d):
    """Group E: covariances of condition number 1e3 at the scales of Julier's and of Merwe's default strategy, against
    ``torch.linalg.cholesky`` in fp64; each pair of points reflects about the mean to one ulp; an all-PD batch leaves
    the flag's other bits alone."""
    c = kc.belief_case(N, d)
    pts, flag = _sigma_points(c["mu"], c["Sigma"], scale, 2)
    assert flag == 2 and pts.guard_intact()
    got = pts.t.cpu()
    _hold("E", f"N={N} d={d} scale={scale:.3g}", "points", got, kc.sigma_points_reference(N, d, scale, torch.float64),
          kc.sigma_points_reference(N, d, scale, torch.float32))
    # the offsets themselves (point minus mean; forming the point cost at most half an ulp of it): the small scale hides
    # nothing behind the mean.  Same rule, on the largest offset.
    want, fp32 = (kc.sigma_points_reference(N, d, scale, dt) for dt in (torch.float64, torch.float32))
    off, off64, off32 = (p.double()[:, 1:] - p.double()[:, :1] for p in (got, want, fp32))
    top = float(off64.abs().max())
    err, ref = float((off - off64).abs().max()) / top, float((off32 - off64).abs().max()) / top
    print(f"KALMAN group=E N={N} d={d} scale={scale:.3g} what=offsets kernel={err:.3e} fp32={ref:.3e}")
    assert err < max(1e-4, 3.0 * ref)
    # fl(m + s) + fl(m - s) = 2m up to half an ulp of each point
    a, b, m = got[:, 1:1 + d].double(), got[:, 1 + d:].double(), got[:, :1].double()
    ulp = torch.from_numpy(np.spacing(np.maximum(np.abs(got[:, 1:1 + d].numpy()), np.abs(got[:, 1 + d:].numpy())))).double()
    assert bool(((a + b - 2.0 * m).abs() <= ulp).all())
    assert torch.equal(got[:, 0], torch.from_numpy(np.array(c["mu"])))


@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("scale", kc.SIGMA_SCALES)
def test_ukf_sigma_points_report_and_collapse_bad_covariances(scale, d):
    """Group E: a negative eigenvalue, the zero matrix and a NaN entry, one in each 256-block of N = 513: the flag gains
    bit 0 (2 -> 3), each bad row's points all equal its mean, and the good rows do not notice."""
    N = 513
    c = kc.belief_case(N, d)
    clean, _ = _sigma_points(c["mu"], c["Sigma"], scale, 2)
    Sigma = np.array(c["Sigma"])
    ev, V = np.linalg.eigh(Sigma[3].astype(np.float64))
    ev[-1] = -0.1
    Sigma[3] = ((V * ev) @ V.T).astype(np.float32)
    Sigma[300] = 0.0
    Sigma[512, d - 1, 0] = float("nan")      # lower triangle (the diagonal for d = 1): the part a Cholesky reads
    bad = [3, 300, 512]
    pts, flag = _sigma_points(c["mu"], Sigma, scale, 2)
    assert flag == 3 and pts.guard_intact()
    got, mu = pts.t.cpu(), torch.from_numpy(np.array(c["mu"]))
    assert torch.equal(got[bad], mu[bad][:, None, :].expand(-1, 2 * d + 1, -1))
    good = [n for n in range(N) if n not in bad]
    assert torch.equal(got[good], clean.t.cpu()[good])


# ------------------------------------------------------------------------------ F: mmf_ukf_moments
@pytest.mark.parametrize("d", kc.DIMS)
@pytest.mark.parametrize("strategy", kc.STRATEGY_NAMES)
@pytest.mark.parametrize("N", kc.NS)
def test_ukf_moments(N, strategy, d):
    """Group F: weighted moments of propagated sigma points (a mild nonlinearity, nonzero ``q_tril``) against fp64 with the
    strategy's weights as doubles.  Julier and Merwe at alpha = 0.5: the fp32 torch yardstick.  Merwe's DEFAULT, alpha =
    1e-2 (``wm0`` ~ -1e4, ``wi`` ~ 1.7e3): the yardstick is the fp32 evaluation about point 0 -- the weighted sum as written
    loses 3e-4 .. 8e-3 there, which is what the kernel did before it took its sums about ``x[0]``.  alpha = 1e-3 is beyond
    fp32 in either form (covariance off by 1e-2) and is not asserted."""
    c = kc.moments_case(N, d, strategy)
    wc0, wm0, wi = c["weights"]
    mu_pred, Sigma_pred = _Out((N,), (d,)), _Out((N,), (d, d))
    _abi().ukf_moments(_d(c["points"]), wm0, wc0, wi, _d(c["q_tril"]), mu_pred.t, Sigma_pred.t)
    torch.cuda.synchronize()
    m64, S64 = kc.moments_reference(N, d, strategy, torch.float64)
    if strategy == "merwe_default":
        m32, S32 = kc.moments_about_point0_fp32(N, d, strategy)
    else:
        m32, S32 = kc.moments_reference(N, d, strategy, torch.float32)
    tag = f"N={N} d={d} strategy={strategy}"
    _hold("F", tag, "mu_pred", mu_pred.t.cpu(), m64, m32)
    _hold("F", tag, "Sigma_pred", Sigma_pred.t.cpu(), S64, S32)
    assert mu_pred.guard_intact() and Sigma_pred.guard_intact()


# ------------------------------------------------------------------------------ N = 0 and argument errors
def test_zero_rows_succeed_and_write_nothing():
    """``N = 0`` returns success from all six entry points and leaves sentinel-filled outputs untouched."""
    d, K = 3, 2
    dev = _dev()
    x = torch.zeros((K, 4, d, d), device=dev)      # any valid device memory: N = 0 reads none of it
    gate = torch.ones(1, dtype=torch.int32, device=dev)
    flag = torch.full((1,), 2, dtype=torch.int32, device=dev)
    o = [_Out((K, 4), (d, d)) for _ in range(5)]
    assert _raw("mmf_ekf_step", x, x, x, x, x, x, o[0].t, o[1].t, o[2].t, o[3].t, 0, d, K, 1, 1) == 0
    assert _raw("mmf_ekf_step_gated", x, x, x, x, x, x, o[0].t, o[1].t, o[2].t, o[3].t, 0, d, K, 2, 1, gate) == 0
    assert _raw("mmf_ekf_step_backward", x, x, x, x, x, x, x, x, *[b.t for b in o], 0, d, K) == 0
    assert _raw("mmf_fuse_virtual_sensors", x, x, x, o[0].t, o[1].t, 0, d, K, 1) == 0
    assert _raw("mmf_fuse_virtual_sensors", x, x, None, o[0].t, o[1].t, 0, d, K, 2) == 0
    assert _raw("mmf_ukf_sigma_points", x, x, 1.5, o[0].t, flag, 0, d) == 0
    assert _raw("mmf_ukf_moments", x, -1.0, 1.0, 1.0 / d, x, o[0].t, o[1].t, 0, d) == 0
    torch.cuda.synchronize()
    assert all(b.untouched() for b in o) and int(flag.item()) == 2


def test_kalman_argument_errors():
    """Group G: refused before any launch (``MMF_EINVAL`` -> ``MmfError``), outputs untouched."""
    abi = _abi()
    dev = _dev()
    N, K = 5, 2

    def step_args(d=3, K=K):
        ins = [torch.zeros((K, N, d, d), device=dev), torch.zeros((K, N, d), device=dev), torch.zeros((K, d, d), device=dev),
               torch.zeros((K, N, d), device=dev), torch.eye(d, device=dev).expand(K, N, d, d).contiguous()]
        w = torch.ones((K, N, d), device=dev)
        outs = [_Out((K, N), (d,)), _Out((K, N), (d, d), init=torch.eye(d, device=dev).expand(K, N, d, d)),
                _Out((N,), (d,)), _Out((N,), (d, d))]
        return ins, w, outs

    def refused_step(ins, w, outs, present, fusion, gate=None):
        before = [o.full.clone() for o in outs]
        with pytest.raises(abi.MmfError):
            abi.ekf_step(*ins, w, outs[0].t, outs[1].t, outs[2].t if present[0] else None,
                         outs[3].t if present[1] else None, fusion=fusion, feedback=1, feedback_gate=gate)
        torch.cuda.synchronize()
        assert all(torch.equal(_bits(o.full), _bits(b)) for o, b in zip(outs, before))

    gate = torch.ones(1, dtype=torch.int32, device=dev)
    for g in (None, gate):                                              # both entry points
        ins, w, outs = step_args(d=5)
        refused_step(ins, w, outs, (True, True), 1, g)                  # d = 5
        ins, w, outs = step_args(K=5)
        refused_step(ins, w, outs, (True, True), 1, g)                  # K = 5 > kMaxK
        ins, w, outs = step_args()
        refused_step(ins, None, outs, (True, True), 1, g)               # fusion 1 without fuse_w
        refused_step(ins, w, outs, (False, True), 1, g)                 # fusion != 0 without mu_f
        refused_step(ins, w, outs, (True, False), 2, g)                 # ... without Sigma_f
        refused_step(ins, w, outs, (True, True), 3, g)                  # fusion 3
        refused_step(ins, w, outs, (True, True), -1, g)

    # backward: d = 5
    ins, w, _ = step_args(d=5)
    go = [_Out((K, N), s) for s in ((5, 5), (5,), (5,), (5, 5), (5, 5))]
    with pytest.raises(abi.MmfError):
        abi.ekf_step_backward(*ins, ins[0], ins[1], ins[0], *[o.t for o in go])
    # sigma points: scale <= 0 (and NaN), d = 5
    flag = torch.full((1,), 2, dtype=torch.int32, device=dev)
    for d, scale in ((3, 0.0), (3, -1.0), (3, float("nan")), (5, 1.0)):
        pts = _Out((N,), (2 * d + 1, d))
        with pytest.raises(abi.MmfError):
            abi.ukf_sigma_points(torch.zeros((N, d), device=dev), torch.eye(d, device=dev).expand(N, d, d).contiguous(),
                                 scale, pts.t, flag)
        go.append(pts)
    # moments: d = 5; weights that do not reproduce a constant (wm0 + 2 d wi != 1)
    for d, (wm0, wi) in ((5, (0.0, 0.1)), (3, (0.0, 1.0)), (3, (0.5, 1.0 / 6.0)), (3, (float("nan"), 1.0 / 6.0))):
        m, S = _Out((N,), (d,)), _Out((N,), (d, d))
        with pytest.raises(abi.MmfError):
            abi.ukf_moments(torch.zeros((N, 2 * d + 1, d), device=dev), wm0, 1.0, wi, torch.zeros((d, d), device=dev), m.t, S.t)
        go += [m, S]
    # fused sensors: d = 4, mode 3, mode 1 without w
    for d, mode, with_w in ((4, 1, True), (3, 3, True), (3, 0, True), (3, 1, False)):
        z_out, t_out = _Out((N,), (d,)), _Out((N,), (d, d))
        with pytest.raises(abi.MmfError):
            abi.fuse_virtual_sensors(torch.zeros((K, N, d), device=dev), torch.eye(d, device=dev).expand(K, N, d, d).contiguous(),
                                     torch.ones((K, N, d), device=dev) if with_w else None, z_out.t, t_out.t, mode)
        go += [z_out, t_out]
    torch.cuda.synchronize()
    assert all(o.untouched() for o in go) and int(flag.item()) == 2


def test_ukf_moments_accept_float32_rounded_weights():
    """``wm0 + 2 d wi = 1`` is checked on the float32 arguments: the default strategy's ``wm0 ~ -1e4`` alone moves by 1e-3
    when rounded, and every built-in strategy at every d must pass."""
    abi = _abi()
    dev = _dev()
    from multimodalfilter_amd import filters

    for s in (filters.JulierSigmaPointStrategy(), filters.MerweSigmaPointStrategy(alpha=0.5), filters.MerweSigmaPointStrategy(),
              filters.MerweSigmaPointStrategy(alpha=1e-3), filters.JulierSigmaPointStrategy(lambd=0.5)):
        for d in kc.DIMS:
            wc0, wm0, wi = s.compute_sigma_weights(d)
            x = torch.ones((2, 2 * d + 1, d), device=dev)
            m, S = _Out((2,), (d,)), _Out((2,), (d, d))
            abi.ukf_moments(x, wm0, wc0, wi, torch.zeros((d, d), device=dev), m.t, S.t)
            # a constant is reproduced exactly, with no spread
            assert torch.equal(m.t, torch.ones_like(m.t)) and torch.equal(S.t, torch.zeros_like(S.t))

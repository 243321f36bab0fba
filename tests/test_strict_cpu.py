"""The bit-exact CPU twin of the engine's strict (exact-fp32) mode, ``oracle/strict``, against
the torch oracle it restates (which ``tests/golden`` pins to the reference): same networks, same
inputs, results within a few fp32 roundings -- so that bit-equality of the HIP engine with the
twin (``tests/test_gpu_strict.py``) is also 1e-6-equality with the reference's arithmetic.
Tolerances are written at each comparison."""
import math

import numpy as np
import pytest
import torch

from oracle import models as om
from oracle import resample as ors
from oracle import strict
from oracle.tf.base import ReplayNoise


def test_deterministic_transcendentals_against_fp64():
    g = np.random.default_rng(0)
    x = -np.abs(g.standard_normal(20000) * 20).astype(np.float32)
    e = strict.det_exp_nonpos(x)
    assert np.array_equal(e, ors.detexp(x))                       # the resampler's numpy definition, bit for bit
    ref = np.exp(x.astype(np.float64))
    assert np.max(np.abs(e - ref) / ref / (1.0 + np.abs(x))) < 1.5e-7   # the argument x log2(e) is rounded once
    s = (1.0 + g.random(20000) * 7).astype(np.float32)              # sums of up to 8 exponentials
    assert np.max(np.abs(strict.det_log(s) - np.log(s.astype(np.float64)))) < 2.5e-7
    wide = np.exp(g.uniform(-80, 80, 20000)).astype(np.float32)
    lw = np.log(wide.astype(np.float64))
    assert np.max(np.abs(strict.det_log(wide) - lw) / np.maximum(1.0, np.abs(lw))) < 2.5e-7
    gte = (g.standard_normal(20000) * 8).astype(np.float32)
    assert np.max(np.abs(strict.det_sigmoid(gte) - 1.0 / (1.0 + np.exp(-gte.astype(np.float64))))) < 3e-7
    a = (g.standard_normal(20000) * 5).astype(np.float32)
    b = (g.standard_normal(20000) * 5).astype(np.float32)
    b[:10] = -np.inf
    a[5:15] = -np.inf
    lae = strict.det_logaddexp(a, b)
    with np.errstate(divide="ignore"):
        want = np.logaddexp(a.astype(np.float64), b.astype(np.float64))
    assert np.all(np.isneginf(lae[5:10])) and np.all(np.isfinite(lae[15:]))
    fin = np.isfinite(want)
    assert np.max(np.abs(lae[fin] - want[fin])) < 1.5e-6


TANH_SEAM = np.float32(0.625)      # mmf_det_tanh: the polynomial below, 2 sigmoid(2|x|) - 1 from it on


def _old_tanh(x):
    """``fmaf(2, mmf_det_sigmoid(2x), -1)``, what the LSTM evaluated before ``mmf_det_tanh`` (2 s is exact: one rounding)."""
    s = strict.det_sigmoid((np.float32(2.0) * x).astype(np.float32))
    return (2.0 * s.astype(np.float64) - 1.0).astype(np.float32)


def test_det_tanh_relative_error_against_fp64():
    """<= 7e-7 RELATIVE (the absolute 7e-7 the LSTM's tanh used to be documented with, turned relative; |tanh| <= 1, so it
    implies the absolute bound): 1e-30 <= |x| <= 20 log-spaced, a dense linear sweep of one octave either side of the seam,
    and every float of the 4096 next to the seam, both signs.  Prints the worst (include/mmf_detmath.h quotes it)."""
    mag = np.concatenate([np.logspace(-30, np.log10(20.0), 400001), np.linspace(0.5 * TANH_SEAM, 2.0 * TANH_SEAM, 400001),
                          TANH_SEAM * (1.0 + np.arange(-2048, 2048) * 2.0 ** -24)]).astype(np.float32)
    x = np.concatenate([mag, -mag])
    want = np.tanh(x.astype(np.float64))
    rel = np.abs(strict.det_tanh(x) - want) / np.abs(want)
    worst = int(np.argmax(rel))
    print(f"mmf_det_tanh: worst relative error {rel[worst]:.3e} at x = {x[worst]!r}; "
          f"below the seam {rel[np.abs(x) < TANH_SEAM].max():.3e}; old form at |x| = 1e-4: "
          f"{abs(float(_old_tanh(np.float32([1e-4]))[0]) - np.tanh(1e-4)) / np.tanh(1e-4):.3e}")
    assert rel.max() <= 7e-7, (rel[worst], x[worst])
    assert np.max(np.abs(strict.det_tanh(x) - want)) <= 7e-7
    # the form it replaces keeps its ABSOLUTE bound and misses the relative one by three orders at 1e-4
    small = np.float32([1e-4, -1e-4, 3e-5])
    assert np.all(np.abs(_old_tanh(small) - np.tanh(small.astype(np.float64))) / np.abs(np.tanh(small.astype(np.float64))) > 1e-4)


def test_det_tanh_zeros_symmetry_saturation_and_seam():
    t = strict.det_tanh
    z = t(np.float32([0.0, -0.0]))
    assert np.array_equal(z, [0.0, 0.0]) and np.array_equal(np.signbit(z), [False, True])
    # denormals and the smallest normals come back as they are (tanh x = x to fp32 there), infinities saturate, NaN stays
    tiny = np.float32([1e-45, 1e-40, 1.1754944e-38, 1e-30, -1e-40])
    assert np.array_equal(t(tiny), tiny)
    assert np.array_equal(t(np.float32([np.inf, -np.inf, 100.0, -100.0])), [1.0, -1.0, 1.0, -1.0]) and np.isnan(t(np.float32([np.nan]))[0])
    # odd, bit for bit
    g = np.random.default_rng(2)
    x = np.concatenate([np.logspace(-38, 1.5, 200001), g.standard_normal(100000) * 3.0, np.linspace(0.3, 1.3, 200001)]).astype(np.float32)
    assert np.array_equal(t(-x).view(np.int32), (-t(x)).view(np.int32))
    # exactly +-1 wherever 2 sigmoid(2x) - 1 was, and exactly 1 from 8.32 on (exp(-2x) <= 2^-24)
    big = np.concatenate([np.linspace(5.0, 30.0, 250001), np.logspace(1, 38, 1000)]).astype(np.float32)
    for s in (np.float32(1.0), np.float32(-1.0)):
        old, new = _old_tanh(s * big), t(s * big)
        assert np.all(new[old == s] == s) and np.any(old == s)
        assert np.all(new[big >= 8.32] == s) and np.all(np.abs(new[big <= 8.3]) < 1.0)
    # for x >= the seam the value IS the old form's (x > 0: the same operations)
    assert np.array_equal(t(big), _old_tanh(big))
    pos = x[x >= TANH_SEAM]
    assert np.array_equal(t(pos), _old_tanh(pos))
    # non-decreasing across the seam: the 64 floats below it against the 64 from it on, and along the whole window
    ulp = np.float32(2.0 ** -24)                                # spacing of floats in [0.5, 1)
    window = (TANH_SEAM + np.arange(-64, 64).astype(np.float32) * ulp).astype(np.float32)
    assert window[64] == TANH_SEAM and np.all(np.diff(window) == ulp)
    y = t(window)
    assert y[63] <= y[64] and y[:64].max() <= y[64:].min()
    assert np.all(np.diff(y) >= 0)
    assert np.all(np.diff(t(-window)) <= 0)


def test_strict_layers_match_the_torch_oracle():
    torch.manual_seed(0)
    task = om.TASKS["door"]
    g = torch.Generator().manual_seed(1)
    N = 5
    img = (torch.randn((N, 32, 32), generator=g) * 0.5).clamp(-1, 1)
    enc = om.image_encoder(64)
    with torch.no_grad():
        want = enc(img[:, None]).numpy()
    got = strict.image_encoder(enc, img)
    assert np.max(np.abs(got - want)) / max(1.0, np.abs(want).max()) < 2e-6
    ve = om.vector_encoder(7, 64)
    x = torch.randn((N, 7), generator=g)
    with torch.no_grad():
        want = ve(x).numpy()
    assert np.max(np.abs(strict.vector_encoder(ve, x) - want)) < 2e-6


def test_strict_weighted_mean_estimate():
    g = np.random.default_rng(3)
    for M in (30, 300, 4096, 5000):
        lw = (g.standard_normal((3, M)) * 2).astype(np.float32)
        x = g.standard_normal((3, M, 3)).astype(np.float32)
        e = ors.quantise(lw)[1].astype(np.float64)
        want = (e[:, :, None] * x).sum(1) / e.sum(1)[:, None]
        assert np.max(np.abs(strict.estimate(lw, x) - want)) < 2e-6


@pytest.mark.parametrize("cls", ["DoorCrossmodalParticleFilter", "PushUnimodalParticleFilter", "DoorParticleFilter"])
def test_strict_particle_filter_tracks_the_torch_oracle(cls):
    """Teacher-forced over 3 steps (the strict twin restarts every step from the torch oracle's belief):
    log-likelihood-driven ancestors certified, posterior means within 2e-6 relative."""
    o = om.build(cls)
    o.load_state_dict(om.seeded_state_dict(o, seed=5, gain=1.0))
    o.eval()
    d = o.state_dim
    N, M, T = 3, 64, 3
    g = torch.Generator().manual_seed(7)
    obs = {"image": (torch.randn((T, N, 32, 32), generator=g) * 0.5).clamp(-1, 1),
           "gripper_pos": torch.randn((T, N, 3), generator=g), "gripper_sensors": torch.randn((T, N, 7), generator=g)}
    ctrl = torch.randn((T, N, 7), generator=g)
    eps0 = torch.randn((N, M, d), generator=g)
    eps = [torch.randn((N, M, d), generator=g) for _ in range(T)]
    us = [torch.rand((N,), generator=g) for _ in range(T)]
    o.num_particles = M
    o.noise = ReplayNoise([eps0] + eps, us)
    s = strict.StrictParticleFilter(o)
    cov = (torch.eye(d) * 0.1)[None].expand(N, d, d)
    with torch.no_grad():
        o.initialize_beliefs(mean=torch.randn((N, d), generator=g), covariance=cov)
        for t in range(T):
            s.set_belief(o.particle_states, o.particle_log_weights)
            before = o.particle_states.clone()
            want = o(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t]).numpy()
            got = s.step(observations={k: v[t] for k, v in obs.items()}, controls=ctrl[t], eps=eps[t], u=us[t])
            assert np.max(np.abs(got - want)) / max(1.0, np.abs(want).max()) < 2e-6, t
            idx_o = o.last_resample_indices.numpy()
            bad = int((idx_o != s.last_resample_indices).sum())
            assert bad <= 2, (t, bad)


def _philox_python(key, ctr, rounds=10):
    """Philox4x32 from its definition (Salmon et al., SC'11), in Python integers."""
    M0, M1, W0, W1, mask = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF
    k0, k1 = key
    c = list(ctr)
    for _ in range(rounds):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [((p1 >> 32) ^ c[1] ^ k0) & mask, p1 & mask, ((p0 >> 32) ^ c[3] ^ k1) & mask, p0 & mask]
        k0, k1 = (k0 + W0) & mask, (k1 + W1) & mask
    return c


def test_counter_based_noise_generator():
    """``include/mmf_philox.h`` as compiled into the checker: Philox4x32-10 against the Random123
    known-answer vectors and a from-the-definition Python restatement; the Box-Muller normals and the
    resampling uniforms against their distributions; blocks are functions of (seed, step, trajectory,
    particle) only, so a shard draws what the whole batch would."""
    kat = [((0, 0), (0, 0, 0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff, 0xffffffff), (0xffffffff,) * 4, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0xa4093822, 0x299f31d0), (0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for key, ctr, want in kat:
        assert tuple(_philox_python(key, ctr)) == want
        assert tuple(strict.philox_raw(key, ctr)) == want
    g = np.random.default_rng(5)
    for _ in range(50):
        key = [int(x) for x in g.integers(0, 2 ** 32, 2)]
        ctr = [int(x) for x in g.integers(0, 2 ** 32, 4)]
        assert strict.philox_raw(key, ctr) == _philox_python(key, ctr)
    from scipy import stats

    z = strict.philox_normals(1234, 7, 64, 4096, 4)
    assert np.all(np.isfinite(z)) and abs(float(z.mean())) < 5e-3 and abs(float(z.var()) - 1.0) < 5e-3
    for i in range(4):
        assert stats.kstest(z[..., i].ravel()[:200000], "norm").pvalue > 1e-3
    assert abs(float(np.corrcoef(z[..., 0].ravel(), z[..., 1].ravel())[0, 1])) < 5e-3
    assert float(np.abs(z).max()) > 4.0          # tails are there (Box-Muller on 23-bit uniforms: up to 5.7 sigma)
    u = strict.philox_uniforms(1234, 0, 500, 100)
    assert float(u.min()) >= 0.0 and float(u.max()) < 1.0 and stats.kstest(u.ravel(), "uniform").pvalue > 1e-3
    # another step / seed / stream: different draws; a shard reproduces its slice of the whole batch
    assert not np.array_equal(z, strict.philox_normals(1234, 8, 64, 4096, 4))
    assert not np.array_equal(z, strict.philox_normals(1235, 7, 64, 4096, 4))
    assert np.array_equal(strict.philox_normals(1234, 7, 16, 4096, 4, traj0=32), z[32:48])
    assert np.array_equal(strict.philox_normals(1234, 7, 64, 4096, 3), z[..., :3])

"""K2 (per-particle networks, f16x3): the vector forms of the tile helpers -- the NaN-keeping ReLU after the join
layer as one IEEE maximum, the range tracking as a three-input packed f16 maximum -- on both tile organisations
``launch_ct`` picks: the pipelined 64-particle tile from 256 * 8 * 64 rows up, the unpipelined 32-particle tile below.  The two promise the same bits; the range flag follows the rule "the hi half
handed to an MFMA is >= 0x7BFF" (``particle_net_tiles.h``).
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

PIPE_ROWS = 256 * 8 * 64      # launch_ct: rows >= this take the pipelined 64-particle variant
M = 4096
N = PIPE_ROWS // M            # 32 trajectories: the smallest pipelined launch at this M
PIECE_N = 8                   # 8 x 4096 rows < PIPE_ROWS: the 32-particle unpipelined variant
UNIT = 5                      # the isolated feature of the probe networks
DYNAMICS, MEASURE = "dynamics", "measure"


def _cuda():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a real MI355X")
    return torch.device("cuda:0")


@pytest.fixture(autouse=True)
def _f16x3():
    from multimodalfilter_amd import engine

    old = engine.DEFAULT_PRECISION
    engine.set_default_precision("f16x3")
    yield
    engine.set_default_precision(old)


class _Net:
    """enc -> join -> res* -> head as the task models build it, with the per-trajectory join term given directly."""

    def __init__(self, d, kind, probe):
        from multimodalfilter_amd import engine, layers

        torch.manual_seed(1000 * d + (kind == MEASURE) + 10 * probe)
        self.d, self.kind = d, kind
        n_res, n_out = (3, d + 1) if kind == DYNAMICS else (2, 1)
        self.encoder = layers.vector_encoder(d, 64)
        self.join = torch.nn.Linear(128, 64)
        self.res = [layers.ResLinear(64) for _ in range(n_res)]
        self.head = torch.nn.Linear(64, n_out)
        if probe:
            # Feature UNIT is cut off from every other one: state component 0 feeds it alone (weight 1, no bias), no
            # layer reads it and no layer writes it, so it carries relu(x_0) up to the join layer and the join row's
            # entry after it, unchanged through the skips, and each operand split sees exactly that value.
            with torch.no_grad():
                w0 = self.encoder[0]
                w0.weight[:, 0] = 0
                w0.weight[UNIT, :] = 0
                w0.weight[UNIT, 0] = 1
                w0.bias[UNIT] = 0
                for rb in [self.encoder[2]] + self.res:
                    rb.block1.weight[:, UNIT] = 0
                    rb.block2.weight[UNIT, :] = 0
                    rb.block2.bias[UNIT] = 0
                self.join.weight[:, 64 + UNIT] = 0
                self.join.weight[UNIT, :] = 0
                self.head.weight[:, UNIT] = 0
        dev = _cuda()
        for m in [self.encoder, self.join, self.head] + self.res:
            m.to(dev)
        self.net = engine.PackedParticleNet(encoder=self.encoder, join=self.join, join_state_off=64, res_blocks=self.res,
                                            head=self.head, relu_after_join=kind == MEASURE)
        g = torch.Generator().manual_seed(7 + d)
        self.scale_tril = torch.diag(torch.rand(d, generator=g) * 0.1 + 0.05).to(dev)

    def run(self, states, bias, noise=None):
        """(n, m, d) states, (n, 64) join rows -> propagated states (dynamics) or log-likelihoods (measurement)"""
        from multimodalfilter_amd import engine

        if self.kind == DYNAMICS:
            return engine.run_dynamics(self.net, states, bias, noise, self.scale_tril)
        out = torch.empty(states.shape[:2], dtype=torch.float32, device=states.device)
        return engine.run_measure(self.net, states, bias, None, 0, out, False)

    def run_in_pieces(self, states, bias, noise=None):
        outs = []
        for n0 in range(0, states.shape[0], PIECE_N):
            s = slice(n0, n0 + PIECE_N)
            assert states[s].numel() // self.d < PIPE_ROWS
            outs.append(self.run(states[s].contiguous(), bias[s].contiguous(), None if noise is None else noise[s].contiguous()))
        return torch.cat(outs, 0)


@functools.lru_cache(maxsize=None)
def _net(d, kind, probe=False):
    return _Net(d, kind, probe)


@functools.lru_cache(maxsize=None)
def _inputs(d):
    g = torch.Generator().manual_seed(31 + d)
    dev = _cuda()
    return (torch.randn((N, M, d), generator=g).to(dev), torch.randn((N, 64), generator=g).to(dev),
            torch.randn((N, M, d), generator=g).to(dev))


def _raised(dev):
    """read and clear the range flag"""
    from multimodalfilter_amd import _abi, engine

    try:
        engine.check_range(dev)
    except _abi.MmfError as e:
        assert "f16x3 operand range" in str(e)
        return True
    return False


# ------------------------------------------------------------------ 1. the two variants, same bits
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("kind", [MEASURE, DYNAMICS])
def test_pipelined_tile_equals_unpipelined_pieces(kind, d):
    """The smallest launch that takes the pipelined 64-particle tile against the same rows in pieces of 8 trajectories
    (the 32-particle unpipelined tile): torch.equal on log-likelihoods / propagated states, with and without noise."""
    from multimodalfilter_amd import engine

    dev = _cuda()
    net = _net(d, kind)
    states, bias, noise = _inputs(d)
    assert states.numel() // d == PIPE_ROWS
    engine.clear_range(dev)
    for eps in ([None] if kind == MEASURE else [None, noise]):
        whole = net.run(states, bias, eps)
        pieces = net.run_in_pieces(states, bias, eps)
        assert bool(torch.isfinite(whole).all())
        assert torch.equal(whole, pieces)
    assert not _raised(dev)


# ------------------------------------------------------------------ 2. the range flag at the boundary
def _rule(a):
    """hi half (round to nearest even, as v_cvt_pk_f16_f32) of the operand a >= 0x7BFF"""
    return int(torch.tensor([a], dtype=torch.float32).half().view(torch.int16)[0]) >= 0x7BFF


F16_MAX = 65504.0
# (value, raised): 65472 is the largest f16 below 65504 (0x7BFE); 65488 is the tie between the two and goes to the even
# 0x7BFE; everything above it rounds to 0x7BFF, and from the tie 65520 on to +inf (0x7C00)
BOUNDARY = [(65472.0, False), (65488.0, False), (float(np.nextafter(np.float32(65488.0), np.float32(np.inf))), True),
            (float(np.nextafter(np.float32(F16_MAX), np.float32(0.0))), True), (F16_MAX, True), (65520.0, True), (1.0e5, True)]
# where the driven activation sits: (trajectory, particle) in the big launch -- column half 0 of the first tile, column
# half 1 of the last tile -- and in the two-tile small launch
BIG_AT = [(0, 5), (N - 1, M - 27)]
SMALL_AT = [(0, 5), (1, 37)]


def _boundary_cases(kind, path):
    cases = list(BOUNDARY)
    if path == "join":  # a negative join term: ignored after the ReLU (measurement), split by magnitude without one (dynamics)
        cases += [(-65472.0, False), (-F16_MAX, kind == DYNAMICS), (-1.0e5, kind == DYNAMICS)]
    return cases


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("path", ["state", "join"])
@pytest.mark.parametrize("kind", [MEASURE, DYNAMICS])
def test_range_flag_at_the_f16_boundary(kind, path, d):
    """One activation driven to just below, to, and above 65504 -- through the first layer (state component 0 of one
    particle) and through one entry of a trajectory's join row -- in both tile variants: the flag is raised exactly when the
    hi half of the value the split sees (v; relu(v) after the measurement's join; |clamp(v)| after the dynamics') is
    >= 0x7BFF, and the outputs are finite."""
    from multimodalfilter_amd import engine

    dev = _cuda()
    net = _net(d, kind, True)
    big_states, big_bias, _ = _inputs(d)
    variants = [(big_states.clone(), big_bias.clone(), BIG_AT), (big_states[:2, :64].clone(), big_bias[:2].clone(), SMALL_AT)]
    engine.clear_range(dev)
    for states, bias, places in variants:
        net.run(states, bias)
        assert not _raised(dev), "the undriven network must stay in range"
        for value, want in _boundary_cases(kind, path):
            seen = value if path == "state" else (max(value, 0.0) if kind == MEASURE else min(abs(value), F16_MAX))
            assert _rule(seen) == want
            for n, p in places:
                target = states[n, p, 0:1] if path == "state" else bias[n, UNIT:UNIT + 1]
                keep = target.clone()
                target.fill_(value)
                out = net.run(states, bias)
                got = _raised(dev)
                target.copy_(keep)
                assert got == want, (kind, d, path, value, n, p, tuple(states.shape), got, want)
                assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------ 3. non-finite inputs
NONFINITE = {"+nan": 0x7FC00000, "-nan": 0xFFC00000, "+inf": 0x7F800000, "-inf": 0xFF800000}


def _bits(pattern, dev):
    return torch.tensor([pattern - (1 << 32) if pattern >= (1 << 31) else pattern], dtype=torch.int32, device=dev).view(torch.float32)


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("path", ["state", "join"])
@pytest.mark.parametrize("kind", [MEASURE, DYNAMICS])
def test_nonfinite_inputs_raise_the_flag_over_finite_outputs(kind, path, d):
    """+NaN, -NaN, +inf, -inf in one particle state / one join-row entry: the flag is raised, the outputs are finite, and
    the pipelined launch and the unpipelined pieces agree bit for bit.

    Two consequences of what the networks compute, not of the number format, are stated as they are:
    * dynamics returns x' = x + dir * sigmoid(gate): the particle whose own state is non-finite gets that state back
      (NaN, or the infinity), in f32 mode as well; every OTHER row, and the network's part of every row, is finite;
    * a -inf join entry in front of the measurement's ReLU is relu(-inf) = 0: no operand leaves the f16 range, the result is
      exact (it equals the one for -65504 there), and the flag stays down, as it did with the i16 tracking."""
    from multimodalfilter_amd import engine

    dev = _cuda()
    net = _net(d, kind)
    states, bias, _ = _inputs(d)
    states, bias = states.clone(), bias.clone()
    n, p = N - 1, M - 27
    engine.clear_range(dev)
    for name, pattern in NONFINITE.items():
        target = states[n, p, 1:2] if path == "state" else bias[n, UNIT:UNIT + 1]
        keep = target.clone()
        target.copy_(_bits(pattern, dev))
        whole = net.run(states, bias)
        got_whole = _raised(dev)
        pieces = net.run_in_pieces(states, bias)
        got_pieces = _raised(dev)
        relu_of_minus_inf = kind == MEASURE and path == "join" and name == "-inf"
        if relu_of_minus_inf:
            target.fill_(-F16_MAX)
            same = net.run(states, bias)
            assert not _raised(dev)
            assert torch.equal(whole, same)
        target.copy_(keep)
        assert got_whole == got_pieces == (not relu_of_minus_inf), (name, got_whole, got_pieces)
        finite = torch.isfinite(whole)
        if kind == DYNAMICS and path == "state":
            assert not bool(finite[n, p, 1]) and bool(torch.equal(torch.isfinite(pieces), finite))
            finite[n, p, 1] = True
            whole[n, p, 1] = 0
            pieces[n, p, 1] = 0
        assert bool(finite.all()), name
        assert torch.equal(whole, pieces), name


@pytest.mark.parametrize("d", [2, 3])
def test_negative_zero_join_entry_equals_positive_zero(d):
    """-0.0 in a join row in front of the measurement's ReLU: the same output bits as +0.0, in both variants -- the
    statement about the OUTPUTS, which is all a launch can show.  It does not tell what relu_keepnan(-0.0) returns: the
    join layer's own zero products already turn the accumulator into +0 (-0 + +0 = +0), and the sign of a zero activation
    could not reach an output anyway -- an activation enters the next layer only through sums of products, where +-0
    changes no bit.  That relu_keepnan(-0.0) is +0 holds by construction: IEEE-754 maximum orders -0 below +0
    (``particle_net_tiles.h``)."""
    dev = _cuda()
    net = _net(d, MEASURE, True)
    states, bias, _ = _inputs(d)
    bias = bias.clone()
    outs = []
    for z in (0.0, -0.0):
        bias[:, UNIT] = z
        outs.append((net.run(states, bias), net.run_in_pieces(states, bias)))
    assert math.copysign(1.0, float(bias[0, UNIT])) == -1.0
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][0], outs[0][1])
    assert not _raised(dev)

"""The fused network training kernel (``particle_net_train_fused_kernel``, ``csrc/particle_net_fused.hip``) against fp64 where
a workgroup WALKS: several groups per workgroup, the running exponent of the resident weight-gradient accumulators rising,
falling and idle, ragged ends, partials accumulated in place, several networks per launch.  Every call goes through the C ABI
(``mmf_particle_net_train_fused`` / ``_multi``) on the margin-filtered rows ``_fused_cases.py`` builds and
``test_fused_cases_cpu.py`` certifies; the bounds are that module's, computed from the fp64 reference and the documented
roundings only.

Every row-indexed output carries ``GUARD_ROWS`` rows of ``SENTINEL`` on both sides and starts out as ``SENTINEL`` itself (a row
the kernel skipped fails its comparison); the guards are checked bit for bit after every call, and so are the slots of ``pw`` /
``pb`` at and beyond the grid.  Each figure is printed before it is asserted (``pytest -s``: lines ``FUSED family=...``); the
module's last test prints the worst ratio per family and quantity -- the table in ``_fused_cases.py``'s docstring."""
import collections
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import _fused_cases as fc
from _fused_case import ROW_OUTPUTS, marshal, output_buffers
from _guarded_gpu import abi, dev

G = fc.GUARD_ROWS
MEASURED = collections.defaultdict(float)   # (family, quantity) -> worst |kernel - fp64| / bound
_INT = {torch.float32: torch.int32, torch.float16: torch.int16}


def _bits(t):
    return t.contiguous().view(_INT[t.dtype])


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


class Guarded:
    """``shape[0]`` rows between two blocks of ``GUARD_ROWS`` guard rows, all ``SENTINEL``; ``t``: the rows."""

    def __init__(self, shape, dtype):
        self.full = torch.full((shape[0] + 2 * G,) + tuple(shape[1:]), fc.SENTINEL, dtype=dtype, device=dev())
        self.t = self.full[G:G + shape[0]]

    def guards_intact(self):
        want = torch.full_like(self.full[:G], fc.SENTINEL)
        return _same(self.full[:G], want) and _same(self.full[self.full.shape[0] - G:], want)


@functools.lru_cache(maxsize=None)
def _model(task, kind, seed=0):
    import multimodalfilter_amd as mmf

    ns = mmf.door_models if task == "door" else mmf.push_models
    P = task.capitalize()
    m = getattr(ns, P + "DynamicsModel")() if kind == "dynamics" else getattr(ns, P + "MeasurementModel")(modalities={"pos", "sensors"})
    m.load_state_dict(fc.state_dict(task, kind, seed))
    return m.to(dev()).eval()


def _prefill(NL, S, seed, scales):
    g = torch.Generator().manual_seed(777 + seed)
    sc = torch.tensor(scales, dtype=torch.float32)
    return (torch.randn((NL, S, 64, 64), generator=g) * sc[:, None, None, None],
            torch.randn((NL, S, 64), generator=g) * sc[:, None, None])


class Call:
    """One prepared call: inputs on the device, guarded outputs, the argument struct."""

    def __init__(self, task, kind, N, M, n_slots, ladder=None, which=0, seed=0, base=None, prefill=None):
        _abi = abi()
        net = _model(task, kind, seed)._net
        c = fc.case(task, kind, N, M, seed)
        self.R, self.d, self.NL, self.S, self.kind = N * M, fc.DIMS[task], 3 + 2 * net.n_res, n_slots, kind
        self.grid = fc.launch(self.R, n_slots)[1]
        self.guarded = {}

        def rows(name, shape, dtype):
            self.guarded[name] = Guarded(shape, dtype)
            return self.guarded[name].t

        self.bufs = output_buffers(self.R, self.d, self.NL, n_slots, dev(), rows=rows)
        # partials: zero where the launch accumulates (or the given prefill), SENTINEL at and beyond the grid
        for n in ("pw", "pb"):
            self.bufs[n].fill_(fc.SENTINEL)
            self.bufs[n][:, :self.grid].zero_()
        if prefill is not None:
            self.bufs["pw"].copy_(prefill[0])
            self.bufs["pb"].copy_(prefill[1])
        self.before = {n: self.bufs[n].clone() for n in ("pw", "pb")}
        self.st, self.tb = c.x.to(dev()), c.tb.to(dev())
        self.g = fc.incoming(task, kind, N, M, ladder, which, seed).to(dev()).contiguous()
        self.base = None
        if base is not None:   # "separate": its own buffer; "alias": d_states itself holds the values to add to
            gen = torch.Generator().manual_seed(991 + self.R)
            self.base_host = 0.5 * torch.randn((self.R, self.d), generator=gen)
            self.base = self.base_host.to(dev())
            if base == "alias":
                self.bufs["d_states"].copy_(self.base)
        base_arg = None if base is None else (self.bufs["d_states"] if base == "alias" else self.base)
        k = 0 if kind == "dynamics" else 1
        self.blob = net.blob(_abi.PREC_F16X3_DUAL)
        self.args = marshal(self.blob, net.n_res, k, self.d, N, M, n_slots, self.st, self.tb, self.bufs,
                            d_out=self.g.reshape(self.R) if k else None, g_next=None if k else self.g, d_states_base=base_arg)

    def set_gradient(self, g):
        self.g.copy_(g.to(dev()))

    def run(self):
        abi().particle_net_train_fused(self.args, self.st)
        torch.cuda.synchronize()
        return self.collect()

    def collect(self):
        """Guards and idle slots checked; the outputs on the host."""
        names = [n for n in ROW_OUTPUTS if self.kind == "dynamics" or n not in ("d_raw", "act", "g_act")]
        for n in ROW_OUTPUTS:
            assert self.guarded[n].guards_intact(), ("guard rows", n)
            if n not in names:   # a measurement network writes none of the dynamics buffers
                assert _same(self.guarded[n].t, torch.full_like(self.guarded[n].t, fc.SENTINEL)), n
        for n in ("pw", "pb"):
            assert _same(self.bufs[n][:, self.grid:], self.before[n][:, self.grid:]), ("slots at and beyond the grid", n)
        out = {n: self.bufs[n].cpu() for n in names + ["pw", "pb"]}
        for n in names:
            assert bool(torch.isfinite(out[n]).all()), ("not finite", n)
        return out


@functools.lru_cache(maxsize=None)
def _run(task, kind, N, M, n_slots, ladder=None):
    """The plain call (first gradient, no base, zeroed partials), made once and shared."""
    return Call(task, kind, N, M, n_slots, ladder).run()


def _note(family, tag, what, r):
    MEASURED[(family, what)] = max(MEASURED[(family, what)], r)
    print(f"FUSED family={family} {tag} what={what} ratio={r:.3e}")
    return r


def _hold_rows(family, tag, kind, out, t, y, base=None):
    """The row outputs against fp64: the compact rows under ``compact_bound``, ``d_states`` (and the dynamics network's
    ``d_raw`` / ``act`` / ``g_act``) per row under ``REL_TOL``.  Every row of the call is compared."""
    bad = []
    NL = len(t.dz)
    for what, got, want, yard, floor in (
            ("dz_first", out["dzf"].double() * out["scf"].double()[:, None], t.dz_first, y.dz_first, True),
            ("dz_join", out["dzj"].double() * out["scj"].double()[:, None], t.dz[2], y.dz[2], True),
            ("h_last", out["hl"].float(), t.a[NL], y.a[NL], False)):
        assert got.shape == want.shape
        if _note(family, tag, what, fc.ratio(got, want, fc.compact_bound(want, yard, floor)[:, None])) >= 1.0:
            bad.append(what)
    if base is None:
        r = float(fc.row_rel(out["d_states"], t.d_states).max()) / fc.REL_TOL
    else:   # the network term plus the base: one more fp32 rounding, of the sum
        want = t.d_states + base.double()
        bound = fc.REL_TOL * t.d_states.abs().amax(1).clamp_min(1e-30) + 2 * fc.EPS_F32 * want.abs().amax(1)
        r = fc.ratio(out["d_states"], want, bound[:, None])
    if _note(family, tag, "d_states", r) >= 1.0:
        bad.append("d_states")
    if kind == "dynamics":
        for what, got, want in (("d_raw", out["d_raw"], t.d_raw), ("act", out["act"], t.a[2]), ("g_act", out["g_act"], t.g_act)):
            if _note(family, tag, what, float(fc.row_rel(got, want).max()) / fc.REL_TOL) >= 1.0:
                bad.append(what)
    assert not bad, (family, tag, bad)


def _hold_weights(family, tag, pw, pb, grid, t, y):
    """``sum_slots pw`` / ``pb`` against fp64 under ``weight_bounds``."""
    bW, bb = fc.weight_bounds(t, y)
    bad, seen = [], []
    for l in range(len(bW)):
        gW, gb = pw[l, :grid].double().sum(0), pb[l, :grid].double().sum(0)
        rW, rb = fc.ratio(gW, t.dW[l], bW[l]), fc.ratio(gb, t.db[l], bb[l])
        seen.append(f"{rW:.2e}/{rb:.2e}")
        if rW >= 1.0 or rb >= 1.0:
            bad.append((l, rW, rb))
        MEASURED[(family, "dW")] = max(MEASURED[(family, "dW")], rW)
        MEASURED[(family, "db")] = max(MEASURED[(family, "db")], rb)
    print(f"FUSED family={family} {tag} what=dW/db ratio per layer: " + " ".join(seen))
    assert not bad, (family, tag, bad)


def _hold(family, tag, task, kind, N, M, out, grid, ladder=None):
    t, y = fc.truth(task, kind, N, M, ladder), fc.yardstick(task, kind, N, M, ladder)
    _hold_weights(family, tag, out["pw"], out["pb"], grid, t, y)
    _hold_rows(family, tag, kind, out, t, y)


# ------------------------------------------------------------------------------ row edges, one group per workgroup
@pytest.mark.parametrize("N,M", fc.EDGE_SHAPES)
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_row_edges_against_fp64(task, kind, N, M):
    """R one short of, at and one past a tile and a group, trajectories straddling both, ``n_slots = ngroups``: every output
    against fp64; a store past ``R`` would break a guard row, a dead lane that contributed (it recomputes row ``R - 1``)
    the weight gradients."""
    R = N * M
    ngroups = fc.launch(R, 10 ** 6)[0]
    out = _run(task, kind, N, M, ngroups)
    _hold("edges", f"task={task} kind={kind} R={R} M={M} slots={ngroups}", task, kind, N, M, out, ngroups)


# ------------------------------------------------------------------------------ the walk
@pytest.mark.parametrize("N,M,n_slots", fc.WALK_SHAPES)
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_walked_launch_against_fp64_and_the_unwalked_rows(task, kind, N, M, n_slots):
    """Fewer slots than groups: accumulators, ``Eacc`` and the prefetched first inputs are carried from group to group.
    ``sum_slots pw`` is held against fp64; the row outputs do not depend on the walk and equal the ``n_slots = ngroups`` run
    of the same inputs bit for bit."""
    R = N * M
    ngroups, grid = fc.launch(R, n_slots)
    assert grid == n_slots < ngroups
    out = _run(task, kind, N, M, n_slots)
    _hold("walk", f"task={task} kind={kind} R={R} M={M} slots={n_slots}", task, kind, N, M, out, grid)
    flat = _run(task, kind, N, M, ngroups)
    for n in out:
        if n not in ("pw", "pb"):
            assert _same(out[n], flat[n]), n


# ------------------------------------------------------------------------------ exponent ladders
@pytest.mark.parametrize("walked", (True, False))
@pytest.mark.parametrize("ladder", [n for n in fc.LADDERS if n != "all_zero"])
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_exponent_ladder_against_fp64(task, kind, ladder, walked):
    """Incoming gradients scaled group by group by exact powers of two (or zero), on one workgroup that walks all the groups
    and on one workgroup per group: the same bound either way.  Ascending ladders rescale the accumulators at every step,
    the descending one never does and drops its last groups whole (``eacc_walk`` on the reference says so)."""
    N, M = fc.ladder_shape(ladder)
    L = len(fc.LADDERS[ladder].groups)
    n_slots = 1 if walked else L
    t = fc.truth(task, kind, N, M, ladder)
    branches = fc.eacc_walk(t, N * M, n_slots)
    if ladder in ("ascending", "steep"):
        assert all(b["rescales"] == (L - 1 if walked else 0) for b in branches)
    if ladder == "descending":
        assert all(b["rescales"] == 0 for b in branches) and all((b["dropped"] >= 128) == walked for b in branches)
    out = _run(task, kind, N, M, n_slots, ladder)
    _hold(fc.FAMILY[ladder], f"task={task} kind={kind} ladder={ladder} slots={n_slots}", task, kind, N, M, out, n_slots, ladder)


@pytest.mark.parametrize("base", (None, "separate"))
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_all_zero_call_adds_nothing(task, kind, base):
    """Every incoming gradient exactly zero (``Eacc`` stays 0): the partials come back bit-identical to what they held,
    ``d_states`` is the base (or zero), every output is finite and within its bound of the reference."""
    N, M = fc.ladder_shape("all_zero")
    NL = 3 + 2 * fc.n_res_of(kind)
    c = Call(task, kind, N, M, 1, "all_zero", base=base, prefill=_prefill(NL, 1, 1, [1.0] * NL))
    out = c.run()
    assert _same(out["pw"], c.before["pw"].cpu()) and _same(out["pb"], c.before["pb"].cpu())
    want = torch.zeros((N * M, c.d)) if base is None else c.base.cpu()
    assert torch.equal(out["d_states"], want)
    t, y = fc.truth(task, kind, N, M, "all_zero"), fc.yardstick(task, kind, N, M, "all_zero")
    _hold_rows("zeros", f"task={task} kind={kind} ladder=all_zero base={base}", kind, out, t, y, None if base is None else c.base.cpu())


# ------------------------------------------------------------------------------ in place
@pytest.mark.parametrize("n_slots", (2, 7))
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_partials_accumulate_in_place(task, kind, n_slots):
    """``pw`` / ``pb`` hold random values, then two calls with different gradients: ``sum_slots`` is what was there plus both
    weight gradients, under the two calls' bounds and the fp32 roundings of the read-modify-writes.  ``n_slots = 7`` on five
    groups: slots 5 and 6 are not the launch's, and stay as they were."""
    N, M = 27, 19
    R = N * M
    grid = fc.launch(R, n_slots)[1]
    refs = [(fc.truth(task, kind, N, M, None, w), fc.yardstick(task, kind, N, M, None, w)) for w in (0, 1)]
    NL = len(refs[0][0].dW)
    pre = _prefill(NL, n_slots, 2, [float(refs[0][0].dW[l].abs().mean()) for l in range(NL)])
    c = Call(task, kind, N, M, n_slots, prefill=pre)
    c.run()
    c.set_gradient(fc.incoming(task, kind, N, M, None, 1))
    out = c.run()
    # one fp32 rounding per slot and call, of at most |what it held| + |the call's partial sums|
    extra = []
    for l in range(NL):
        mag = [t.dz[l].abs().t() @ t.a[l].abs() for t, _ in refs]
        magb = [t.dz[l].abs().sum(0) for t, _ in refs]
        extra.append((2 * fc.EPS_F32 * (pre[0][l, :grid].abs().double().sum(0) + mag[0] + mag[1]),
                      2 * fc.EPS_F32 * (pre[1][l, :grid].abs().double().sum(0) + magb[0] + magb[1])))
    bW = [fc.weight_bounds(t, y) for t, y in refs]
    sums = [(bW[0][0][l] + bW[1][0][l] + extra[l][0], bW[0][1][l] + bW[1][1][l] + extra[l][1]) for l in range(NL)]
    bad = []
    for l in range(NL):
        gW = out["pw"][l, :grid].double().sum(0) - pre[0][l, :grid].double().sum(0)
        gb = out["pb"][l, :grid].double().sum(0) - pre[1][l, :grid].double().sum(0)
        rW = fc.ratio(gW, refs[0][0].dW[l] + refs[1][0].dW[l], sums[l][0])
        rb = fc.ratio(gb, refs[0][0].db[l] + refs[1][0].db[l], sums[l][1])
        _note("in place", f"task={task} kind={kind} slots={n_slots} layer={l}", "dW", rW)
        _note("in place", f"task={task} kind={kind} slots={n_slots} layer={l}", "db", rb)
        if rW >= 1.0 or rb >= 1.0:
            bad.append((l, rW, rb))
    assert not bad, bad
    # the row outputs are those of the second call alone
    _hold_rows("in place", f"task={task} kind={kind} slots={n_slots}", kind, out, *refs[1])


@pytest.mark.parametrize("N,M,n_slots", ((3, 43, 2), (27, 19, 2)))
@pytest.mark.parametrize("base", ("separate", "alias"))
@pytest.mark.parametrize("task,kind", fc.NETS)
def test_d_states_adds_to_its_base(task, kind, base, N, M, n_slots):
    """``d_states_base`` as a buffer of its own and as ``d_states`` itself (accumulate in place): every row is the network
    term plus the base (the null base is every other test of this module); nothing else changes, bit for bit."""
    c = Call(task, kind, N, M, n_slots, base=base)
    out = c.run()
    t, y = fc.truth(task, kind, N, M), fc.yardstick(task, kind, N, M)
    _hold_rows("in place", f"task={task} kind={kind} R={N * M} base={base}", kind, out, t, y, c.base.cpu())
    assert _same(c.base.cpu(), c.base_host)   # the base itself is read only
    plain = _run(task, kind, N, M, n_slots)
    for n in out:
        if n != "d_states":
            assert _same(out[n], plain[n]), n


# ------------------------------------------------------------------------------ several networks in one launch
@pytest.mark.parametrize("n", (2, 3))
@pytest.mark.parametrize("task", fc.TASKS)
def test_multi_launch_equals_one_launch_each(task, n):
    """``mmf_particle_net_train_fused_multi``: ``n`` measurement networks of different weights (and rows) on ``blockIdx.y`` of
    one walked launch; every output of every network is bit-identical to a launch of its own."""
    N, M, n_slots = fc.MULTI_SHAPE
    calls = [Call(task, "measure", N, M, n_slots, seed=s) for s in range(n)]
    abi().particle_net_train_fused_multi([c.args for c in calls], calls[0].st)
    torch.cuda.synchronize()
    for s, c in enumerate(calls):
        got = c.collect()
        want = Call(task, "measure", N, M, n_slots, seed=s).run()
        for name in want:
            assert _same(got[name], want[name]), (s, name)
        if s == 0:
            assert all(_same(got[name], _run(task, "measure", N, M, n_slots)[name]) for name in want)
        else:
            assert not _same(got["d_states"], calls[0].bufs["d_states"].cpu())


def test_report_measured_ratios():
    """Prints the worst ratio to the bound per family and quantity of whatever ran before it in this module."""
    fams = ("edges", "walk", "ascending", "descending", "zeros", "in place")
    whats = ("dW", "db", "dz_first", "dz_join", "h_last", "d_states", "d_raw", "act", "g_act")
    print("FUSED measured worst |kernel - fp64| / bound:")
    print("    family      " + "".join(f"{w:>10}" for w in whats))
    for f in fams:
        print(f"    {f:<12}" + "".join(f"{MEASURED[(f, w)]:>10.3f}" if (f, w) in MEASURED else f"{'-':>10}" for w in whats))
    assert all(v < 1.0 for v in MEASURED.values())

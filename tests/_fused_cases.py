"""Inputs, fp64 references and error bounds for the fused network training kernel (``particle_net_train_fused_kernel``,
``csrc/particle_net_fused.hip``; C ABI ``mmf_particle_net_train_fused`` / ``_multi``): pure torch-CPU, shared by
``test_fused_cases_cpu.py`` (which certifies them without a GPU) and ``test_gpu_fused_training.py`` (which runs the kernel).

ROWS are chosen as in ``_jacobian_cases.py`` (its ``kept_rows`` / ``MARGIN`` / ``MIN_KEPT_SHARE``): a candidate row is a state
and the per-trajectory term of its trajectory; it is kept, in the order drawn, when the fp64 margin over every ReLU site of the
network (9 for the dynamics network, 8 for a measurement network) is at least ``MARGIN``.  The kernel's f16x3 recompute is
about 1e-6 from fp64, so no ReLU mask of a kept row can differ and nothing is excused at comparison time.

The TRUTH is ``reference``: the network and its backward pass written out in torch ops (no autograd, no engine), in fp64; the
same formulas in fp32 are the YARDSTICK of the forward arithmetic.  The CPU test pins it to autograd through the oracle's
modules at 1e-12.

BOUNDS come from the fp64 reference and the roundings the kernel documents, never from what the kernel returns
(``weight_bounds``, ``compact_bound``); each term names its source line.  ``YARD = 4``: the kernel multiplies in f16x3 (hi hi +
hi lo + lo hi: the dropped lo lo term is 2^-22 of a product) where the yardstick multiplies in fp32 (2^-24), in the recompute
and in the backward data path alike.

LADDERS scale the incoming gradient of every 128-row group by an exact power of two (or zero) so that the running exponent of
the weight-gradient accumulators (``Eacc``, ``rescale``, ``delta``) goes through every branch; ``eacc_walk`` restates that
logic on the reference to say which branches a launch takes.

One term was added to the model the issue of these tests sets out, by reading, before any run: the compact ``dz`` rows are
f16 relative to their 32-row TILE's largest magnitude, not their row's (``dz_store_h``), so a row far below its neighbours --
the ladders' 2^-120 row -- is held to ``2^-25`` of the tile's largest entry on top of ``2^-11`` of its own.

NOT YET MEASURED on an MI355X: ``test_gpu_fused_training.py::test_report_measured_ratios`` prints the worst
``|kernel - fp64| / bound`` per family (edges, walk, ascending, descending, zeros, in place) and quantity (``pytest -s``, lines
``FUSED ...``); the table belongs here once a GPU run has produced it.  On the CPU, the fp32 evaluation of the same formulas
sits at 0.003 .. 0.022 of the bounds.
"""
import functools
import math
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch

from oracle import models as om

import _jacobian_cases as jc
from _jacobian_cases import MARGIN, MIN_KEPT_SHARE, _frozen  # noqa: F401 (read as fc.* by the tests)
from _kalman_cases import GUARD_ROWS, SENTINEL  # noqa: F401
from _tol import REL_TOL  # noqa: F401

# ------------------------------------------------------------------------------ the launch geometry, next to its source
TILE_ROWS = 32                       # kernel: ntiles = (a.R + 31) / 32 -- a wave's tile is 32 particles (the lane index)
WAVES = 4                            # __launch_bounds__(256, 1): four waves; base = (grp * 4 + wave) * 32
GROUP_ROWS = WAVES * TILE_ROWS       # kernel: ngroups = (ntiles + 3) / 4 -- 128 rows per pass of a workgroup
MAX_GRID = 256                       # launch_fused: cap = ... (a.slots < 256 ? a.slots : 256)
UNITS = 64
MAX_MEAS = 4                         # include/mmf.h: MMF_LOOP_MAX_MEAS

TASKS = ("door", "push")
KINDS = ("dynamics", "measure")
NETS = tuple((t, k) for t in TASKS for k in KINDS)
DIMS = {"door": 3, "push": 2}
GAIN = 1.4                           # as the Jacobian cases: keeps the activations of seeded weights alive through nine layers
STATE_SCALE = 0.7                    # as tests/_fused_case.py
CANDIDATE_FACTOR = 1.6               # candidates drawn per trajectory: M * 1.6 + 8 (0.8 would just do at the minimum share)
YARD = 4.0
FLOOR_F16 = 2.0 ** -25               # half the spacing of f16 sub-normals
EPS_F16 = 2.0 ** -11                 # f16 round-to-nearest, relative
EPS_F32 = 2.0 ** -24


def launch(R, n_slots):
    """``(ngroups, grid)`` of the backward parts of a call (launch_fused: ``grid = min(ngroups, n_slots, 256)``, at least 1).
    The encoder-forward part of the dynamics network ignores ``n_slots`` (``cap = 256``) and writes no partial."""
    ntiles = -(-R // TILE_ROWS)
    ngroups = -(-ntiles // WAVES)
    return ngroups, max(1, min(ngroups, n_slots, MAX_GRID))


def walk(R, n_slots) -> List[List[int]]:
    """The groups each workgroup visits, in order: ``for (grp = blockIdx.x; grp < ngroups; grp += gridDim.x)``."""
    ngroups, grid = launch(R, n_slots)
    return [list(range(b, ngroups, grid)) for b in range(grid)]


def group_rows(grp, R):
    return slice(grp * GROUP_ROWS, min(R, (grp + 1) * GROUP_ROWS))


# (N, M) of the row-edge cases: R in {1, 31, 32, 33, 127, 128, 129, 257} -- one short of, at and one past a tile and a group --
# with M = 1, N = 1 and trajectories that straddle a tile end (3 x 11: rows 22..32) and a group end (3 x 43: rows 86..128);
# then M = 7 across a tile, a group and two groups, and N = 2 with M = 129.
EDGE_SHAPES = ((1, 1), (31, 1), (1, 32), (3, 11), (127, 1), (1, 128), (3, 43), (1, 257),
               (5, 7), (19, 7), (37, 7), (2, 129))
# (N, M, n_slots) of the walked launches: R = 129 (second group: one live row, three dead tiles), 513 (workgroups of 5, 3 + 2
# and 2 + 2 + 1 groups), 1025 (9 groups on 4 workgroups)
WALK_SHAPES = ((3, 43, 1), (27, 19, 1), (27, 19, 2), (27, 19, 3), (25, 41, 4))
MULTI_SHAPE = (27, 19, 2)
LADDER_M = 64                        # a ladder of L groups runs on N = 2 L trajectories of 64 rows


class Ladder(NamedTuple):
    groups: Tuple[Optional[int], ...]          # the power of two of each 128-row group, in walk order; None: zero
    rows: Tuple[Tuple[int, Optional[int]], ...] = ()   # single rows overriding their group's


LADDERS: Dict[str, Ladder] = {
    "ascending": Ladder((0, 3, 13, 31, 40)),             # a rescale at every step
    "steep": Ladder((-60, -25, 8, 40)),                  # every step >= 2^32: nothing of the sum so far survives in fp32's 24 bits
    "descending": Ladder((40, 31, 13, 3, 0)),            # delta grows past 32: the last groups are dropped whole
    "up_down_up": Ladder((0, 30, -4, 40)),               # the third group more than 2^32 below the running exponent
    "zero_groups": Ladder((None, 0, None, 5, None)),     # Eacc == 0 ("nothing yet") first; zero groups in the middle and last
    "specks": Ladder((0, 0), ((5, None), (37, -120), (133, None))),   # ok == false: a zero row, a row with e <= 16
    "all_zero": Ladder((None, None)),
}
FAMILY = {"ascending": "ascending", "steep": "ascending", "up_down_up": "ascending", "descending": "descending",
          "zero_groups": "zeros", "specks": "zeros", "all_zero": "zeros"}


def ladder_shape(name):
    L = len(LADDERS[name].groups)
    return 2 * L, LADDER_M


def row_scale(name, R) -> torch.Tensor:
    """``(R,)`` float32: the exact factor of each row's incoming gradient under the ladder ``name`` (``None``: all ones)."""
    s = torch.ones(R, dtype=torch.float32)
    if name is None:
        return s
    lad = LADDERS[name]
    assert R == GROUP_ROWS * len(lad.groups)
    for grp, k in enumerate(lad.groups):
        s[group_rows(grp, R)] = 0.0 if k is None else 2.0 ** k
    for r, k in lad.rows:
        s[r] = 0.0 if k is None else 2.0 ** k
    return s


# ------------------------------------------------------------------------------ weights
@functools.lru_cache(maxsize=None)
def state_dict(task, kind, seed=0):
    """``om.seeded_state_dict`` of the oracle's model that owns the network (the measurement model on ``pos`` and ``sensors``,
    as tests/_fused_case.py builds it); loads into the engine's model of the same name."""
    spec = om.TASKS[task]
    m = om.DynamicsModel(spec) if kind == "dynamics" else om.MeasurementModel(spec, modalities=("pos", "sensors"))
    return om.seeded_state_dict(m, seed=seed, gain=GAIN)


def n_res_of(kind):
    return 3 if kind == "dynamics" else 2


def join_state_off(kind):
    return UNITS if kind == "dynamics" else 2 * UNITS   # the state features follow the control / the two observation blocks


def params(task, kind, seed=0) -> List[torch.Tensor]:
    """The network's tensors in the order of ``PackedParticleNet._sources`` (float32), the join weight cut to its state block."""
    sd = state_dict(task, kind, seed)
    off = join_state_off(kind)
    ts = [sd["state_layers.0.weight"], sd["state_layers.0.bias"]]
    for b in ("state_layers.2.block1", "state_layers.2.block2"):
        ts += [sd[b + ".weight"], sd[b + ".bias"]]
    ts.append(sd["shared_layers.0.weight"][:, off:off + UNITS].contiguous())
    first = 1 if kind == "dynamics" else 2   # the measurement model has its nn.ReLU at index 1
    for i in range(n_res_of(kind)):
        for b in ("block1", "block2"):
            ts += [sd[f"shared_layers.{first + i}.{b}.weight"], sd[f"shared_layers.{first + i}.{b}.bias"]]
    ts += [sd["shared_layers.4.weight"], sd["shared_layers.4.bias"]]
    return ts


# ------------------------------------------------------------------------------ the network and its backward, written out
class Ref(NamedTuple):
    a: List[torch.Tensor]        # a[l] (R, 64): the input of 64 x 64 layer l, l < NL; a[NL]: the head's input
    dz: List[torch.Tensor]       # dz[l] (R, 64): dL / d (pre-activation output of layer l)
    dW: List[torch.Tensor]       # dz[l]^T a[l] (64, 64)
    db: List[torch.Tensor]       # sum_p dz[l][p] (64,)
    dz_first: torch.Tensor       # (R, 64): dL / d (pre-activation of the d -> 64 layer)
    d_states: torch.Tensor       # (R, d): through the network only
    d_traj_bias: torch.Tensor    # (N, 64)
    d_raw: torch.Tensor          # (R, n_out): dL / d head output (dynamics: through x' = x + dir sigmoid(gate); else the input)
    g_act: torch.Tensor          # (R, 64): dL / d a[2], before a[2]'s ReLU mask
    out: torch.Tensor            # (R, n_out)
    pre: torch.Tensor            # (R, sites, 64): the pre-activation of every ReLU
    dW_in: torch.Tensor          # (64, d)
    db_in: torch.Tensor
    dW_head: torch.Tensor        # (n_out, 64)
    db_head: torch.Tensor


def reference(ps, kind, M, x, tb, g, dtype) -> Ref:
    """``Ref`` of states ``x (R, d)``, per-trajectory terms ``tb (N, 64)`` and incoming gradient ``g`` -- ``(R, 1)`` = dL / d
    log-likelihood of a measurement network, ``(R, d)`` = dL / d x' of the dynamics -- under the tensors ``ps``; every
    operation in ``dtype``."""
    p = [t.to(dtype) for t in ps]
    x, tb, g = x.to(dtype), tb.to(dtype), g.to(dtype)
    n_res = (len(p) - 9) // 4
    NL = 3 + 2 * n_res
    relu_join = kind == "measure"
    W = [p[2], p[4], p[6]] + [p[7 + 4 * i + 2 * k] for i in range(n_res) for k in range(2)]
    B = [p[3], p[5], None] + [p[8 + 4 * i + 2 * k] for i in range(n_res) for k in range(2)]
    pres = []

    def act(pre):
        pres.append(pre)
        return torch.relu(pre)

    a = [act(x @ p[0].t() + p[1])]
    a.append(act(a[0] @ W[0].t() + B[0]))
    a.append(act(a[0] + a[1] @ W[1].t() + B[1]))
    jn = a[2] @ W[2].t() + tb.repeat_interleave(M, dim=0)
    a.append(act(jn) if relu_join else jn)
    for i in range(n_res):
        l1 = 3 + 2 * i
        a.append(act(a[l1] @ W[l1].t() + B[l1]))
        a.append(act(a[l1] + a[l1 + 1] @ W[l1 + 1].t() + B[l1 + 1]))
    assert len(a) == NL + 1
    out = a[NL] @ p[-2].t() + p[-1]

    if kind == "dynamics":
        d = x.shape[1]
        s = torch.sigmoid(out[:, d:])
        d_raw = torch.cat((g * s, (g * out[:, :d]).sum(1, keepdim=True) * s * (1 - s)), dim=1)
    else:
        d_raw = g
    keep = lambda t: (t > 0).to(dtype)
    dz = [None] * NL
    G = (d_raw @ p[-2]) * keep(a[NL])
    for i in reversed(range(n_res)):
        l1 = 3 + 2 * i
        dz[l1 + 1] = G
        dz[l1] = (G @ W[l1 + 1]) * keep(a[l1 + 1])
        G = G + dz[l1] @ W[l1]
        if l1 > 3 or relu_join:
            G = G * keep(a[l1])
    dz[2] = G
    g_act = G @ W[2]
    dz[1] = g_act * keep(a[2])
    dz[0] = (dz[1] @ W[1]) * keep(a[1])
    dz_first = (dz[1] + dz[0] @ W[0]) * keep(a[0])
    return Ref(a=a, dz=dz, dW=[dz[l].t() @ a[l] for l in range(NL)], db=[dz[l].sum(0) for l in range(NL)],
               dz_first=dz_first, d_states=dz_first @ p[0], d_traj_bias=dz[2].view(-1, M, UNITS).sum(1), d_raw=d_raw,
               g_act=g_act, out=out, pre=torch.stack(pres, dim=1), dW_in=dz_first.t() @ x, db_in=dz_first.sum(0),
               dW_head=d_raw.t() @ a[NL], db_head=d_raw.sum(0))


def n_sites(kind):
    return 3 + (1 if kind == "measure" else 0) + 2 * n_res_of(kind)


# ------------------------------------------------------------------------------ cases
class Case(NamedTuple):
    x: torch.Tensor          # (R, d) float32
    tb: torch.Tensor         # (N, 64) float32
    g: Tuple[torch.Tensor, torch.Tensor]   # two incoming gradients (R, n_in) float32, before any ladder
    kept_share: float        # of the candidates drawn
    candidates: int
    M: int


@functools.lru_cache(maxsize=None)
def case(task, kind, N, M, seed=0) -> Case:
    """``N`` trajectories of ``M`` rows under ``params(task, kind, seed)``: per trajectory a term ``tb = randn`` and, of its
    ``1.6 M + 8`` candidates ``x = 0.7 randn``, the first ``M`` that keep the margin TOGETHER WITH that term."""
    d = DIMS[task]
    g = torch.Generator().manual_seed(40009 + 1009 * N + 17 * M + 101 * NETS.index((task, kind)) + 7919 * seed)
    C = int(CANDIDATE_FACTOR * M) + 8
    tb = torch.randn((N, UNITS), generator=g)
    cand = STATE_SCALE * torch.randn((N, C, d), generator=g)
    n_in = d if kind == "dynamics" else 1
    grads = tuple(_frozen(torch.randn((N * M, n_in), generator=g)) for _ in range(2))
    pre = reference(params(task, kind, seed), kind, C, cand.reshape(N * C, d), tb, torch.zeros((N * C, n_in)), torch.float64).pre
    pre = pre.view(N, C, n_sites(kind), UNITS)
    picks, shares = zip(*(jc.kept_rows(pre[n], M, n_sites(kind)) for n in range(N)))
    x = torch.stack([cand[n, picks[n]] for n in range(N)]).reshape(N * M, d)
    return Case(_frozen(x), _frozen(tb), grads, sum(shares) / N, N * C, M)


def incoming(task, kind, N, M, ladder=None, which=0, seed=0) -> torch.Tensor:
    """The incoming gradient of a call: gradient ``which`` of the case times the ladder's exact row factors (float32)."""
    c = case(task, kind, N, M, seed)
    return c.g[which] * row_scale(ladder, N * M)[:, None]


@functools.lru_cache(maxsize=64)
def truth(task, kind, N, M, ladder=None, which=0, seed=0, dtype=torch.float64) -> Ref:
    c = case(task, kind, N, M, seed)
    return reference(params(task, kind, seed), kind, M, c.x, c.tb, incoming(task, kind, N, M, ladder, which, seed), dtype)


def yardstick(task, kind, N, M, ladder=None, which=0, seed=0) -> Ref:
    return truth(task, kind, N, M, ladder, which, seed, torch.float32)


# ------------------------------------------------------------------------------ bounds, from the reference alone
def weight_bounds(t: Ref, y: Ref):
    """Per-entry bounds ``(bW[l] (64, 64), bb[l] (64,))`` of ``|dW_l - fp64|`` and ``|db_l - fp64|`` for one call, from the fp64
    ``t`` and the fp32 ``y``.  ``dW_l[i][j] = sum_p dz_l[p, i] a_l[p, j]`` over the rows of the call."""
    bW, bb = [], []
    ngroups = launch(t.dz[0].shape[0], 1)[0]
    for l in range(len(t.dz)):
        adz, aa = t.dz[l].abs(), t.a[l].abs()
        gmax = adz.max()
        # both MFMA operands of the weight-gradient product are f16: `bs.hi[k][0] * fac8` (the hi half of the backward's operand
        # split, bwd_layer) and `sv[k]` (the hi half of the forward's, park_ksteps): 2^-11 each, products exact in fp32
        w = 2 * EPS_F16 * (adz.t() @ aa)
        # dz is exchanged as fixed point under the layer's running exponent (header: "their error is 2^-25 of the largest";
        # `fac32 = ... (delta < 32u) ? fac_all : 0.f` drops rows 2^-32 below it, `ok` rows below 2^-110 and zero rows)
        w = w + FLOOR_F16 * gmax * aa.sum(0)[None, :]
        # a_l below 2^-14 is an f16 sub-normal (split_pair_plain's convertvector; mask_by_halves: "below 2^-25 counts as 0")
        w = w + FLOOR_F16 * adz.sum(0)[:, None]
        # `accW = mfma_f32_32x32x16_f16(A, B, accW)`: eight accumulating products a group, each rounding the fp32 sum so far
        w = w + EPS_F32 * 8 * ngroups * (adz.t() @ aa)
        # the recompute and the data path in f16x3 where the yardstick is fp32: YARD times its worst entry against fp64
        w = w + YARD * (y.dW[l].double() - t.dW[l]).abs().max()
        # db_l: the same with a = 1 (`bsum = fdot2(A[2 d2 .. 2 d2 + 1], one2, bsum)` on the exchanged dz: 32 a group)
        b = (2 * EPS_F16 + EPS_F32 * 32 * ngroups) * adz.sum(0) + FLOOR_F16 * gmax * adz.shape[0]
        b = b + YARD * (y.db[l].double() - t.db[l]).abs().max()
        bW.append(w)
        bb.append(b)
    return bW, bb


def compact_bound(want, yard, tile_floor=True):
    """Per-row bound ``(R,)`` of a compact f16 row against ``want (R, 64)`` (fp64): ``2^-11`` of the row's largest entry plus
    ``YARD`` times the yardstick's worst entry of the row.  ``tile_floor``: plus ``2^-25`` of the largest entry of the row's
    32-row TILE -- dz_store_h divides by ``tile_absmax`` (particle_net_train_common.h: "An element's error is max(2^-11 |v|,
    2^-25 tile max)"), so a row far below its tile's largest is stored in f16 sub-normals; for ``h_last_h`` (plain f16,
    stash_store_h) the floor is 2^-25 itself."""
    R = want.shape[0]
    row = want.abs().amax(1)
    b = EPS_F16 * row + YARD * (yard.double() - want).abs().amax(1)
    if tile_floor:
        pad = torch.zeros(-(-R // TILE_ROWS) * TILE_ROWS, dtype=row.dtype)
        pad[:R] = row
        b = b + FLOOR_F16 * pad.view(-1, TILE_ROWS).amax(1).repeat_interleave(TILE_ROWS)[:R]
    else:
        b = b + FLOOR_F16
    return b


def row_rel(got, want, floor=1e-30):
    """``(R,)``: ``max |got - want| / max |want|`` of each row (the per-row measure of tests/_fused_case.py)."""
    return (got.double() - want.double()).abs().amax(1) / want.double().abs().amax(1).clamp_min(floor)


def ratio(got, want, bound) -> float:
    """Worst ``|got - want| / bound``; an entry whose bound is zero must be met exactly."""
    diff = (got.double() - want.double()).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(diff)
    r = torch.where(bound > 0, diff / bound.clamp_min(1e-300), torch.where(diff > 0, math.inf, 0.0))
    return float(r.max()) if r.numel() else 0.0


# ------------------------------------------------------------------------------ the running exponent, restated
def eacc_walk(t: Ref, R, n_slots):
    """What ``bwd_layer``'s exponent logic does on a launch, from the fp64 ``dz``: per layer the number of ``rescale``s that
    found a sum to scale (``Eacc != 0``), of rows dropped at ``delta >= 32``, of rows with ``ok == false`` (zero or below
    2^-110) and of groups met with ``Eacc == 0`` that leave it there."""
    def field(v):   # the biased exponent of the fp32 nearest to v
        return 0 if v == 0 else int(math.frexp(float(torch.tensor(v, dtype=torch.float32)))[1]) + 126

    out = []
    for dz in t.dz:
        m = dz.abs().amax(1)
        rescales = dropped = not_ok = idle = 0
        for groups in walk(R, n_slots):
            eacc = 0
            for grp in groups:
                rows = m[group_rows(grp, R)]
                eG = field(float(rows.max()))
                if 40 < eG < 255 and eG > eacc:
                    rescales += eacc != 0
                    eacc = eG
                idle += eacc == 0
                for v in rows.tolist():
                    e = field(v)
                    ok = 16 < e < 255
                    not_ok += not ok
                    dropped += ok and eacc != 0 and eacc - e >= 32
        out.append(dict(rescales=rescales, dropped=dropped, not_ok=not_ok, idle=idle))
    return out


# ------------------------------------------------------------------------------ faults, emulated on the reference
def partial(t: Ref, l, rows):
    """The rows' share of ``dW_l``."""
    return t.dz[l][rows].t() @ t.a[l][rows]


def top_group_last_row(t: Ref, R, l=0):
    """The last row of the group whose ``dz_l`` is largest."""
    ngroups = launch(R, 1)[0]
    top = max(range(ngroups), key=lambda g: float(t.dz[l][group_rows(g, R)].abs().max()))
    return group_rows(top, R).stop - 1


def faults(t: Ref, R, n_slots, l):
    """``{name: dW_l as a structurally wrong kernel would return it}`` for the launch ``(R, n_slots)``.  Ladders put their
    weight on one group; the faults strike the group with the largest incoming gradient (elsewhere they are below fp32's own
    resolution of the sum, whatever the kernel does)."""
    ngroups, grid = launch(R, n_slots)
    tops = [float(t.dz[l][group_rows(g, R)].abs().max()) for g in range(ngroups)]
    top = max(range(ngroups), key=lambda g: tops[g])
    rows = group_rows(top, R)
    last_tile = slice(max(rows.start, (-(-rows.stop // TILE_ROWS) - 1) * TILE_ROWS), rows.stop)
    slot = top % grid
    slot_rows = torch.cat([torch.arange(R)[group_rows(g, R)] for g in range(slot, ngroups, grid)])
    dW = t.dW[l]
    return {"last live tile dropped": dW - partial(t, l, last_tile),
            "last row dropped": dW - partial(t, l, slice(rows.stop - 1, rows.stop)),
            "group scaled by 2": dW + partial(t, l, rows),
            "group scaled by 1/2": dW - 0.5 * partial(t, l, rows),
            "slot's partial lost": dW - partial(t, l, slot_rows)}

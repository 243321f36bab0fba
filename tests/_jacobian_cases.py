"""Inputs and references for the forward-mode Jacobian kernel K5 (the ``kJacobian`` instantiation of ``particle_net_kernel``,
``csrc/particle_net.hip``): pure torch-CPU, shared by ``test_jacobian_cases_cpu.py`` (which certifies them without a GPU),
``test_gpu_jacobian.py`` (which runs the kernel on them) and the K6-for-K5 test of ``test_gpu_training.py``.

A Jacobian through ReLUs is discontinuous in the masks: one pre-activation within rounding of zero, and the fp32 Jacobian of
that row is off by up to 1e-1 of its norm from the fp64 one, while every other row agrees to 2e-5.  So the rows are CHOSEN:
a pool keeps, in the order drawn, the candidates whose fp64 ``margin`` -- ``|pre| / max |pre of that layer in that row|``,
minimised over the nine ReLU sites of the state path -- is at least ``MARGIN``.  No fp32 evaluation flips a mask there
(certified by the CPU test), and nothing has to be excused at comparison time.

The truth is ``reference``: the network's forward-mode recursion written out in torch -- the tangents ``d . / d x_c`` follow
the primal's ``pre > 0`` mask through every ReLU; ``x' = x + dir s``, ``d x'_i / d x_c = d dir_i s + dir_i s (1 - s) d gate
+ [i == c]`` with ``s = sigmoid(gate)`` -- in fp64, and in fp32 as the yardstick of the GPU test's error rule.  It calls
neither autograd nor the engine; the CPU test pins it to the oracle's autograd ``DynamicsModel.jacobian`` in fp64 to 1e-12.

Every array is built once per ``(task, seed)`` (``functools.lru_cache``) and shared: no test writes to one.
"""
import functools
from typing import NamedTuple, Tuple

import torch

from oracle import models as om

from _kalman_cases import GUARD_ROWS, SENTINEL  # noqa: F401 (read as jc.* by the tests)

# ------------------------------------------------------------------------------ the launch shapes, next to their source
GROUP = 4            # mmf_dynamics_jacobian: a.R = 4 * N, a.M = 4 -- a row is a group of {primal, e_1 .. e_3} columns
WAVES = 2 * 4        # launch_variant: waves = WPS * 4 with WPS = 2 (both calls of launch_ct)
TILE_COLS = 32       # launch_variant: tile = 32 * CT
MAX_GRID = 256       # launch_variant: if (grid > 256) grid = 256
BIG_COLS = 256 * 8 * 64  # launch_ct: big = a.R >= 256 * 8 * 64 -> CT = 2

TILE_ROWS = TILE_COLS // GROUP                # 8 rows in a 32-column tile
WORKGROUP_ROWS = WAVES * TILE_ROWS            # 64 rows in one pass of a workgroup
PASS_ROWS = MAX_GRID * WORKGROUP_ROWS         # 16384 rows in one pass of the capped grid at CT = 1
BIG_N = BIG_COLS // GROUP                     # 32768: the first row count of the 64-column organisation
BIG_TILE_ROWS = 2 * TILE_ROWS                 # 16 rows in a 64-column tile
POOL_ROWS = BIG_N + TILE_ROWS + 1             # 32777: one more tile, its first half full, its second half one live row

NS = (1, 2,                                                     # one and two groups
      TILE_ROWS - 1, TILE_ROWS, TILE_ROWS + 1,                  # a 32-column tile
      WORKGROUP_ROWS - 1, WORKGROUP_ROWS, WORKGROUP_ROWS + 1,   # a workgroup pass
      4 * WORKGROUP_ROWS + 1,                                   # several workgroups
      PASS_ROWS, PASS_ROWS + 1,                                 # last row of one pass / first row of a wave's second tile
      BIG_N - 1,                                                # every wave takes two tiles; last 32-column size
      BIG_N,                                                    # first 64-column size, one pass
      POOL_ROWS)

TASKS = ("door", "push")
PRECISIONS = ("f32", "f16x3")
GAIN = 1.4
MARGIN = 1e-4
MIN_KEPT_SHARE = 0.8
SCALES = (0.3, 1.0, 3.0)
CANDIDATES = 40960       # drawn per pool: 32777 / 0.88 = 37247 are needed at the measured share
N_SITES = 9              # first state layer; the state resblock's two; two in each of the three shared resblocks
TIE_UNITS = 16
TIE_ROWS = 64
TIE_CANDIDATES = 512
TIE_MIN_DIFF = 1e-2      # the >= mask Jacobian is at least this far from the > mask one, of the latter's norm
MULTI_SEEDS = (0, 1, 2)
# the pool of the single-launch tests, of the tie case and of test_k6_dynamics_with_jacobian_matches_fp64_autograd: of the three
# seeds the one whose Jacobians are far from the identity on BOTH tasks (||J - I||_F: median 6.1 door, 5.0 push, 90 % of the
# rows above 1.7; at seed 0 push's gate is nearly shut -- median 2e-2, 4e-3 over the first 9 rows -- and J = I + little
# would pass the norm-wise bar whatever the kernel's tangents were)
MAIN_SEED = 2
K6_NS = (1, 3, TILE_ROWS + 1, 50, WORKGROUP_ROWS + 1)
MULTI_CONFIGS = ((3, TILE_ROWS + 1), (3, WORKGROUP_ROWS + 1), (2, POOL_ROWS))
FP32_CAP = 1e-4          # the fp32 reference against the fp64 one, per row: a condition on the pools
X_BAR = 1e-5             # x': max|diff| / max|fp64|, the bar of test_k2_f16x3_error_against_fp64 in both precisions


# ------------------------------------------------------------------------------ weights
@functools.lru_cache(maxsize=None)
def state_dict(task, seed, tie=False):
    """``om.seeded_state_dict(seed, gain=1.4)`` of the task's dynamics model (float32); ``tie``: the first ``TIE_UNITS``
    biases of the first state layer zeroed."""
    sd = om.seeded_state_dict(om.DynamicsModel(om.TASKS[task]), seed=seed, gain=GAIN)
    if tie:
        sd["state_layers.0.bias"][:TIE_UNITS] = 0.0
    return sd


def oracle_model(task, seed, dtype, tie=False):
    """The oracle's ``DynamicsModel`` on the CPU holding ``state_dict(task, seed, tie)`` in ``dtype``."""
    m = om.DynamicsModel(om.TASKS[task])
    m.load_state_dict(state_dict(task, seed, tie))
    return m.to(dtype)


# ------------------------------------------------------------------------------ the recursion, written out
class Ref(NamedTuple):
    x_next: torch.Tensor   # (N, d)
    J: torch.Tensor        # (N, d, d): J[n, i, c] = d x'_i / d x_c
    pre: torch.Tensor      # (N, 9, 64): the pre-activation of every ReLU of the state path


def forward_mode(sd, x, u, dtype, mask_ge=False):
    """``Ref`` of ``x (N, d)``, ``u (N, 7)`` under the weights ``sd``, every operation in ``dtype``.  ``mask_ge``: the
    tangents pass where ``pre >= 0`` (the rule the kernel must NOT follow; for the tie case)."""
    w = {k: v.to(dtype) for k, v in sd.items()}
    x, u = x.to(dtype), u.to(dtype)
    d = x.shape[1]
    pres = []

    def lin(name, a):
        return a @ w[name + ".weight"].t() + w[name + ".bias"]

    def tan(name, t, cols=slice(None)):  # tangents carry no bias
        return t @ w[name + ".weight"][:, cols].t()

    def gate(pre, a, t):
        pres.append(pre)
        keep = (pre >= 0) if mask_ge else (pre > 0)
        return torch.relu(a), t * keep[:, None, :].to(dtype)

    def resblock(name, a, t):
        p1 = lin(name + ".block1", a)
        h, th = gate(p1, p1, tan(name + ".block1", t))
        p2 = lin(name + ".block2", h) + a
        return gate(p2, p2, tan(name + ".block2", th) + t)

    # control path: no tangents
    c = torch.relu(lin("control_layers.0", u))
    c1 = torch.relu(lin("control_layers.2.block1", c))
    c = torch.relu(lin("control_layers.2.block2", c1) + c)
    # state path
    p0 = lin("state_layers.0", x)
    t0 = w["state_layers.0.weight"].t()[None].expand(x.shape[0], d, -1)  # d p0 / d x_c = column c of the weight
    a, t = gate(p0, p0, t0)
    a, t = resblock("state_layers.2", a, t)
    units = a.shape[1]
    a = lin("shared_layers.0", torch.cat((c, a), dim=1))
    t = tan("shared_layers.0", t, slice(units, 2 * units))
    for k in (1, 2, 3):
        a, t = resblock(f"shared_layers.{k}", a, t)
    out = lin("shared_layers.4", a)
    dout = tan("shared_layers.4", t)                  # (N, c, d + 1)
    direction, s = out[:, :d], torch.sigmoid(out[:, d:])
    ddir, dgate = dout[:, :, :d], dout[:, :, d:]      # (N, c, i), (N, c, 1)
    x_next = x + direction * s
    J = ddir * s[:, :, None] + (direction * s * (1 - s))[:, None, :] * dgate + torch.eye(d, dtype=dtype)
    return Ref(x_next, J.transpose(1, 2).contiguous(), torch.stack(pres, dim=1))


def margin(pre, skip_first=0, n_sites=N_SITES):
    """``min |pre| / max |pre of that layer in that row|`` over the ``n_sites`` sites, per row; ``skip_first``: that many
    leading units of the first site are left out (the tie case's exact zeros)."""
    assert pre.shape[1] == n_sites
    rel = pre.abs() / pre.abs().amax(dim=2, keepdim=True)
    if skip_first:
        rel = rel.clone()
        rel[:, 0, :skip_first] = 1.0
    return rel.flatten(1).amin(dim=1)


def kept_rows(pre, rows, n_sites=N_SITES):
    """The pool rule, also of ``_fused_cases.py``: the indices of the first ``rows`` candidates, in the order drawn, whose
    fp64 ``margin`` is at least ``MARGIN``, and the share of ALL the candidates that keep it."""
    keep = margin(pre, n_sites=n_sites) >= MARGIN
    idx = torch.nonzero(keep)[:rows, 0]
    assert idx.numel() == rows, (rows, int(keep.sum()))
    return idx, float(keep.double().mean())


def _frozen(t):
    """A tensor that refuses in-place numpy writes and is not meant to be written: shared between tests."""
    t = t.contiguous()
    t.numpy().setflags(write=False)
    return t


# ------------------------------------------------------------------------------ pools
class Pool(NamedTuple):
    x: torch.Tensor        # (POOL_ROWS, d) float32
    u: torch.Tensor        # (POOL_ROWS, 7) float32
    kept_share: float      # of the candidates drawn


@functools.lru_cache(maxsize=None)
def pool(task, seed):
    """``POOL_ROWS`` rows of ``(x, u)`` for the weights ``state_dict(task, seed)``: candidates ``x = randn * s`` with ``s``
    cycling over ``SCALES`` row by row and ``u = randn``, from a fixed generator; kept, in order, where the fp64 margin is
    at least ``MARGIN``."""
    d = om.TASKS[task].state_dim
    g = torch.Generator().manual_seed(20011 + 7919 * seed + 101 * TASKS.index(task))
    scale = torch.tensor(SCALES)[torch.arange(CANDIDATES) % len(SCALES)]
    x = torch.randn((CANDIDATES, d), generator=g) * scale[:, None]
    u = torch.randn((CANDIDATES, 7), generator=g)
    idx, share = kept_rows(forward_mode(state_dict(task, seed), x, u, torch.float64).pre, POOL_ROWS)
    return Pool(_frozen(x[idx]), _frozen(u[idx]), share)


def case(task, seed, N):
    """The first ``N`` rows of ``pool(task, seed)``: ``(x, u)``, views of the shared arrays."""
    p = pool(task, seed)
    assert 0 <= N <= POOL_ROWS
    return p.x[:N], p.u[:N]


@functools.lru_cache(maxsize=2)
def reference(task, seed, dtype):
    """``Ref`` of the whole ``pool(task, seed)`` evaluated in ``dtype`` (a size's reference is its first ``N`` rows)."""
    p = pool(task, seed)
    return Ref(*(_frozen(t) for t in forward_mode(state_dict(task, seed), p.x, p.u, dtype)))


@functools.lru_cache(maxsize=None)
def outputs(task, seed, dtype) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(x', J)`` of ``reference(task, seed, dtype)``, kept for every pool (the pre-activations, 150 MB a pool in fp64,
    are not)."""
    r = reference(task, seed, dtype)
    return r.x_next, r.J


# ------------------------------------------------------------------------------ the tie case
class Tie(NamedTuple):
    x: torch.Tensor        # (TIE_ROWS, d) float32, all zero
    u: torch.Tensor        # (TIE_ROWS, 7) float32
    kept: int              # of the first TIE_ROWS candidates, those that keep the margin
    diff: torch.Tensor     # (TIE_ROWS,): || J(>=) - J(>) ||_F / || J(>) ||_F in fp64


@functools.lru_cache(maxsize=None)
def tie_case(task):
    """``TIE_ROWS`` rows with ``x = 0`` exactly under ``state_dict(task, MAIN_SEED, tie=True)``: the first ``TIE_UNITS``
    pre-activations of the first layer are ``0 w + 0`` in any precision.  The controls are kept, in order, where every
    OTHER pre-activation has the margin and the ``>=``-mask Jacobian is at least ``TIE_MIN_DIFF`` from the ``>``-mask one."""
    d = om.TASKS[task].state_dim
    sd = state_dict(task, MAIN_SEED, tie=True)
    g = torch.Generator().manual_seed(30011 + 101 * TASKS.index(task))
    u = torch.randn((TIE_CANDIDATES, 7), generator=g)
    x = torch.zeros((TIE_CANDIDATES, d))
    gt = forward_mode(sd, x, u, torch.float64)
    ge = forward_mode(sd, x, u, torch.float64, mask_ge=True)
    diff = (ge.J - gt.J).flatten(1).norm(dim=1) / gt.J.flatten(1).norm(dim=1)
    safe = margin(gt.pre, skip_first=TIE_UNITS) >= MARGIN
    idx = torch.nonzero(safe & (diff >= TIE_MIN_DIFF))[:TIE_ROWS, 0]
    assert idx.numel() == TIE_ROWS, (task, int(safe.sum()))
    return Tie(_frozen(x[idx]), _frozen(u[idx]), int(safe[:TIE_ROWS].sum()), _frozen(diff[idx]))


@functools.lru_cache(maxsize=None)
def tie_reference(task, dtype, mask_ge=False):
    t = tie_case(task)
    return Ref(*(_frozen(a) for a in forward_mode(state_dict(task, MAIN_SEED, tie=True), t.x, t.u, dtype, mask_ge=mask_ge)))


def x_err(got, want):
    """``max |got - want| / max |want|``: the measure of ``test_k2_f16x3_error_against_fp64``."""
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())

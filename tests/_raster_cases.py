"""Inputs and fp64 reference of the belief-map rasteriser (``include/mmf.h``: ``MmfPfRasterArgs`` / ``mmf_pf_raster``), in numpy
/ torch on the CPU; shared by ``test_raster_cases_cpu.py`` and ``test_gpu_maps.py``.

The reference is the header's definition in fp64 on the fp32 inputs: weights as in ``_score_cases``
(``_summary_cases.weights64``: the kernel's own two fp32 operations on the log-weights, then fp64), the cell centres by the
fp32 formula ``u_i = fmaf(float(i) - 0.5f (Gx - 1), step_x, c_x)`` and then widened, the two separable factors and one matrix
product per row, live particles only.

The bar is ``_tol.REL_TOL`` under ``rel_err_elementwise(floor=1e-3)`` taken PER ROW, every cell against max(its own value, 1e-3
of the row's largest cell); NaN exactly on the rows where the definition puts it.  ``CAP = REL_TOL / 3`` is the condition on
the INPUTS that makes the bar fair: the same definition in fp32 torch ops (separable factors, then ``bmm``) must stay within
it on every case of the family.  What the cases keep to for that:
  * every bandwidth is at least ``span / 64`` (``span = cells * step``): the window is at most 64 bandwidths wide, so the
    exponents of the cells that count stay small, and their fp32 rounding with them;
  * every bandwidth is thousands of ulps of the coordinates (here >= 0.3 beside coordinates of a few units): the cell
    centres of the definition are fp32 numbers, and a bandwidth of a few ulps of ``c`` is not resolved by them;
  * every window lies within six bandwidths of a live particle that carries the row's largest weight, so a row's largest
    reference cell is far above ``1e-30`` and nothing that counts is an fp32 underflow.
On this family the fp32 torch formulation is within 2.4e-6 of fp64 at its worst (``test_raster_cases_cpu.py`` prints the
figure per size).  Every fp32 evaluation loses everything (error 1.0) where the map underflows, a window some 25 and more
bandwidths from every particle -- which the tests of ``test_gpu_maps.py`` visit for finiteness and sign, and this family does
not."""
import functools
import math

import numpy as np

import _score_cases as sk
import _summary_cases as sm
from _summary_cases import GUARD_ROWS, MAX_M, SENTINEL  # noqa: F401 (read as rc.* by the tests)
from _tol import REL_TOL

# the kernel's own sizes (csrc/pf_raster.hip): four waves take contiguous chunks of ceil(M / WAVES) particles, each staged STAGE
# at a time; a workgroup rasterises BLOCK x BLOCK cells in TILE x TILE MFMA tiles
WAVES, STAGE, BLOCK, TILE, MAX_CELLS = 4, 64, 64, 32, 128
MS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4096)
ONE_STAGE = WAVES * STAGE            # up to here every wave stages once (255, 257 are in MS)
TWO_STAGES = 2 * WAVES * STAGE
EDGE_MS = (TWO_STAGES - 1, TWO_STAGES, TWO_STAGES + 1)
ALL_MS = tuple(sorted(set(MS + EDGE_MS)))
SMALL = 257                          # up to here the whole cross; beyond, every variant once
CELLS = ((2, 2), (31, 33), (32, 32), (33, 31), (64, 64), (65, 63), (128, 128), (128, 2))
DIMS = {2: ((0, 1), (1, 0)), 3: ((0, 1), (2, 0), (1, 2)), 4: ((0, 1), (3, 0), (2, 3), (1, 2))}  # a reversed pair, (d - 1, 0)
RS = (1, 3)
SET_VARIANTS = ("plain", "uniform", "only_a", "only_b", "dead_row")     # of _summary_cases.weighted_set
VARIANTS = SET_VARIANTS + ("nan_center", "bad_bandwidth")
BAD_BANDWIDTHS = (0.0, -0.5, math.nan, math.inf)
H_BASE = (0.3, 0.5)
CAP = sk.CAP                         # REL_TOL / 3
assert CAP <= REL_TOL / 3 and ONE_STAGE - 1 in MS and ONE_STAGE + 1 in MS


def make_case(M, d, R, variant="plain", cells=(64, 64), dims=(0, 1), seed=0):
    """``dict(states (R, M, d), log_a, log_b (R, M) or None, center (R, 2), bandwidth (R, 2), dims, cells, step)``: the
    weighted set of ``_summary_cases.weighted_set``; bandwidths ``H_BASE`` times U[1, 1.5] per row; steps ``H_BASE * min(0.5,
    48 / cells)``, so that ``span <= 48 H_BASE``; centres cycling per row through the heaviest live particle (a cell centre hits
    it with an odd count), the live weighted mean, and that particle shifted by 1.5 bandwidths.  ``"nan_center"``: a NaN in row
    ``R // 2``'s centre; ``"bad_bandwidth"``: one of ``BAD_BANDWIDTHS`` in that row's bandwidths."""
    assert variant in VARIANTS and len(cells) == 2 and len(dims) == 2
    rng = np.random.default_rng(3000017 * M + 1013 * d + 103 * R + 11 * VARIANTS.index(variant) + 7 * cells[0] + cells[1]
                                + 5 * dims[0] + dims[1] + seed)
    X, la, lb, live = sm.weighted_set(rng, M, d, R, variant if variant in SET_VARIANTS else "plain")
    case = dict(states=X, log_a=la, log_b=lb, dims=tuple(dims), cells=tuple(cells))
    h = (np.asarray(H_BASE) * rng.uniform(1.0, 1.5, (R, 2))).astype(np.float32)
    case["step"] = tuple(float(np.float32(H_BASE[k] * min(0.5, 48.0 / cells[k]))) for k in range(2))
    W = sm.weights64(case)
    c = np.zeros((R, 2), np.float32)
    for r in range(R):
        if not live[r].any():
            continue
        x = X[r][:, list(dims)]
        top = x[int(np.argmax(W[r]))]
        mean = (W[r][live[r], None] * x[live[r]].astype(np.float64)).sum(0) / W[r][live[r]].sum()
        c[r] = (top, mean, top + 1.5 * h[r])[(r + M + seed) % 3]
    if variant == "nan_center":
        c[R // 2, (M + R) % 2] = np.nan
    if variant == "bad_bandwidth":
        h[R // 2, (M + cells[0]) % 2] = BAD_BANDWIDTHS[(M + cells[1] + d) % len(BAD_BANDWIDTHS)]
    case.update(center=c, bandwidth=h)
    return case


def family():
    """``(M, d, R, variant, cells, dims)``: up to ``SMALL`` particles the whole cross of sizes, cells, state dimensions, rows
    and variants, the ``dims`` of a state dimension cycling; beyond it every variant once, cells, dimension and ``dims``
    cycling (three rows for ``plain``, ``dead_row``, ``nan_center`` and ``bad_bandwidth``, one otherwise)."""
    n = 0
    for M in ALL_MS:
        if M <= SMALL:
            for cells in CELLS:
                for d in sorted(DIMS):
                    for R in RS:
                        for variant in VARIANTS:
                            n += 1
                            yield M, d, R, variant, cells, DIMS[d][n % len(DIMS[d])]
            continue
        for i, variant in enumerate(VARIANTS):
            d = sorted(DIMS)[(i + M) % len(DIMS)]
            yield M, d, 1 if variant in ("uniform", "only_a", "only_b") else 3, variant, CELLS[(i + M) % len(CELLS)], DIMS[d][i % len(DIMS[d])]


def axes(center, step, cells):
    """The cell centres ``(u (R, Gx), v (R, Gy))`` float32: ``fmaf(float(i) - 0.5f (G - 1), step, c)`` -- the product is exact
    in fp64, the sum rounded once more to fp32."""
    out = []
    for k in range(2):
        i = (np.arange(cells[k], dtype=np.float32) - np.float32(0.5) * np.float32(cells[k] - 1)).astype(np.float64)
        with np.errstate(invalid="ignore"):
            out.append((i[None, :] * float(np.float32(step[k])) + center[:, k, None].astype(np.float64)).astype(np.float32))
    return out[0], out[1]


def nan_rows(case, W=None):
    """The rows whose map the definition makes NaN: no live particle, a NaN in the centre, a bandwidth not positive and finite."""
    W = sm.weights64(case) if W is None else W
    h = case["bandwidth"].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return ~(W > 0).any(-1) | np.isnan(case["center"]).any(-1) | ~((h > 0) & np.isfinite(h)).all(-1)


def reference_rows(X, W, center, bandwidth, dims, cells, step):
    """The definition on ``X (R, M, d)`` under unnormalised fp64 weights ``W (R, M)`` -> ``density (R, Gy, Gx)`` float64."""
    R = X.shape[0]
    Gx, Gy = cells
    u, v = axes(center, step, cells)
    bad = nan_rows(dict(center=center, bandwidth=bandwidth), W)
    out = np.full((R, Gy, Gx), np.nan)
    for r in range(R):
        if bad[r]:
            continue
        live = W[r] > 0
        x = X[r][live][:, list(dims)].astype(np.float64)
        w = W[r][live] / W[r][live].sum()
        hx, hy = (float(b) for b in bandwidth[r])
        kx = np.exp(-0.5 * ((u[r].astype(np.float64)[None, :] - x[:, 0, None]) / hx) ** 2)      # (n, Gx)
        ky = np.exp(-0.5 * ((v[r].astype(np.float64)[None, :] - x[:, 1, None]) / hy) ** 2)      # (n, Gy)
        out[r] = (ky * w[:, None]).T @ kx / (2.0 * math.pi * hx * hy)
    return out


def reference(case):
    return reference_rows(case["states"], sm.weights64(case), case["center"], case["bandwidth"], case["dims"], case["cells"],
                          case["step"])


@functools.lru_cache(maxsize=512)
def family_case(M, d, R, variant, cells, dims):
    """A family case with its reference, computed once and shared between neighbouring tests (treat both as read-only)."""
    case = make_case(M, d, R, variant, cells, dims)
    return case, reference(case)


def torch_formulation(case, dtype=None, device=None, chunk=None):
    """The same definition in torch ops, fp32 on the CPU unless told otherwise: weights ``exp(t) / sum``, dead particles
    (weight 0) with their rows zeroed, the two ``(R, M, G)`` factor tensors and ``bmm``, in chunks of ``chunk`` rows.  What a
    caller without the kernel would write -> ``(R, Gy, Gx)`` tensor."""
    import torch

    dtype = dtype or torch.float32
    to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device=device, dtype=dtype)
    with np.errstate(invalid="ignore"):
        t = to(sm.log_weight32(case))
    u, v = axes(case["center"], case["step"], case["cells"])
    return torch_rows(to(case["states"]), t, to(u), to(v), to(case["center"]), to(case["bandwidth"]), case["dims"], chunk)


def torch_rows(X, t, u, v, center, h, dims, chunk=None):
    """``torch_formulation`` on tensors: ``X (R, M, d)``, ``t (R, M)`` the log-weights minus their row maximum, the cell
    centres ``u (R, Gx)``, ``v (R, Gy)``, ``center`` and ``h (R, 2)``."""
    import torch

    R = X.shape[0]
    out = []
    for r0 in range(0, R, chunk or max(R, 1)):
        s = slice(r0, r0 + (chunk or R))
        w = torch.where(t[s] <= 0, torch.exp(t[s]), torch.zeros_like(t[s]))
        live = w > 0
        S = w.sum(-1, keepdim=True)
        W = w / S
        x = torch.where(live[..., None], X[s][..., list(dims)], torch.zeros_like(X[s][..., :2]))
        hs = h[s]
        kx = torch.exp(-0.5 * ((u[s][:, None, :] - x[:, :, 0, None]) / hs[:, 0, None, None]) ** 2)             # (R, M, Gx)
        ky = torch.exp(-0.5 * ((v[s][:, None, :] - x[:, :, 1, None]) / hs[:, 1, None, None]) ** 2) * W[..., None]
        dens = torch.bmm(ky.transpose(1, 2), kx) / (2.0 * math.pi * hs[:, 0] * hs[:, 1])[:, None, None]
        bad = ~(S[:, 0] > 0) | torch.isnan(center[s]).any(-1) | ~((hs > 0) & torch.isfinite(hs)).all(-1)
        out.append(torch.where(bad[:, None, None], torch.full_like(dens, math.nan), dens))
    return torch.cat(out) if out else X.new_zeros((0, v.shape[1], u.shape[1]))


def map_err(got, want, what=""):
    """Holds maps ``(R, Gy, Gx)`` to their reference row by row: a NaN row exactly where the reference has one (and no NaN
    elsewhere), and the worst ``rel_err_elementwise(floor=1e-3)`` of a row against its own largest cell over the rest."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    worst = 0.0
    for r in range(len(want)):
        worst = max(worst, sk.compare(got[r], want[r], (what, "row", r)))
    return worst

"""What the belief maps cost (profiles/maps/README.md): ``belief_maps`` with 64 x 64 cells around the true states on the history
of the door crossmodal particle filter at 32 x 4096 x T = 20 and 32 x 300 x T = 100 -- the density alone and with the
likelihood maps --, ``mmf_pf_raster`` alone on the same tensors, the likelihood maps alone, ``mmf_pf_density`` from the same
run as the known yardstick, and the formulation a caller would write today in torch ops on the same device: fp32 softmax
weights, the two separable ``(rows, M, G)`` factor tensors and ``torch.bmm``, in chunks of rows sized so that the two factor
tensors together stay within 256 MiB.  Device time from HIP events around ``inner`` back-to-back calls, after a warm-up call of
each, median / min / max per call over ``--reps`` windows, the runs alternating.

    python scripts/bench_maps.py [--reps 7] [--out FILE]

One JSON document.  ``multiply_adds``: ``R M Gx Gy`` per call, what both formulations spend on the map; ``raster_tflops``: twice
that over the median device time of ``hip_raster`` (a call's time, not a kernel's share of peak).  ``difference``: the kernel and
the fp32 torch formulation against the same torch ops in fp64, the largest ``|got - fp64| / max(|fp64|, 1e-3 of the row's
largest cell)`` over the rows whose largest cell is at least 1e-30."""
import math
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20
CELLS = 64
DIMS = (0, 1)


def torch_maps(states, log_a, log_b, center2, h2, step, cells, dims, dtype=torch.float32):
    """The definition of ``include/mmf.h`` in torch ops, fp32 unless told otherwise: ``density (T, N, Gy, Gx)``.  Dead
    particles (weight 0, NaN rows) are zeroed before any difference is taken."""
    from multimodalfilter_amd.pf_summaries import map_cell_centres

    T, N, M, d = states.shape
    R = T * N
    Gx, Gy = cells
    W = torch.softmax((log_a + log_b).reshape(R, M).to(dtype), dim=-1)
    live = W > 0
    X = torch.where(live[..., None], states.reshape(R, M, d)[..., list(dims)].to(dtype), torch.zeros((), dtype=dtype, device=states.device))
    u, v = (a.to(dtype) for a in map_cell_centres(center2.reshape(R, 2), step, cells))
    h = h2.reshape(R, 2).to(dtype)
    out = torch.empty((R, Gy, Gx), dtype=dtype, device=states.device)
    rows = max(1, CHUNK_BYTES // (X.element_size() * M * (Gx + Gy)))
    for r0 in range(0, R, rows):
        s = slice(r0, r0 + rows)
        kx = torch.exp(-0.5 * ((u[s][:, None, :] - X[s][:, :, 0, None]) / h[s][:, 0, None, None]) ** 2)
        ky = torch.exp(-0.5 * ((v[s][:, None, :] - X[s][:, :, 1, None]) / h[s][:, 1, None, None]) ** 2) * W[s][..., None]
        out[s] = torch.bmm(ky.transpose(1, 2), kx) / (2.0 * math.pi * h[s][:, 0] * h[s][:, 1])[:, None, None]
    return out.view(T, N, Gy, Gx)


def _exponentials_per_particle(cells):
    """What the kernel spends on a particle of a row: 32 per 32-cell tile along x and along y, in every 64 x 64 block."""
    tiles = lambda g, b0: -(-min(64, g - b0) // 32)
    return sum(32 * (tiles(cells[0], i0) + tiles(cells[1], j0)) for i0 in range(0, cells[0], 64) for j0 in range(0, cells[1], 64))


def _difference(got, want):
    """``|got - want| / max(|want|, 1e-3 of the row's largest cell)`` at its worst, over the rows whose largest cell is at
    least 1e-30 -- below it the fp32 products underflow -- and how many rows are left out."""
    top = want.nan_to_num(0.0).amax(dim=(-1, -2), keepdim=True)
    ok = torch.isfinite(want) & torch.isfinite(got) & (top >= 1e-30)
    diff = torch.where(ok, (got - want).abs() / torch.maximum(want.abs(), 1e-3 * top).clamp_min(1e-300), torch.zeros_like(want))
    return {"max_rel_difference": float(diff.max()), "rows_below_1e-30_left_out": int((top < 1e-30).sum()),
            "nan_placement_equal": bool(torch.equal(torch.isnan(got), torch.isnan(want)))}


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, truth, d = door.f, door.f.last_history, door.truth, door.dims[3]
    f.belief_maps(truth, (1.0, 1.0), dims=DIMS, cells=CELLS)                       # (for the bandwidths: the window is 32 of them)
    span = tuple(float(32.0 * f.last_maps.bandwidth[..., k].nan_to_num(0.0).median()) for k in range(2))
    f.belief_maps(truth, span, dims=DIMS, cells=CELLS)
    rec = f.last_maps
    c2, h2, step, cells = rec.center, rec.bandwidth, rec.step, rec.cells
    density = torch.empty_like(rec.density)
    dens_out = dict(log_density=torch.empty((T, N, M), dtype=torch.float32, device=dev),
                    entropy=torch.empty((T, N), dtype=torch.float32, device=dev),
                    mode=torch.empty((T, N, d), dtype=torch.float32, device=dev),
                    mode_index=torch.empty((T, N), dtype=torch.int32, device=dev),
                    bandwidth_out=torch.empty((T, N, d), dtype=torch.float32, device=dev))
    h_only = torch.empty((T, N, d), dtype=torch.float32, device=dev)
    floor = (1e-6,) * d
    sets = (h.states, h.log_weights_in, h.log_likelihoods)

    runs = {"belief_maps": (lambda: f.belief_maps(truth, span, dims=DIMS, cells=CELLS), 4),
            "belief_maps_with_likelihoods": (lambda: f.belief_maps(truth, span, dims=DIMS, cells=CELLS, likelihoods=True), 1),
            "hip_raster": (lambda: _abi.pf_raster(*sets, c2, h2, density, dims=DIMS, step=step), 20),   # mmf_pf_raster alone
            "hip_bandwidths": (lambda: _abi.pf_density(*sets, None, rule="silverman", min_bandwidth=floor, bandwidth_out=h_only), 20),
            "likelihood_maps": (lambda: f._likelihood_maps(truth, DIMS, step, cells, h.observations), 1),
            "torch_ops": (lambda: torch_maps(*sets, c2, h2, step, cells, DIMS), 2),
            "hip_density": (lambda: _abi.pf_density(*sets, None, rule="silverman", min_bandwidth=floor, **dens_out), 2)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        _abi.pf_raster(*sets, c2, h2, density, dims=DIMS, step=step)
        torch32 = torch_maps(*sets, c2, h2, step, cells, DIMS).double()
        want = torch_maps(*sets, c2, h2, step, cells, DIMS, dtype=torch.float64)
        difference = {"kernel_against_torch_fp64": _difference(density.double(), want),
                      "torch_fp32_against_torch_fp64": _difference(torch32, want)}
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    macs = float(T) * N * M * cells[0] * cells[1]
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "rule": "silverman",
            "rows": T * N, "cells": list(cells), "dims": list(DIMS), "span": list(span), "step": list(step),
            "multiply_adds": macs, "exponentials": float(T) * N * M * _exponentials_per_particle(cells),
            "workgroups": T * N * ((cells[0] + 63) // 64) * ((cells[1] + 63) // 64),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * M * (cells[0] + cells[1]))),
            "torch_factor_bytes": 4.0 * T * N * M * (cells[0] + cells[1]),
            "inner_calls_per_window": {k: inner for k, (_, inner) in runs.items()},
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_raster"],
            "raster_tflops": 2.0 * macs / (1e-3 * med["hip_raster"]) / 1e12,
            "difference": difference,
            "rows_with_a_nan_map": int(torch.isnan(density).all(dim=-1).all(dim=-1).sum()),
            "mean_mass": float(rec.mass.nan_to_num(0.0).double().mean()),
            "mean_bandwidth": [float(x) for x in h2.nan_to_num(0.0).mean((0, 1))]}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 4096, 20), (32, 300, 100))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

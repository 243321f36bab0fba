"""What the two-slice smoothing moments cost (profiles/pair_moments/README.md): ``mmf_pf_smooth_pair_moments`` on the history of
the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20 (the sizes of ``bench_marginal_smooth.py``),
next to ``mmf_pf_smooth_marginal`` on the same history -- whose weights and ``logD`` it reads -- and next to a torch-ops
restatement of the two-slice sums on the same inputs (its ``(N, rows, M, d)`` differences chunked over the rows so that they fit
in memory).  Device time from HIP events around each call, after a warm-up call, median of ``--reps`` calls, the three
alternating.

    python scripts/bench_pair_moments.py [--reps 7] [--out FILE]

One JSON document.  ``pairs`` counts the particle pairs the call visits, ``(T - 1) N M^2``; the marginal call evaluates twice
as many transition densities (one pass for ``logD``, one for the sweep).
"""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 1 << 30  # most a torch-ops temporary of (N, rows, M, d) may take


def torch_pair_moments(X, F, ll, lw, L, S, logd):
    """The sums of ``include/mmf.h`` ("two-slice smoothing moments") in torch ops, from the same smoothed weights ``S`` and
    ``logD``: per step and chunk of rows the ``(N, rows, M, d)`` residuals (difference first, then the triangular solve), the
    ``(N, rows, M)`` pair weights, and two contractions.  The finite log-weights of a benchmark run need no dead-particle
    handling."""
    T, N, M, d = X.shape
    logW = torch.log_softmax(ll + lw, dim=-1)
    Linv_t = torch.linalg.inv(L).t().contiguous()
    rows = max(1, min(M, CHUNK_BYTES // (4 * N * M * d)))
    mean = torch.zeros((T - 1, N, d), dtype=torch.float32, device=X.device)
    second = torch.zeros((T - 1, N, d, d), dtype=torch.float32, device=X.device)
    for t in range(T - 1):
        total = torch.zeros((N,), dtype=torch.float32, device=X.device)
        for i0 in range(0, M, rows):
            e = X[t + 1][:, None, :, :] - F[t][:, i0:i0 + rows, None, :]
            z = e @ Linv_t
            xi = torch.exp(logW[t][:, i0:i0 + rows, None] - 0.5 * (z * z).sum(-1) - logd[t][:, None, :]) * S[t + 1][:, None, :]
            total += xi.sum(dim=(1, 2))
            xe = xi[..., None] * e
            mean[t] += xe.sum(dim=(1, 2))
            second[t] += torch.einsum("nijc,nijk->nck", xe, e)
        mean[t] /= total[:, None]
        second[t] /= total[:, None, None]
    return mean, second


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, ctrl, d = door.f, door.f.last_history, door.ctrl, door.dims[3]
    dyn = f.dynamics_model
    L = dyn.scale_tril().detach().float().contiguous()
    with torch.no_grad():
        ctx = dyn.encode_controls(ctrl[1:].reshape((T - 1) * N, -1))
        F = dyn.propagate_encoded(h.states[:-1].reshape((T - 1) * N, M, d), ctx, None).reshape(T - 1, N, M, d)
    weights = torch.empty((T, N, M), device=dev)
    mean, cov, ess = torch.empty((T, N, d), device=dev), torch.empty((T, N, d, d), device=dev), torch.empty((T, N), device=dev)
    logd = torch.empty((T - 1, N, M), device=dev)
    rmean, rsecond = torch.empty((T - 1, N, d), device=dev), torch.empty((T - 1, N, d, d), device=dev)
    ws_floats = _abi.pf_smooth_pair_workspace_floats(T, N, M, d)
    ws = torch.empty((ws_floats,), device=dev)

    def hip_marginal():
        _abi.pf_smooth_marginal(h.states, F, h.log_likelihoods, h.log_weights_in, L, weights, mean, cov, ess, logd)
        return weights, logd

    def hip_pairs():
        _abi.pf_smooth_pair_moments(h.states, F, h.log_likelihoods, h.log_weights_in, L, weights, logd, rmean, rsecond, ws)
        return rmean, rsecond

    runs = {"hip_marginal": hip_marginal,     # mmf_pf_smooth_marginal alone, F given (it leaves what the other two read)
            "hip_pair_moments": hip_pairs,    # mmf_pf_smooth_pair_moments alone
            "torch_pair_moments": lambda: torch_pair_moments(h.states, F, h.log_likelihoods, h.log_weights_in, L, weights, logd)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        out = {k: fn() for k, fn in runs.items()}

    def rel(a, b):  # worst row against its own norm (floored at 1e-3 of the largest)
        den = b.double().flatten(2).norm(dim=-1)
        return float(((a - b).double().flatten(2).norm(dim=-1) / den.clamp_min(1e-3 * float(den.max()))).max())

    hip, ref = out["hip_pair_moments"], out["torch_pair_moments"]
    pairs = 1.0 * (T - 1) * N * M * M
    med = {k: statistics.median(v) for k, v in times.items()}
    q_hat = torch.sqrt(torch.diagonal(hip[1].double().mean(dim=(0, 1))))
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d,
            "pairs": pairs, "workspace_bytes": 4 * ws_floats,
            "ms_per_call": {k: bc.stats(v) for k, v in times.items()},
            "pairs_per_second": {k: pairs / (1e-3 * med[k]) for k in ("hip_pair_moments", "torch_pair_moments")},
            "pair_moments_over_marginal": med["hip_pair_moments"] / med["hip_marginal"],
            "torch_over_hip": med["torch_pair_moments"] / med["hip_pair_moments"],
            "hip_against_torch": {"residual_mean": rel(hip[0], ref[0]), "residual_second_moment": rel(hip[1], ref[1])},
            "model_noise_diag": [float(x) for x in torch.diagonal(L)],
            "refitted_noise_diag": [float(x) for x in q_hat]}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

"""What marginal particle smoothing costs (profiles/marginal_smooth/README.md): ``smooth(method="marginal")`` on the history of
the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, next to the obvious torch-ops implementation
of the same recursion on the same history and the same predictions (its ``(rows, M, d)`` differences chunked over the rows so
that they fit in memory).  Device time from HIP events around each call, after a warm-up call, median of ``--reps`` calls,
the two implementations alternating.

    python scripts/bench_marginal_smooth.py [--reps 7] [--out FILE]

One JSON document.  ``pairs`` counts the transition densities the recursion evaluates, ``2 (T - 1) N M^2``.
"""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 1 << 30  # most a torch-ops temporary of (N, rows, M, d) may take


def torch_marginal(X, F, ll, lw, L):
    """The recursion of ``include/mmf.h`` ("marginal particle smoothing") in torch ops: per step the ``(N, M, M)`` table of
    ``log W_t[i] + lp_t[i, j]`` (difference first, then the triangular solve), a ``logsumexp`` over ``i`` and a weighted sum
    over ``j``.  The finite log-weights of a benchmark run need no dead-particle handling."""
    T, N, M, d = X.shape
    logW = torch.log_softmax(ll + lw, dim=-1)
    Linv_t = torch.linalg.inv(L).t().contiguous()
    S = torch.empty_like(ll)
    S[T - 1] = logW[T - 1].exp()
    rows = max(1, min(M, CHUNK_BYTES // (4 * N * M * d)))
    term = torch.empty((N, M, M), dtype=torch.float32, device=X.device)
    for t in range(T - 2, -1, -1):
        for i0 in range(0, M, rows):
            z = (X[t + 1][:, None, :, :] - F[t][:, i0:i0 + rows, None, :]) @ Linv_t
            term[:, i0:i0 + rows] = logW[t][:, i0:i0 + rows, None] - 0.5 * (z * z).sum(-1)
        logD = torch.logsumexp(term, dim=1)
        term.sub_(logD[:, None, :]).exp_()
        w = torch.bmm(term, S[t + 1][:, :, None])[:, :, 0]
        S[t] = w / w.sum(-1, keepdim=True)
    mean = torch.einsum("tnm,tnmd->tnd", S, X)
    dx = X - mean[:, :, None, :]
    cov = torch.einsum("tnm,tnmi,tnmj->tnij", S, dx, dx)
    return S, mean, cov, 1.0 / (S * S).sum(-1)


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

    def hip_recursion():
        _abi.pf_smooth_marginal(h.states, F, h.log_likelihoods, h.log_weights_in, L, weights, mean, cov, ess, logd)
        return weights, mean, cov, ess

    runs = {"smooth_marginal": lambda: f.smooth(method="marginal"),      # the prediction F and the recursion
            "hip_recursion": hip_recursion,                              # mmf_pf_smooth_marginal alone, F given
            "torch_recursion": lambda: torch_marginal(h.states, F, h.log_likelihoods, h.log_weights_in, L)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        out = {k: fn() for k, fn in runs.items()}

    def rel(a, b):  # worst row against its own norm (floored at 1e-3 of the largest: a collapsed step has no spread to speak of)
        den = b.double().flatten(2).norm(dim=-1)
        return float(((a - b).double().flatten(2).norm(dim=-1) / den.clamp_min(1e-3 * float(den.max()))).max())

    hip, ref = out["hip_recursion"], out["torch_recursion"]
    pairs = 2.0 * (T - 1) * N * M * M
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d,
            "pairs": pairs, "workspace_bytes": 4 * (T - 1) * N * M, "prediction_bytes": 4 * d * (T - 1) * N * M,
            "ms_per_call": {k: bc.stats(v) for k, v in times.items()},
            "pairs_per_second": {k: pairs / (1e-3 * med[k]) for k in ("hip_recursion", "torch_recursion")},
            "torch_over_hip": med["torch_recursion"] / med["hip_recursion"],
            "hip_against_torch": {"weights": rel(hip[0], ref[0]), "mean": rel(hip[1], ref[1]), "cov": rel(hip[2].flatten(2), ref[2].flatten(2))},
            "mean_smoothed_ess_first_step": float(f.last_smoothed.ess[0].mean()),
            "mean_smoothed_ess_last_step": float(f.last_smoothed.ess[-1].mean())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)
    slower = [c for c in doc["cases"] if c["torch_over_hip"] <= 1.0]
    if slower:
        sys.exit("the HIP recursion is not faster than the torch one at " + ", ".join(f"{c['batch']} x {c['particles']}" for c in slower))


if __name__ == "__main__":
    main()

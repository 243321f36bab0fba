"""What the particle-posterior scores cost (profiles/scores/README.md): ``belief_scores(truth)`` on the history of the door
crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, ``mmf_pf_scores`` alone on the same tensors, and the
formulation a caller would write today in torch ops on the same device -- fp32 softmax weights, then the pair term from
``torch.cdist`` (the norm) and broadcast ``|x_i - x_j|`` per dimension, contracted with the weights by ``bmm``, over chunks of
rows sized so that a chunk's ``(rows, M, M)`` array stays within 256 MiB.  Device time from HIP events around each call, after
a warm-up call of each, median / min / max of ``--reps`` calls, the three alternating.

    python scripts/bench_scores.py [--reps 7] [--out FILE]

One JSON document.  ``pairs``: ``R M^2`` per call, what both formulations visit.  ``max_abs_difference`` /
``max_rel_difference``: the largest element-wise difference between the kernel and the torch formulation per output
(relative: against ``max(|value|, 1e-3 x the output's largest)``)."""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20


def torch_scores(states, log_a, log_b, truth):
    """The definition of ``include/mmf.h`` in fp32 torch ops: ``crps (T, N, d)``, ``energy (T, N)``, ``spread (T, N, d + 1)``.
    Dead particles (weight 0, NaN rows) are zeroed before any difference is taken."""
    T, N, M, d = states.shape
    R = T * N
    W = torch.softmax((log_a + log_b).reshape(R, M), dim=-1)
    X = torch.where((W > 0)[..., None], states.reshape(R, M, d), torch.zeros((), device=states.device))
    y = truth.reshape(R, 1, d)
    spread = torch.empty((R, d + 1), dtype=torch.float32, device=states.device)
    rows = max(1, CHUNK_BYTES // (4 * M * M))
    for c in range(0, R, rows):
        x, w = X[c:c + rows], W[c:c + rows]
        left, right = w[:, None, :], w[:, :, None]
        spread[c:c + rows, d] = (left @ torch.cdist(x, x) @ right)[:, 0, 0]
        for k in range(d):
            spread[c:c + rows, k] = (left @ (x[:, :, None, k] - x[:, None, :, k]).abs() @ right)[:, 0, 0]
    e = X - y
    crps = (W[..., None] * e.abs()).sum(1) - 0.5 * spread[:, :d]
    energy = (W * torch.linalg.vector_norm(e, dim=-1)).sum(1) - 0.5 * spread[:, d]
    return crps.view(T, N, d), energy.view(T, N), spread.view(T, N, d + 1)


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, truth, d = door.f, door.f.last_history, door.truth, door.dims[3]
    crps = torch.empty((T, N, d), dtype=torch.float32, device=dev)
    energy = torch.empty((T, N), dtype=torch.float32, device=dev)
    spread = torch.empty((T, N, d + 1), dtype=torch.float32, device=dev)

    def hip_scores():
        _abi.pf_scores(h.states, h.log_weights_in, h.log_likelihoods, truth, crps, energy, spread)

    def hip_spread_only():
        _abi.pf_scores(h.states, h.log_weights_in, h.log_likelihoods, None, None, None, spread)

    runs = {"belief_scores": lambda: f.belief_scores(truth),
            "hip_scores": hip_scores,                                      # mmf_pf_scores alone: all three outputs
            "hip_spread_only": hip_spread_only,                            # no truth
            "torch_ops": lambda: torch_scores(h.states, h.log_weights_in, h.log_likelihoods, truth)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        hip_scores()
        t_crps, t_energy, t_spread = torch_scores(h.states, h.log_weights_in, h.log_likelihoods, truth)
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    pairs = float(T) * N * M * M
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d,
            "rows": T * N, "pairs": pairs, "workgroups": T * N * ((M + 511) // 512),
            "workspace_bytes": _abi.pf_scores_workspace_bytes(T * N, M, d),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * M * M)),
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_scores"],
            "hip_pairs_per_second": pairs / (1e-3 * med["hip_scores"]),
            "torch_pairs_per_second": pairs / (1e-3 * med["torch_ops"]),
            "difference": {"crps": bc.max_difference(crps, t_crps), "energy": bc.max_difference(energy, t_energy),
                           "spread": bc.max_difference(spread, t_spread)},
            "rows_without_a_live_particle": int(torch.isnan(energy).sum()),
            "mean_crps": [float(v) for v in crps.nan_to_num(0.0).mean((0, 1))], "mean_energy": float(energy.nan_to_num(0.0).mean())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

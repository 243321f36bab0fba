"""What the particle-posterior density costs (profiles/density/README.md): ``belief_density(truth)`` under Silverman's rule on
the history of the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, ``mmf_pf_density`` alone on the
same tensors, and the formulation a caller would write today in torch ops on the same device -- fp32 softmax weights, the
weighted moments and the rule of thumb, then per chunk of rows and of queries the broadcast differences ``(q - x) / h`` and
``torch.logsumexp`` over the particles, a chunk sized so that its ``(rows, queries, M, d)`` array stays within 256 MiB.  Device
time from HIP events around each call, after a warm-up call of each, median / min / max of ``--reps`` calls, the runs
alternating.

    python scripts/bench_density.py [--reps 7] [--out FILE]

One JSON document.  ``pairs``: ``R M^2`` per call, what both formulations visit (the ``R M`` pairs of the truth beside them).
``max_log_difference``: the largest ``|kernel - torch| / max(1, |torch|)`` per log-valued output; ``mode_agreement``: the share
of the rows whose ``mode_index`` is the same."""
import math
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20
QUERIES = 256


def torch_density(states, log_a, log_b, truth, min_bandwidth=1e-6):
    """The definition of ``include/mmf.h`` under Silverman's rule in fp32 torch ops: ``log_density (T, N, M)``, ``log_score
    (T, N)``, ``entropy (T, N)``, ``mode_index (T, N)``, ``bandwidth (T, N, d)``.  Dead particles (weight 0, NaN rows) are
    zeroed before any difference is taken and carry ``log W = -inf``."""
    T, N, M, d = states.shape
    R = T * N
    W = torch.softmax((log_a + log_b).reshape(R, M), dim=-1)
    live = W > 0
    X = torch.where(live[..., None], states.reshape(R, M, d), torch.zeros((), device=states.device))
    mu = (W[..., None] * X).sum(1)
    var = (W[..., None] * (X - mu[:, None, :]) ** 2).sum(1)
    n_eff = 1.0 / (W * W).sum(-1)
    c = (4.0 / ((d + 2.0) * n_eff)) ** (1.0 / (d + 4.0))
    h = (var.sqrt() * c[:, None]).clamp_min(min_bandwidth)
    logw = torch.where(live, torch.log(W), torch.full_like(W, -math.inf))
    const = h.log().sum(-1) + 0.5 * d * math.log(2.0 * math.pi)
    Q = torch.cat([X, truth.reshape(R, 1, d)], dim=1)                    # the M particles and the truth: M + 1 queries
    lp = torch.empty((R, M + 1), dtype=torch.float32, device=states.device)
    rows = max(1, CHUNK_BYTES // (4 * QUERIES * M * d))
    for r0 in range(0, R, rows):
        x, lw, ih = X[r0:r0 + rows, None, :, :], logw[r0:r0 + rows, None, :], 1.0 / h[r0:r0 + rows, None, None, :]
        for q0 in range(0, M + 1, QUERIES):
            e = (Q[r0:r0 + rows, q0:q0 + QUERIES, None, :] - x) * ih
            lp[r0:r0 + rows, q0:q0 + QUERIES] = torch.logsumexp(lw - 0.5 * (e * e).sum(-1), dim=-1)
    lp -= const[:, None]
    ld = torch.where(live, lp[:, :M], torch.full_like(W, -math.inf))
    entropy = -torch.where(live, W * lp[:, :M], torch.zeros_like(W)).sum(-1)
    return ld.view(T, N, M), lp[:, M].reshape(T, N), entropy.view(T, N), torch.argmax(ld, dim=-1).view(T, N), h.view(T, N, d)


def _log_difference(got, want):
    ok = torch.isfinite(got) & torch.isfinite(want)
    diff = torch.where(ok, (got - want).abs() / want.abs().clamp_min(1.0), torch.zeros_like(got))
    same = torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isinf(got), torch.isinf(want))
    return {"max_log_difference": float(diff.max()), "nan_and_inf_placement_equal": bool(same)}


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, truth, d = door.f, door.f.last_history, door.truth, door.dims[3]
    out = dict(log_density=torch.empty((T, N, M), dtype=torch.float32, device=dev),
               log_score=torch.empty((T, N), dtype=torch.float32, device=dev),
               entropy=torch.empty((T, N), dtype=torch.float32, device=dev),
               mode=torch.empty((T, N, d), dtype=torch.float32, device=dev),
               mode_index=torch.empty((T, N), dtype=torch.int32, device=dev),
               bandwidth_out=torch.empty((T, N, d), dtype=torch.float32, device=dev))
    floor = (1e-6,) * d

    def hip_density():
        _abi.pf_density(h.states, h.log_weights_in, h.log_likelihoods, truth, rule="silverman", min_bandwidth=floor, **out)

    def hip_log_score_only():
        _abi.pf_density(h.states, h.log_weights_in, h.log_likelihoods, truth, rule="silverman", min_bandwidth=floor,
                        log_score=out["log_score"])

    runs = {"belief_density": lambda: f.belief_density(truth),
            "hip_density": hip_density,                                    # mmf_pf_density alone: all six outputs
            "hip_log_score_only": hip_log_score_only,                      # the truth alone: R M pairs
            "torch_ops": lambda: torch_density(h.states, h.log_weights_in, h.log_likelihoods, truth)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        hip_density()
        t_ld, t_score, t_entropy, t_index, t_h = torch_density(h.states, h.log_weights_in, h.log_likelihoods, truth)
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    pairs = float(T) * N * M * M
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "rule": "silverman",
            "rows": T * N, "pairs": pairs, "workgroups": T * N * ((M + 511) // 512),
            "workspace_bytes": _abi.pf_density_workspace_bytes(T * N, M, d),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * QUERIES * M * d)), "torch_queries_per_chunk": QUERIES,
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_density"],
            "hip_pairs_per_second": pairs / (1e-3 * med["hip_density"]),
            "torch_pairs_per_second": pairs / (1e-3 * med["torch_ops"]),
            "difference": {"log_density": _log_difference(out["log_density"], t_ld), "log_score": _log_difference(out["log_score"], t_score),
                           "entropy": _log_difference(out["entropy"], t_entropy),
                           "bandwidth_max_rel": float(((out["bandwidth_out"] - t_h).abs() / t_h.abs()).nan_to_num(0.0).max())},
            "mode_agreement": float((out["mode_index"].long() == t_index).float().mean()),
            "rows_without_a_live_particle": int((out["mode_index"] < 0).sum()),
            "mean_log_score": float(out["log_score"][torch.isfinite(out["log_score"])].double().mean()),
            "mean_entropy": float(out["entropy"].nan_to_num(0.0).double().mean()),
            "mean_bandwidth": [float(v) for v in out["bandwidth_out"].nan_to_num(0.0).mean((0, 1))]}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

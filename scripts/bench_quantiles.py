"""What the particle-posterior quantiles cost (profiles/quantiles/README.md): ``belief_quantiles((0.025, 0.5, 0.975), truth=)``
on the history of the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, ``mmf_pf_quantiles`` alone
on the same tensors, and the formulation a caller would write today in torch ops on the same device -- ``torch.sort`` +
``cumsum`` + ``searchsorted`` + ``gather`` in fp32 over ``(T, N, M, d)``, the cdf as a masked sum.  Device time from HIP
events around each call, after a warm-up call of each, median / min / max of ``--reps`` calls, the three alternating.

    python scripts/bench_quantiles.py [--reps 7] [--out FILE]

One JSON document.  ``kernel_bytes_per_particle``: what the one launch moves through HBM per particle of a row, ``4 (d + 2)``
in (the row's log-weights are read by each of the ``d`` workgroups of a row; the repeats hit L2) -- its outputs are ``4 d (Q
+ 1)`` bytes per ROW.  ``agreement`` compares the torch formulation's picks with the kernel's (they differ where the fp32
cumulative sum crosses elsewhere than the integer CDF)."""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PROBS = (0.025, 0.5, 0.975)


def torch_quantiles(states, log_a, log_b, probs, truth):
    """The formulation in torch ops: normalised fp32 weights, a sort per dimension, the cumulative sum in sorted order, the
    first crossing of ``p``, a gather; the cdf as a masked sum.  Dead particles (NaN rows, weight 0) sort last."""
    T, N, M, d = states.shape
    w = torch.softmax(log_a + log_b, dim=-1)                                    # (T, N, M)
    x = states.permute(0, 1, 3, 2)                                              # (T, N, d, M)
    xs, order = torch.sort(x, dim=-1)
    cs = torch.cumsum(torch.gather(w[:, :, None, :].expand(T, N, d, M), 3, order), dim=-1)
    p = torch.tensor(probs, dtype=torch.float32, device=states.device).expand(T, N, d, len(probs)).contiguous()
    j = torch.searchsorted(cs, p * cs[..., -1:]).clamp_max(M - 1)
    quant = torch.gather(xs, 3, j).permute(0, 1, 3, 2)                          # (T, N, Q, d)
    pit = (w[..., None] * (states <= truth[:, :, None, :])).sum(dim=2)          # (T, N, d)
    return quant, pit


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, truth, d = door.f, door.f.last_history, door.truth, door.dims[3]
    quant = torch.empty((T, N, len(PROBS), d), dtype=torch.float32, device=dev)
    pit = torch.empty((T, N, d), dtype=torch.float32, device=dev)

    def hip_quantiles():
        _abi.pf_quantiles(h.states, h.log_weights_in, h.log_likelihoods, PROBS, quant, truth, pit)

    def hip_quantiles_only():
        _abi.pf_quantiles(h.states, h.log_weights_in, h.log_likelihoods, PROBS, quant)

    def hip_pit_only():
        _abi.pf_quantiles(h.states, h.log_weights_in, h.log_likelihoods, (), None, truth, pit)

    runs = {"belief_quantiles": lambda: f.belief_quantiles(PROBS, truth=truth),
            "hip_quantiles": hip_quantiles,                                # mmf_pf_quantiles alone: quantiles and pit
            "hip_quantiles_only": hip_quantiles_only,                      # no query
            "hip_pit_only": hip_pit_only,                                  # Q == 0: no sort
            "torch_ops": lambda: torch_quantiles(h.states, h.log_weights_in, h.log_likelihoods, PROBS, truth)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        hip_quantiles()
        tq, tp = torch_quantiles(h.states, h.log_weights_in, h.log_likelihoods, PROBS, truth)
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    particles = float(T) * N * M
    live = ~torch.isnan(quant)
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "probs": list(PROBS),
            "rows": T * N, "workgroups": T * N * d, "lds_bytes_per_workgroup": _abi.pf_quantiles_lds_bytes(M),
            "kernel_bytes_per_particle": 4 * (d + 2), "kernel_output_bytes_per_row": 4 * d * (len(PROBS) + 1),
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_quantiles"],
            "particles_per_second": particles / (1e-3 * med["hip_quantiles"]),
            "input_gb_per_second": particles * 4 * (d + 2) / (1e-3 * med["hip_quantiles"]) / 1e9,
            "agreement": {"quantiles_equal_share": float((tq[live] == quant[live]).float().mean()),
                          "pit_max_abs_difference": float((tp - pit).abs().nan_to_num(0.0).max()),
                          "rows_without_a_live_particle": int(torch.isnan(pit).any(-1).sum())},
            "pit_mean": float(pit.nan_to_num(0.5).mean())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

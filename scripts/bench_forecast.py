"""What the k-step-ahead forecasts cost (profiles/forecast/README.md): ``belief_forecast(H, truth)`` on the history of the door
crossmodal particle filter at 32 x 4096 x T = 20 with H = 5 and at 32 x 300 x T = 100 with H = 10; its two parts alone -- the
H noise-free K2 calls of the roll-out, and ``mmf_pf_predictive`` on the centres of every lead (all six outputs; the pair pass
alone; the O(M) outputs alone) --; and the same definition in chunked fp32 torch ops on the same device and the same centres:
``softmax`` weights, dead particles' rows zeroed, per chunk of rows and per dimension the broadcast differences through
``erf`` and ``exp`` contracted with the weights by ``bmm``, a chunk's ``(rows, M, M)`` array within 256 MiB.  Device time from
HIP events around each call, after a warm-up call of each, median / min / max of ``--reps`` calls, alternating.

    python scripts/bench_forecast.py [--reps 5] [--out FILE]

One JSON document.  ``pairs``: ``sum_h (T - h) N M^2`` per call, what both formulations visit.  ``difference``: the largest
element-wise difference between the kernel and the torch formulation per output over all leads (relative: against
``max(|value|, 1e-3 x the output's largest)``)."""
import math
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20
OUTPUTS = ("mean", "covariance", "log_score", "pit", "spread", "crps")


def _expected_abs(m, s):
    return m * torch.erf(m / (s * math.sqrt(2.0))) + s * math.sqrt(2.0 / math.pi) * torch.exp(-m * m / (2.0 * s * s))


def torch_predictive(centres, log_a, log_b, tril, truth):
    """The definition of ``include/mmf.h`` in fp32 torch ops on ``centres (n, N, M, d)``: a dict of the six outputs with the
    leading ``(n, N)``.  Dead particles (weight 0, NaN rows) are zeroed before any difference is taken."""
    n, N, M, d = centres.shape
    R = n * N
    W = torch.softmax((log_a + log_b).reshape(R, M), dim=-1)
    X = torch.where((W > 0)[..., None], centres.reshape(R, M, d), torch.zeros((), device=centres.device))
    y = truth.reshape(R, 1, d)
    Q = tril @ tril.t()
    sigma = torch.sqrt(torch.diagonal(Q))
    mean = (W[..., None] * X).sum(1)
    e = X - mean[:, None, :]
    cov = torch.einsum("rm,rmi,rmj->rij", W, e, e) + Q
    spread = torch.empty((R, d), dtype=torch.float32, device=centres.device)
    rows = max(1, CHUNK_BYTES // (4 * M * M))
    for c in range(0, R, rows):
        x, w = X[c:c + rows], W[c:c + rows]
        left, right = w[:, None, :], w[:, :, None]
        for k in range(d):
            pair = _expected_abs(x[:, :, None, k] - x[:, None, :, k], math.sqrt(2.0) * sigma[k])
            spread[c:c + rows, k] = (left @ pair @ right)[:, 0, 0]
    m = y - X
    z = torch.linalg.solve_triangular(tril, m.transpose(-1, -2), upper=False)
    log_score = (torch.logsumexp(torch.log(W) - 0.5 * (z * z).sum(1), dim=1) - torch.log(torch.diagonal(tril)).sum()
                 - 0.5 * d * math.log(2.0 * math.pi))
    pit = (W[..., None] * (0.5 * torch.erfc(-m / (sigma * math.sqrt(2.0))))).sum(1)
    crps = (W[..., None] * _expected_abs(m, sigma)).sum(1) - 0.5 * spread
    return {"mean": mean.view(n, N, d), "covariance": cov.view(n, N, d, d), "log_score": log_score.view(n, N),
            "pit": pit.view(n, N, d), "spread": spread.view(n, N, d), "crps": crps.view(n, N, d)}


def case(N, M, T, H, reps, dev):
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, evaluation
    from multimodalfilter_amd.utils import tree_map

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, truth, d = door.f, door.f.last_history, door.truth, door.dims[3]
    la, lb = h.log_weights_in, h.log_likelihoods

    def forecast():
        f.noise = mmf.CounterNoise(11)  # (the same blocks every call)
        return f.belief_forecast(H, truth)

    with torch.no_grad():
        forecast()
        rec = f.last_forecast
        # the centres of every lead, as belief_forecast rolls them out, kept for the parts that are timed alone
        f.noise = mmf.CounterNoise(11)
        centres, X = [], h.states
        for k in range(1, H + 1):
            n = T - k
            F, tril = f._transition_means(X[:n], tree_map(h.controls, lambda c: c[k:T]), "bench_forecast")
            tril = tril.detach().to(torch.float32).contiguous()
            centres.append(F)
            if k < H:
                X = F + (f.noise.gaussian((n * N, M, d), like=F) @ tril.t()).reshape(n, N, M, d)
        last_sets = [h.states] + centres[:-1]  # what each K2 call reads (the noise of the timed calls is left out)
        E = lambda *tail: torch.empty((H, T, N) + tail, dtype=torch.float32, device=dev)
        out = {"mean": E(d), "covariance": E(d, d), "log_score": E(), "pit": E(d), "spread": E(d), "crps": E(d)}

        def hip(names, with_truth=True):
            for k in range(1, H + 1):
                n = T - k
                _abi.pf_predictive(centres[k - 1], la[:n], lb[:n], tril, truth[k:] if with_truth else None,
                                   **{name: out[name][k - 1, :n] for name in names})

        def k2_calls():
            for k in range(1, H + 1):
                f._transition_means(last_sets[k - 1][:T - k], tree_map(h.controls, lambda c: c[k:T]), "bench_forecast")

        def torch_ops():
            return [torch_predictive(centres[k - 1], la[:T - k], lb[:T - k], tril, truth[k:]) for k in range(1, H + 1)]

        runs = {"belief_forecast": forecast,
                "hip_predictive": lambda: hip(OUTPUTS),                          # mmf_pf_predictive alone: all six outputs, H calls
                "hip_pairs_only": lambda: hip(("spread",), with_truth=False),    # the pair pass
                "hip_rows_only": lambda: hip(("mean", "covariance", "log_score", "pit")),  # the O(M) outputs
                "k2_calls": k2_calls,                                            # the H noise-free dynamics calls
                "torch_ops": torch_ops}
        times = bc.time_alternating(runs, reps)
        hip(OUTPUTS)
        want = torch_ops()
        torch.cuda.synchronize()
        difference = {}
        for name in OUTPUTS:
            per_lead = [bc.max_difference(out[name][k - 1, :T - k], want[k - 1][name]) for k in range(1, H + 1)]
            difference[name] = {"max_abs_difference": max(p["max_abs_difference"] for p in per_lead),
                                "max_rel_difference": max(p["max_rel_difference"] for p in per_lead),
                                "nan_placement_equal": all(p["nan_placement_equal"] for p in per_lead)}
        same = all(torch.equal(out[name][k - 1, :T - k].view(torch.int32), getattr(rec, name)[k - 1, :T - k].view(torch.int32))
                   for name in OUTPUTS for k in range(1, H + 1))
    med = {k: statistics.median(x) for k, x in times.items()}
    rows = sum((T - k) * N for k in range(1, H + 1))
    pairs = float(rows) * M * M
    summary = evaluation.forecast_summary(rec, start=0)
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "horizon": H, "state_dim": d,
            "rows": rows, "pairs": pairs, "pair_workgroups": rows * ((M + 511) // 512),
            "workspace_bytes_lead_1": _abi.pf_predictive_workspace_bytes((T - 1) * N, M, d),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * M * M)),
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_predictive"],
            "hip_pairs_per_second": pairs / (1e-3 * med["hip_pairs_only"]),
            "torch_pairs_per_second": pairs / (1e-3 * med["torch_ops"]),
            "difference": difference, "parts_have_the_bits_of_belief_forecast": bool(same),
            "rows_without_a_live_particle": int(torch.isnan(rec.log_score[0, :T - 1]).sum()),
            "rmse_per_lead": [[float(v) for v in row] for row in summary["rmse"]],
            "crps_per_lead": [[float(v) for v in row] for row in summary["crps"]],
            "log_score_per_lead": [float(v) for v in summary["log_score"]]}


def main():
    ap = bc.arg_parser(__doc__)
    ap.set_defaults(reps=5)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, H, args.reps, dev) for N, M, T, H in ((32, 4096, 20, 5), (32, 300, 100, 10))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

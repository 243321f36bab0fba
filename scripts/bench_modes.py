"""What the particle-posterior modes cost (profiles/modes/README.md): ``belief_modes()`` under Silverman's rule on the history
of the door crossmodal particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, ``mmf_pf_modes`` alone on the same tensors
(the log density and the bandwidths computed beforehand), and the formulation a caller would write today in torch ops on the
same device -- per chunk of rows and of i-particles the broadcast differences ``(x_i - x_j) / h``, the order and radius masks
and a masked ``argmin`` for the links, a chunk sized so that its ``(rows, i, M, d)`` array stays within 256 MiB; then
``ceil(log2 M)`` gathers for the labels and an ``index_add_`` for the masses.  Device time from HIP events around each call,
after a warm-up call of each, median / min / max of ``--reps`` calls, the runs alternating.

    python scripts/bench_modes.py [--reps 7] [--out FILE]

One JSON document.  ``pairs``: ``R M^2`` per call, what both formulations visit.  ``agreement``: the share of the particles
whose ``parent`` / ``labels`` are the same in both, of the rows whose ``count`` is, and the largest difference of the masses
of the roots."""
import math
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CHUNK_BYTES = 256 << 20
QUERIES = 256


def torch_modes(states, log_a, log_b, log_density, bandwidth, tau):
    """The definition of ``include/mmf.h`` in fp32 torch ops: ``parent``, ``labels (T, N, M)`` int64, ``count (T, N)`` and the
    mass of every particle's tree at its root ``(T, N, M)`` (0 elsewhere).  Dead particles (weight 0, NaN rows) are zeroed
    before any difference is taken and carry a NaN level, which is above nothing."""
    T, N, M, d = states.shape
    R = T * N
    dev = states.device
    W = torch.softmax((log_a + log_b).reshape(R, M), dim=-1)
    ell = log_density.reshape(R, M)
    part = (W > 0) & ~torch.isnan(ell)
    X = torch.where(part[..., None], states.reshape(R, M, d), torch.zeros((), device=dev))
    ell = torch.where(part, ell, torch.full_like(ell, math.nan))
    ih = 1.0 / bandwidth.reshape(R, 1, 1, d)
    idx = torch.arange(M, device=dev)
    parent = torch.empty((R, M), dtype=torch.int64, device=dev)
    rows = max(1, CHUNK_BYTES // (4 * QUERIES * M * d))
    tau2 = tau * tau
    for r0 in range(0, R, rows):
        x, l = X[r0:r0 + rows], ell[r0:r0 + rows]
        for q0 in range(0, M, QUERIES):
            e = (x[:, q0:q0 + QUERIES, None, :] - x[:, None, :, :]) * ih[r0:r0 + rows]
            d2 = (e * e).sum(-1)                                                      # (rows, i, M)
            li, lj = l[:, q0:q0 + QUERIES, None], l[:, None, :]
            above = (lj > li) | ((lj == li) & (idx[None, None, :] < idx[None, q0:q0 + QUERIES, None]))
            d2 = torch.where(above & (d2 <= tau2), d2, torch.full_like(d2, math.inf))
            best, j = d2.min(dim=-1)                                                  # (the first minimum: the lowest j)
            parent[r0:r0 + rows, q0:q0 + QUERIES] = torch.where(torch.isinf(best), torch.full_like(j, -1), j)
    lab = torch.where(part & (parent >= 0), parent, idx[None, :].expand(R, M))
    for _ in range(max(1, math.ceil(math.log2(max(M, 2))))):
        lab = torch.gather(lab, 1, lab)
    mass = torch.zeros((R * M,), dtype=torch.float32, device=dev)
    mass.index_add_(0, (lab + M * torch.arange(R, device=dev)[:, None]).reshape(-1), torch.where(part, W, torch.zeros_like(W)).reshape(-1))
    count = (part & (parent < 0)).sum(-1)
    labels = torch.where(part, lab, torch.full_like(lab, -1))
    return parent.view(T, N, M), labels.view(T, N, M), count.view(T, N), mass.view(T, N, M)


def case(N, M, T, reps, dev, K=4, tau=3.0):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, d = door.f, door.f.last_history, door.dims[3]
    dens = torch.empty((T, N, M), dtype=torch.float32, device=dev)
    bw = torch.empty((T, N, d), dtype=torch.float32, device=dev)
    _abi.pf_density(h.states, h.log_weights_in, h.log_likelihoods, None, rule="silverman", min_bandwidth=(1e-6,) * d,
                    log_density=dens, bandwidth_out=bw)
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=dev)
    f32 = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)
    out = dict(parent=i32(T, N, M), labels=i32(T, N, M), count=i32(T, N), index=i32(T, N, K), modes=f32(T, N, K, d),
               mass=f32(T, N, K), mean=f32(T, N, K, d))

    def hip_modes():
        _abi.pf_modes(h.states, h.log_weights_in, h.log_likelihoods, dens, bw, link_radius=tau, max_modes=K, **out)

    def hip_links_only():
        _abi.pf_modes(h.states, h.log_weights_in, h.log_likelihoods, dens, bw, link_radius=tau, max_modes=K, parent=out["parent"])

    runs = {"belief_modes": lambda: f.belief_modes(max_modes=K, link_radius=tau),   # mmf_pf_density + mmf_pf_modes + the record
            "hip_modes": hip_modes,                                                 # mmf_pf_modes alone: all seven outputs
            "hip_links_only": hip_links_only,                                       # the pair pass without the finish
            "torch_ops": lambda: torch_modes(h.states, h.log_weights_in, h.log_likelihoods, dens, bw, tau)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        hip_modes()
        t_parent, t_labels, t_count, t_mass = torch_modes(h.states, h.log_weights_in, h.log_likelihoods, dens, bw, tau)
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    pairs = float(T) * N * M * M
    at = out["index"].clamp_min(0).long()
    t_top = torch.where(out["index"] >= 0, torch.gather(t_mass, 2, at), torch.zeros_like(out["mass"]))
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "rule": "silverman",
            "link_radius": tau, "max_modes": K, "rows": T * N, "pairs": pairs, "link_workgroups": T * N * ((M + 511) // 512),
            "finish_workgroups": T * N, "workspace_bytes": _abi.pf_modes_workspace_bytes(T * N, M, d),
            "torch_rows_per_chunk": max(1, CHUNK_BYTES // (4 * QUERIES * M * d)), "torch_queries_per_chunk": QUERIES,
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "torch_over_hip": med["torch_ops"] / med["hip_modes"],
            "hip_pairs_per_second": pairs / (1e-3 * med["hip_modes"]),
            "hip_link_pairs_per_second": pairs / (1e-3 * med["hip_links_only"]),
            "torch_pairs_per_second": pairs / (1e-3 * med["torch_ops"]),
            "agreement": {"parent": float((out["parent"].long() == t_parent).float().mean()),
                          "labels": float((out["labels"].long() == t_labels).float().mean()),
                          "count": float((out["count"].long() == t_count).float().mean()),
                          "reported_mass_max_abs_difference": float((out["mass"] - t_top).abs().max())},
            "mean_count": float(out["count"].double().mean()), "max_count": int(out["count"].max()),
            "share_of_steps_with_more_than_one_mode": float((out["count"] > 1).double().mean()),
            "mean_top_mass": float(out["mass"][..., 0].double().mean())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

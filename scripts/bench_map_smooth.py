"""What MAP path smoothing costs (profiles/map_smooth/README.md): ``smooth(method="map")`` on the history of the door crossmodal
particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, next to ``smooth(method="marginal")`` of the same commit on the
same history -- the same ``(T - 1) N M^2`` pairs per pass (the marginal smoother makes two passes), no ``exp``, and the same
``T - 1`` serial launches -- and the split of the MAP call between its forward launches and its backtrack.  Device time from
HIP events around each call, after a warm-up call, median of ``--reps`` calls, the implementations alternating; the split
from one profiled call (kernel durations by name).

    python scripts/bench_map_smooth.py [--reps 7] [--out FILE]

One JSON document.  ``pairs`` counts the transition densities the recursion evaluates, ``(T - 1) N M^2``.
"""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _kernel_split(fn):
    """Device microseconds of one call of ``fn`` by kernel: the forward launches, the backtrack, step 0.  ``None`` where the
    profiler reports no kernels."""
    from torch.profiler import ProfilerActivity, profile

    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    split = {"forward": 0.0, "backtrack": 0.0, "first": 0.0}
    launches = dict.fromkeys(split, 0)
    for e in prof.events():
        for k in split:
            if f"pf_map_{k}_kernel" in e.name:
                split[k] += float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
                launches[k] += 1
    if not any(launches.values()):
        return None
    return {"us": split, "launches": launches}


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi, evaluation

    door = bc.recorded_door_run(N, M, T, dev)
    f, h, d = door.f, door.f.last_history, door.dims[3]
    with torch.no_grad():
        F, L = f._smoothing_transition(h, "map")
    new = lambda *shape, dtype=torch.float32: torch.empty(shape, dtype=dtype, device=dev)
    v, step_max, psi = new(T, N, M), new(T, N), new(T, N, M, dtype=torch.int32)
    indices, path, logpost = new(T, N, dtype=torch.int32), new(T, N, d), new(N)
    weights, mean, cov, ess, logd = new(T, N, M), new(T, N, d), new(T, N, d, d), new(T, N), new(T - 1, N, M)

    def hip_map():
        _abi.pf_smooth_map(h.states, F, h.log_likelihoods, h.log_weights_in, L, indices, path, logpost, v, step_max, psi)

    def hip_marginal():
        _abi.pf_smooth_marginal(h.states, F, h.log_likelihoods, h.log_weights_in, L, weights, mean, cov, ess, logd)

    runs = {"smooth_map": lambda: f.smooth(method="map"),            # the prediction F and the recursion
            "smooth_marginal": lambda: f.smooth(method="marginal"),
            "hip_map": hip_map,                                      # mmf_pf_smooth_map alone, F given
            "hip_marginal": hip_marginal}                            # mmf_pf_smooth_marginal alone, F given
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        split = _kernel_split(hip_map)
        map_path = f.smooth(method="map")
        rec = f.last_smoothed
        own = evaluation.path_log_density(f, rec.indices)
        smoothed = f.smooth(method="marginal")
    pairs = float(T - 1) * N * M * M
    med = {k: statistics.median(x) for k, x in times.items()}
    err = ((rec.log_posterior.double() - own).abs() / own.abs().clamp_min(1.0)).max()
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "pairs": pairs,
            "workspace_bytes": 4 * (2 * T * N * M + T * N), "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "pairs_per_second": {"hip_map": pairs / (1e-3 * med["hip_map"]), "hip_marginal": 2.0 * pairs / (1e-3 * med["hip_marginal"])},
            "map_over_marginal": {"hip": med["hip_map"] / med["hip_marginal"], "smooth": med["smooth_map"] / med["smooth_marginal"]},
            "map_kernels": split,
            "log_posterior_against_path_log_density": float(err),
            "alive_trajectories": int((rec.indices[0] >= 0).sum()),
            "rms_distance_of_the_path_from_the_marginal_mean": float((map_path - smoothed).pow(2).sum(-1).mean().sqrt())}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

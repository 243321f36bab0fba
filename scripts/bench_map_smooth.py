"""What MAP path smoothing costs (profiles/map_smooth/README.md): ``smooth(method="map")`` on the history of the door crossmodal
particle filter at 32 x 300 x T = 100 and 32 x 4096 x T = 20, next to ``smooth(method="marginal")`` of the same commit on the
same history -- the same ``(T - 1) N M^2`` pairs per pass (the marginal smoother makes two passes), no ``exp``, and the same
``T - 1`` serial launches -- and the split of the MAP call between its forward launches and its backtrack.  Device time from
HIP events around each call, after a warm-up call, median of ``--reps`` calls, the implementations alternating; the split
from one profiled call (kernel durations by name).

    python scripts/bench_map_smooth.py [--reps 7] [--out FILE]

One JSON document.  ``pairs`` counts the transition densities the recursion evaluates, ``(T - 1) N M^2``.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


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
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import _abi, evaluation, synthetic

    d = 3
    torch.manual_seed(0)
    f = mmf.door_models.DoorCrossmodalParticleFilter().to(dev).eval()
    synthetic.stabilise_dynamics(f)
    traj = bench.to_device(synthetic.make_trajectories(state_dim=d, T=T, N=N, seed=5), dev)
    obs = {k: traj[k][1:] for k in ("image", "gripper_pos", "gripper_sensors")}
    ctrl = traj["controls"][1:]
    cal = traj["states"][0][:, None, :] + 0.3 * torch.randn((N, 256, d), device=dev)
    synthetic.calibrate_measurement_heads(f, {k: v[0] for k, v in obs.items()}, cal)
    f.num_particles = M
    f.record_history = True
    f.noise = mmf.CounterNoise(7)
    f.initialize_beliefs(mean=traj["states"][0], covariance=(torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d))
    f.forward_loop(observations=obs, controls=ctrl)
    h = f.last_history
    assert h.states.shape == (T, N, M, d)
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
        for fn in runs.values():  # warm-up: code objects, allocator
            fn()
        torch.cuda.synchronize()
        times = {k: [] for k in runs}
        for _ in range(reps):
            for k, fn in runs.items():  # alternating
                times[k].append(_event_ms(fn)[0])
        split = _kernel_split(hip_map)
        map_path = f.smooth(method="map")
        rec = f.last_smoothed
        own = evaluation.path_log_density(f, rec.indices)
        smoothed = f.smooth(method="marginal")
    pairs = float(T - 1) * N * M * M
    med = {k: statistics.median(x) for k, x in times.items()}
    err = ((rec.log_posterior.double() - own).abs() / own.abs().clamp_min(1.0)).max()
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "pairs": pairs,
            "workspace_bytes": 4 * (2 * T * N * M + T * N), "ms_per_call": {k: _stats(x) for k, x in times.items()},
            "pairs_per_second": {"hip_map": pairs / (1e-3 * med["hip_map"]), "hip_marginal": 2.0 * pairs / (1e-3 * med["hip_marginal"])},
            "map_over_marginal": {"hip": med["hip_map"] / med["hip_marginal"], "smooth": med["smooth_map"] / med["smooth_marginal"]},
            "map_kernels": split,
            "log_posterior_against_path_log_density": float(err),
            "alive_trajectories": int((rec.indices[0] >= 0).sum()),
            "rms_distance_of_the_path_from_the_marginal_mean": float((map_path - smoothed).pow(2).sum(-1).mean().sqrt())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 300, 100), (32, 4096, 20))]}
    text = json.dumps(doc, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()

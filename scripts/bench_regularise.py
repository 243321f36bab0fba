"""What regularised resampling costs and what it buys (profiles/regularise/README.md): the door crossmodal particle filter at
32 x 4096 x T = 20 and 32 x 300 x T = 100, the runs alternating on one build:

  hip_regularise_tensor / _counter   ``mmf_pf_regularise`` alone on one (N, M, d) set, its normals from a tensor or generated
                                     in the kernel (20 back-to-back calls per timing)
  loop_regularised                   ``forward_loop`` with ``regularisation = 1.0`` (counter jitter noise): the loop of launches
                                     with one jitter launch per step
  loop_launches_plain                the switch off, the persistent form and the run table switched off too: the same launches
                                     without the jitter, so that the kernel's cost is separated from the cost of losing those
                                     two paths
  loop_default                       the switch off, the default path (persistent launch or run table where eligible)

Every ``loop_*`` timing is a whole ``forward_loop`` call from a fresh belief (encoders included, the same for all three).
Device time from HIP events, after a warm-up call of each, median / min / max of ``--reps`` calls.  At both filter sizes a call of
the kernel alone is the time of one launch issued through the Python binding, not of its traffic, so ``streaming`` times it once
more on 2048 x 4096 synthetic particles (101 MB of states), where the bytes decide.

    python scripts/bench_regularise.py [--reps 7] [--out FILE]

One JSON document.  ``quality``: with and without the switch on the same data and process noise -- the mean ``unique`` of
``smooth()`` (the distinct particles of a step still alive on the final paths), the mean CRPS of ``belief_scores`` against the
true states (filtered sets), the RMS error of the estimates, and the mean number of distinct particles in the final set; without
shrinkage and with it (``regularisation_shrink``)."""
import os
import statistics
import sys

import torch

import _bench_common as bc

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SCALE = 1.0


def _loop(door, *, regularisation, default_path, history=False, shrink=False):
    """One ``forward_loop`` of the recorded filter from a fresh belief; returns the estimates."""
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import engine

    f = door.f
    f.regularisation, f.regularisation_shrink = regularisation, shrink
    f.record_history = history
    f.noise = mmf.CounterNoise(7)
    f.regularisation_noise = mmf.CounterNoise(7, stream=mmf.CounterNoise.JITTER)
    f.initialize_beliefs(mean=door.traj["states"][0], covariance=door.cov0)
    if default_path:
        return f.forward_loop(observations=door.obs, controls=door.ctrl)
    dedup, engine.PF_DEDUP = engine.PF_DEDUP, False
    try:
        with engine.persistent_forms(pf=False):
            return f.forward_loop(observations=door.obs, controls=door.ctrl)
    finally:
        engine.PF_DEDUP = dedup


def _quality(door, regularisation, shrink=False):
    T, N, M, d = door.dims
    est = _loop(door, regularisation=regularisation, default_path=True, history=True, shrink=shrink)
    f = door.f
    final = f.particle_states
    distinct = [int(torch.unique(final[n], dim=0).shape[0]) for n in range(N)]
    f.smooth()
    unique = f.last_smoothed.unique.double()
    crps = f.belief_scores(door.truth).double()
    rec = f.last_regularisation
    out = {"mean_unique_of_smooth": float(unique.mean()), "mean_unique_first_step": float(unique[0].mean()),
           "mean_crps_filtered": float(crps[torch.isfinite(crps)].mean()),
           "rms_error_of_estimates": float((est - door.truth).double().pow(2).sum(-1).mean().sqrt()),
           "mean_distinct_particles_final_set": statistics.mean(distinct)}
    if rec is not None:
        h = rec.bandwidth
        out["mean_bandwidth"] = float(h[torch.isfinite(h)].double().mean())
    f.record_history = False
    f.last_history = f.last_smoothed = None
    return out


def case(N, M, T, reps, dev):
    from multimodalfilter_amd import _abi

    door = bc.recorded_door_run(N, M, T, dev, run=False)
    d = door.dims[3]
    # one set with its record for the kernel alone: the belief after one recorded step
    f = door.f
    f.record_belief = True
    _loop(door, regularisation=None, default_path=True)
    cov, ess = f.last_belief.covariance[-1].contiguous(), f.last_belief.ess[-1].contiguous()
    f.record_belief = False
    states = f.particle_states.clone()
    eps = torch.randn((N, M, d), device=dev)
    h = torch.empty((N,), dtype=torch.float32, device=dev)
    runs = {"hip_regularise_tensor": (lambda: _abi.pf_regularise(states, cov, ess, scale=SCALE, noise=eps, bandwidth=h), 20),
            "hip_regularise_counter": (lambda: _abi.pf_regularise(states, cov, ess, scale=SCALE, counter=(7, 0, 0), bandwidth=h), 20),
            "loop_regularised": lambda: _loop(door, regularisation=SCALE, default_path=True),
            "loop_launches_plain": lambda: _loop(door, regularisation=None, default_path=False),
            "loop_default": lambda: _loop(door, regularisation=None, default_path=True)}
    with torch.no_grad():
        times = bc.time_alternating(runs, reps)
        quality = {"plain": _quality(door, None), "regularised": _quality(door, SCALE),
                   "regularised_shrink": _quality(door, SCALE, shrink=True)}
        torch.cuda.synchronize()
    med = {k: statistics.median(x) for k, x in times.items()}
    particles = float(N) * M
    return {"filter": "DoorCrossmodalParticleFilter", "batch": N, "particles": M, "steps": T, "state_dim": d, "scale": SCALE,
            "workgroups": min(N * ((M + 255) // 256), 8192),
            "bytes_per_call": {"tensor": particles * 12 * d, "counter": particles * 8 * d},
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "kernel_gb_per_second": {"tensor": particles * 12 * d / (1e6 * med["hip_regularise_tensor"]),
                                     "counter": particles * 8 * d / (1e6 * med["hip_regularise_counter"])},
            "ms_per_step": {"jitter_in_the_loop": (med["loop_regularised"] - med["loop_launches_plain"]) / T,
                            "losing_persistent_and_run_table": (med["loop_launches_plain"] - med["loop_default"]) / T,
                            "switch_on_over_default": (med["loop_regularised"] - med["loop_default"]) / T},
            "quality": quality}


def streaming(N, M, d, reps, dev):
    """The kernel alone where its bytes decide: synthetic centred sets, covariance 0.1 I, ESS 100."""
    from multimodalfilter_amd import _abi

    states, eps = torch.randn((N, M, d), device=dev), torch.randn((N, M, d), device=dev)
    mean, spare = torch.zeros((N, d), device=dev), torch.empty((N, M, d), device=dev)
    cov = (0.1 * torch.eye(d, device=dev))[None].expand(N, d, d).contiguous()
    ess = torch.full((N,), 100.0, device=dev)
    runs = {"tensor": (lambda: _abi.pf_regularise(states, cov, ess, scale=SCALE, noise=eps), 10),
            "counter": (lambda: _abi.pf_regularise(states, cov, ess, scale=SCALE, counter=(7, 0, 0)), 10),
            "tensor_shrink": (lambda: _abi.pf_regularise(states, cov, ess, scale=SCALE, noise=eps, shrink=True, mean=mean), 10),
            "device_copy_same_bytes": (lambda: spare.copy_(states), 10)}  # 8 d bytes per particle: torch's copy kernel
    times = bc.time_alternating(runs, reps)
    med = {k: statistics.median(x) for k, x in times.items()}
    nbytes = {"tensor": 12.0 * d, "counter": 8.0 * d, "tensor_shrink": 12.0 * d, "device_copy_same_bytes": 8.0 * d}
    return {"batch": N, "particles": M, "state_dim": d, "workgroups": min(N * ((M + 255) // 256), 8192),
            "ms_per_call": {k: bc.stats(x) for k, x in times.items()},
            "gb_per_second": {k: N * M * nbytes[k] / (1e6 * med[k]) for k in med}}


def main():
    args = bc.arg_parser(__doc__).parse_args()
    dev = torch.device("cuda:0")
    doc = {"device": torch.cuda.get_device_name(0),
           "cases": [case(N, M, T, args.reps, dev) for N, M, T in ((32, 4096, 20), (32, 300, 100))],
           "streaming": streaming(2048, 4096, 3, args.reps, dev)}
    bc.write_document(doc, args.out)


if __name__ == "__main__":
    main()

"""What the feature benchmarks ``scripts/bench_<feature>.py`` share: the recorded run of the door crossmodal particle filter
they measure on, the timing loop, and the argument parser and writer of their one JSON document.  A script imports this module
by name (its own directory is on ``sys.path`` when it runs) and puts the repository's root on ``sys.path`` itself; ``bench``
and the package are imported inside the functions that need them, so a script still imports without a device."""
import argparse
import json
import os
import statistics
from types import SimpleNamespace

import torch


def recorded_door_run(N, M, T, dev, *, run=True):
    """The history every feature benchmark measures on: the door crossmodal particle filter with stabilised dynamics and
    measurement heads calibrated on 256 states around the first one (so that the weights do degenerate), ``N`` synthetic
    trajectories of ``T`` steps, ``M`` particles, counter noise 7, from a belief of covariance 0.1 I.  The order is part of the
    definition: the model's construction draws from the CPU generator and the calibration states from the device's, both
    seeded by the ``manual_seed(0)`` at the top.  Returns a record of ``f`` (``last_history`` set), ``traj``, ``obs``,
    ``ctrl``, ``truth (T, N, d)``, ``cov0`` and ``dims = (T, N, M, d)``.  ``run=False`` stops once the filter is calibrated and
    sized, for a script that records, seeds and runs the loop its own way."""
    import bench
    import multimodalfilter_amd as mmf
    from multimodalfilter_amd import synthetic

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
    cov0 = (torch.eye(d, device=dev) * 0.1)[None].expand(N, d, d)
    if run:
        f.record_history = True
        f.noise = mmf.CounterNoise(7)
        f.initialize_beliefs(mean=traj["states"][0], covariance=cov0)
        f.forward_loop(observations=obs, controls=ctrl)
        assert f.last_history.states.shape == (T, N, M, d)
    return SimpleNamespace(f=f, traj=traj, obs=obs, ctrl=ctrl, truth=traj["states"][1:].contiguous(), cov0=cov0, dims=(T, N, M, d))


def event_ms(fn, inner=1):
    """Device milliseconds per call of ``fn``: HIP events around ``inner`` back-to-back calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def time_alternating(runs, reps):
    """``runs``: name -> ``fn`` or ``(fn, inner)``.  A warm-up call of each, a synchronise, then ``reps`` windows in each of
    which every run is timed once, in the dict's order: ``{name: [ms per call, ...]}``.  The caller keeps its own
    ``torch.no_grad()``."""
    runs = {k: v if isinstance(v, tuple) else (v, 1) for k, v in runs.items()}
    for fn, _ in runs.values():  # warm-up: code objects, allocator
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in runs}
    for _ in range(reps):
        for k, (fn, inner) in runs.items():  # alternating
            times[k].append(event_ms(fn, inner))
    return times


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def max_difference(got, want):
    """The largest element-wise ``|got - want|`` over the entries finite in both, absolute and relative to
    ``max(|want|, 1e-3 x the largest |want|)``, and whether the NaNs sit in the same places."""
    ok = torch.isfinite(got) & torch.isfinite(want)
    diff = torch.where(ok, (got - want).abs(), torch.zeros_like(got)).double()
    top = float(torch.where(ok, want.abs(), torch.zeros_like(want)).max())
    rel = diff / want.abs().double().clamp_min(1e-3 * top) if top > 0 else diff
    return {"max_abs_difference": float(diff.max()), "max_rel_difference": float(torch.where(ok, rel, torch.zeros_like(rel)).max()),
            "nan_placement_equal": bool(torch.equal(torch.isnan(got), torch.isnan(want)))}


def arg_parser(doc):
    """``--reps`` (7) and ``--out``; a script with a further option, or another default, sets it on the parser returned."""
    ap = argparse.ArgumentParser(description=doc, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    return ap


def write_document(doc, out):
    """Prints ``doc`` as JSON and, with ``out``, writes the same text and a newline there (the directory is made)."""
    text = json.dumps(doc, indent=1)
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as fh:
            fh.write(text + "\n")
